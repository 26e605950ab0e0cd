"""CPU suite of the checkpoint schema.  Pure host code on hand-made dicts: no device, no library call.

1. Every refusal of the checkpoint layer, character for character: tests/golden/checkpoint_refusals.json holds, for a
   detector's and a fleet's checkpoint under every configuration, the outcome of several thousand mutations — the full
   message, or null where nothing is refused — recorded at the commit named in its `written_by`.  The recording is this
   module run as a program with CHECKPOINT_REFUSALS_COMMIT=<hash> set; it calls public functions only, so the same
   code records at one commit and checks at a later one.
2. The schema table of gdn_amd/checkpoint.py is the only list of keys: the valid dicts pass, and walking the table,
   every required key is refused when it is missing and every unknown key when it is added."""
import json
import os

import numpy as np
import pytest

import test_cpu_stream_checkpoint as own
from test_cpu_fleet_checkpoint import CAP, CONFIGS, DOWN, M, N, U, _expect, _sd
from test_cpu_fleet_units import OTHER, SHA, _fleet_sd, _stream_expect

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "checkpoint_refusals.json")
FULL = ("mix_all",)                                  # the configuration (every option on) that takes the per-key dtype / shape mutations


def _harness():
    from gdn_amd import harness
    return harness


def _name(cfg):
    if cfg == dict(gaps=True, recal=64, events=True, prep=True):
        return "all"
    return "-".join(f"{k}{v}" for k, v in cfg.items()) or "plain"


def fleet_configs():
    """name -> (fleet dict, expect): CONFIGS of test_cpu_fleet_checkpoint and the mixes of test_cpu_fleet_units that add
    the optional keys."""
    out = {}
    for cfg in CONFIGS:
        sd = _sd(**cfg)
        out[_name(cfg)] = (sd, _expect(sd))
    for mix in ("recal_threshold", "recal_sensor", "all", "prep_units"):
        sd = _fleet_sd(mix)
        out["mix_" + mix] = (sd, _expect(sd, **({"prep_units": SHA} if mix == "prep_units" else {})))
    return out


def detector_configs():
    """name -> (detector dict, expect): unit 1 of every fleet configuration as a detector's dict, and the hand-made dicts
    of test_cpu_stream_checkpoint."""
    h = _harness()
    out = {name: (h.fleet_unit_to_stream(sd, 1), _stream_expect(sd)) for name, (sd, _) in fleet_configs().items()}
    out["own"] = (own._dict(), own._expect())
    out["own_no_counts"] = (own._dict(counts=False), own._expect())
    out["own_plain"] = (own._dict(gaps=False, recal=0, prep=False), own._expect(recal=0, down=None))
    return out


def _wrong_dtype(a):
    if a.dtype.kind == "U":
        return np.array(3, dtype=np.int64)
    if a.dtype.kind == "f":
        return a.astype(np.float32 if a.dtype != np.float32 else np.float64)
    if a.dtype.kind == "u":
        return a.astype(np.int8)
    return a.astype(np.int32 if a.dtype != np.int32 else np.int64)


def _wrong_shape(a):
    if a.ndim == 0:
        return a.reshape(1)
    return np.zeros(a.shape[:-1] + (a.shape[-1] + 1,), a.dtype)


def i64(v):
    return np.array(v, dtype=np.int64)


def _universe():
    """Every key any configuration of either kind holds, with a value to add it with, and one nobody knows."""
    keys = {"weights": np.zeros((3,))}
    for configs in (detector_configs(), fleet_configs()):
        for sd, _ in configs.values():
            for k, v in sd.items():
                keys.setdefault(k, v)
    return keys


def mutations(kind, name, sd, ex, universe):
    """[(mutation, dict, expect)] of one valid checkpoint."""
    out = []

    def add(label, changes=None, **expect):
        new = dict(sd)
        for k, v in (changes or {}).items():
            if v is None:
                new.pop(k, None)
            else:
                new[k] = v
        out.append((label, new, dict(ex, **expect)))
    events = {"on": 2, "off": 3, "cap": CAP, "m": M}
    for k in sd:
        a = np.asarray(sd[k])
        add("drop:" + k, {k: None})
        if a.ndim == 0 and a.dtype == np.int64:
            add("negative:" + k, {k: i64(-1)})
        if name in FULL and (a.ndim or k in ("handed", "calib", "model_sha256", "recal_threshold")):
            add("dtype:" + k, {k: _wrong_dtype(a)})
            add("shape:" + k, {k: _wrong_shape(a)})
            if a.ndim and a.dtype.kind == "i":
                add("negative:" + k, {k: np.full(a.shape, -2, a.dtype)})
    for k, v in universe.items():
        if k not in sd:
            add("add:" + k, {k: v})
    # the loader's side
    add("expect:units", units=4)
    add("expect:units_same", units=int(sd.get("units", 1)))
    for k in ("n", "w", "abi"):
        add("expect:" + k, **{k: ex[k] + 1})
    for k in ("state_bytes", "calib_bytes"):
        add("expect:" + k, **{k: ex[k] + 8})
    add("expect:prep_toggled", prep_down=None if ex["prep_down"] is not None else DOWN, prep_n=ex["n"])
    add("expect:prep_down", prep_down=10, prep_n=ex["n"])
    add("expect:prep_n", prep_n=69)
    add("expect:model", model="cd" * 32)
    add("expect:model_none", model=None)
    add("expect:events_none", events=None)
    add("expect:events", events=events)
    add("expect:events_off", events=dict(events, off=1))
    add("expect:events_cap", events=dict(events, cap=16))
    for margin in (None, 1.25, 2.0):
        add(f"expect:recal_threshold_{margin}", recal_threshold=margin)
    for sha in (None, SHA, OTHER):
        add(f"expect:prep_units_{sha and sha[:2]}", prep_units=sha)
    # the file's side
    add("format=2", {"format": i64(2)})
    add("units=0", {"units": i64(0)})
    add("calib=median", {"calib": np.array("median")})
    add("calib=flipped", {"calib": np.array("tick" if str(sd["calib"]) == "sensor" else "sensor")})
    add("events_cfg:m", {"events_cfg": np.array([2, 3, CAP, M + 1], dtype=np.int64)})
    add("events_cfg:on=0", {"events_cfg": np.array([0, 3, CAP, M], dtype=np.int64)})
    add("events_cfg:cap", {"events_cfg": np.array([2, 3, CAP + 1, M], dtype=np.int64)})
    add("prep_down=4", {"prep_down": i64(4)})
    add("prep_down=0", {"prep_down": i64(0)})
    add("prep=0", {"prep": i64(0)})
    add("raw_handed=4", {"raw_handed": i64(4)})
    add("recal=0", {"recal": i64(0)})
    add("with_gaps=flipped", {"with_gaps": i64(1 - int(sd["with_gaps"]))})
    if kind == "fleet":
        for bad in ([1, DOWN, 0], [-1, 0, 0], [0, 0, 99], [DOWN - 1, 0, 0]):
            add(f"pending={bad}", {"pending": np.array(bad, dtype=np.int32)})
        add("recal_kept:-1", {"recal_kept": np.array([1, -1, 0], dtype=np.int32)})
        add("calib_kept:-1", {"calib_kept": np.array([1, -1, 0], dtype=np.int64)})
        add("calib_counts:-1", {"calib_counts": np.full((U, N), -1, dtype=np.int32)})
        add("prep_units_sha256=3", {"prep_units_sha256": np.array(3)}, prep_units=SHA)
        add("prep_units_sha256=other", {"prep_units_sha256": np.array(OTHER)}, prep_units=SHA)
    else:
        for bad in (DOWN, -1, 1):
            add(f"raw_pending={bad}", {"raw_pending": i64(bad)})
        add("calib_kept=-2", {"calib_kept": i64(-2)})
        add("calib_kept=5", {"calib_kept": i64(5)})
    add("recal_threshold:float32", {"recal_threshold": np.array(1.25, dtype=np.float32)})
    add("recal_threshold:-1", {"recal_threshold": np.array(-1.0)})
    add("recal_threshold:nan", {"recal_threshold": np.array(float("nan"))})
    add("recal_threshold:2", {"recal_threshold": np.array(2.0)}, recal_threshold=1.25)
    add("clear_frac:alone", {"clear_frac": universe["clear_frac"], "recal_threshold": None})
    # two faults at once: which one is named is part of the behaviour
    add("two:n+abi", n=ex["n"] + 1, abi=ex["abi"] + 1)
    add("two:missing+foreign", {"med_iqr": None, "weights": np.zeros((3,))})
    add("two:model+prep", model="cd" * 32, prep_down=None if ex["prep_down"] is not None else DOWN, prep_n=ex["n"])
    add("two:format+units", {"format": i64(2), "units": None})
    add("two:units+n", {"units": i64(0)}, n=ex["n"] + 1)
    add("two:negative+misshapen", {"handed": i64(-1), "state": np.zeros((3,), np.uint8)})
    add("two:events+recal_threshold", events=None, recal_threshold=2.0)
    add("two:foreign+misshapen", {"weights": np.zeros((3,)), "threshold": np.zeros((7,))})
    add("two:calib+w", {"calib": np.array("median")}, w=ex["w"] + 1)
    return out


def _outcome(fn, *args):
    try:
        fn(*args)
    except (ValueError, TypeError) as e:
        return f"{type(e).__name__}: {e}"
    return None


def hand_over(name, fleet, stream):
    """{mutation: outcome} of the two converters for one configuration."""
    h = _harness()
    got = {}
    for u in (-1, U):
        got[f"to_stream:unit={u}"] = _outcome(h.fleet_unit_to_stream, fleet, u)
    got["to_stream:pending"] = _outcome(h.fleet_unit_to_stream, dict(fleet, pending=np.array([1, DOWN, 0], dtype=np.int32)), 1)
    got["to_stream:detector"] = _outcome(h.fleet_unit_to_stream, stream, 0)
    got["to_stream:format"] = _outcome(h.fleet_unit_to_stream, dict(fleet, format=i64(2)), 0)
    for k in fleet:
        got["to_stream:drop:" + k] = _outcome(h.fleet_unit_to_stream, {j: v for j, v in fleet.items() if j != k}, 1)
    for k, v in fleet.items():
        if np.asarray(v).ndim == 0 and np.asarray(v).dtype == np.int64:
            got["to_fleet:fleet:" + k] = _outcome(h.stream_to_fleet_unit, stream, dict(fleet, **{k: i64(int(v) + 1)}))
    changes = {"calib": np.array("tick" if str(fleet["calib"]) == "sensor" else "sensor"),
               "model_sha256": np.array("00" * 32), "events_cfg=on5": np.array([5, 3, CAP, M], dtype=np.int64),
               "events_cfg=cap16": np.array([2, 3, 16, M], dtype=np.int64),
               "events_cfg=same": np.array([2, 3, CAP, M], dtype=np.int64),
               "recal_threshold=2": np.array(2.0), "recal_threshold=1.25": np.array(1.25)}
    for k, v in changes.items():
        got["to_fleet:fleet:" + k] = _outcome(h.stream_to_fleet_unit, stream, dict(fleet, **{k.split("=")[0]: v}))
    for k in ("events_cfg", "recal_threshold"):
        got["to_fleet:fleet:drop:" + k] = _outcome(h.stream_to_fleet_unit, stream, {j: v for j, v in fleet.items() if j != k})
    for k in stream:
        got["to_fleet:drop:" + k] = _outcome(h.stream_to_fleet_unit, {j: v for j, v in stream.items() if j != k}, fleet)
    got["to_fleet:format"] = _outcome(h.stream_to_fleet_unit, dict(stream, format=i64(9)), fleet)
    got["to_fleet:fleet_file"] = _outcome(h.stream_to_fleet_unit, fleet, fleet)
    got["to_fleet:other_clock"] = _outcome(h.stream_to_fleet_unit, dict(stream, chunk=i64(2), recal_every=i64(0),
                                                                       handed=i64(7)), fleet)
    return got


def collect():
    """{section: {configuration: {mutation: outcome}}} under the code as it stands."""
    h = _harness()
    universe = _universe()
    fleets, detectors = fleet_configs(), detector_configs()
    got = {"detector": {}, "fleet": {}, "detector_file_to_fleet_checker": {}, "fleet_file_to_detector_checker": {},
           "hand_over": {}}
    for kind, configs, check in (("detector", detectors, h.stream_checkpoint_check),
                                 ("fleet", fleets, h.fleet_checkpoint_check)):
        for name, (sd, ex) in configs.items():
            assert _outcome(check, sd, ex) is None, (kind, name)                 # the valid dict passes
            got[kind][name] = {label: _outcome(check, new, expect)
                               for label, new, expect in mutations(kind, name, sd, ex, universe)}
    for name, (sd, ex) in detectors.items():
        got["detector_file_to_fleet_checker"][name] = {"": _outcome(h.fleet_checkpoint_check, sd, ex)}
    for name, (sd, ex) in fleets.items():
        got["fleet_file_to_detector_checker"][name] = {"": _outcome(h.stream_checkpoint_check, sd, ex)}
        got["hand_over"][name] = hand_over(name, sd, detectors[name][0])
    return got


def grouped(got):
    """{section: {mutation: {outcome ("": nothing is refused): the configurations with that outcome, space-separated}}}:
    the form of the file — most mutations read alike under every configuration."""
    out = {}
    for section, configs in got.items():
        for name, outcomes in configs.items():
            for label, text in outcomes.items():
                out.setdefault(section, {}).setdefault(label, {}).setdefault(text or "", []).append(name)
    return {s: {label: {t: " ".join(names) for t, names in by.items()} for label, by in labels.items()}
            for s, labels in out.items()}


@pytest.fixture(scope="module")
def recorded():
    with open(PATH) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def collected():
    return collect()


def test_the_recording_names_the_commit_that_wrote_it_and_is_no_empty_list(recorded):
    assert len(recorded["written_by"]) == 40
    texts = [t for sec in recorded["refusals"].values() for by in sec.values() for t, names in by.items()
             for _ in names.split(" ")]
    assert len(texts) > 3000 and sum(t != "" for t in texts) > 2000 and sum(t == "" for t in texts) > 100


@pytest.mark.parametrize("section", ["detector", "fleet", "detector_file_to_fleet_checker",
                                     "fleet_file_to_detector_checker", "hand_over"])
def test_every_refusal_reads_character_for_character_as_it_was_recorded(section, recorded, collected):
    want, got = recorded["refusals"][section], grouped(collected)[section]
    assert sorted(got) == sorted(want)
    for label in want:
        assert got[label] == want[label], (section, label)


# ------------------------------------------------------------------------------------ the table is the only list
def _kinds():
    from gdn_amd import checkpoint
    h = _harness()
    return {"detector": (checkpoint.DETECTOR, detector_configs(), h.stream_checkpoint_check),
            "fleet": (checkpoint.FLEET, fleet_configs(), h.fleet_checkpoint_check)}


@pytest.mark.parametrize("kind", ["detector", "fleet"])
def test_walking_the_schema_table_every_required_key_is_missed_and_every_unknown_key_is_foreign(kind):
    from gdn_amd import checkpoint
    record, configs, check = _kinds()[kind]
    known = set(record.ints) | set(record.strs) | {e.key(record) for e in checkpoint.ENTRIES if e.key(record)}
    known |= set(record.optional_strs)
    seen = set()
    for name, (sd, ex) in configs.items():
        assert set(sd) <= known, (name, set(sd) - known)             # no dict holds a key the table does not know
        check(sd, ex)
        ints = {k: int(sd[k]) for k in record.ints}
        present = checkpoint.present(record, sd, ints, str(sd["calib"]))
        required = [e.key(record) for e in checkpoint.ENTRIES if e.key(record) and e.required(present)]
        assert set(required) <= set(sd), name
        for key in list(record.ints) + list(record.strs) + required:
            with pytest.raises(ValueError, match=record.who + ": .*" + repr(key)[1:-1]):
                check({k: v for k, v in sd.items() if k != key}, ex)
            seen.add(key)
        for e in checkpoint.ENTRIES:                                 # what this configuration neither needs nor allows
            key = e.key(record)
            if key and key not in sd and not e.admits(present):
                with pytest.raises(ValueError, match=record.who + ": "):
                    check(dict(sd, **{key: np.zeros((1,))}), ex)
        with pytest.raises(ValueError, match=record.who + ": key 'no_such_key' does not belong to this configuration"):
            check(dict(sd, no_such_key=np.zeros((1,))), ex)
    assert seen >= {e.key(record) for e in checkpoint.ENTRIES if e.key(record) and e.required is not checkpoint.never}


if __name__ == "__main__":
    commit = os.environ["CHECKPOINT_REFUSALS_COMMIT"]
    with open(PATH, "w") as f:
        f.write('{"written_by": "%s", "refusals": {\n' % commit)                 # one line per mutation
        sections = grouped(collect())
        f.write(",\n".join('"%s": {\n%s\n}' % (s, ",\n".join(json.dumps(label) + ": " + json.dumps(by, sort_keys=True)
                                                              for label, by in sorted(labels.items())))
                           for s, labels in sorted(sections.items())))
        f.write("\n}}\n")
    print(PATH, os.path.getsize(PATH), "bytes")
