"""CPU suite of DESIGN §3.8m: per-unit prep tables (gdn_fleet_prep_ticks_units' C-ABI surface, PrepUnits, fleet_check_prep,
the fleet checkpoint's optional `prep_units_sha256`) and unit hand-over (harness.fleet_unit_to_stream /
stream_to_fleet_unit) on hand-made dicts.  Pure host code: no device is needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_cpu_fleet_checkpoint import ABI, CAP, DOWN, M, N, R, STATE_BYTES, U, W, _expect, _sd, _with

GDN_ERR_ARG, GDN_ERR_UNSUPPORTED = -1, -3
FAKE = 4096          # a non-null, 16-byte aligned address that is never dereferenced on the host
NAME = "gdn_fleet_prep_ticks_units"


def _harness():
    from gdn_amd import harness
    return harness


# ------------------------------------------------------------------------------------------------- the entry point
def test_the_new_symbol_is_declared_bound_and_exported_with_the_shared_forms_signature():
    from gdn_amd import _lib as binding
    header = open(os.path.join(ROOT, "include", "gdn_hip.h")).read()
    declared = dict((name, ret) for ret, name in re.findall(r"^(int|long long)\s+(gdn_\w+)\s*\(", header, flags=re.M))
    lib = binding.load()
    assert declared[NAME] == "int" and binding.SIGNATURES[NAME] == binding.SIGNATURES["gdn_fleet_prep_ticks"]
    fn = getattr(lib, NAME)
    assert fn.argtypes == binding.SIGNATURES[NAME] and fn.restype is ctypes.c_int
    params = re.search(NAME + r"\s*\(([^)]*)\)\s*;", header).group(1)
    assert len(params.split(",")) == len(binding.SIGNATURES[NAME])
    assert "#define GDN_ABI_VERSION 23" in header and binding.ABI_VERSION == 23 and lib.gdn_abi_version() == 23


def _ticks(rows=40, f64=0, units=3, c=4, n=127, down=10, **kw):
    from gdn_amd import _lib as binding
    a = dict(raw=FAKE, raw_counts=FAKE, pend=FAKE, tables=FAKE, out=FAKE, counts=FAKE)
    a.update(kw)
    return getattr(binding.load(), NAME)(a["raw"], rows, f64, a["raw_counts"], a["pend"], units, c, n, down, a["tables"],
                                         a["out"], a["counts"], None)


def test_the_refusals_are_those_of_the_shared_form_all_before_any_launch():
    for null in ("raw", "raw_counts", "pend", "tables", "out", "counts"):
        for f64 in (0, 1):
            assert _ticks(f64=f64, **{null: None}) == GDN_ERR_ARG, null
    for rows in (0, -1, 41, 1 << 30):
        assert _ticks(rows=rows) == GDN_ERR_ARG, rows
    for shape in (dict(units=4097, c=1), dict(units=1, c=4097), dict(units=17, c=241), dict(units=0), dict(c=0),
                  dict(n=4097), dict(n=0), dict(down=0), dict(down=65), dict(down=-3)):
        assert _ticks(rows=1, **shape) == GDN_ERR_UNSUPPORTED, shape


def test_the_wrapper_given_per_unit_tables_still_has_no_cpu_fallback():
    from gdn_amd import _lib as binding, ops
    raw, cnt, pend = torch.zeros((3, 8, 9)), torch.zeros(3, dtype=torch.int32), torch.zeros(64, dtype=torch.int64)
    with pytest.raises(binding.GdnHipError, match="no CPU fallback"):
        ops.fleet_prep_ticks(raw, cnt, pend, 4, torch.zeros((3, 9, 2), dtype=torch.float64), torch.zeros((3, 2, 9)), cnt)


# ------------------------------------------------------------------------------------------------------- PrepUnits
def _prep(n=9, down=4, shift=0.0):
    from gdn_amd.prep import Prep
    table = torch.stack([torch.full((n,), 1.0 + shift, dtype=torch.float64),
                         torch.full((n,), shift, dtype=torch.float64)], dim=1)
    return Prep(table, torch.full((n, 4), shift, dtype=torch.float64), down)


def test_prep_units_stacks_preps_hands_out_a_unit_and_round_trips_through_one_npz(tmp_path):
    import gdn_amd
    from gdn_amd.prep import Prep, PrepUnits
    assert gdn_amd.PrepUnits is PrepUnits
    preps = [_prep(shift=0.5 * u) for u in range(3)]
    pu = PrepUnits.from_preps(preps)
    assert (pu.units, pu.n, pu.down) == (3, 9, 4) and pu.tables.shape == (3, 9, 2) and pu.stats.shape == (3, 9, 4)
    for u in range(3):
        one = pu.unit(u)
        assert isinstance(one, Prep) and one.down == 4 and one.names == pu.names
        assert torch.equal(one.table, preps[u].table) and torch.equal(one.stats, preps[u].stats)
    with pytest.raises(ValueError, match=r"unit\(3\)"):
        pu.unit(3)
    path = str(tmp_path / "units.npz")
    pu.save(path)
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == ["down", "names", "stats", "tables"]
    back = PrepUnits.load(path, device="cpu")
    assert torch.equal(back.tables, pu.tables) and torch.equal(back.stats, pu.stats) and back.down == 4
    assert back.names == pu.names and back.fingerprint() == pu.fingerprint()
    other = PrepUnits.from_preps([preps[0], preps[2], preps[1]])
    assert other.fingerprint() != pu.fingerprint()                   # the order of the units is part of it
    assert PrepUnits.from_preps([_prep(down=5)] * 3).fingerprint() != PrepUnits.from_preps([_prep()] * 3).fingerprint()


def test_from_preps_refuses_unequal_down_and_n_by_name():
    from gdn_amd.prep import PrepUnits
    with pytest.raises(ValueError, match="down: unit 1 has down = 5, unit 0 has down = 4"):
        PrepUnits.from_preps([_prep(), _prep(down=5)])
    with pytest.raises(ValueError, match="n: unit 2 was fitted on 10 sensors, unit 0 on 9"):
        PrepUnits.from_preps([_prep(), _prep(), _prep(n=10)])
    with pytest.raises(ValueError, match="at least one Prep"):
        PrepUnits.from_preps([])
    with pytest.raises(ValueError, match=r"tables \[U >= 1, n, 2\]"):
        PrepUnits(torch.zeros((9, 2), dtype=torch.float64), torch.zeros((9, 4), dtype=torch.float64), 4)
    with pytest.raises(ValueError, match=r"stats \[3, 9, 4\]"):
        PrepUnits(torch.zeros((3, 9, 2), dtype=torch.float64), torch.zeros((9, 4), dtype=torch.float64), 4)


def test_fleet_check_prep_learns_the_per_unit_form_and_refuses_another_u_before_any_device_work():
    from gdn_amd.prep import PrepUnits
    h = _harness()
    pu = PrepUnits.from_preps([_prep(shift=u) for u in range(3)])
    h.fleet_check_prep(pu, 3, 4, 9)
    h.fleet_check_prep(_prep(), 5, 4, 9)                             # a shared table serves any number of units
    with pytest.raises(ValueError, match="prep: per-unit tables of 3 units, the fleet has units = 4"):
        h.fleet_check_prep(pu, 4, 4, 9)
    with pytest.raises(ValueError, match="prep: fitted on 9 sensors, the model has 10"):
        h.fleet_check_prep(pu, 3, 4, 10)
    assert h.prep_units(pu) == pu.fingerprint() and h.prep_units(_prep()) is None and h.prep_units(None) is None


def test_the_constructor_refuses_per_unit_tables_of_another_u_on_the_host():
    from gdn_amd import GDN
    from gdn_amd.prep import PrepUnits
    h = _harness()
    model = GDN([torch.zeros((2, 1), dtype=torch.long)], 9, dim=16, input_dim=5, topk=3)
    pu = PrepUnits.from_preps([_prep(shift=u) for u in range(2)])
    with pytest.raises(ValueError, match="prep: per-unit tables of 2 units, the fleet has units = 3"):
        h.StreamFleet(model, torch.zeros((3, 9, 2), dtype=torch.float64), 1.0, torch.zeros((3, 9, 5)), 4, prep=pu)


# ------------------------------------------------------------------------------------ the checkpoint's optional key
SHA, OTHER = "cd" * 32, "ef" * 32


def test_the_checkpoint_checker_tells_shared_from_per_unit_tables_and_one_set_of_tables_from_another():
    h = _harness()
    shared = _sd(prep=True)
    units = _with(shared, prep_units_sha256=np.array(SHA))
    h.fleet_checkpoint_check(shared, _expect(shared))                # a file without the new key passes as it did
    h.fleet_checkpoint_check(shared, _expect(shared, prep_units=None))
    h.fleet_checkpoint_check(units, _expect(units, prep_units=SHA))
    who = "fleet checkpoint: prep_units_sha256"
    with pytest.raises(ValueError, match=who + ".*per-unit prep tables and is resumed with one shared Prep"):
        h.fleet_checkpoint_check(units, _expect(units))
    with pytest.raises(ValueError, match=who + ".*one shared prep table and is resumed with per-unit tables"):
        h.fleet_checkpoint_check(shared, _expect(shared, prep_units=SHA))
    with pytest.raises(ValueError, match=who + " differs from the per-unit tables given"):
        h.fleet_checkpoint_check(units, _expect(units, prep_units=OTHER))
    plain = _with(_sd(), prep_units_sha256=np.array(SHA))
    with pytest.raises(ValueError, match="fleet checkpoint: key 'prep_units_sha256' without a prep"):
        h.fleet_checkpoint_check(plain, _expect(plain))
    with pytest.raises(ValueError, match="fleet checkpoint: 'prep_units_sha256' must be one string"):
        h.fleet_checkpoint_check(_with(units, prep_units_sha256=np.array(3)), _expect(units, prep_units=SHA))


# --------------------------------------------------------------------------------------------------- unit hand-over
MARGIN = 1.25
MIXES = {"plain": dict(), "gaps": dict(gaps=True), "events": dict(events=True), "recal_tick": dict(recal=R),
         "recal_sensor": dict(gaps=True, recal=R, calib="sensor"), "recal_threshold": dict(recal=R, events=True),
         "prep": dict(prep=True), "prep_units": dict(prep=True), "all": dict(gaps=True, recal=R, events=True, prep=True),
         "no_log": dict(log=0)}


def _fleet_sd(mix):
    sd = _sd(**MIXES[mix])
    rng = np.random.default_rng(11)
    if mix in ("recal_threshold", "all"):
        sd["recal_threshold"] = np.array(MARGIN, dtype=np.float64)
        sd["clear_frac"] = rng.random((U,))
    if mix in ("recal_sensor", "all"):
        sd["calib_counts"] = rng.integers(0, 99, (U, N)).astype(np.int32)
        sd["calib_kept"] = rng.integers(0, 99, (U,)).astype(np.int64)
    if mix == "prep_units":
        sd["prep_units_sha256"] = np.array(SHA)
    return sd


def _stream_expect(sd_fleet, **kw):
    h = _harness()
    recal, prep = int(sd_fleet["recal"]), int(sd_fleet["prep"])
    e = {"n": N, "w": W, "abi": ABI, "state_bytes": STATE_BYTES, "calib_bytes": h.stream_calib_bytes(N, recal),
         "model": "ab" * 32, "prep_down": DOWN if prep else None, "prep_n": N if prep else None}
    e.update(kw)
    return e


PER_UNIT = ("state", "med_iqr", "threshold", "log_ticks", "log_sensors", "gaps", "ring_keys", "ring_keep", "recal_counts",
            "recal_kept", "events", "clear", "clear_frac", "calib_counts", "calib_kept", "pending", "pending_ticks")


@pytest.mark.parametrize("mix", list(MIXES))
def test_fleet_to_stream_to_fleet_reproduces_the_units_arrays_byte_for_byte(mix):
    h = _harness()
    fleet = _fleet_sd(mix)
    h.fleet_checkpoint_check(fleet, _expect(fleet, prep_units=SHA if mix == "prep_units" else None))
    config_only = {k: v for k, v in fleet.items() if np.asarray(v).ndim == 0 or k == "events_cfg"}
    for u in range(U):
        stream = h.fleet_unit_to_stream(fleet, u)
        h.stream_checkpoint_check(stream, _stream_expect(fleet))     # what StreamDetector.load_state_dict runs first
        assert "units" not in stream and "prep_units_sha256" not in stream
        assert int(stream["chunk"]) == int(fleet["chunk"]) and int(stream["handed"]) == int(fleet["handed"])
        assert int(stream["recal_every"]) == int(fleet["recal_every"])
        if int(fleet["prep"]):
            p = int(fleet["pending"][u])
            assert int(stream["raw_pending"]) == p and stream["pending"].shape == (p, N)
        for sd_config in (fleet, config_only):
            unit = h.stream_to_fleet_unit(stream, sd_config)
            assert sorted(unit) == sorted(k for k in PER_UNIT if k in fleet)
            for k, got in unit.items():
                want = np.asarray(fleet[k])[u]
                if k == "pending_ticks":                             # the open group: the rest of the plane is no state
                    want = want[:int(fleet["pending"][u])]
                want = np.array(want)                                # (a contiguous copy; a 0-d entry stays 0-d)
                assert got.dtype == want.dtype and got.shape == want.shape, (k, got.dtype, got.shape)
                assert got.tobytes() == want.tobytes(), (u, k)      # NaN payloads of the ring's filler included
    with pytest.raises(ValueError, match=f"unit {U}: the file holds units 0 .. {U - 1}"):
        h.fleet_unit_to_stream(fleet, U)


def test_a_detectors_own_dict_without_recal_counts_becomes_a_unit_of_a_tick_calibrated_fleet():
    h = _harness()
    fleet = _fleet_sd("recal_tick")
    stream = h.fleet_unit_to_stream(fleet, 1)
    kept = int(stream["recal_kept"])
    assert kept == int(fleet["recal_kept"][1])
    del stream["recal_counts"]                                       # (a detector under calib="tick" keeps none)
    unit = h.stream_to_fleet_unit(stream, fleet)
    assert unit["recal_counts"].dtype == np.int32 and unit["recal_counts"].tolist() == [kept] * N
    sensor = _fleet_sd("recal_sensor")
    stream = h.fleet_unit_to_stream(sensor, 2)
    counts = sensor["recal_counts"][2]
    done = counts[counts >= int(sensor["recal_min"])]
    assert int(stream["recal_kept"]) == int(done.min()) and stream["recal_counts"].dtype == np.int64


def i64(v):
    return np.array(v, dtype=np.int64)


def test_every_hand_over_refusal_names_its_field():
    h = _harness()
    fleet = _fleet_sd("all")
    stream = h.fleet_unit_to_stream(fleet, 0)

    def refused(field, sd_stream=stream, **changes):
        with pytest.raises(ValueError, match="unit hand-over: " + field):
            h.stream_to_fleet_unit(sd_stream, _with(fleet, **changes))
    refused("n = 70, the fleet was built with n = 71", n=i64(71))
    refused("w = 5, the fleet was built with w = 6", w=i64(6))
    refused("top_m = 2, the fleet was built with top_m = 3", top_m=i64(3))
    refused("log = 6, the fleet was built with log = 7", log=i64(7))
    refused("with_gaps = 1, the fleet was built with with_gaps = 0", with_gaps=i64(0))
    refused("recal = 64, the fleet was built with recal = 128", recal=i64(128))
    refused("exclude_alarms = 1, the fleet was built with exclude_alarms = 0", exclude_alarms=i64(0))
    refused("recal_min = 16, the fleet was built with recal_min = 8", recal_min=i64(8))
    refused("calib = 'tick', the fleet was built with calib = 'sensor'", calib=np.array("sensor"))
    refused("wide = 0, the fleet was built with wide = 1 .the route is per launch", wide=i64(1))
    refused("prep = 1, the fleet was built with prep = 0", prep=i64(0))
    refused("prep_down = 4, the fleet was built with prep_down = 10", prep_down=i64(10))
    refused("abi = 23, the fleet has abi = 24", abi=i64(24))
    refused("state_bytes = 4096, the fleet has state_bytes = 4104", state_bytes=i64(4104))
    refused("model_sha256 differs", model_sha256=np.array("00" * 32))
    refused("events: the detector keeps an episode table, the fleet does not", events_cfg=None)
    refused("events.on = 2, the fleet was built with events.on = 5", events_cfg=np.array([5, 3, CAP, M], dtype=np.int64))
    refused("events.cap = 8, the fleet was built with events.cap = 16",
            events_cfg=np.array([2, 3, 16, M], dtype=np.int64))
    refused("recal_threshold = 1.25, the fleet was built with recal_threshold = None", recal_threshold=None)
    refused("recal_threshold = 1.25, the fleet was built with recal_threshold = 2.0",
            recal_threshold=np.array(2.0, dtype=np.float64))
    bare = h.fleet_unit_to_stream(_fleet_sd("plain"), 0)
    with pytest.raises(ValueError, match="unit hand-over: events: the detector keeps no episode table, the fleet does"):
        h.stream_to_fleet_unit(bare, _fleet_sd("events"))
    with pytest.raises(ValueError, match="stream checkpoint: format = 9"):
        h.stream_to_fleet_unit(_with(stream, format=i64(9)), fleet)
    with pytest.raises(ValueError, match="fleet checkpoint: key 'units' is missing: this is a single detector's"):
        h.fleet_unit_to_stream(stream, 0)
    # chunk and recal_every are the fleet's: a detector that ran in other cuts on another clock is taken
    h.stream_to_fleet_unit(_with(stream, chunk=i64(2), recal_every=i64(0), handed=i64(7)), fleet)
