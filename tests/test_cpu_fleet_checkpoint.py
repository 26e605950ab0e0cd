"""CPU suite of a fleet's checkpoint (harness.fleet_checkpoint_check, write_ / read_stream_checkpoint): pure host code on
hand-made dicts, so no device is needed."""
import os

import numpy as np
import pytest

U, N, W, M, LOG, R, DOWN, CAP = 3, 70, 5, 2, 6, 64, 4, 8
ABI, STATE_BYTES, CALIB_BYTES = 23, 4096, U * (8 * N * R + R)
FIELDS = ("on", "off", "cap", "m")


def _harness():
    from gdn_amd import harness
    return harness


def _sd(gaps=False, recal=0, calib="tick", events=False, prep=False, log=LOG):
    """A fleet checkpoint as StreamFleet.state_dict() lays it out, with numbers instead of a stream."""
    h = _harness()
    rng = np.random.default_rng(7)
    ints = {"format": h.FLEET_CHECKPOINT_FORMAT, "units": U, "abi": ABI, "state_bytes": STATE_BYTES,
            "calib_bytes": CALIB_BYTES if recal else 0, "n": N, "w": W, "chunk": 4, "top_m": M, "log": log,
            "with_gaps": int(gaps), "recal": recal, "exclude_alarms": 1, "recal_every": 48 if recal else 0,
            "recal_min": 16 if recal else 0, "wide": 0, "prep": int(prep), "prep_down": DOWN if prep else 0,
            "handed": 31, "raw_handed": 125 if prep else 0, "recals": 1 if recal else 0}
    sd = {k: np.array(v, dtype=np.int64) for k, v in ints.items()}
    sd["calib"], sd["model_sha256"] = np.array(calib), np.array("ab" * 32)
    sd["state"] = rng.integers(0, 255, (U, STATE_BYTES)).astype(np.uint8)
    sd["med_iqr"], sd["threshold"] = rng.random((U, N, 2)), rng.random((U,))
    sd["log_ticks"] = rng.integers(0, 99, (U, log)).astype(np.int64)
    sd["log_sensors"] = rng.integers(0, N, (U, log, M)).astype(np.int32)
    if gaps:
        sd["gaps"] = rng.integers(0, 9, (U, 2, N)).astype(np.int64)
    if recal:
        sd["ring_keys"] = rng.random((U, N, recal))
        sd["ring_keys"][1, 2, 3] = np.frombuffer(np.int64(-1).tobytes(), dtype=np.float64)[0]      # the filler: a NaN payload
        sd["ring_keep"] = rng.integers(0, 2, (U, recal)).astype(np.uint8)
        sd["recal_counts"] = rng.integers(0, recal, (U, N)).astype(np.int32)
        if calib == "tick":
            sd["recal_kept"] = rng.integers(0, recal, (U,)).astype(np.int32)
    if events:
        sd["events"] = rng.integers(0, 99, (U, h.events_bytes(M, CAP) // 8)).astype(np.int64)
        sd["clear"] = rng.random((U,))
        sd["events_cfg"] = np.array([2, 3, CAP, M], dtype=np.int64)
    if prep:
        sd["pending_ticks"] = rng.random((U, DOWN, N))
        sd["pending"] = np.array([1, 0, 3], dtype=np.int32)
    return sd


def _expect(sd, **kw):
    e = {"n": N, "w": W, "abi": ABI, "state_bytes": STATE_BYTES, "calib_bytes": int(sd["calib_bytes"]), "model": "ab" * 32,
         "prep_down": DOWN if int(sd["prep"]) else None, "prep_n": N if int(sd["prep"]) else None}
    e.update(kw)
    return e


ALL = dict(gaps=True, recal=R, events=True, prep=True)
CONFIGS = [dict(), dict(gaps=True), dict(recal=R), dict(gaps=True, recal=R, calib="sensor"), dict(events=True),
           dict(prep=True), ALL, dict(log=0)]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()) or "plain")
def test_a_hand_made_dict_passes_the_check_and_round_trips_through_the_file_bit_for_bit(cfg, tmp_path):
    h = _harness()
    sd = _sd(**cfg)
    h.fleet_checkpoint_check(sd, _expect(sd))
    h.fleet_checkpoint_check(sd, _expect(sd, units=U, events={"on": 2, "off": 3, "cap": CAP, "m": M}
                                         if cfg.get("events") else None))
    h.fleet_checkpoint_check(sd, _expect(sd, model=None))            # check_model=False
    path = str(tmp_path / "fleet.npz")
    h.write_stream_checkpoint(path, sd)
    assert os.listdir(tmp_path) == ["fleet.npz"]                     # exactly `path`, the temporary file is gone
    back = h.read_stream_checkpoint(path)
    assert sorted(back) == sorted(sd)
    for k, v in sd.items():
        assert back[k].dtype == np.asarray(v).dtype and back[k].shape == np.asarray(v).shape, k
        assert back[k].tobytes() == np.asarray(v).tobytes(), k       # NaN payloads of the ring's filler included
    h.fleet_checkpoint_check(back, _expect(sd))
    assert h.fleet_checkpoint_config(back)["units"] == U


def _refused(sd, field, **expect):
    with pytest.raises(ValueError, match="fleet checkpoint: .*" + field):
        _harness().fleet_checkpoint_check(sd, _expect(sd, **expect))


def _with(sd, **changes):
    out = dict(sd)
    for k, v in changes.items():
        if v is None:
            del out[k]
        else:
            out[k] = v
    return out


def i64(v):
    return np.array(v, dtype=np.int64)


def test_every_identity_refusal_names_its_field():
    sd = _sd(**ALL)
    _refused(_with(sd, format=i64(2)), "format = 2")
    _refused(_with(sd, format=None), "'format'")
    _refused(_with(sd, units=None), "'units' is missing: this is a single detector's checkpoint")
    _refused(_with(sd, units=i64(0)), "units = 0")
    _refused(sd, "units = 3, this fleet has units = 4", units=4)
    _refused(sd, "n = 70, the model has n = 71", n=71)
    _refused(sd, "w = 5, the model has w = 6", w=6)
    _refused(sd, "abi = 23", abi=24)
    _refused(sd, "state_bytes", state_bytes=STATE_BYTES + 8)
    _refused(sd, "calib_bytes", calib_bytes=CALIB_BYTES + 8)
    _refused(sd, "prep: the fleet was saved with", prep_down=None)
    _refused(_sd(), "prep: the fleet was saved without", prep_down=DOWN, prep_n=N)
    _refused(sd, "prep_down = 4, the prep given has down = 10", prep_down=10)
    _refused(sd, "prep: fitted on 69 sensors", prep_n=69)
    _refused(_with(_sd(), prep_down=i64(4)), "prep_down = 4 without a prep")
    _refused(_with(_sd(), raw_handed=i64(4)), "raw_handed = 4 without a prep")
    _refused(sd, "model_sha256", model="cd" * 32)
    _harness().fleet_checkpoint_check(sd, _expect(sd, model=None))   # check_model=False overrides it
    _refused(_with(sd, calib=np.array("median")), "calib = 'median'")
    _refused(sd, "events: the fleet was saved with", events=None)
    _refused(_sd(), "events: the fleet was saved without", events={"on": 1, "off": 1, "cap": CAP, "m": M})
    _refused(sd, "events.off = 3, this fleet was built with events.off = 1", events={"on": 2, "off": 1, "cap": CAP, "m": M})
    _refused(_with(sd, events_cfg=np.array([2, 3, CAP, M + 1], dtype=np.int64)), "events.m = 3, top_m = 2")
    _refused(_with(sd, events_cfg=np.array([0, 3, CAP, M], dtype=np.int64)), "events_cfg")


def test_missing_foreign_and_misshapen_keys_are_refused_by_name():
    sd = _sd(**ALL)
    for key in ("state", "med_iqr", "threshold", "log_ticks", "log_sensors", "gaps", "ring_keys", "ring_keep",
                "recal_counts", "recal_kept", "pending_ticks", "pending", "handed", "raw_handed", "recals", "chunk",
                "model_sha256", "calib", "abi"):
        _refused(_with(sd, **{key: None}), repr(key) + " is missing")
    for key in ("events", "clear", "events_cfg"):
        _refused(_with(sd, **{key: None}), "without the rest of events, events_cfg, clear")
    _refused(_with(sd, raw_pending=i64(0)), "'raw_pending' does not belong")
    _refused(_with(_sd(), gaps=np.zeros((U, 2, N), np.int64)), "'gaps' does not belong")
    _refused(_with(_sd(), pending=np.zeros((U,), np.int32)), "'pending' does not belong")
    _refused(_with(_sd(gaps=True, recal=R, calib="sensor"), recal_kept=np.zeros((U,), np.int32)), "'recal_kept' does not")
    wrong = {"state": np.zeros((U, STATE_BYTES), np.int8), "med_iqr": np.zeros((U, N, 2), np.float32),
             "threshold": np.zeros((1,)), "log_ticks": np.zeros((U, LOG + 1), np.int64),
             "log_sensors": np.zeros((U, LOG, M + 1), np.int32), "gaps": np.zeros((2, N), np.int64),
             "ring_keys": np.zeros((U, N, R + 1)), "ring_keep": np.zeros((U, R), np.int8),
             "recal_counts": np.zeros((U, N), np.int64), "recal_kept": np.zeros((U, 1), np.int32),
             "events": np.zeros((U, 3), np.int64), "clear": np.zeros((U,), np.float32),
             "pending_ticks": np.zeros((U, DOWN - 1, N)), "pending": np.zeros((U, 2), np.int32),
             "calib_kept": np.zeros((U,), np.int32), "calib_counts": np.zeros((U, N + 1), np.int32)}
    for key, value in wrong.items():
        _refused(_with(sd, **{key: value}), repr(key) + " must be")
    _refused(_with(sd, handed=np.array(3, dtype=np.int32)), "'handed' must be one int64")
    _refused(_with(sd, model_sha256=i64(3)), "'model_sha256' must be one string")
    # the optional keys fit
    _harness().fleet_checkpoint_check(_with(sd, calib_kept=np.zeros((U,), np.int64),
                                            calib_counts=np.zeros((U, N), np.int32)), _expect(sd))


def test_a_pending_count_outside_an_open_group_and_a_negative_counter_are_refused():
    sd = _sd(**ALL)
    for bad in ([1, DOWN, 0], [-1, 0, 0], [0, 0, 99]):
        _refused(_with(sd, pending=np.array(bad, dtype=np.int32)), "pending = .* outside an open group of prep_down = 4")
    _harness().fleet_checkpoint_check(_with(sd, pending=np.array([DOWN - 1, 0, 0], dtype=np.int32)), _expect(sd))
    for key in ("handed", "raw_handed", "recals", "recal_every", "recal_min"):
        _refused(_with(sd, **{key: i64(-1)}), key + " = -1 is negative")
    _refused(_with(sd, recal_kept=np.array([1, -1, 0], dtype=np.int32)), "recal_kept holds a negative count")
    _refused(_with(sd, recal_counts=np.full((U, N), -2, dtype=np.int32)), "recal_counts holds a negative count")
    _refused(_with(sd, calib_kept=np.array([1, -1, 0], dtype=np.int64)), "calib_kept holds a negative count")


def _detector_sd():
    """A single detector's checkpoint for the same model, hand-made."""
    h = _harness()
    ints = dict.fromkeys(h._CKPT_INTS, 0)
    ints.update({"format": h.STREAM_CHECKPOINT_FORMAT, "abi": ABI, "state_bytes": STATE_BYTES, "n": N, "w": W,
                 "chunk": 4, "top_m": M, "log": LOG, "calib_kept": -1})
    sd = {k: np.array(v, dtype=np.int64) for k, v in ints.items()}
    sd["calib"], sd["model_sha256"] = np.array("tick"), np.array("ab" * 32)
    sd["state"], sd["med_iqr"] = np.zeros((STATE_BYTES,), np.uint8), np.zeros((N, 2))
    sd["threshold"] = np.ones((1,))
    sd["log_ticks"], sd["log_sensors"] = np.zeros((LOG,), np.int64), np.zeros((LOG, M), np.int32)
    return sd


def test_a_detector_file_is_refused_by_the_fleet_checker_and_a_fleet_file_by_the_detectors():
    h = _harness()
    det, expect = _detector_sd(), _expect(_sd())
    h.stream_checkpoint_check(det, expect)                           # (it IS a detector's checkpoint)
    with pytest.raises(ValueError, match="fleet checkpoint: key 'units' is missing: this is a single detector's"):
        h.fleet_checkpoint_check(det, expect)
    for cfg in CONFIGS:
        fleet = _sd(**cfg)
        with pytest.raises(ValueError, match="stream checkpoint: "):
            h.stream_checkpoint_check(fleet, _expect(fleet))
    # even a fleet dict dressed with the detector's scalar keys stays foreign to it: `units` is no key of a detector's
    dressed = dict(_sd(), recal_kept=i64(0), calib_kept=i64(-1), raw_pending=i64(0))
    with pytest.raises(ValueError, match="stream checkpoint: key '(units|raw_handed)' does not belong"):
        h.stream_checkpoint_check(dressed, _expect(_sd()))


def test_a_half_written_save_leaves_the_previous_file_loadable(tmp_path, monkeypatch):
    h = _harness()
    path = str(tmp_path / "fleet.npz")
    first = _sd(**ALL)
    h.write_stream_checkpoint(path, first)
    second = _with(first, handed=i64(99))
    real = np.savez

    def dies_half_way(f, **arrays):
        real(f, **{k: arrays[k] for k in list(arrays)[:5]})
        raise OSError("the disk is full")
    monkeypatch.setattr(np, "savez", dies_half_way)
    with pytest.raises(OSError, match="disk is full"):
        h.write_stream_checkpoint(path, second)
    monkeypatch.undo()
    assert os.listdir(tmp_path) == ["fleet.npz"]
    back = h.read_stream_checkpoint(path)
    h.fleet_checkpoint_check(back, _expect(first))
    assert int(back["handed"]) == 31 and all(back[k].tobytes() == np.asarray(first[k]).tobytes() for k in first)
    h.write_stream_checkpoint(path, second)
    assert int(h.read_stream_checkpoint(path)["handed"]) == 99
