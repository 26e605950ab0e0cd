"""CPU suite of the streaming detector's checkpoint: the file format and every refusal, on hand-built
dicts through the pure helpers harness.stream_checkpoint_check / model_fingerprint / write_stream_checkpoint /
read_stream_checkpoint, and the command line's flag checks.  No device."""
import copy
import os

import numpy as np
import pytest
import torch

N, W, M, LOG, R, DOWN = 5, 4, 3, 8, 64, 4


def _state_bytes(n, w):
    return (32 + 24 * n + 4 * n * w + 7) // 8 * 8           # include/gdn_hip.h "streaming detector": the state's layout


def _calib_bytes(n, r):
    return (8 * n * r + r + 7) // 8 * 8                     # ... "Rolling calibration": 8 n R + R, rounded up to 8


def _model(seed=0):
    from gdn_amd import GDN
    torch.manual_seed(seed)
    return GDN([torch.zeros((2, 1), dtype=torch.long)], N, dim=16, input_dim=W, topk=3).eval()


def _dict(model_hash="0" * 64, gaps=True, recal=R, prep=True, pending=3, counts=True):
    """A checkpoint of a gaps=True, recal=R, calib="sensor", prep= detector as state_dict() lays it out, from a seeded
    generator: every optional array is present."""
    g = np.random.default_rng(7)
    ints = {"format": 1, "abi": 23, "state_bytes": _state_bytes(N, W), "calib_bytes": _calib_bytes(N, recal) if recal else 0,
            "n": N, "w": W, "chunk": 8, "top_m": M, "log": LOG, "with_gaps": int(gaps), "recal": recal,
            "exclude_alarms": 1, "recal_every": 48 if recal else 0, "recal_min": 16 if recal else 0, "wide": 0,
            "prep": int(prep), "prep_down": DOWN if prep else 0, "handed": 59, "recals": 1, "recal_kept": 40,
            "calib_kept": -1, "raw_pending": pending if prep else 0}
    sd = {k: np.array(v, dtype=np.int64) for k, v in ints.items()}
    sd["calib"] = np.array("sensor" if gaps and recal else "tick")
    sd["model_sha256"] = np.array(model_hash)
    sd["state"] = g.integers(0, 256, size=_state_bytes(N, W), dtype=np.uint8)
    sd["med_iqr"] = g.random((N, 2))
    sd["threshold"] = g.random((1,))
    sd["log_ticks"] = g.integers(0, 1000, size=LOG, dtype=np.int64)
    sd["log_sensors"] = g.integers(0, N, size=(LOG, M), dtype=np.int32)
    if gaps:
        sd["gaps"] = g.integers(0, 50, size=(2, N), dtype=np.int64)
    if recal:
        keys = g.random((N, recal))
        keys.view(np.int64)[:, ::7] = -1                    # the filler: a NaN whose payload must survive the file
        sd["ring_keys"], sd["ring_keep"] = keys, g.integers(0, 2, size=recal, dtype=np.uint8)
    if prep:
        sd["pending"] = g.random((pending, N))
    if counts:
        sd["calib_counts"] = g.integers(0, 200, size=N, dtype=np.int32)
        sd["recal_counts"] = g.integers(0, 64, size=N, dtype=np.int64)
    return sd


def _expect(model_hash="0" * 64, recal=R, down=DOWN):
    return {"n": N, "w": W, "abi": 23, "state_bytes": _state_bytes(N, W),
            "calib_bytes": _calib_bytes(N, recal) if recal else 0, "model": model_hash, "prep_down": down, "prep_n": N}


def test_the_hand_built_sizes_are_the_librarys_and_a_valid_dict_passes():
    from gdn_amd import _lib, harness
    lib = _lib.load()
    assert lib.gdn_abi_version() == 23 == _lib.ABI_VERSION
    assert lib.gdn_stream_state_bytes(N, W) == _state_bytes(N, W) and lib.gdn_stream_state_bytes(70, 5) == _state_bytes(70, 5)
    assert lib.gdn_stream_calib_bytes(N, R) == _calib_bytes(N, R) and lib.gdn_stream_calib_bytes(70, 100) == _calib_bytes(70, 100)
    harness.stream_checkpoint_check(_dict(), _expect())
    harness.stream_checkpoint_check(_dict(counts=False), _expect())                      # the two optional arrays
    harness.stream_checkpoint_check(_dict(gaps=False, recal=0, prep=False), _expect(recal=0, down=None))
    harness.stream_checkpoint_check(_dict(model_hash="f" * 64), dict(_expect(), model=None))     # check_model=False
    cfg = harness.stream_checkpoint_config(_dict())
    assert cfg == {"n": N, "w": W, "chunk": 8, "top_m": M, "log": LOG, "with_gaps": 1, "recal": R, "exclude_alarms": 1,
                   "recal_every": 48, "recal_min": 16, "calib": "sensor", "wide": 0, "prep": 1, "prep_down": DOWN}


def test_a_round_trip_through_the_file_keeps_every_dtype_shape_and_byte(tmp_path):
    from gdn_amd import harness
    sd = _dict()
    path = str(tmp_path / "det.ckpt")
    harness.write_stream_checkpoint(path, sd)
    assert sorted(os.listdir(tmp_path)) == ["det.ckpt"]     # exactly `path`: no suffix appended, no temporary left
    with np.load(path, allow_pickle=False) as z:            # no Python objects in it
        assert sorted(z.files) == sorted(sd)
    back = harness.read_stream_checkpoint(path)
    assert sorted(back) == sorted(sd)
    for k, a in sd.items():
        assert back[k].dtype == a.dtype and back[k].shape == a.shape, k
        assert back[k].tobytes() == a.tobytes(), k
    assert int((back["ring_keys"].view(np.int64) == -1).sum()) == N * len(range(0, R, 7))
    harness.stream_checkpoint_check(back, _expect())


def _drop(key):
    def f(sd, ex):
        del sd[key]
    return f


def _set(key, value):
    def f(sd, ex):
        sd[key] = value
    return f


def _ring_of_another_r(sd, ex):
    sd["ring_keys"], sd["ring_keep"] = np.zeros((N, R + 1)), np.zeros((R + 1,), np.uint8)


def _no_prep_given(sd, ex):
    ex["prep_down"] = None


def _prep_given_to_a_plain_file(sd, ex):
    for k in ("prep", "prep_down", "raw_pending"):
        sd[k] = np.array(0, dtype=np.int64)
    del sd["pending"]


REFUSALS = {
    "a_dropped_array": (_drop("med_iqr"), "med_iqr"),
    "a_dropped_counter": (_drop("handed"), "handed"),
    "a_dropped_ring": (_drop("ring_keep"), "ring_keep"),
    "a_ring_of_the_wrong_r": (_ring_of_another_r, "ring_keys"),
    "a_float32_table": (_set("med_iqr", np.zeros((N, 2), np.float32)), "med_iqr"),
    "a_truncated_state": (_set("state", np.zeros((_state_bytes(N, W) - 8,), np.uint8)), "state"),
    "an_abi_one_higher": (_set("abi", np.array(24, dtype=np.int64)), "abi"),
    "another_state_size": (_set("state_bytes", np.array(_state_bytes(N, W) + 8, dtype=np.int64)), "state_bytes"),
    "another_ring_size": (_set("calib_bytes", np.array(_calib_bytes(N, R) + 8, dtype=np.int64)), "calib_bytes"),
    "an_unknown_format": (_set("format", np.array(2, dtype=np.int64)), "format"),
    "another_n": (_set("n", np.array(N + 1, dtype=np.int64)), "n = "),
    "another_w": (_set("w", np.array(W + 1, dtype=np.int64)), "w = "),
    "a_prep_missing": (_no_prep_given, "prep"),
    "a_prep_against_the_files_word": (_prep_given_to_a_plain_file, "prep"),
    "a_prep_of_another_down": (_set("prep_down", np.array(DOWN + 1, dtype=np.int64)), "prep_down"),
    "a_pending_plane_of_another_length": (_set("pending", np.zeros((2, N))), "pending"),
    "a_counter_that_is_no_int64": (_set("recals", np.array(1, dtype=np.int32)), "recals"),
    "a_foreign_key": (_set("weights", np.zeros((3,))), "weights"),
    "a_pickled_looking_calib": (_set("calib", np.array(3, dtype=np.int64)), "calib"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_every_refusal_is_a_value_error_that_names_its_field(case):
    from gdn_amd import harness
    change, field = REFUSALS[case]
    sd, ex = _dict(), _expect()
    change(sd, ex)
    with pytest.raises(ValueError, match="stream checkpoint.*" + field):
        harness.stream_checkpoint_check(sd, ex)


def test_a_prep_fitted_on_other_sensors_is_refused():
    from gdn_amd import harness
    with pytest.raises(ValueError, match="prep"):
        harness.stream_checkpoint_check(_dict(), dict(_expect(), prep_n=N + 1))


def test_the_fingerprint_follows_the_weights_and_one_ulp_is_refused_by_name():
    from gdn_amd import harness
    model = _model()
    with torch.no_grad():
        model.gnn_layers[0].bn.running_mean.copy_(torch.linspace(-0.1, 0.1, 16))
    want = harness.model_fingerprint(model)
    assert len(want) == 64 and int(want, 16) >= 0
    fresh = _model(seed=1)
    assert harness.model_fingerprint(fresh) != want
    fresh.load_state_dict(copy.deepcopy(model.state_dict()))
    assert harness.model_fingerprint(fresh) == want
    harness.stream_checkpoint_check(_dict(model_hash=want), _expect(model_hash=harness.model_fingerprint(fresh)))
    with torch.no_grad():                                   # one weight, one ulp
        weight = fresh.embedding.weight
        weight[2, 3] = torch.nextafter(weight[2, 3], torch.tensor(float("inf")))
    moved = harness.model_fingerprint(fresh)
    assert moved != want
    with pytest.raises(ValueError, match="model_sha256.*check_model"):
        harness.stream_checkpoint_check(_dict(model_hash=want), _expect(model_hash=moved))
    fresh.load_state_dict(copy.deepcopy(model.state_dict()))
    with torch.no_grad():
        fresh.gnn_layers[0].bn.running_mean[0] += 0.5
    assert harness.model_fingerprint(fresh) != want         # a BatchNorm running statistic is part of the scores


def test_a_save_that_fails_half_way_leaves_the_old_file_loadable(tmp_path, monkeypatch):
    from gdn_amd import harness
    path = str(tmp_path / "det.npz")
    old = _dict()
    harness.write_stream_checkpoint(path, old)
    seen = []

    def dies(file, *args, **kw):
        seen.append(os.path.exists(path + ".tmp"))          # the temporary file is beside the checkpoint by now
        file.write(b"PK\x03\x04 half a zip")
        raise OSError("disk full")
    monkeypatch.setattr(np, "savez", dies)
    new = _dict()
    new["handed"] = np.array(9999, dtype=np.int64)
    with pytest.raises(OSError, match="disk full"):
        harness.write_stream_checkpoint(path, new)
    monkeypatch.undo()
    assert seen == [True] and sorted(os.listdir(tmp_path)) == ["det.npz"]
    back = harness.read_stream_checkpoint(path)
    harness.stream_checkpoint_check(back, _expect())
    assert int(back["handed"]) == 59 and all(back[k].tobytes() == old[k].tobytes() for k in old)


def test_the_save_and_resume_flags_need_a_stream():
    from gdn_amd import main as cli
    with pytest.raises(ValueError, match="-stream_save needs -stream"):
        cli.check_stream_checkpoint(True, False, False)
    with pytest.raises(ValueError, match="-stream_resume needs -stream"):
        cli.check_stream_checkpoint(False, True, False)
    cli.check_stream_checkpoint(True, True, True)
    cli.check_stream_checkpoint(False, False, False)
    with pytest.raises(ValueError, match="-stream_save needs -stream"):
        cli.from_args(["-dataset", "msl", "-stream_save", "det.npz"])
    with pytest.raises(ValueError, match="-stream_resume needs -stream"):
        cli.from_args(["-dataset", "msl", "-stream_resume", "det.npz"])
    args = cli.build_parser().parse_args(["-stream", "16", "-stream_save", "a.npz", "-stream_resume", "b.npz"])
    assert (args.stream_save, args.stream_resume) == ("a.npz", "b.npz")
