"""CPU suite of the streaming detector's rolling calibration: the float64 yardstick of the GPU tests
(tests/_stream_recal_ref.py) against a brute-force restatement and against oracle.score_oracle, the table switch of
the chunked scoring reference, the three additive entry points in header, bindings and library, and the refusals that
harness.StreamDetector decides on host facts (no device is needed)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _stream_recal_ref as rref
import _stream_ref as ref
from conftest import ROOT, load_golden

GDN_ERR_ARG, GDN_ERR_UNSUPPORTED = -1, -3
FAKE = 4096          # a non-null, 16-byte aligned address that is never dereferenced on the host
NEW = ["gdn_stream_calib_bytes", "gdn_stream_calib_write", "gdn_stream_calib_write_gaps"]
CASES = ["score_T1000_N27", "score_T65_N7"]
MIN_TICKS = 48       # `recal_min` of these tests: T65 has 65 ticks in all, about three of them alarmed


# ------------------------------------------------------------------------------------------- the yardstick
def _fixture(case):
    """(pred, gt, alarm [T]): the alarmed ticks are those whose anomaly score (the fixture's own scores: the
    oracle's, max over sensors) lies above its 95th percentile — about 5 % of the ticks."""
    from oracle import score_oracle
    data, _ = load_golden(case)
    pred, gt = data["pred"], data["gt"]
    anomaly = score_oracle.anomaly_score(score_oracle.full_err_scores(pred, gt))
    alarm = (anomaly > np.percentile(anomaly, 95)).astype(np.int32)
    assert 0 < alarm.sum() <= 0.06 * len(alarm) + 1
    return pred, gt, alarm


@pytest.mark.parametrize("exclude", [True, False], ids=["exclude_alarms", "keep_alarms"])
@pytest.mark.parametrize("R", [64, 100])
@pytest.mark.parametrize("case", CASES)
def test_the_ring_is_the_last_R_ticks_without_the_alarmed_however_the_stream_is_cut(case, R, exclude):
    from oracle import score_oracle
    pred, gt, alarm = _fixture(case)
    T, n = pred.shape
    want_keys, want_keep = rref.brute_force(pred, gt, alarm, R, exclude_alarms=exclude)
    last = np.arange(max(0, T - R), T)
    kept_rows = last[alarm[last] == 0] if exclude else last
    assert MIN_TICKS <= len(kept_rows) == int(want_keep.sum())               # enough stays kept to recalibrate
    assert exclude == (len(kept_rows) < len(last))                           # ... and an alarmed tick is among the last R
    want_table = np.array([score_oracle.err_median_and_iqr(pred[kept_rows, i], gt[kept_rows, i]) for i in range(n)])
    for chunk in (1, 3, 37, 64):
        ring = rref.CalibRing(n, R, exclude_alarms=exclude, min_ticks=MIN_TICKS)
        for s in range(0, T, chunk):
            ring.push(pred[s:s + chunk], gt[s:s + chunk], alarm[s:s + chunk])
        assert ring.ticks == T
        np.testing.assert_array_equal(ring.keep, want_keep, err_msg=str(chunk))
        np.testing.assert_array_equal(rref.bits(ring.keys), rref.bits(want_keys), err_msg=str(chunk))
        # a slot that is not kept holds the filler in every sensor; a kept one holds no filler
        filler = rref.bits(ring.keys) == rref.FILLER_BITS
        assert filler[:, ring.keep == 0].all() and not filler[:, ring.keep != 0].any()
        np.testing.assert_array_equal(ring.table(), want_table, err_msg=str(chunk))
        table = np.zeros((n, 2))
        assert ring.recalibrate(table) == len(kept_rows)
        np.testing.assert_array_equal(table, want_table)


def test_too_few_kept_ticks_write_nothing_and_a_dropped_tick_clears_its_slot():
    pred, gt, _alarm = _fixture("score_T65_N7")
    n = pred.shape[1]
    ring = rref.CalibRing(n, 64)                                             # min_ticks = 64
    ring.push(pred[:63], gt[:63], np.zeros(63))
    table = np.full((n, 2), 7.0)
    assert ring.recalibrate(table) == 0 and (table == 7.0).all()
    ring.push(pred[63:64], gt[63:64], np.zeros(1))
    assert ring.recalibrate(table) == 64 and not (table == 7.0).any()
    # tick 64 returns to slot 0; alarmed, it clears what tick 0 left there
    ring.push(pred[64:65], gt[64:65], np.ones(1))
    assert ring.keep[0] == 0 and (rref.bits(ring.keys)[:, 0] == rref.FILLER_BITS).all() and ring.total() == 63
    # a tick with a missing reading in ANY sensor is not kept, whatever its alarm flag
    ring = rref.CalibRing(n, 64, exclude_alarms=False)
    valid = np.ones((3, n), dtype=bool)
    valid[1, n - 1] = False
    ring.push(pred[:3], gt[:3], np.ones(3), valid)
    assert ring.keep[:4].tolist() == [1, 0, 1, 0]
    want, _keep = rref.brute_force(pred[:3], gt[:3], np.ones(3), 64, exclude_alarms=False, valid=valid)
    np.testing.assert_array_equal(rref.bits(ring.keys), rref.bits(want))


def test_seeding_fills_the_ring_from_the_back_and_the_stream_overwrites_the_oldest_last():
    pred, gt, _alarm = _fixture("score_T1000_N27")
    n = pred.shape[1]
    for R, t in ((100, 40), (64, 300)):
        ring = rref.CalibRing(n, R)
        s = ring.seed(pred[:t], gt[:t])
        assert s == min(R, t) and ring.keep.tolist() == [0] * (R - s) + [1] * s
        np.testing.assert_array_equal(ring.keys[:, R - s:], rref.keys_of(pred[t - s:t], gt[t - s:t]).T)
        from oracle import score_oracle
        want = np.array([score_oracle.err_median_and_iqr(pred[t - s:t, i], gt[t - s:t, i]) for i in range(n)])
        np.testing.assert_array_equal(ring.table(), want)
    # R = 64 seeded full: five stream ticks replace the five OLDEST seeded ticks (slots 0 .. 4)
    ring.push(pred[500:505], gt[500:505], np.zeros(5))
    np.testing.assert_array_equal(ring.keys[:, :5], rref.keys_of(pred[500:505], gt[500:505]).T)
    np.testing.assert_array_equal(ring.keys[:, 5:], rref.keys_of(pred[241:300], gt[241:300]).T)


@pytest.mark.parametrize("case", CASES)
def test_after_a_table_switch_the_scores_do_not_depend_on_the_push_size(case):
    """A switch falls between two pushes.  Said per tick: tick t is normalised with the table in force at t, and the
    4-tap mean takes its three predecessors as they were normalised — the carry does exactly that."""
    from oracle import score_oracle
    data, _ = load_golden(case)
    pred, gt = data["pred"], data["gt"]
    T, n = pred.shape
    delta = rref.keys_of(pred, gt)
    first = np.array([score_oracle.err_median_and_iqr(pred[:, i], gt[:, i]) for i in range(n)])
    s = 320 if T > 320 else 40               # T1000: a push boundary of 1, 5 and 64; T65: of 1 and 5, 64 pushes 40 + 25
    second = np.array([score_oracle.err_median_and_iqr(pred[:s, i], gt[:s, i]) for i in range(n)]) * [1.5, 0.5] + [0.01, 0.0]
    # per tick, no chunking: the definition
    a = np.where(np.arange(T)[:, None] < s, (delta - first[:, 0]) / (np.abs(first[:, 1]) + ref.SCORE_EPS),
                 (delta - second[:, 0]) / (np.abs(second[:, 1]) + ref.SCORE_EPS))
    want = np.zeros((T, n))
    for t in range(3, T):
        want[t] = (((a[t - 3] + a[t - 2]) + a[t - 1]) + a[t]) / 4.0
    m = min(3, n)
    thr = float(np.percentile(want.max(axis=1), 90))
    outs = {}
    for chunk in (1, 5, 64):
        sm, vals, idx, flags, state = rref.run_switched(delta, [(0, first), (s, second)], chunk, m=m, threshold=thr)
        np.testing.assert_array_equal(sm, want, err_msg=str(chunk))
        outs[chunk] = (sm, vals, idx, flags, state.carry, np.array([t for t, _ in state.log]))
    assert outs[1][3].any() and not outs[1][3].all()
    for chunk, got in outs.items():
        for u, v in zip(got, outs[1]):
            np.testing.assert_array_equal(u, v, err_msg=str(chunk))
    # without a switch the wrapper IS _stream_ref.run_chunked
    plain = ref.run_chunked(delta, first, 5, m=m, threshold=thr)
    same = rref.run_switched(delta, [(0, first)], 5, m=m, threshold=thr)
    np.testing.assert_array_equal(same[0], plain[0].T)
    for u, v in zip(same[1:4], plain[1:4]):
        np.testing.assert_array_equal(u, v)


# ------------------------------------------------------------------------------------------- library and bindings
def _lib():
    from gdn_amd import _lib as binding
    return binding.load()


def test_the_three_symbols_are_declared_bound_and_exported_and_the_abi_stays():
    from gdn_amd import _lib as binding
    header = open(os.path.join(ROOT, "include", "gdn_hip.h")).read()
    declared = dict((name, ret) for ret, name in re.findall(r"^(int|long long)\s+(gdn_\w+)\s*\(", header, flags=re.M))
    lib = binding.load()
    for name in NEW:
        want = "long long" if name.endswith("_bytes") else "int"
        assert declared.get(name) == want and name in binding.SIGNATURES, name
        fn = getattr(lib, name)                      # AttributeError: the symbol is missing
        assert fn.argtypes == binding.SIGNATURES[name]
        assert fn.restype is (ctypes.c_longlong if name.endswith("_bytes") else ctypes.c_int)
        params = re.search(r"^(?:int|long long)\s+" + name + r"\s*\(([^)]*)\)\s*;", header, flags=re.M).group(1)
        assert len(params.split(",")) == len(binding.SIGNATURES[name]), name
    assert "#define GDN_ABI_VERSION 23" in header and binding.ABI_VERSION == 23 and lib.gdn_abi_version() == 23
    p, i = ctypes.c_void_p, ctypes.c_int
    # (state, pred, chunk, alarm, c, count, n, R, exclude_alarms, ring_keys, ring_keep, stream)
    assert binding.SIGNATURES["gdn_stream_calib_write"] == [p, p, p, p, i, i, i, i, i, p, p, p]
    # ... with `valid` after the alarm flags
    assert binding.SIGNATURES["gdn_stream_calib_write_gaps"] == [p, p, p, p, p, i, i, i, i, i, p, p, p]
    from gdn_amd import harness, ops
    assert callable(ops.stream_calib_ring)
    assert "valid" in inspect.signature(ops.stream_calib_write).parameters
    assert not hasattr(ops, "stream_calib_write_gaps")
    prm = inspect.signature(harness.StreamDetector.__init__).parameters
    assert (prm["recal"].default, prm["exclude_alarms"].default, prm["recal_every"].default, prm["recal_min"].default) \
        == (0, True, 0, None)
    assert callable(harness.StreamDetector.recalibrate) and callable(harness.StreamDetector.calibration)


@pytest.mark.parametrize("n,R", [(1, 64), (5, 64), (5, 100), (27, 101), (127, 32768), (4096, 65536), (256, 1 << 20)])
def test_calib_bytes_inside_the_envelope(n, R):
    want = (8 * n * R + R + 7) // 8 * 8
    assert _lib().gdn_stream_calib_bytes(n, R) == want and want % 8 == 0


@pytest.mark.parametrize("n,R", [(0, 64), (-1, 64), (4097, 64), (5, 63), (5, 0), (5, -64), (5, (1 << 20) + 1),
                                 (257, 1 << 20), (4096, 65537)])
def test_calib_bytes_is_zero_outside_the_envelope(n, R):
    assert _lib().gdn_stream_calib_bytes(n, R) == 0


def _write(gaps=False, c=16, count=16, n=27, R=64, exclude=1, **kw):
    a = dict(state=FAKE, pred=FAKE, chunk=FAKE, alarm=FAKE, valid=FAKE, keys=FAKE, keep=FAKE)
    a.update(kw)
    if gaps:
        return _lib().gdn_stream_calib_write_gaps(a["state"], a["pred"], a["chunk"], a["alarm"], a["valid"], c, count,
                                                  n, R, exclude, a["keys"], a["keep"], None)
    return _lib().gdn_stream_calib_write(a["state"], a["pred"], a["chunk"], a["alarm"], c, count, n, R, exclude,
                                         a["keys"], a["keep"], None)


@pytest.mark.parametrize("gaps", [False, True], ids=["plain", "gaps"])
def test_every_refusal_of_the_ring_writer_is_decided_before_any_launch(gaps):
    for null in ("state", "pred", "chunk", "alarm", "keys", "keep") + (("valid",) if gaps else ()):
        assert _write(gaps, **{null: None}) == GDN_ERR_ARG, null
    for count, c in ((0, 16), (17, 16), (-1, 16), (1, 0)):
        assert _write(gaps, c=c, count=count) == GDN_ERR_ARG, (count, c)
    assert _write(gaps, c=65, count=1, R=64) == GDN_ERR_ARG                  # two rows of a push would share a slot
    for shape in (dict(n=0), dict(n=4097), dict(R=63), dict(R=(1 << 20) + 1), dict(n=257, R=1 << 20)):
        assert _write(gaps, **shape) == GDN_ERR_UNSUPPORTED, shape


# ------------------------------------------------------------------------------------------- the detector's refusals
def _host_detector(**kw):
    """Host tensors throughout: whatever is refused here was refused on host facts, before any device work (the
    first device check of the constructor raises GdnHipError, not ValueError)."""
    from gdn_amd import GDN, harness
    n, w = 9, 5
    model = GDN([torch.zeros((2, 1), dtype=torch.long)], n, dim=16, input_dim=w, topk=3)
    return harness.StreamDetector(model, torch.zeros((n, 2), dtype=torch.float64), 1.0, torch.zeros((n, w)),
                                  kw.pop("chunk", 16), **kw)


def test_the_detector_refuses_on_host_facts_and_names_the_argument():
    from gdn_amd import _lib as binding, harness
    with pytest.raises(ValueError, match=r"recal = 15"):
        _host_detector(recal=15)                                             # recal < chunk
    with pytest.raises(ValueError, match=r"recal = 100.*chunk = 128"):
        _host_detector(chunk=128, recal=100)
    with pytest.raises(ValueError, match=r"recal = 32"):
        _host_detector(chunk=16, recal=32)                                   # R < 64: outside gdn_stream_calib_bytes
    with pytest.raises(ValueError, match=r"recal = 2097152"):
        _host_detector(recal=1 << 21)
    with pytest.raises(ValueError, match=r"recal_every = 50"):
        _host_detector(recal_every=50)                                       # no ring to recalibrate from
    with pytest.raises(ValueError, match=r"recal_min = 65"):
        _host_detector(recal=64, recal_min=65)
    with pytest.raises(ValueError, match=r"recal_min = 10"):
        _host_detector(recal_min=10)
    # a well-formed request passes every host check and only then meets the device check
    with pytest.raises(binding.GdnHipError, match="HIP device"):
        _host_detector(recal=64, recal_every=50)
    det = object.__new__(harness.StreamDetector)
    det.recal = 0
    with pytest.raises(ValueError, match=r"recalibrate\(\).*recal=0"):
        det.recalibrate()


def test_the_command_line_knows_the_two_flags():
    from gdn_amd import main as cli
    args = cli.build_parser().parse_args(["-stream", "16", "-stream_recal", "4096", "-stream_recal_every", "500"])
    assert (args.stream, args.stream_recal, args.stream_recal_every) == (16, 4096, 500)
    args = cli.build_parser().parse_args([])
    assert (args.stream_recal, args.stream_recal_every) == (0, 0)


# ------------------------------------------------------------------------------------------- the staged ring write
@pytest.mark.parametrize("n", rref.STAGE_N)
@pytest.mark.parametrize("mode", ["plain", "gaps", "sensor"])
def test_the_staged_ring_write_cases_meet_a_kept_tick_a_filler_and_the_rings_end(mode, n):
    """The reference alone, on the inputs of the GPU stage test (test_gpu_stream_recal.py): every (mode, n) meets a
    kept tick and a filler, the inputs hold a complete and a broken tick, an alarm on the first row and none on the
    last, exactly `count` slots leave the sentinel, and the third staged counter wraps the ring's end inside a push."""
    met_kept = met_filler = wrapped = False
    sentinel = rref.bits(np.array(rref.SENTINEL_KEY))
    for count, R in rref.STAGE_COUNT_R:
        pred, chunk, alarm, valid = rref.stage_inputs(n, count)
        assert alarm[-1] == 0 and valid[-1].all()
        assert count == 1 or (alarm[0] != 0 and not valid[0].all())
        assert rref.stage_ticks(count, R)[:2] == (0, R - 1)
        for ticks in rref.stage_ticks(count, R):
            for exclude in (True, False):
                keys, keep = rref.stage_ring(mode, n, R, ticks, exclude, pred, chunk, alarm, valid)
                written = keep != rref.SENTINEL_KEEP
                assert int(written.sum()) == count and set(keep[written]) <= {0, 1}
                assert ((keys != sentinel).all(axis=0) == written).all()
                slots = (ticks + np.arange(count)) % R
                assert written[slots].all()
                wrapped |= count > 1 and slots[0] > slots[-1]
                # a slot that is not kept holds the filler in every sensor
                assert (keys[:, keep == 0] == rref.FILLER_BITS).all()
                if mode != "sensor":
                    assert not (keys[:, keep == 1] == rref.FILLER_BITS).any()
                met_kept |= bool((keep == 1).any())
                met_filler |= bool((keys == rref.FILLER_BITS).any())
    assert met_kept and met_filler and wrapped
