"""CPU suite of the streaming detector's missing readings: the three additive entry points
(gdn_stream_fill / _score_gaps / _advance_gaps) in header, bindings and library, their host-side refusals (decided
before any launch: no device is needed), and the float64 yardstick of the GPU tests (tests/_stream_gaps_ref.py):
all-valid it IS tests/_stream_ref.py, and its results do not depend on how a stream is cut into pushes."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _stream_gaps_ref as gref
import _stream_ref as ref
from conftest import ROOT, load_golden

GDN_ERR_ARG, GDN_ERR_UNSUPPORTED = -1, -3
FAKE = 4096          # a non-null, 16-byte aligned address that is never dereferenced on the host
NEW = ["gdn_stream_fill", "gdn_stream_score_gaps", "gdn_stream_advance_gaps"]


def _lib():
    from gdn_amd import _lib as binding
    return binding.load()


def test_the_three_symbols_are_declared_bound_and_exported_and_the_abi_stays():
    from gdn_amd import _lib as binding
    header = open(os.path.join(ROOT, "include", "gdn_hip.h")).read()
    declared = dict((name, ret) for ret, name in re.findall(r"^(int|long long)\s+(gdn_\w+)\s*\(", header, flags=re.M))
    lib = binding.load()
    for name in NEW:
        assert declared.get(name) == "int" and name in binding.SIGNATURES
        fn = getattr(lib, name)                      # AttributeError: the symbol is missing
        assert fn.argtypes == binding.SIGNATURES[name] and fn.restype is ctypes.c_int
        params = re.search(name + r"\s*\(([^)]*)\)\s*;", header).group(1)
        assert len(params.split(",")) == len(binding.SIGNATURES[name]), name
    assert "#define GDN_ABI_VERSION 23" in header and binding.ABI_VERSION == 23 and lib.gdn_abi_version() == 23
    p, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    # (state, raw_chunk, c, count, n, w, filled_chunk, valid, gap_chunk, stream)
    assert binding.SIGNATURES["gdn_stream_fill"] == [p, p, i, i, i, i, p, p, p, p]
    # gdn_stream_score with `valid` after the chunk
    assert binding.SIGNATURES["gdn_stream_score_gaps"] == [p, p, p, p, p, p, i, i, i, i, p, p, p, p]
    # gdn_stream_advance with `valid, gap_chunk` after pred and `gaps` before the stream
    assert binding.SIGNATURES["gdn_stream_advance_gaps"] == [p, p, p, p, p, p, p, p, i, i, i, i, i, p, p, ll, p, p]
    # the plain entry points keep their argument lists
    assert binding.SIGNATURES["gdn_stream_score"] == [p, p, p, p, p, i, i, i, i, p, p, p, p]
    assert binding.SIGNATURES["gdn_stream_advance"] == [p, p, p, p, p, p, i, i, i, i, i, p, p, ll, p]
    import inspect
    from gdn_amd import harness, ops
    assert callable(ops.stream_fill)
    assert "valid" in inspect.signature(ops.stream_score).parameters
    assert {"valid", "gap_chunk", "gaps"} <= set(inspect.signature(ops.stream_advance).parameters)
    assert not hasattr(ops, "stream_score_gaps") and not hasattr(ops, "stream_advance_gaps")
    assert inspect.signature(harness.StreamDetector.__init__).parameters["gaps"].default is False
    assert callable(harness.StreamDetector.status_gaps)


def _fill(c=16, count=16, n=127, w=15, **kw):
    a = dict(state=FAKE, raw=FAKE, filled=FAKE, valid=FAKE, gap_chunk=FAKE)
    a.update(kw)
    return _lib().gdn_stream_fill(a["state"], a["raw"], c, count, n, w, a["filled"], a["valid"], a["gap_chunk"], None)


def _score(c=16, count=16, n=127, m=3, **kw):
    a = dict(state=FAKE, pred=FAKE, chunk=FAKE, valid=FAKE, med=FAKE, thr=FAKE, scores=FAKE, sensors=FAKE, alarm=FAKE)
    a.update(kw)
    return _lib().gdn_stream_score_gaps(a["state"], a["pred"], a["chunk"], a["valid"], a["med"], a["thr"], c, count, n,
                                        m, a["scores"], a["sensors"], a["alarm"], None)


def _advance(c=16, count=16, n=127, w=15, m=3, log_len=8, **kw):
    a = dict(state=FAKE, chunk=FAKE, pred=FAKE, valid=FAKE, gap_chunk=FAKE, med=FAKE, alarm=FAKE, sensors=FAKE,
             log_ticks=FAKE, log_sensors=FAKE, gaps=FAKE)
    a.update(kw)
    return _lib().gdn_stream_advance_gaps(a["state"], a["chunk"], a["pred"], a["valid"], a["gap_chunk"], a["med"],
                                          a["alarm"], a["sensors"], c, count, n, w, m, a["log_ticks"],
                                          a["log_sensors"], log_len, a["gaps"], None)


def test_every_null_pointer_is_an_argument_error():
    for null in ("state", "raw", "filled", "valid", "gap_chunk"):
        assert _fill(**{null: None}) == GDN_ERR_ARG, null
    for null in ("state", "pred", "chunk", "valid", "med", "thr", "scores", "sensors", "alarm"):
        assert _score(**{null: None}) == GDN_ERR_ARG, null
    for null in ("state", "chunk", "pred", "valid", "gap_chunk", "med", "alarm", "sensors", "gaps"):
        assert _advance(**{null: None}) == GDN_ERR_ARG, null
    assert _advance(log_ticks=None) == GDN_ERR_ARG and _advance(log_sensors=None) == GDN_ERR_ARG
    assert _advance(log_len=-1) == GDN_ERR_ARG
    assert _advance(log_len=0, log_ticks=None, log_sensors=None, n=4097) == GDN_ERR_UNSUPPORTED


@pytest.mark.parametrize("count,c", [(0, 16), (17, 16), (-1, 16), (1, 0)], ids=["count0", "count_gt_c", "count_neg", "c0"])
def test_count_outside_one_to_c_is_an_argument_error(count, c):
    assert _fill(c=c, count=count) == GDN_ERR_ARG
    assert _score(c=c, count=count) == GDN_ERR_ARG
    assert _advance(c=c, count=count) == GDN_ERR_ARG


@pytest.mark.parametrize("shape", [dict(n=4097), dict(n=0), dict(w=0), dict(w=1025)], ids=["n4097", "n0", "w0", "w1025"])
def test_shapes_outside_the_envelope_are_refused(shape):
    assert _fill(**shape) == GDN_ERR_UNSUPPORTED
    assert _advance(**shape) == GDN_ERR_UNSUPPORTED
    if "n" in shape:
        assert _score(**shape) == GDN_ERR_UNSUPPORTED


@pytest.mark.parametrize("m,n", [(0, 27), (9, 27), (4, 3), (-1, 27)], ids=["m0", "m9", "m_gt_n", "m_neg"])
def test_score_and_advance_refuse_m_outside_one_to_eight_and_beyond_n(m, n):
    assert _score(m=m, n=n) == GDN_ERR_UNSUPPORTED
    assert _advance(m=m, n=n) == GDN_ERR_UNSUPPORTED


def test_wrappers_and_detector_refuse_host_tensors_by_name():
    from gdn_amd import GDN, _lib as binding, harness, ops
    with pytest.raises(binding.GdnHipError, match="HIP device"):
        ops.stream_fill(torch.zeros(64, dtype=torch.int64), torch.zeros((4, 9)), 5, torch.zeros((4, 9)),
                        torch.zeros((4, 9), dtype=torch.uint8), torch.zeros((2, 9), dtype=torch.int32))
    model = GDN([torch.zeros((2, 1), dtype=torch.long)], 9, dim=16, input_dim=5, topk=3)
    with pytest.raises(binding.GdnHipError, match="HIP device"):
        harness.StreamDetector(model, torch.zeros((9, 2), dtype=torch.float64), 1.0, torch.zeros((9, 5)), 4, gaps=True)


# ------------------------------------------------------------------------------------------- the yardstick
def test_ffill_by_hand_five_ticks_two_sensors():
    nan, inf = float("nan"), float("inf")
    raw = np.array([[nan, 1.0], [2.0, inf], [nan, -inf], [nan, 4.0], [5.0, nan]], dtype=np.float32)
    filled, valid, missing, trailing = gref.ffill(raw, np.array([9.0, 8.0], dtype=np.float32))
    np.testing.assert_array_equal(filled, np.array([[9, 1], [2, 1], [2, 1], [2, 4], [5, 4]], dtype=np.float32))
    np.testing.assert_array_equal(valid, [[False, True], [True, False], [False, False], [False, True], [True, False]])
    np.testing.assert_array_equal(missing, [3, 3])
    np.testing.assert_array_equal(trailing, [0, 1])
    # the counters of the stream, however it is pushed: missing_total and missing_run literally
    for chunk in (1, 2, 3, 5):
        f, v, total, run = gref.ffill_chunked(raw, np.array([9.0, 8.0], dtype=np.float32), chunk)
        np.testing.assert_array_equal(f, filled)
        np.testing.assert_array_equal(v, valid)
        np.testing.assert_array_equal(total, [3, 3])
        np.testing.assert_array_equal(run, [0, 1])
        state = gref.run_chunked(np.zeros((5, 2)), v, np.ones((2, 2)), chunk)[4]
        np.testing.assert_array_equal(state.missing_total, [3, 3])
        np.testing.assert_array_equal(state.missing_run, [0, 1])
    # a chunk with no real reading at all: the seed is held and the trailing run is the whole chunk
    filled, valid, missing, trailing = gref.ffill(np.full((3, 2), nan, dtype=np.float32), np.array([9.0, 8.0]))
    np.testing.assert_array_equal(filled, [[9, 8]] * 3)
    np.testing.assert_array_equal(missing, [3, 3])
    np.testing.assert_array_equal(trailing, [3, 3])


@pytest.mark.parametrize("chunk", [1, 2, 3, 5, 64])
@pytest.mark.parametrize("case", ["score_T64_N5", "score_T65_N7", "score_T1000_N27", "perf_T777_N5_ties"])
def test_all_valid_the_ref_is_the_plain_stream_ref(case, chunk):
    from oracle import score_oracle
    data, _ = load_golden(case)
    pred, gt = data["pred"], data["gt"]
    med_iqr = np.array([score_oracle.err_median_and_iqr(pred[:, i], gt[:, i]) for i in range(pred.shape[1])])
    delta = np.abs(pred.astype(np.float64) - gt.astype(np.float64))
    m = min(3, pred.shape[1])
    want = ref.run_chunked(delta, med_iqr, chunk, m=m, threshold=0.5)
    got = gref.run_chunked(delta, np.ones(delta.shape, dtype=bool), med_iqr, chunk, m=m, threshold=0.5)
    for a, b in zip(got[:4], want[:4]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(got[4].carry, want[4].carry)
    assert (got[4].ticks, got[4].alarms) == (want[4].ticks, want[4].alarms)
    assert [t for t, _ in got[4].log] == [t for t, _ in want[4].log]
    assert not got[4].missing_total.any() and not got[4].missing_run.any()


def _gappy_series(T=70, n=6, w=4, seed=0):
    """raw [T, n] with the fixed pattern of the issue: a run across the boundary of every push size used (ticks 4 ..
    6 and 62 .. 66), a sensor missing for more than w ticks, a tick with every sensor missing, and +-inf."""
    rng = np.random.default_rng(seed)
    raw = rng.random((T, n)).astype(np.float32)
    raw[4:7, 1] = np.nan
    raw[62:67, 2] = np.nan
    raw[20:20 + w + 3, 3] = np.nan
    raw[33, :] = np.nan
    raw[40, 0], raw[41, 0], raw[50, 4] = np.inf, -np.inf, -np.inf
    raw[T - 2:, 5] = np.nan                                        # the stream ends inside a run
    return raw


def test_the_ref_does_not_depend_on_how_the_stream_is_cut_into_pushes():
    w = 4
    raw = _gappy_series(w=w)
    T, n = raw.shape
    rng = np.random.default_rng(1)
    seed = rng.random(n).astype(np.float32)
    pred = rng.random((T, n)).astype(np.float32)
    med_iqr = np.stack([rng.random(n) * 0.1, rng.random(n) * 0.2 + 0.05], axis=1)
    outs = {}
    for chunk in (1, 2, 3, 5, 64):
        filled, valid, total, run = gref.ffill_chunked(raw, seed, chunk)
        delta = np.abs(pred.astype(np.float64) - filled.astype(np.float64))
        assert np.isfinite(filled).all()
        sm, vals, idx, flags, state = gref.run_chunked(delta, valid, med_iqr, chunk, m=3, threshold=1.0)
        np.testing.assert_array_equal(state.missing_total, total)
        np.testing.assert_array_equal(state.missing_run, run)
        outs[chunk] = (filled, valid, sm, vals, idx, flags, total, run, state.carry, np.array([t for t, _ in state.log]))
    assert outs[1][5].any() and not outs[1][5].all()               # the threshold separates
    for chunk in (2, 3, 5, 64):
        for a, b in zip(outs[chunk], outs[1]):
            np.testing.assert_array_equal(a, b)
    filled, valid, sm, _vals, _idx, _flags, total, run = outs[1][:8]
    np.testing.assert_array_equal(total, [3, 4, 6, w + 4, 2, 3])
    np.testing.assert_array_equal(run, [0, 0, 0, 0, 0, 2])
    assert (filled[20:20 + w + 3, 3] == raw[19, 3]).all() and filled[33, 0] == raw[32, 0]
    np.testing.assert_array_equal(valid, np.isfinite(raw))
    # neutral: a sensor whose four taps are all missing scores exactly 0.0
    assert (sm[3, 23:20 + w + 3] == 0.0).all() and np.isfinite(sm).all()
