"""CPU suite of the streaming detector (gdn_stream_* entry points, harness.StreamDetector): the C-ABI surface and the
host-side refusals (decided before any launch, so no device is needed), and the float64 yardstick of the GPU tests
(tests/_stream_ref.py) pinned to the oracle: chunked scoring with a carry IS the batch arithmetic."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _stream_ref as ref
from conftest import ROOT, load_golden

GDN_ERR_ARG, GDN_ERR_UNSUPPORTED = -1, -3
FAKE = 4096          # a non-null, 16-byte aligned address that is never dereferenced on the host
NEW = ["gdn_stream_state_bytes", "gdn_stream_init", "gdn_stream_windows", "gdn_stream_score", "gdn_stream_advance"]


def _lib():
    from gdn_amd import _lib as binding
    return binding.load()


def test_header_signatures_and_exports_agree_and_the_abi_stays():
    from gdn_amd import _lib as binding
    header = open(os.path.join(ROOT, "include", "gdn_hip.h")).read()
    declared = dict((name, ret) for ret, name in re.findall(r"^(int|long long)\s+(gdn_\w+)\s*\(", header, flags=re.M))
    lib = binding.load()
    for name in NEW:
        assert name in declared and name in binding.SIGNATURES
        fn = getattr(lib, name)                      # AttributeError: the symbol is missing
        assert fn.argtypes == binding.SIGNATURES[name]
        assert fn.restype is (ctypes.c_longlong if declared[name] == "long long" else ctypes.c_int)
    assert declared["gdn_stream_state_bytes"] == "long long"
    assert [declared[n] for n in NEW[1:]] == ["int"] * 4
    assert "#define GDN_ABI_VERSION 23" in header and binding.ABI_VERSION == 23 and lib.gdn_abi_version() == 23
    p, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert binding.SIGNATURES["gdn_stream_state_bytes"] == [i, i]
    assert binding.SIGNATURES["gdn_stream_init"] == [p, p, ll, i, i, p]
    assert binding.SIGNATURES["gdn_stream_windows"] == [p, p, i, i, i, i, p, p]
    assert binding.SIGNATURES["gdn_stream_score"] == [p, p, p, p, p, i, i, i, i, p, p, p, p]
    assert binding.SIGNATURES["gdn_stream_advance"] == [p, p, p, p, p, p, i, i, i, i, i, p, p, ll, p]
    # the argument lists of the header, counted: a parameter added on one side only shows here
    for name in NEW:
        params = re.search(name + r"\s*\(([^)]*)\)\s*;", header).group(1)
        assert len(params.split(",")) == len(binding.SIGNATURES[name]), name
    from gdn_amd import GDN, harness, ops
    assert all(callable(getattr(ops, f)) for f in ("stream_state", "stream_windows", "stream_score", "stream_advance"))
    assert callable(harness.StreamDetector) and callable(harness.StreamDetector.from_calibration)
    import inspect
    assert inspect.signature(GDN.forward_into).parameters["guard"].default is False


def test_state_bytes_are_positive_aligned_and_hold_the_documented_layout():
    lib = _lib()
    for n, w in [(1, 1), (5, 4), (127, 15), (130, 65), (4096, 1024), (3, 1)]:
        b = lib.gdn_stream_state_bytes(n, w)
        assert b > 0 and b % 8 == 0
        assert b >= 3 * 8 + 3 * n * 8 + n * w * 4            # three counters, carry[3, n] float64, hist[n, w] fp32
        assert b <= 4 * 8 + 3 * n * 8 + n * w * 4 + 8
    for n, w in [(4097, 15), (0, 15), (127, 0), (127, 1025)]:
        assert lib.gdn_stream_state_bytes(n, w) == 0


def _init(h=20, n=127, w=15, state=FAKE, history=FAKE):
    return _lib().gdn_stream_init(state, history, h, n, w, None)


def _windows(c=16, count=16, n=127, w=15, state=FAKE, chunk=FAKE, x=FAKE):
    return _lib().gdn_stream_windows(state, chunk, c, count, n, w, x, None)


def _score(c=16, count=16, n=127, m=3, **kw):
    a = dict(state=FAKE, pred=FAKE, chunk=FAKE, med=FAKE, thr=FAKE, scores=FAKE, sensors=FAKE, alarm=FAKE)
    a.update(kw)
    return _lib().gdn_stream_score(a["state"], a["pred"], a["chunk"], a["med"], a["thr"], c, count, n, m, a["scores"],
                                   a["sensors"], a["alarm"], None)


def _advance(c=16, count=16, n=127, w=15, m=3, log_len=8, **kw):
    a = dict(state=FAKE, chunk=FAKE, pred=FAKE, med=FAKE, alarm=FAKE, sensors=FAKE, log_ticks=FAKE, log_sensors=FAKE)
    a.update(kw)
    return _lib().gdn_stream_advance(a["state"], a["chunk"], a["pred"], a["med"], a["alarm"], a["sensors"], c, count, n,
                                     w, m, a["log_ticks"], a["log_sensors"], log_len, None)


def test_init_refuses_a_history_shorter_than_the_window():
    assert _init(h=14, w=15) == GDN_ERR_ARG                 # a cold start
    assert _init(h=0, w=1) == GDN_ERR_ARG
    assert _init(state=None) == GDN_ERR_ARG and _init(history=None) == GDN_ERR_ARG


@pytest.mark.parametrize("shape", [dict(n=4097), dict(n=0), dict(w=0), dict(w=1025)], ids=["n4097", "n0", "w0", "w1025"])
def test_shapes_outside_the_envelope_are_refused(shape):
    big_h = dict(h=2000)
    assert _init(**big_h, **shape) == GDN_ERR_UNSUPPORTED
    assert _windows(**shape) == GDN_ERR_UNSUPPORTED
    assert _advance(**shape) == GDN_ERR_UNSUPPORTED
    if "n" in shape:
        assert _score(**shape) == GDN_ERR_UNSUPPORTED
    from gdn_amd import _lib as binding
    full = dict(n=127, w=15)
    full.update(shape)
    with pytest.raises(binding.GdnHipError, match="GDN_ERR_UNSUPPORTED"):
        binding.call("gdn_stream_windows", FAKE, FAKE, 16, 16, full["n"], full["w"], FAKE, None)


@pytest.mark.parametrize("m,n", [(0, 27), (9, 27), (4, 3), (-1, 27)], ids=["m0", "m9", "m_gt_n", "m_neg"])
def test_score_and_advance_refuse_m_outside_one_to_eight_and_beyond_n(m, n):
    assert _score(m=m, n=n) == GDN_ERR_UNSUPPORTED
    assert _advance(m=m, n=n) == GDN_ERR_UNSUPPORTED


@pytest.mark.parametrize("count,c", [(0, 16), (17, 16), (-1, 16), (1, 0)], ids=["count0", "count_gt_c", "count_neg", "c0"])
def test_count_outside_one_to_c_is_an_argument_error(count, c):
    assert _windows(c=c, count=count) == GDN_ERR_ARG
    assert _score(c=c, count=count) == GDN_ERR_ARG
    assert _advance(c=c, count=count) == GDN_ERR_ARG


def test_every_null_pointer_is_an_argument_error():
    for null in ("state", "chunk", "x"):
        assert _windows(**{null: None}) == GDN_ERR_ARG, null
    for null in ("state", "pred", "chunk", "med", "thr", "scores", "sensors", "alarm"):
        assert _score(**{null: None}) == GDN_ERR_ARG, null
    for null in ("state", "chunk", "pred", "med", "alarm", "sensors"):
        assert _advance(**{null: None}) == GDN_ERR_ARG, null
    # a log of L > 0 entries needs both tables; L = 0 needs neither (checked: it passes on to the shape refusals)
    assert _advance(log_ticks=None) == GDN_ERR_ARG and _advance(log_sensors=None) == GDN_ERR_ARG
    assert _advance(log_len=-1) == GDN_ERR_ARG
    assert _advance(log_len=0, log_ticks=None, log_sensors=None, n=4097) == GDN_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("chunk", [1, 2, 3, 5, 64])
@pytest.mark.parametrize("case", ["score_T64_N5", "score_T65_N7", "score_T1000_N27", "perf_T777_N5_ties"])
def test_chunked_scoring_with_a_carry_equals_the_score_oracle_exactly(case, chunk):
    from oracle import score_oracle
    data, _ = load_golden(case)
    pred, gt = data["pred"], data["gt"]
    want = score_oracle.full_err_scores(pred, gt)
    med_iqr = np.array([score_oracle.err_median_and_iqr(pred[:, i], gt[:, i]) for i in range(pred.shape[1])])
    delta = np.abs(pred.astype(np.float64) - gt.astype(np.float64))
    got, vals, idx, flags, state = ref.run_chunked(delta, med_iqr, chunk, m=min(3, pred.shape[1]))
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(vals[:, 0], want.max(axis=0))
    assert state.ticks == len(pred) and not flags.any() and state.alarms == 0


def test_stream_helper_orders_flags_and_logs():
    med_iqr = np.array([[0.0, 0.99], [0.0, 0.99], [0.0, 0.99]])              # den = 1: a = delta
    delta = np.zeros((12, 3))
    delta[4] = [4.0, 8.0, 8.0]                                                # a tie between sensors 1 and 2
    delta[9] = np.nan                                                         # every score of ticks 9 .. 11 is NaN
    for chunk in (1, 2, 12):
        got, vals, idx, flags, state = ref.run_chunked(delta, med_iqr, chunk, m=2, threshold=1.5)
        np.testing.assert_array_equal(idx[4], [1, 2])
        np.testing.assert_array_equal(vals[4], [2.0, 2.0])
        np.testing.assert_array_equal(np.nonzero(flags)[0], [4, 5, 6, 7])     # 2.0 > 1.5 while the spike is in the mean
        assert np.isnan(vals[9:, 0]).all() and not flags[9:].any()            # a NaN score never alarms
        assert state.alarms == 4 and [t for t, _ in state.log] == [4, 5, 6, 7]
        assert (got[:, :3] == 0).all()
        assert not (vals[:, 0] > 2.0).any() and not flags[8]                  # strict: 0 > 1.5 is false, so is 1.5 > 1.5
    assert not ref.run_chunked(delta[:9], med_iqr, 3, m=1, threshold=2.0)[3].any()


# ------------------------------------------------------------------------------------------- StreamDetector, host side
def _cpu_model(n=9, w=5, **kw):
    from gdn_amd import GDN
    return GDN([torch.zeros((2, 1), dtype=torch.long)], n, dim=16, input_dim=w, topk=3, **kw)


def _detector(model, n=9, w=5, **kw):
    from gdn_amd import harness
    args = dict(med_iqr=torch.zeros((n, 2), dtype=torch.float64), threshold=1.0, history=torch.zeros((n, w)), chunk=4)
    args.update(kw)
    return harness.StreamDetector(model, args.pop("med_iqr"), args.pop("threshold"), args.pop("history"),
                                  args.pop("chunk"), **args)


@pytest.mark.parametrize("chunk", [0, -3, 4097])
def test_detector_refuses_a_chunk_outside_one_to_4096(chunk):
    with pytest.raises(ValueError, match="chunk"):
        _detector(_cpu_model(), chunk=chunk)


def test_detector_refuses_a_window_buffer_beyond_256_mb():
    n, w = 4096, 64                                          # 1 MB of windows per tick: 256 ticks fit, 257 do not
    model = _cpu_model(n=n, w=w)
    with pytest.raises(ValueError, match="256 MB"):
        _detector(model, n=n, w=w, chunk=257)


@pytest.mark.parametrize("top_m", [0, 9, 10])
def test_detector_refuses_top_m_outside_one_to_eight_and_beyond_n(top_m):
    with pytest.raises(ValueError, match="top_m"):
        _detector(_cpu_model(), top_m=top_m)
    with pytest.raises(ValueError, match="top_m"):
        _detector(_cpu_model(n=4), n=4, top_m=5)


def test_detector_refuses_an_mlp_head_without_a_fast_path_by_name():
    from gdn_amd import _lib as binding
    model = _cpu_model(out_layer_num=2, out_layer_inter_dim=600)          # hidden 600: neither eval tail takes it
    with pytest.raises(binding.GdnHipError, match="OutLayer"):
        _detector(model)


def test_detector_and_wrappers_refuse_host_tensors_by_name():
    from gdn_amd import _lib as binding, ops
    with pytest.raises(binding.GdnHipError, match="HIP device"):
        _detector(_cpu_model())                                            # history on the host
    with pytest.raises(binding.GdnHipError, match="HIP device"):
        ops.stream_state(torch.zeros((9, 5)), 5)
    with pytest.raises(binding.GdnHipError, match="HIP device"):
        ops.stream_windows(torch.zeros(64, dtype=torch.int64), torch.zeros((4, 9)), 5, torch.zeros((4, 9, 5)))
