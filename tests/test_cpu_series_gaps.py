"""CPU suite of the resident series with missing readings: the additive entry points in header,
bindings and library, their host-side refusals, the Python surface (SeriesEvaluator(gaps=, min_kept=),
StreamDetector.from_calibration(calib_gaps=)), and the yardstick of the GPU tests (tests/_series_gaps_ref.py): the
whole-series form must equal the chunked form of tests/_stream_gaps_ref.py for every push size, and its table must be
numpy's on the kept rows."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import _series_gaps_ref as sref
import _stream_gaps_ref as gref
from conftest import ROOT

GDN_ERR_ARG, GDN_ERR_UNSUPPORTED = -1, -3
FAKE = 4096          # a non-null, 16-byte aligned address that is never dereferenced on the host
NEW = {"gdn_series_fill_workspace_bytes": "long long", "gdn_series_fill": "int", "gdn_score_keys_keep": "int",
       "gdn_score_smooth_max_gaps": "int", "gdn_score_smooth_topm_gaps": "int"}
SHAPES = ((5, 3), (65, 3), (130, 15), (20, 5))


def test_the_symbols_are_declared_bound_and_exported_and_the_abi_stays():
    from gdn_amd import _lib as binding
    header = open(os.path.join(ROOT, "include", "gdn_hip.h")).read()
    declared = dict((name, ret) for ret, name in re.findall(r"^(int|long long)\s+(gdn_\w+)\s*\(", header, flags=re.M))
    lib = binding.load()
    for name, ret in NEW.items():
        assert declared.get(name) == ret and name in binding.SIGNATURES, name
        fn = getattr(lib, name)                      # AttributeError: the symbol is missing
        assert fn.argtypes == binding.SIGNATURES[name]
        assert fn.restype is (ctypes.c_longlong if ret == "long long" else ctypes.c_int)
        params = re.search(name + r"\s*\(([^)]*)\)\s*;", header).group(1)
        assert len(params.split(",")) == len(binding.SIGNATURES[name]), name
    assert "#define GDN_ABI_VERSION 23" in header and binding.ABI_VERSION == 23 and lib.gdn_abi_version() == 23
    p, i = ctypes.c_void_p, ctypes.c_int
    # (raw, n, t_raw, w, filled, gt, valid, keep, counters, workspace, stream)
    assert binding.SIGNATURES["gdn_series_fill"] == [p, i, i, i, p, p, p, p, p, p, p]
    # gdn_score_keys with `keep` after gt
    assert binding.SIGNATURES["gdn_score_keys_keep"] == [p, p, p, i, i, i, p, p]
    # the plain argument lists plus `valid, halo_valid` before the stream
    for plain in ("gdn_score_smooth_max", "gdn_score_smooth_topm"):
        assert binding.SIGNATURES[plain + "_gaps"] == binding.SIGNATURES[plain][:-1] + [p, p, p]
    assert binding.SIGNATURES["gdn_score_smooth_max"] == [p, p, p, i, i, i, p, p, p, p, p]
    assert binding.SIGNATURES["gdn_score_smooth_topm"] == [p, p, p, i, i, i, p, p, i, p, p, p]
    from gdn_amd import ops
    assert callable(ops.series_fill)
    assert "keep" in inspect.signature(ops.score_keys).parameters
    for f in ("score_smooth_max", "score_smooth_topm"):
        assert {"valid", "halo_valid"} <= set(inspect.signature(getattr(ops, f)).parameters)
    assert not any(hasattr(ops, f) for f in ("score_keys_keep", "score_smooth_max_gaps", "score_smooth_topm_gaps"))


def test_evaluator_and_from_calibration_accept_the_new_arguments():
    from gdn_amd import harness
    ev = inspect.signature(harness.SeriesEvaluator.__init__).parameters
    assert ev["gaps"].default is False and ev["min_kept"].default == 64
    cal = inspect.signature(harness.StreamDetector.from_calibration).parameters
    assert cal["calib_gaps"].default is False and cal["min_kept"].default == 64
    assert callable(harness.SeriesEvaluator.status_gaps)
    from gdn_amd import main as cli
    args = cli.build_parser().parse_args(["-stream", "16", "-stream_gaps", "-stream_calib_gaps"])
    assert args.stream_calib_gaps is True and cli.build_parser().parse_args([]).stream_calib_gaps is False


def test_workspace_bytes_and_host_side_refusals():
    from gdn_amd import _lib as binding
    lib = binding.load()
    size = lib.gdn_series_fill_workspace_bytes
    assert size(127, 32783) > 0 and size(127, 32783) % 8 == 0 and size(1, 2) > 0 and size(4096, 100) > 0
    assert size(127, 32783) >= 12 * 127 * ((32783 + 63) // 64)       # three 4-byte planes of [n, blocks]
    for n, t_raw in ((0, 100), (4097, 100), (5, 1), (5, 0), (-1, 100)):
        assert size(n, t_raw) == 0, (n, t_raw)

    def fill(n=5, t_raw=40, w=3, **kw):
        a = dict(raw=FAKE, filled=2 * FAKE, gt=FAKE, valid=FAKE, keep=FAKE, counters=FAKE, ws=FAKE)
        a.update(kw)
        return lib.gdn_series_fill(a["raw"], n, t_raw, w, a["filled"], a["gt"], a["valid"], a["keep"], a["counters"],
                                   a["ws"], None)
    for null in ("raw", "filled", "gt", "valid", "keep", "counters", "ws"):
        assert fill(**{null: None}) == GDN_ERR_ARG, null
    assert fill(filled=FAKE) == GDN_ERR_ARG                          # filled must not alias raw
    for shape in (dict(n=0), dict(n=4097), dict(w=0), dict(t_raw=3), dict(t_raw=2)):
        assert fill(**shape) == GDN_ERR_UNSUPPORTED, shape

    def keys(t=40, n=5, pitch=40, **kw):
        a = dict(pred=FAKE, gt=FAKE, keep=FAKE, keys=FAKE)
        a.update(kw)
        return lib.gdn_score_keys_keep(a["pred"], a["gt"], a["keep"], t, n, pitch, a["keys"], None)
    for null in ("pred", "gt", "keep", "keys"):
        assert keys(**{null: None}) == GDN_ERR_ARG, null
    assert keys(pitch=39) == GDN_ERR_ARG and keys(t=0) == GDN_ERR_ARG and keys(n=0) == GDN_ERR_ARG

    def smooth_max(first=0, **kw):
        a = dict(pred=FAKE, gt=FAKE, med=FAKE, hp=None, hg=None, scores=None, anomaly=FAKE, valid=FAKE, hv=None)
        a.update(kw)
        return lib.gdn_score_smooth_max_gaps(a["pred"], a["gt"], a["med"], 40, 5, first, a["hp"], a["hg"], a["scores"],
                                             a["anomaly"], a["valid"], a["hv"], None)

    def smooth_topm(first=0, m=3, **kw):
        a = dict(pred=FAKE, gt=FAKE, med=FAKE, hp=None, hg=None, ts=FAKE, ti=FAKE, valid=FAKE, hv=None)
        a.update(kw)
        return lib.gdn_score_smooth_topm_gaps(a["pred"], a["gt"], a["med"], 40, 5, first, a["hp"], a["hg"], m, a["ts"],
                                              a["ti"], a["valid"], a["hv"], None)
    assert smooth_max(valid=None) == GDN_ERR_ARG and smooth_topm(valid=None) == GDN_ERR_ARG
    assert smooth_max(first=8, hp=FAKE, hg=FAKE) == GDN_ERR_ARG      # a halo without its validity rows
    assert smooth_topm(first=8, hp=FAKE, hg=FAKE) == GDN_ERR_ARG
    assert smooth_max(anomaly=None) == GDN_ERR_ARG and smooth_topm(ts=None) == GDN_ERR_ARG
    assert smooth_topm(m=0) == GDN_ERR_UNSUPPORTED and smooth_topm(m=9) == GDN_ERR_UNSUPPORTED
    assert smooth_topm(m=6) == GDN_ERR_UNSUPPORTED                   # m > n = 5


# ------------------------------------------------------------------------------------------- the yardstick
def test_missing_is_the_exponent_field_and_fill_by_hand():
    bits = np.array([0x7fc00000, 0x7fc12345, 0x7f800001, 0xffc00000, 0x7f800000, 0xff800000, 0x7f7fffff, 0x00000001,
                     0x80000000], dtype=np.uint32)
    np.testing.assert_array_equal(sref.missing(bits.view(np.float32)), [True] * 6 + [False] * 3)
    nan, inf = float("nan"), float("inf")
    raw = np.array([[9.0, 8.0, nan, 2.0, nan, nan, 5.0],
                    [7.0, 6.0, 1.0, inf, -inf, 4.0, nan]], dtype=np.float32)
    filled, gt, valid, keep, total, run = sref.fill(raw, 2)
    np.testing.assert_array_equal(filled, [[9, 8, 8, 2, 2, 2, 5], [7, 6, 1, 1, 1, 4, 4]])
    np.testing.assert_array_equal(gt, filled[:, 2:].T)
    np.testing.assert_array_equal(valid.T, [[False, True, False, False, True], [True, False, False, True, False]])
    np.testing.assert_array_equal(keep, [False, False, False, False, False])
    np.testing.assert_array_equal(total, [3, 3])
    np.testing.assert_array_equal(run, [0, 1])
    with pytest.raises(ValueError, match=r"(?s)series.*gaps"):
        sref.fill(np.array([[nan, 1.0, 2.0]], dtype=np.float32), 2)


def _cases():
    for n, w in SHAPES:
        for t in sref.LENGTHS:
            for pattern in sref.PATTERNS:
                if pattern == "d" and t < 300:
                    continue
                yield n, w, t, pattern


def test_every_pattern_leaves_min_kept_complete_ticks_and_is_what_it_says():
    seen = set()
    for n, w, t, pattern in _cases():
        clean = sref.clean_series(n, w, t)
        raw = sref.with_pattern(clean, w, pattern)                   # (asserts kept >= MIN_KEPT itself)
        gone = sref.missing(raw)
        np.testing.assert_array_equal(raw[~gone], clean[~gone])
        _filled, _gt, valid, keep, total, run = sref.fill(raw, w)
        assert keep.sum() >= sref.MIN_KEPT
        seen.add(pattern)
        if pattern == "a":
            assert not gone.any() and keep.all()
        if pattern == "b":
            assert gone.sum() == 6 and np.isinf(raw[gone]).sum() == 2 and total.max() <= 2
        if pattern == "c":
            assert total.max() == w + 3 > w
        if pattern == "d":
            assert total.max() == 140 >= 130 and gone[1 % n, 128:192].all()
        if pattern == "e":
            assert (~valid).all(axis=1).sum() == 1
        if pattern == "f":
            assert not valid[0].all() and not valid[-1].all() and run.max() == 2 and (run > 0).sum() == 2
    assert seen == set(sref.PATTERNS)


@pytest.mark.parametrize("chunk", [1, 5, 37])
def test_the_whole_series_form_equals_the_chunked_stream_ref(chunk):
    for n, w, t, pattern in _cases():
        if t == 129:
            continue                                                 # (64, 65 and 300 carry the edges; keeps this quick)
        raw = sref.with_pattern(sref.clean_series(n, w, t), w, pattern)
        filled, gt, valid, keep, total, run = sref.fill(raw, w)
        f, v, tot, rn = gref.ffill_chunked(raw[:, w:].T.copy(), raw[:, w - 1], chunk)
        what = (n, w, t, pattern)
        np.testing.assert_array_equal(gt, f, err_msg=str(what))
        np.testing.assert_array_equal(valid, v, err_msg=str(what))
        np.testing.assert_array_equal(total, tot, err_msg=str(what))
        np.testing.assert_array_equal(run, rn, err_msg=str(what))
        np.testing.assert_array_equal(keep, v.all(axis=1))
        np.testing.assert_array_equal(filled[:, :w], raw[:, :w])
        rng = np.random.default_rng(n + t)
        pred = rng.random((t, n)).astype(np.float32)
        med_iqr = sref.table(pred, gt, keep)
        m = min(3, n)
        sm, vals, idx = sref.scores(pred, gt, valid, med_iqr, m)
        delta = np.abs(pred.astype(np.float64) - gt.astype(np.float64))
        sm2, vals2, idx2, _flags, state = gref.run_chunked(delta, v, med_iqr, chunk, m=m)
        np.testing.assert_array_equal(sm, sm2, err_msg=str(what))    # bit for bit: the same float64 operations
        np.testing.assert_array_equal(vals, vals2, err_msg=str(what))
        np.testing.assert_array_equal(idx, idx2, err_msg=str(what))
        np.testing.assert_array_equal(state.missing_total, total)
        np.testing.assert_array_equal(state.missing_run, run)
        assert (sm.T[3:][~(valid[3:] | valid[2:-1] | valid[1:-2] | valid[:-3])] == 0.0).all()


def test_the_table_is_numpy_on_the_kept_rows():
    from oracle import score_oracle
    for n, w, t, pattern in _cases():
        raw = sref.with_pattern(sref.clean_series(n, w, t), w, pattern)
        _filled, gt, _valid, keep, _total, _run = sref.fill(raw, w)
        pred = np.random.default_rng(n + t).random((t, n)).astype(np.float32)
        med_iqr = sref.table(pred, gt, keep)
        rows = np.nonzero(keep)[0]
        assert len(rows) == keep.sum() >= sref.MIN_KEPT
        for i in range(n):
            delta = np.abs(pred[rows, i].astype(np.float64) - gt[rows, i].astype(np.float64))
            assert med_iqr[i, 0] == np.median(delta)
            assert med_iqr[i, 1] == np.percentile(delta, 75) - np.percentile(delta, 25)
            if i < 3:                                                # the reference's own functions (scipy's iqr)
                med, rng = score_oracle.err_median_and_iqr(pred[rows, i], gt[rows, i])
                assert med_iqr[i, 0] == med and med_iqr[i, 1] == rng
        if pattern == "a":                                           # no gap: the plain table
            plain = np.array([score_oracle.err_median_and_iqr(pred[:, i], gt[:, i]) for i in range(min(n, 3))])
            np.testing.assert_array_equal(med_iqr[:min(n, 3)], plain)
