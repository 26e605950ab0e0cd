"""CPU suite of training on a resident series with missing readings: the float64 restatement
(tests/_train_gaps_ref.py) on hand-made cases, the C-ABI surface of the three new entry points, their refusals (decided
before any launch, so no device is needed) and the host-side refusals of the Python and command-line layers."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _train_gaps_ref as ref
from conftest import ROOT

FAKE = 4096          # a non-null, 16-byte aligned address that is never dereferenced on the host
NEW = ["gdn_windows_gather_gaps", "gdn_mse_loss_grad_masked", "gdn_mse_batch_means_masked"]


# ------------------------------------------------------------------------------------------------ the restatement
def test_missing_is_the_exponent_test_and_fill_holds_the_last_real_reading():
    raw = np.array([[1.0, 2.0, np.nan, np.inf, 5.0, -np.inf], [7.0, 8.0, 9.0, np.nan, np.nan, 12.0]], dtype=np.float32)
    raw.view(np.uint32)[0, 2] = 0x7fc12345                          # a NaN with a payload
    assert ref.missing(raw).tolist() == [[False, False, True, True, False, True], [False, False, False, True, True, False]]
    filled, valid = ref.fill(raw, 2)
    assert filled.tolist() == [[1.0, 2.0, 2.0, 2.0, 5.0, 5.0], [7.0, 8.0, 9.0, 9.0, 9.0, 12.0]]
    assert valid.dtype == np.uint8 and valid.tolist() == [[0, 1], [0, 0], [1, 0], [0, 1]]
    with pytest.raises(ValueError, match="series.*gaps"):
        ref.fill(raw, 3)


def test_gather_cuts_windows_targets_and_validity_rows_and_zeros_outside():
    raw = np.arange(24, dtype=np.float32).reshape(2, 12)
    raw[1, 7] = np.nan
    filled, valid = ref.fill(raw, 3)
    x, y, v, rv = ref.gather(filled, valid, [7, 3, 12, 2], 3, batch=5)
    assert x[0].tolist() == [[4.0, 5.0, 6.0], [16.0, 17.0, 18.0]] and y[0].tolist() == [7.0, 18.0]
    assert v.tolist() == [[1, 0], [1, 1], [0, 0], [0, 0], [0, 0]] and rv.tolist() == [1, 2, 0, 0, 0]
    assert rv.dtype == np.int32 and not x[2:].any() and not y[2:].any()


@pytest.mark.parametrize("case", ["some", "all", "none"])
def test_masked_loss_equals_a_float64_loop_and_its_autograd(case):
    rng = np.random.default_rng(3)
    out, y = rng.standard_normal((4, 5)), rng.standard_normal((4, 5))
    v = {"some": ref.burst_mask((4, 5), 0.3, 2, seed=1), "all": np.ones((4, 5), np.uint8), "none": np.zeros((4, 5), np.uint8)}[case]
    if case != "all":                                               # what a masked slot holds must not matter
        out[v == 0], y[v == 0] = np.nan, np.inf
    loss, d_out, m = ref.masked_loss(out, y, v)
    want, want_m = ref.masked_loss_loop(out, y, v)
    assert m == want_m == int(v.sum())
    np.testing.assert_allclose(loss, want, rtol=1e-14, atol=0)
    auto_loss, auto_grad = ref.masked_loss_autograd(out, y, v)
    np.testing.assert_allclose(auto_loss, want, rtol=1e-14, atol=0)
    np.testing.assert_allclose(auto_grad, d_out, rtol=1e-14, atol=0)
    assert np.isfinite(d_out).all() and (d_out[v == 0] == 0.0).all()
    if case == "all":
        o = torch.tensor(out, requires_grad=True)
        f = torch.nn.functional.mse_loss(o, torch.tensor(y), reduction="mean")
        f.backward()
        np.testing.assert_allclose(loss, float(f), rtol=1e-14, atol=0)
        np.testing.assert_allclose(d_out, o.grad.numpy(), rtol=1e-14, atol=0)
    if case == "none":
        assert loss == 0.0 and m == 0 and not d_out.any()


def test_masked_batch_means_leave_an_empty_minibatch_out_of_the_mean_of_means():
    rng = np.random.default_rng(5)
    pred, y = rng.random((7, 3), dtype=np.float32), rng.random((7, 3), dtype=np.float32)
    v = np.ones((7, 3), dtype=np.uint8)
    v[3:6] = 0                                                      # minibatch 1 of 3 (rows 3 .. 5) has no real target
    v[0, 1] = 0
    pred[4, 0], y[5, 2] = np.nan, np.inf
    means, counts, mean = ref.masked_batch_means(pred, y, v, 3)
    assert counts.tolist() == [8, 0, 3] and means[1] == 0.0
    d = (pred - y).astype(np.float32).astype(np.float64) ** 2
    want0 = sum(d[r, c] for r in range(3) for c in range(3) if v[r, c]) / 8
    want2 = sum(d[6, c] for c in range(3)) / 3
    np.testing.assert_allclose(means[[0, 2]], [want0, want2], rtol=1e-14, atol=0)
    np.testing.assert_allclose(mean, (want0 + want2) / 2, rtol=1e-14, atol=0)
    assert ref.masked_batch_means(pred, y, np.zeros((7, 3), np.uint8), 3)[2] == 0.0
    import _train_series_ref as plain                              # every target real: gdn_mse_batch_means' yardstick
    pred, y = rng.random((7, 3), dtype=np.float32), rng.random((7, 3), dtype=np.float32)
    all_means, all_counts, all_mean = ref.masked_batch_means(pred, y, np.ones((7, 3), np.uint8), 3)
    want_means, want_mean = plain.mse_batch_means(pred, y, 3)
    np.testing.assert_allclose(all_means, want_means, rtol=1e-15, atol=0)
    np.testing.assert_allclose(all_mean, want_mean, rtol=1e-15, atol=0)
    assert all_counts.tolist() == [9, 9, 3]


# ------------------------------------------------------------------------------------------------ the C ABI
def test_header_signatures_and_exports_agree_and_the_abi_stays():
    from gdn_amd import _lib
    header = open(os.path.join(ROOT, "include", "gdn_hip.h")).read()
    declared = dict((name, ret) for ret, name in re.findall(r"^(int|long long)\s+(gdn_\w+)\s*\(", header, flags=re.M))
    lib = _lib.load()
    for name in NEW:
        assert declared.get(name) == "int" and name in _lib.SIGNATURES
        fn = getattr(lib, name)                      # AttributeError: the symbol is missing
        assert fn.argtypes == _lib.SIGNATURES[name] and fn.restype is ctypes.c_int
    assert "#define GDN_ABI_VERSION 23" in header and _lib.ABI_VERSION == 23 and lib.gdn_abi_version() == 23
    p, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert _lib.SIGNATURES["gdn_windows_gather_gaps"] == [p, i, ll, p, ll, p, ll, i, i, p, p, p, p, p, p]
    assert _lib.SIGNATURES["gdn_mse_loss_grad_masked"] == [p, p, p, p, i, i, p, p, p, p, p]
    assert _lib.SIGNATURES["gdn_mse_batch_means_masked"] == [p, p, p, ll, i, ll, p, p, p, p, p]
    from gdn_amd import harness
    assert all(callable(getattr(harness, f)) for f in ("fill_series", "masked_share"))


@pytest.mark.parametrize("bad", [dict(series=None), dict(starts=None), dict(x=None), dict(y=None), dict(valid=None),
                                 dict(valid_out=None), dict(row_valid=None), dict(batch=0), dict(w=0), dict(w=1025),
                                 dict(n=0), dict(n=4097), dict(count=0), dict(series_len=15), dict(first=-1)])
def test_windows_gather_gaps_refuses_before_any_launch(bad):
    from gdn_amd import _lib
    a = dict(series=FAKE, n=127, series_len=1000, starts=FAKE, count=64, cursor=None, first=0, batch=64, w=15, x=FAKE,
             y=FAKE, valid=FAKE, valid_out=FAKE, row_valid=FAKE)
    a.update(bad)
    assert _lib.load().gdn_windows_gather_gaps(a["series"], a["n"], a["series_len"], a["starts"], a["count"], a["cursor"],
                                               a["first"], a["batch"], a["w"], a["x"], a["y"], a["valid"],
                                               a["valid_out"], a["row_valid"], None) != 0


@pytest.mark.parametrize("bad", [dict(out=None), dict(y=None), dict(valid=None), dict(row_valid=None), dict(ws=None),
                                 dict(loss=None), dict(d_out=None), dict(batch=0), dict(n=0)])
def test_mse_loss_grad_masked_refuses_before_any_launch(bad):
    from gdn_amd import _lib
    a = dict(out=FAKE, y=FAKE, valid=FAKE, row_valid=FAKE, batch=32, n=5, ws=FAKE, loss=FAKE, d_out=FAKE)
    a.update(bad)
    assert _lib.load().gdn_mse_loss_grad_masked(a["out"], a["y"], a["valid"], a["row_valid"], a["batch"], a["n"], a["ws"],
                                                a["loss"], a["d_out"], None, None) != 0


@pytest.mark.parametrize("bad", [dict(pred=None), dict(y=None), dict(valid=None), dict(means=None), dict(counts=None),
                                 dict(mean=None), dict(batch=0), dict(n=0), dict(n=4097), dict(rows=0)])
def test_mse_batch_means_masked_refuses_before_any_launch(bad):
    from gdn_amd import _lib
    a = dict(pred=FAKE, y=FAKE, valid=FAKE, rows=70, n=5, batch=32, means=FAKE, counts=FAKE, mean=FAKE)
    a.update(bad)
    assert _lib.load().gdn_mse_batch_means_masked(a["pred"], a["y"], a["valid"], a["rows"], a["n"], a["batch"],
                                                  a["means"], a["counts"], a["mean"], None, None) != 0


# ------------------------------------------------------------------------------------------------ the layers above
def test_train_gaps_with_no_hip_graph_is_refused_by_name():
    from gdn_amd import main
    with pytest.raises(ValueError, match="-train_gaps.*-no_hip_graph"):
        main.main(["-dataset", "msl", "-train_gaps", "-no_hip_graph"])
    args = main.build_parser().parse_args(["-train_gaps"])
    assert args.train_gaps is True and main.build_parser().parse_args([]).train_gaps is False
    main.check_train_gaps(True, True), main.check_train_gaps(False, False)      # neither pair is refused


def test_a_series_that_does_not_begin_on_real_readings_is_refused_by_name():
    """One host read at construction, before any launch: no device is needed to be refused."""
    from gdn_amd import harness
    series = torch.rand((3, 40))
    series[1, 4] = float("nan")                                     # inside the first w = 5 ticks
    with pytest.raises(ValueError, match="series.*gaps"):
        harness.fill_series(series, 5)
    with pytest.raises(ValueError, match="series.*gaps"):
        harness.SeriesTrainer(None, series, 5, torch.arange(5, 40), 8, gaps=True)
    with pytest.raises(ValueError, match="series.*gaps"):
        harness.train_series(None, "", {"train_gaps": True}, series, 5, torch.arange(5, 40))
    series[1, 4] = float("inf")
    with pytest.raises(ValueError, match="series.*gaps"):
        harness.train_series(None, "", {}, series, 5, torch.arange(5, 40), gaps=True)


def test_the_step_forms_and_wrappers_take_the_new_keywords():
    import inspect
    from gdn_amd import harness, ops
    for fn, names in ((harness.GraphedTrainStep, ["gaps"]), (harness.NativeTrainStep.__init__, ["gaps"]),
                      (harness.AutogradTrainStep.__init__, ["gaps"]), (harness.SeriesTrainer.__init__, ["gaps"]),
                      (harness.validate_series, ["valid"]), (harness.train_series, ["gaps"]),
                      (ops.windows_gather, ["valid", "valid_out", "row_valid"]),
                      (ops.mse_loss_grad, ["valid", "row_valid", "m_out"]), (ops.mse_batch_means, ["valid"])):
        params = inspect.signature(fn).parameters
        for name in names:
            assert name in params and params[name].default in (None, False), (fn, name)
