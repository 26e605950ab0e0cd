"""CPU suite of the epochs-from-the-resident-series entry points (gdn_windows_gather, gdn_epoch_advance,
gdn_mse_batch_means; harness.epoch_order): the C-ABI surface, the host-side refusals (decided before any launch, so no
device is needed), the epoch order against an iterated DataLoader, and the float64 yardstick of the GPU tests
(tests/_train_series_ref.py) against harness.test's formula."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader, TensorDataset

import _train_series_ref as ref
from conftest import ROOT

FAKE = 4096          # a non-null, 16-byte aligned address that is never dereferenced on the host
NEW = ["gdn_windows_gather", "gdn_epoch_advance", "gdn_mse_batch_means"]


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
    assert _lib.SIGNATURES["gdn_windows_gather"] == [p, i, ll, p, ll, p, ll, i, i, p, p, p]
    assert _lib.SIGNATURES["gdn_epoch_advance"] == [p, p, p, ll, p]
    assert _lib.SIGNATURES["gdn_mse_batch_means"] == [p, p, ll, i, ll, p, p, p, p]
    from gdn_amd import harness, ops
    assert all(callable(getattr(ops, f)) for f in ("windows_gather", "epoch_advance", "mse_batch_means"))
    assert all(callable(getattr(harness, f)) for f in ("epoch_order", "validate_series", "SeriesTrainer", "train_series"))


def _gather(**kw):
    from gdn_amd import _lib
    a = dict(series=FAKE, n=127, series_len=1000, starts=FAKE, count=64, cursor=None, first=0, batch=64, w=15,
             x=FAKE, y=FAKE)
    a.update(kw)
    return _lib.load().gdn_windows_gather(a["series"], a["n"], a["series_len"], a["starts"], a["count"], a["cursor"],
                                          a["first"], a["batch"], a["w"], a["x"], a["y"], None)


@pytest.mark.parametrize("bad", [dict(series=None), dict(starts=None), dict(x=None), dict(y=None), dict(batch=0),
                                 dict(batch=-3), dict(w=0), dict(w=1025), dict(n=0), dict(n=4097), dict(count=0)])
def test_windows_gather_refuses_before_any_launch(bad):
    assert _gather(**bad) != 0


@pytest.mark.parametrize("bad", [dict(loss=None), dict(cursor=None), dict(table=None), dict(table_len=0)])
def test_epoch_advance_refuses_before_any_launch(bad):
    from gdn_amd import _lib
    a = dict(loss=FAKE, cursor=FAKE, table=FAKE, table_len=8)
    a.update(bad)
    assert _lib.load().gdn_epoch_advance(a["loss"], a["cursor"], a["table"], a["table_len"], None) != 0


@pytest.mark.parametrize("bad", [dict(pred=None), dict(y=None), dict(means=None), dict(mean=None), dict(batch=0),
                                 dict(n=0), dict(n=4097), dict(rows=0)])
def test_mse_batch_means_refuses_before_any_launch(bad):
    from gdn_amd import _lib
    a = dict(pred=FAKE, y=FAKE, rows=70, n=5, batch=32, means=FAKE, mean=FAKE)
    a.update(bad)
    assert _lib.load().gdn_mse_batch_means(a["pred"], a["y"], a["rows"], a["n"], a["batch"], a["means"], a["mean"],
                                           None, None) != 0


@pytest.mark.parametrize("shuffle", [True, False])
def test_epoch_order_is_the_order_and_the_draws_of_an_iterated_loader(shuffle):
    from gdn_amd import harness
    idx = torch.arange(1000, 1000 + 169)             # 169: five batches of 32 and a ragged one of 9
    def loader():
        return DataLoader(TensorDataset(idx), batch_size=32, shuffle=shuffle, num_workers=0)
    torch.manual_seed(11)
    want_loader = loader()
    want = [torch.cat([b for (b,) in want_loader]) for _epoch in range(3)]
    want_next = torch.rand(1)
    torch.manual_seed(11)
    got_loader = loader()
    got = [harness.epoch_order(got_loader) for _epoch in range(3)]
    got_next = torch.rand(1)
    for g, wnt in zip(got, want):
        assert g.dtype == torch.int64 and g.shape == (169,)
        assert torch.equal(idx[g], wnt)
    assert torch.equal(got_next, want_next)
    if shuffle:
        assert not torch.equal(got[0], got[1]) and sorted(got[0].tolist()) == list(range(169))
    else:
        assert torch.equal(got[0], torch.arange(169))


@pytest.mark.parametrize("rows,batch,n", [(70, 32, 5), (32, 32, 5), (7, 3, 1), (200, 64, 27)])
def test_mse_restatement_equals_the_eval_loop_formula(rows, batch, n):
    """tests/_train_series_ref.mse_batch_means against harness.test's arithmetic (test.py:43-62: F.mse_loss per
    minibatch, sum(losses) / len(losses)) carried out in float64 on the fp32 differences: 1e-12 relative, the
    project's bar for float64 scoring arithmetic."""
    g = torch.Generator().manual_seed(rows * 131 + batch)
    pred, y = torch.rand((rows, n), generator=g), torch.rand((rows, n), generator=g)
    losses = []
    for s in range(0, rows, batch):
        diff = pred[s:s + batch] - y[s:s + batch]                           # fp32, as F.mse_loss forms it
        losses.append(F.mse_loss(diff.double(), torch.zeros_like(diff, dtype=torch.float64), reduction="mean"))
    want = float(torch.stack(losses).sum().item() / len(losses))
    means, mean = ref.mse_batch_means(pred.numpy(), y.numpy(), batch)
    np.testing.assert_allclose(means, torch.stack(losses).numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(mean, want, rtol=1e-12, atol=0)
    # and harness.test's own fp32 losses are this number to fp32 rounding
    fp32 = [F.mse_loss(pred[s:s + batch], y[s:s + batch], reduction="mean") for s in range(0, rows, batch)]
    np.testing.assert_allclose(float(torch.stack(fp32).double().sum().item() / len(fp32)), mean, rtol=1e-6)


def test_windows_restatement_is_series_windows_batch():
    """The gather's yardstick is SeriesWindows.batch's indexing (gdn_amd/main.py) on the host."""
    from gdn_amd.main import SeriesWindows
    series = torch.rand((5, 40))
    win = SeriesWindows(series, torch.zeros(40, dtype=torch.float64), 3, 2, "train")
    pos = torch.tensor([0, 7, 7, 18, 3])
    x, y, _lab = win.batch(pos)
    rx, ry = ref.windows(series.numpy(), win.starts[pos].numpy(), 3)
    assert np.array_equal(x.numpy(), rx) and np.array_equal(y.numpy(), ry)


def test_train_series_refuses_more_than_one_rank(monkeypatch):
    from gdn_amd import _lib, harness
    monkeypatch.setattr(harness, "world", lambda: (0, 2))
    with pytest.raises(_lib.GdnHipError, match="one process"):
        harness.train_series(model=None, series=None, train_loader_or_indices=torch.arange(5, 9))
