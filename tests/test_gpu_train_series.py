"""GPU suite of the epochs from the resident series: gdn_windows_gather against SeriesWindows.batch's indexing,
gdn_epoch_advance, gdn_mse_batch_means against its float64 restatement (tests/_train_series_ref.py, pinned on the CPU
by tests/test_cpu_train_series.py), and the loops built on them — SeriesTrainer / train_series against harness.train
fed by main.IndexLoader (bitwise: both hand the same step the same bits), validate_series against model(x)."""
import numpy as np
import pytest
import torch

import _train_series_ref as ref
from conftest import load_golden, meta

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the kernels
def _series(n, t, seed, device):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((n, t), generator=g).to(device)


def _ticks(w, series_len, batch, seed):
    """`batch` target ticks that include tick w and tick series_len - 1, a repeated tick and a descending stretch."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(w, series_len, (batch,), generator=g)
    fixed = [series_len - 1, w, w, series_len - 1][: batch]          # both ends, repeated, descending then ascending
    t[: len(fixed)] = torch.tensor(fixed)
    if batch >= 7:
        t[4:7] = torch.tensor([series_len - 2, series_len - 3, series_len - 4])
    return t.to(torch.int64)


def _indexed(series, at, w):
    """SeriesWindows.batch's expressions (gdn_amd/main.py)."""
    offs = torch.arange(-w, 0, device=series.device)
    cols = at.view(-1, 1) + offs.view(1, -1)
    return series[:, cols].permute(1, 0, 2).contiguous(), series[:, at].t().contiguous()


@pytest.mark.parametrize("n,w,series_len,batch", [(1, 1, 9, 1), (5, 3, 40, 7), (127, 15, 600, 64), (130, 65, 400, 3),
                                                  (33, 100, 1200, 5)])
def test_gather_equals_torch_indexing(n, w, series_len, batch, gpu_device):
    from gdn_amd import ops
    series = _series(n, series_len, 7 * n + w, gpu_device)
    at = _ticks(w, series_len, batch, n + batch).to(gpu_device)
    x = torch.full((batch, n, w), -7.0, device=gpu_device)
    y = torch.full((batch, n), -7.0, device=gpu_device)
    ops.windows_gather(series, at, batch, w, x, y)                  # cursor = NULL, first = 0
    want_x, want_y = _indexed(series, at, w)
    assert torch.equal(x, want_x) and torch.equal(y, want_y)


def test_gather_follows_the_cursor_and_first(gpu_device):
    from gdn_amd import ops
    n, w, series_len, batch = 5, 3, 40, 7
    series = _series(n, series_len, 3, gpu_device)
    table = _ticks(w, series_len, 4 * batch + 2, 9).to(gpu_device)
    cursor = torch.tensor([2], dtype=torch.int64, device=gpu_device)
    x = torch.empty((batch, n, w), device=gpu_device)
    y = torch.empty((batch, n), device=gpu_device)
    ops.windows_gather(series, table, batch, w, x, y, first=3, cursor=cursor)
    want_x, want_y = _indexed(series, table[3 + 2 * batch: 3 + 3 * batch], w)
    assert torch.equal(x, want_x) and torch.equal(y, want_y)
    assert int(cursor.item()) == 2                                  # the gather only reads it


def test_gather_writes_zeros_beyond_the_table_and_outside_the_series(gpu_device):
    from gdn_amd import ops
    n, w, series_len, batch = 5, 3, 40, 7
    series = _series(n, series_len, 4, gpu_device)
    table = _ticks(w, series_len, 10, 5).to(gpu_device)
    x = torch.full((batch, n, w), -7.0, device=gpu_device)
    y = torch.full((batch, n), -7.0, device=gpu_device)
    ops.windows_gather(series, table, batch, w, x, y, first=6)     # entries 6 .. 12 of a table of 10
    want_x, want_y = _indexed(series, table[6:10], w)
    assert torch.equal(x[:4], want_x) and torch.equal(y[:4], want_y)
    assert not x[4:].any() and not y[4:].any()
    # `count` shorter than the tensor, and ticks outside [w, series_len)
    bad = torch.tensor([w - 1, series_len, -5, 2 ** 40, w, series_len - 1, w + 1], dtype=torch.int64, device=gpu_device)
    x.fill_(-7.0), y.fill_(-7.0)
    ops.windows_gather(series, bad, batch, w, x, y, count=6)
    want_x, want_y = _indexed(series, bad[4:6], w)
    assert not x[:4].any() and not y[:4].any() and not x[6].any() and not y[6].any()
    assert torch.equal(x[4:6], want_x) and torch.equal(y[4:6], want_y)


def test_gather_offsets_are_64_bit(gpu_device):
    """n * series_len = 4096 * 524 300 > 2^31 elements: the smallest shape at which a 32-bit element offset wraps (in
    the last sensor's row, from column 475 148 on: both windows lie beyond it).  Only the columns that are read are
    filled."""
    from gdn_amd import ops
    n, series_len, w, batch = 4096, 524_300, 4, 2
    free, _total = torch.cuda.mem_get_info(gpu_device)
    if free < 10 * 2 ** 30:
        pytest.skip("less than 10 GB of device memory free")
    series = torch.empty((n, series_len), dtype=torch.float32, device=gpu_device)
    at = torch.tensor([series_len - 1, series_len - 3], dtype=torch.int64, device=gpu_device)
    g = torch.Generator().manual_seed(2)
    series[:, series_len - 8:] = torch.rand((n, 8), generator=g).to(gpu_device)
    x = torch.empty((batch, n, w), device=gpu_device)
    y = torch.empty((batch, n), device=gpu_device)
    ops.windows_gather(series, at, batch, w, x, y)
    want_x, want_y = _indexed(series, at, w)
    # the first element read of the last sensor's rows lies beyond what a signed 32-bit element offset reaches
    assert n * series_len > 2 ** 31 and (n - 1) * series_len + (series_len - 3 - w) > 2 ** 31 - 1
    assert torch.equal(x, want_x) and torch.equal(y, want_y)
    assert torch.equal(x[0, n - 1], series[n - 1, series_len - 5: series_len - 1])    # the last rows' far end


def test_epoch_advance_records_losses_and_moves_the_cursor(gpu_device):
    from gdn_amd import ops
    cursor = torch.zeros((1,), dtype=torch.int64, device=gpu_device)
    table = torch.full((4,), -1.0, device=gpu_device)
    loss = torch.zeros((), device=gpu_device)
    values = [0.5, 0.25, 3.0, 1e-3, 7.0]
    for v in values:                                                # the fifth launch finds r == table_len
        loss.fill_(v)
        ops.epoch_advance(loss, cursor, table)
    assert int(cursor.item()) == 5
    assert torch.equal(table.cpu(), torch.tensor(values[:4], dtype=torch.float32))


@pytest.mark.parametrize("rows,batch,n", [(70, 32, 5), (32, 32, 5)])
def test_mse_batch_means_equals_the_float64_restatement_bit_for_bit_twice(rows, batch, n, gpu_device):
    from gdn_amd import ops
    g = torch.Generator().manual_seed(rows + n)
    pred, y = torch.rand((rows, n), generator=g), torch.rand((rows, n), generator=g)
    want_means, want_mean = ref.mse_batch_means(pred.numpy(), y.numpy(), batch)
    runs = []
    for _ in range(2):
        means, mean = ops.mse_batch_means(pred.to(gpu_device), y.to(gpu_device), batch)
        runs.append((means.cpu(), mean.cpu()))
    assert runs[0][0].dtype == torch.float64 and runs[0][0].shape == (len(want_means),)
    np.testing.assert_allclose(runs[0][0].numpy(), want_means, rtol=1e-12, atol=0)
    np.testing.assert_allclose(float(runs[0][1]), want_mean, rtol=1e-12, atol=0)
    assert torch.equal(runs[0][0].view(torch.int64), runs[1][0].view(torch.int64))
    assert torch.equal(runs[0][1].view(torch.int64), runs[1][1].view(torch.int64))


# ------------------------------------------------------------------------------------------------ the loops
N, W, K, D, BATCH = 12, 5, 3, 16, 32


def _model(seed, device, p_drop=None, n=N, w=W, k=K, d=D, out_layer_num=1, inter=256):
    from gdn_amd import GDN
    torch.manual_seed(seed)
    model = GDN([torch.zeros((2, 1), dtype=torch.long)], n, dim=d, input_dim=w, topk=k, out_layer_num=out_layer_num,
                out_layer_inter_dim=inter)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        gnn = model.gnn_layers[0].gnn
        for t in (gnn.att_em_i, gnn.att_em_j):
            t.copy_(torch.rand(t.shape, generator=g) * 0.2 - 0.1)
    if p_drop is not None:
        model.dp.p = p_drop
    return model.to(device)


def _coupled_series(n, t, seed, device):
    """Sensors that follow one another with a lag (so that training and validation losses move), in [0, 1]."""
    rng = np.random.default_rng(seed)
    tt = np.arange(t)[None, :]
    phase = rng.uniform(0, 6.28, size=(n, 1))
    s = 0.5 + 0.35 * np.sin(0.11 * tt + phase) + 0.03 * rng.standard_normal((n, t))
    return torch.from_numpy(s.astype(np.float32)).to(device)


def _loaders(series, n_windows_val, device):
    """main.Main.get_loaders' pair over a SeriesWindows of stride 2: a contiguous validation block, the rest shuffled."""
    from gdn_amd.main import IndexLoader, SeriesWindows
    windows = SeriesWindows(series, torch.zeros(series.shape[1], dtype=torch.float64, device=device), W, 2, "train")
    idx = torch.arange(len(windows))
    val_idx = idx[60:60 + n_windows_val]
    train_idx = torch.cat([idx[:60], idx[60 + n_windows_val:]])
    return (windows, IndexLoader(windows, train_idx, BATCH, True, None),
            IndexLoader(windows, val_idx, BATCH, False, None) if n_windows_val else None)


def _state(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def _assert_same_state(a, b):
    assert a.keys() == b.keys()
    for key in a:
        assert torch.equal(a[key], b[key]), key


def _epoch_through_train(native, device):
    """Copy A: one epoch of harness.train fed by main.IndexLoader with the captured step."""
    from gdn_amd import harness
    series = _coupled_series(N, 343, 1, device)                     # ticks 5, 7, .. 341: 169 windows = 5 x 32 + 9
    windows, train_loader, _ = _loaders(series, 0, device)
    assert len(windows) == 169
    model = _model(21, device, p_drop=None if native else 0.0)
    assert harness.NativeTrainStep.applicable(model)
    torch.manual_seed(33)
    real = harness.GraphedTrainStep
    try:
        if not native:
            harness.GraphedTrainStep = lambda *a, **kw: real(*a, native=False, **kw)
        losses = harness.train(model, "", {"epoch": 1}, train_loader, None, use_graph=True)
    finally:
        harness.GraphedTrainStep = real
    return losses, _state(model)


def _epoch_through_trainer(native, use_graph, device):
    """Copy B: the same epoch through SeriesTrainer.epoch(epoch_order(...))."""
    from gdn_amd import harness
    series = _coupled_series(N, 343, 1, device)
    windows, train_loader, _ = _loaders(series, 0, device)
    model = _model(21, device, p_drop=None if native else 0.0)
    torch.manual_seed(33)
    starts = windows.starts[train_loader.loader.dataset.tensors[0].to(device)]
    trainer = harness.SeriesTrainer(model, series, W, starts, BATCH, lr=0.001, weight_decay=0, wide=False,
                                    use_graph=use_graph, native=None if native else False)
    assert isinstance(trainer.step, harness.NativeTrainStep if native else harness.AutogradTrainStep)
    losses = trainer.epoch(harness.epoch_order(train_loader.loader))
    return losses, _state(model)


@pytest.fixture(scope="module")
def epoch_a(gpu_device):
    return {native: _epoch_through_train(native, gpu_device) for native in (True, False)}


@pytest.mark.parametrize("native,use_graph", [(True, True), (True, False), (False, True)],
                         ids=["native-graph", "native-eager", "autograd-graph"])
def test_an_epoch_of_the_trainer_is_an_epoch_of_train_bit_for_bit(native, use_graph, epoch_a, gpu_device):
    """n = 12, w = 5, k = 3, d = 16, batch 32, 169 windows: five captured steps and a ragged tail of 9.  Both paths
    hand the same step the same bits, and the step is reproducible (no floating-point atomics; the autograd form with
    dropout 0 and fused Adam is too): every parameter, BatchNorm buffer and step loss is equal — for the captured
    trainer, for the native trainer launched eagerly, and for the autograd step (the hooks are captured there too)."""
    want_losses, want_state = epoch_a[native]
    losses, state = _epoch_through_trainer(native, use_graph, gpu_device)
    print("step losses:", want_losses, losses)
    assert len(want_losses) == 6 and losses == want_losses
    _assert_same_state(state, want_state)


@pytest.mark.parametrize("case", ["single", "mlp2"])
def test_validate_series_is_the_eval_loop(case, gpu_device):
    from gdn_amd import harness
    if case == "single":
        n, w, k, d, layers, inter = N, W, K, D, 1, 256
    else:
        m = meta(load_golden("mlp2_n20_w8_k6")[0])
        n, w, k, d, layers, inter = m["n"], m["w"], m["k"], m["d"], m["out_layer_num"], m["inter"]
        assert layers == 2
    model = _model(5, gpu_device, n=n, w=w, k=k, d=d, out_layer_num=layers, inter=inter).eval()
    series = _coupled_series(n, 300, 2, gpu_device)
    at = _ticks(w, 300, 70, 6).to(gpu_device)
    val_loss, pred, gt = harness.validate_series(model, series, at, 32)
    x, y = _indexed(series, at, w)
    with torch.no_grad():
        want = model(x, None)
    err = float((pred - want).abs().max())
    print(f"validate_series[{case}]: max|pred - model(x)| = {err:.3e}, val_loss = {val_loss!r}")
    assert err < 2e-5
    assert torch.equal(gt, y)
    _means, want_loss = ref.mse_batch_means(pred.cpu().numpy(), gt.cpu().numpy(), 32)
    np.testing.assert_allclose(val_loss, want_loss, rtol=1e-12, atol=0)


def test_train_series_is_train_over_three_epochs(gpu_device, tmp_path, monkeypatch):
    """Three epochs with a validation block: the same list of step losses and the same saved state_dict as
    harness.train fed by the index loaders, from the same seeds.  The validation losses (fp32 minibatch losses there,
    float64 means here) agree to 1e-6 relative, and no checkpoint decision lies within that band."""
    from gdn_amd import harness
    seen = {"train": [], "series": []}
    real_test, real_validate = harness.test, harness.validate_series

    def spy_test(*a, **kw):
        out = real_test(*a, **kw)
        seen["train"].append(out[0])
        return out

    def spy_validate(*a, **kw):
        out = real_validate(*a, **kw)
        seen["series"].append(out[0])
        return out

    monkeypatch.setattr(harness, "test", spy_test)
    monkeypatch.setattr(harness, "validate_series", spy_validate)
    runs = {}
    for which in ("train", "series"):
        series = _coupled_series(N, 423, 3, gpu_device)             # 209 windows: 40 for validation, 169 to train on
        _windows, train_loader, val_loader = _loaders(series, 40, gpu_device)
        model = _model(22, gpu_device)
        torch.manual_seed(44)
        path = str(tmp_path / f"best_{which}.pt")
        if which == "train":
            losses = harness.train(model, path, {"epoch": 3}, train_loader, val_loader, use_graph=True)
        else:
            losses = harness.train_series(model, path, {"epoch": 3}, series, W, train_loader, val_loader)
        runs[which] = (losses, torch.load(path, weights_only=True), _state(model), torch.rand(1))
    print("validation losses:", seen)
    assert len(runs["train"][0]) == 18 and runs["series"][0] == runs["train"][0]
    _assert_same_state(runs["series"][2], runs["train"][2])
    _assert_same_state(runs["series"][1], runs["train"][1])
    assert torch.equal(runs["series"][3], runs["train"][3])          # the generator ends where train() leaves it
    assert len(seen["train"]) == len(seen["series"]) == 3
    np.testing.assert_allclose(seen["series"], seen["train"], rtol=1e-6, atol=0)
    best = 1e8
    for v in seen["train"]:                                         # no `val_loss < min_loss` decision inside the band
        assert abs(v - best) > 4e-6 * max(v, best)
        best = min(best, v)
