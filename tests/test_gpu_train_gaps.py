"""GPU suite of training on a resident series with missing readings: gdn_windows_gather_gaps,
gdn_mse_loss_grad_masked and gdn_mse_batch_means_masked against the float64 restatement (tests/_train_gaps_ref.py,
pinned on the CPU by tests/test_cpu_train_gaps.py), and the layers above them — SeriesTrainer(gaps=True) against
gaps=False on a finite series (bitwise), captured against eager on a gappy one (bitwise), three steps against a loop of
plain torch, validate_series(valid=) and train_series(gaps=True)."""
import numpy as np
import pytest
import torch

import _train_gaps_ref as ref

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the gather
def _gappy(n, series_len, w, seed, share=0.15, length=3):
    """(raw, filled, valid) numpy of a random series with bursts of missing readings after its first w ticks."""
    clean = np.random.default_rng(seed).random((n, series_len), dtype=np.float32)
    raw = ref.burst_series(clean, w, share, min(length, series_len - w), seed=seed + 1)
    filled, valid = ref.fill(raw, w)
    return raw, filled, valid


def _gather_gpu(filled, valid, table, batch, w, dev, **kw):
    from gdn_amd import ops
    n = filled.shape[0]
    x = torch.full((batch, n, w), -7.0, device=dev)
    y = torch.full((batch, n), -7.0, device=dev)
    v = torch.full((batch, n), 9, dtype=torch.uint8, device=dev)
    rv = torch.full((batch,), -3, dtype=torch.int32, device=dev)
    ops.windows_gather(torch.from_numpy(filled).to(dev), table, batch, w, x, y, valid=torch.from_numpy(valid).to(dev),
                       valid_out=v, row_valid=rv, **kw)
    return x.cpu(), y.cpu(), v.cpu(), rv.cpu()


def _assert_gather(got, want):
    for name, g, wnt in zip(("x", "y", "valid_out", "row_valid"), got, want):
        assert g.dtype == torch.from_numpy(wnt).dtype and torch.equal(g, torch.from_numpy(wnt)), name


@pytest.mark.parametrize("n,w", [(1, 1), (5, 3), (17, 4), (130, 8), (4096, 1)])
def test_gather_with_validity_equals_numpy(n, w, gpu_device):
    """Batch 3.  (1, 1) the smallest shape; (5, 3) small and odd; (17, 4) rows of the plane start at any byte;
    (130, 8) 1040 flat elements = a second chunk, which must not write the validity row again; (4096, 1) the
    full-width count (one window's tick is complete: row_valid = 4096)."""
    series_len = w + 23
    _raw, filled, valid = _gappy(n, series_len, w, 7 * n + w)
    valid[series_len - 1 - w] = 1                                   # the first window's tick: every reading real
    valid[0, n // 2] = 0                                            # the second window's: at least one is not
    ticks = np.array([series_len - 1, w, w + 11], dtype=np.int64)
    want = ref.gather(filled, valid, ticks, w)
    assert want[3][0] == n and want[3][1] < n
    got = _gather_gpu(filled, valid, torch.from_numpy(ticks).to(gpu_device), 3, w, gpu_device)
    _assert_gather(got, want)


def test_gather_with_validity_follows_the_cursor_and_first(gpu_device):
    n, w, series_len, batch = 5, 3, 40, 7
    _raw, filled, valid = _gappy(n, series_len, w, 3)
    table = torch.randint(w, series_len, (4 * batch + 2,), generator=torch.Generator().manual_seed(9))
    cursor = torch.tensor([2], dtype=torch.int64, device=gpu_device)
    got = _gather_gpu(filled, valid, table.to(gpu_device), batch, w, gpu_device, first=3, cursor=cursor)
    _assert_gather(got, ref.gather(filled, valid, table[3 + 2 * batch: 3 + 3 * batch].numpy(), w))
    assert int(cursor.item()) == 2                                  # the gather only reads it


def test_gather_with_validity_writes_zeros_beyond_the_table_and_outside_the_series(gpu_device):
    n, w, series_len, batch = 5, 3, 40, 7
    _raw, filled, valid = _gappy(n, series_len, w, 4)
    table = torch.randint(w, series_len, (10,), generator=torch.Generator().manual_seed(5))
    got = _gather_gpu(filled, valid, table.to(gpu_device), batch, w, gpu_device, first=6)    # entries 6 .. 12 of 10
    _assert_gather(got, ref.gather(filled, valid, table[6:10].numpy(), w, batch=batch))
    assert not got[2][4:].any() and not got[3][4:].any()
    bad = torch.tensor([w - 1, series_len, -5, 2 ** 40, w, series_len - 1, w + 1], dtype=torch.int64)
    got = _gather_gpu(filled, valid, bad.to(gpu_device), batch, w, gpu_device, count=6)
    _assert_gather(got, ref.gather(filled, valid, bad[:6].numpy(), w, batch=batch))
    assert not got[2][:4].any() and not got[3][:4].any() and not got[2][6].any() and int(got[3][6]) == 0


def test_gather_plane_offsets_are_64_bit(gpu_device):
    """(series_len - w) * n = 524 296 * 4096 bytes > 2^31: the validity rows of both windows start beyond what a signed
    32-bit byte offset reaches.  tests/test_gpu_train_series.py::test_gather_offsets_are_64_bit's shape and memory
    guard (the plane adds 2 GB); only the columns and rows that are read are filled."""
    from gdn_amd import ops
    n, series_len, w, batch = 4096, 524_300, 4, 2
    free, _total = torch.cuda.mem_get_info(gpu_device)
    if free < 13 * 2 ** 30:
        pytest.skip("less than 13 GB of device memory free")
    series = torch.empty((n, series_len), dtype=torch.float32, device=gpu_device)
    plane = torch.empty((series_len - w, n), dtype=torch.uint8, device=gpu_device)
    g = torch.Generator().manual_seed(2)
    series[:, series_len - 8:] = torch.rand((n, 8), generator=g).to(gpu_device)
    tail = (torch.rand((8, n), generator=g) < 0.7).to(torch.uint8)
    plane[series_len - w - 8:] = tail.to(gpu_device)
    at = torch.tensor([series_len - 1, series_len - 3], dtype=torch.int64, device=gpu_device)
    x = torch.empty((batch, n, w), device=gpu_device)
    y = torch.empty((batch, n), device=gpu_device)
    v = torch.full((batch, n), 9, dtype=torch.uint8, device=gpu_device)
    rv = torch.full((batch,), -3, dtype=torch.int32, device=gpu_device)
    ops.windows_gather(series, at, batch, w, x, y, valid=plane, valid_out=v, row_valid=rv)
    assert (series_len - 3 - w) * n > 2 ** 31 - 1
    assert torch.equal(v.cpu(), torch.stack([tail[7], tail[5]]))
    assert rv.cpu().tolist() == [int(tail[7].sum()), int(tail[5].sum())]
    assert torch.equal(y, series[:, at].t())


# ------------------------------------------------------------------------------------------------ the masked loss
def _loss_case(shape, seed, share=0.1):
    g = torch.Generator().manual_seed(seed)
    out, y = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    size = shape[0] * shape[1]
    v = torch.from_numpy(ref.burst_mask(shape, share, min(5, max(1, size // 2)), seed=seed))
    return out, y, v


@pytest.mark.parametrize("shape", [(1, 2), (3, 7), (512, 127), (4096, 127)])
def test_masked_loss_and_gradient_against_float64_autograd(shape, gpu_device):
    """About 10 % of the targets missing in bursts, y = inf and out = nan planted in every masked slot; the workspace is
    reused three times and ends zeroed.  Bounds of test_fused_mse_loss_and_gradient."""
    from gdn_amd import ops
    ws = ops.mse_workspace(gpu_device)
    m_out = torch.full((), -1, dtype=torch.int64, device=gpu_device)
    for rep in range(3):
        out, y, v = _loss_case(shape, 10 * shape[0] + rep)
        assert 0 < int(v.sum()) < v.numel()
        out[v == 0], y[v == 0] = float("nan"), float("inf")
        want_loss, want_grad = ref.masked_loss_autograd(out.numpy(), y.numpy(), v.numpy())
        rv = v.sum(dim=1).to(torch.int32)
        loss, d_out = ops.mse_loss_grad(out.to(gpu_device), y.to(gpu_device), ws, valid=v.to(gpu_device),
                                        row_valid=rv.to(gpu_device), m_out=m_out)
        d_out = d_out.cpu()
        print(f"masked loss {shape} rep {rep}: hip {float(loss)!r} float64 {want_loss!r} m {int(m_out)}")
        assert int(m_out) == int(v.sum())
        np.testing.assert_allclose(float(loss), want_loss, rtol=2e-7, atol=0)
        np.testing.assert_allclose(d_out.numpy(), want_grad, rtol=1e-6, atol=1e-12)
        assert bool((d_out[v == 0] == 0.0).all()) and bool(torch.isfinite(d_out).all())
    assert float(ws.abs().sum()) >= 0 and int(ws.view(torch.int64)[0]) == 0


@pytest.mark.parametrize("shape", [(1, 2), (3, 7), (512, 127), (4096, 127)])
def test_masked_loss_all_valid_is_the_plain_launch_none_valid_is_zero_and_both_repeat(shape, gpu_device):
    from gdn_amd import ops
    ws = ops.mse_workspace(gpu_device)
    out, y, v = (t.to(gpu_device) for t in _loss_case(shape, 77 + shape[0]))
    ones = torch.ones(shape, dtype=torch.uint8, device=gpu_device)
    full = torch.full((shape[0],), shape[1], dtype=torch.int32, device=gpu_device)
    plain_loss, plain_grad = ops.mse_loss_grad(out, y, ws)
    loss, d_out = ops.mse_loss_grad(out, y, ws, valid=ones, row_valid=full)
    assert torch.equal(loss.view(torch.int32), plain_loss.view(torch.int32))
    assert torch.equal(d_out.view(torch.int32), plain_grad.view(torch.int32))
    m_out = torch.full((), -1, dtype=torch.int64, device=gpu_device)
    loss, d_out = ops.mse_loss_grad(out, y, ws, valid=torch.zeros_like(ones), row_valid=torch.zeros_like(full), m_out=m_out)
    assert float(loss) == 0.0 and not d_out.any() and int(m_out) == 0
    rv = v.sum(dim=1).to(torch.int32)
    a = ops.mse_loss_grad(out, y, ws, valid=v, row_valid=rv)
    b = ops.mse_loss_grad(out, y, ws, valid=v, row_valid=rv)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


@pytest.mark.parametrize("rows,batch,n", [(7, 3, 5), (1000, 128, 27)])
def test_masked_batch_means_equal_the_float64_restatement_and_repeat(rows, batch, n, gpu_device):
    from gdn_amd import ops
    g = torch.Generator().manual_seed(rows + n)
    pred, y = torch.rand((rows, n), generator=g), torch.rand((rows, n), generator=g)
    v = torch.from_numpy(ref.burst_mask((rows, n), 0.1, 4, seed=rows))
    v[batch:2 * batch] = 0                                          # minibatch 1 has no real target
    pred[v == 0], y[v == 0] = float("nan"), float("inf")
    want_means, want_counts, want_mean = ref.masked_batch_means(pred.numpy(), y.numpy(), v.numpy(), batch)
    assert want_counts[1] == 0 and (want_counts[[0, 2]] > 0).all()
    runs = [tuple(t.cpu() for t in ops.mse_batch_means(pred.to(gpu_device), y.to(gpu_device), batch,
                                                       valid=v.to(gpu_device))) for _ in range(2)]
    means, mean, counts = runs[0]
    assert means.dtype == torch.float64 and counts.dtype == torch.int64 and means.shape == (len(want_means),)
    assert counts.tolist() == want_counts.tolist() and float(means[1]) == 0.0
    np.testing.assert_allclose(means.numpy(), want_means, rtol=1e-12, atol=0)
    np.testing.assert_allclose(float(mean), want_mean, rtol=1e-12, atol=0)
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    none = ops.mse_batch_means(pred.to(gpu_device), y.to(gpu_device), batch, valid=torch.zeros_like(v).to(gpu_device))
    assert float(none[1]) == 0.0 and not none[2].any()


# ------------------------------------------------------------------------------------------------ the loops
N, W, K, D, BATCH = 12, 5, 3, 16, 32          # the small model of tests/test_gpu_train_series.py


def _model(seed, device, p_drop=None):
    from gdn_amd import GDN
    torch.manual_seed(seed)
    model = GDN([torch.zeros((2, 1), dtype=torch.long)], N, dim=D, input_dim=W, topk=K, out_layer_num=1)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        gnn = model.gnn_layers[0].gnn
        for t in (gnn.att_em_i, gnn.att_em_j):
            t.copy_(torch.rand(t.shape, generator=g) * 0.2 - 0.1)
    if p_drop is not None:
        model.dp.p = p_drop
    return model.to(device)


def _coupled_series(n, t, seed):
    """Sensors that follow one another with a lag, in [0, 1] (numpy fp32)."""
    rng = np.random.default_rng(seed)
    tt = np.arange(t)[None, :]
    s = 0.5 + 0.35 * np.sin(0.11 * tt + rng.uniform(0, 6.28, size=(n, 1))) + 0.03 * rng.standard_normal((n, t))
    return s.astype(np.float32)


T_LEN = 343
STARTS = torch.arange(W, T_LEN, 2)                                  # ticks 5, 7, .. 341: 169 windows = 5 x 32 + 9
ALL_GONE = 105                                                      # a training tick whose n readings are all missing


def _gappy_training_series(fill_value=float("nan")):
    """About 2 % of the readings missing in bursts of 8, the first W columns clean, every reading of tick ALL_GONE gone."""
    raw = ref.burst_series(_coupled_series(N, T_LEN, 1), W, 0.02, 8, seed=11)
    raw[:, ALL_GONE] = np.nan
    assert not ref.missing(raw)[:, :W].any() and 0.01 < ref.missing(raw).mean() < 0.04
    raw[ref.missing(raw)] = fill_value
    return raw


def _order(total):
    return torch.randperm(STARTS.numel(), generator=torch.Generator().manual_seed(5))[:total]


def _epoch(series_np, device, native, use_graph, gaps, total=169, p_drop=None, seed=21):
    """One SeriesTrainer.epoch over `total` shuffled windows; returns (losses, everything the epoch leaves behind)."""
    from gdn_amd import harness
    model = _model(seed, device, p_drop=p_drop if native else 0.0)
    torch.manual_seed(33)
    extra = {"gaps": True} if gaps else {}
    trainer = harness.SeriesTrainer(model, torch.from_numpy(series_np).to(device), W, STARTS, BATCH, lr=0.001,
                                    weight_decay=0, wide=False, use_graph=use_graph, native=None if native else False,
                                    **extra)
    assert isinstance(trainer.step, harness.NativeTrainStep if native else harness.AutogradTrainStep)
    losses = trainer.epoch(_order(total))
    left = {"model/" + k: v.detach().clone() for k, v in model.state_dict().items()}
    if native:
        left.update(exp_avg=trainer.step.exp_avg.clone(), exp_avg_sq=trainer.step.exp_avg_sq.clone(),
                    steps=trainer.step.state.clone())
    else:
        for i, p in enumerate(model.parameters()):
            for key, val in trainer.optimizer.state[p].items():
                left[f"adam/{i}/{key}"] = val.detach().clone()
    return losses, left, trainer


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for key in a:
        assert torch.equal(a[key], b[key]), key


@pytest.mark.parametrize("native,use_graph", [(True, True), (True, False), (False, True), (False, False)],
                         ids=["native-graph", "native-eager", "autograd-graph", "autograd-eager"])
def test_on_a_finite_series_an_epoch_with_gaps_writes_the_bits_of_one_without(native, use_graph, gpu_device):
    """Contract point 4: five steps of 32 windows, every validity byte set — parameters, BatchNorm buffers, Adam state
    and step losses are equal bit for bit."""
    series = _coupled_series(N, T_LEN, 1)
    want_losses, want, _ = _epoch(series, gpu_device, native, use_graph, gaps=False, total=160)
    losses, got, trainer = _epoch(series, gpu_device, native, use_graph, gaps=True, total=160)
    print("step losses:", want_losses, losses)
    assert len(losses) == 5 and losses == want_losses
    _assert_same(got, want)
    total, run = trainer.status_gaps()
    assert not total.any() and not run.any() and torch.equal(trainer.series, trainer.raw_series)
    assert bool(trainer.step.valid.all()) and trainer.step.row_valid.tolist() == [N] * BATCH


def test_on_a_finite_series_the_ragged_tail_with_gaps_is_the_eager_tail(gpu_device):
    """169 windows: the five captured steps as above, then a tail of 9 windows.  Without gaps the tail's loss is torch's
    fp32 reduction (F.mse_loss), with gaps the masked launch's float64 accumulation rounded once: the same gradient
    formula, two roundings of the loss.  Bound on the tail's loss: torch adds 108 fp32 squares pairwise, an error of at
    most about log2(108) + 2 = 9 roundings of 2^-24 = 5.4e-7 relative; 1e-6.  Bound on the parameters: one Adam step
    moves a parameter by at most lr = 1e-3, and a gradient that differs by 1e-6 relative (the bound of the gradient
    test) moves that by less than 1e-9; 1e-7 absolute."""
    series = _coupled_series(N, T_LEN, 1)
    want_losses, want, _ = _epoch(series, gpu_device, True, True, gaps=False)
    losses, got, _ = _epoch(series, gpu_device, True, True, gaps=True)
    print("step losses:", want_losses, losses)
    assert len(losses) == 6 and losses[:5] == want_losses[:5]
    np.testing.assert_allclose(losses[5], want_losses[5], rtol=1e-6, atol=0)
    for key in want:
        if want[key].is_floating_point():
            worst = float((got[key] - want[key]).abs().max())
            print(f"tail: max|gaps - plain| of {key} = {worst:.3e}")
            assert worst <= 1e-7, key


@pytest.fixture(scope="module")
def gappy_runs(gpu_device):
    """The gappy epoch (169 windows, tail included) once per step form and launch mode, shared by the tests below."""
    raw = _gappy_training_series()
    return {(native, use_graph): _epoch(raw, gpu_device, native, use_graph, gaps=True, p_drop=None)
            for native in (True, False) for use_graph in (True, False)}


@pytest.mark.parametrize("native", [True, False], ids=["native", "autograd"])
def test_on_a_gappy_series_the_captured_epoch_is_the_eager_epoch(native, gappy_runs, gpu_device):
    losses, left, trainer = gappy_runs[(native, True)]
    eager_losses, eager_left, _ = gappy_runs[(native, False)]
    print("step losses:", losses, eager_losses)
    assert len(losses) == 6 and all(np.isfinite(losses)) and losses == eager_losses
    _assert_same(left, eager_left)
    for key, val in left.items():
        assert bool(torch.isfinite(val).all()), key
    # the step's validity bytes after the last replay: the plane's rows of the last full batch's ticks
    ticks = STARTS[_order(169)][4 * BATCH: 5 * BATCH].to(gpu_device)
    raw = _gappy_training_series()
    filled, valid = ref.fill(raw, W)
    assert torch.equal(trainer.valid.cpu(), torch.from_numpy(valid)) and torch.equal(trainer.series.cpu(), torch.from_numpy(filled))
    assert torch.equal(trainer.step.valid, trainer.valid[ticks - W])
    assert torch.equal(trainer.step.row_valid, trainer.valid[ticks - W].sum(dim=1).to(torch.int32))
    assert torch.equal(trainer.step.y, trainer.series[:, ticks].t())
    total, _run = trainer.status_gaps()
    assert total.tolist() == ref.missing(raw)[:, W:].sum(axis=1).tolist()
    assert ALL_GONE in STARTS[_order(169)].tolist() and not valid[ALL_GONE - W].any()


def test_on_a_gappy_series_what_a_missing_reading_holds_changes_no_bit(gappy_runs, gpu_device):
    losses, left, _ = gappy_runs[(True, True)]
    inf_losses, inf_left, _ = _epoch(_gappy_training_series(float("inf")), gpu_device, True, True, gaps=True)
    assert inf_losses == losses
    _assert_same(inf_left, left)


def _distance(model, other, init, losses, other_losses):
    """(parameters, losses): the l2 norm of the difference over all parameters relative to the l2 norm of what the
    three steps moved them by, and the largest relative difference of a step loss.  A norm and not a maximum: Adam's
    first steps move a parameter by about lr * sign(gradient), so single elements whose gradient is rounding noise
    differ by up to 2 lr in any two fp32 implementations, and a maximum would measure only those."""
    with torch.no_grad():
        per = [(name, float(((p - q) ** 2).sum()), float(((q - i) ** 2).sum()))
               for (name, p), q, i in zip(model.named_parameters(), other.parameters(), init)]
    print("  per tensor, |native - torch| / |torch - init|:",
          ", ".join(f"{name} {(a / b) ** 0.5 if b else 0.0:.1e}" for name, a, b in per))
    num, den = sum(a for _n, a, _b in per), sum(b for _n, _a, b in per)
    rel = max(abs(a - b) / abs(b) for a, b in zip(losses, other_losses))
    return (num / den) ** 0.5, rel


def _three_steps(series_np, device, gaps):
    """Three native captured steps of SeriesTrainer against three steps of plain torch on the same windows: x, y and v
    cut by torch indexing from the numpy fill, the masked mean written out, loss.backward(), torch.optim.Adam."""
    from gdn_amd import harness
    filled_np, valid_np = ref.fill(series_np, W)
    order = _order(3 * BATCH)
    model = _model(21, device, p_drop=0.0)
    extra = {"gaps": True} if gaps else {}
    trainer = harness.SeriesTrainer(model, torch.from_numpy(series_np).to(device), W, STARTS, BATCH, lr=0.001,
                                    weight_decay=0, wide=False, use_graph=True, **extra)
    assert isinstance(trainer.step, harness.NativeTrainStep)
    losses = trainer.epoch(order)
    other = _model(21, device, p_drop=0.0).train()
    init = [p.detach().clone() for p in other.parameters()]
    adam = torch.optim.Adam(other.parameters(), lr=0.001)
    filled, plane = torch.from_numpy(filled_np).to(device), torch.from_numpy(valid_np).to(device)
    offs = torch.arange(-W, 0, device=device)
    other_losses = []
    for s in range(3):
        at = STARTS[order[s * BATCH:(s + 1) * BATCH]].to(device)
        x = filled[:, at.view(-1, 1) + offs.view(1, -1)].permute(1, 0, 2).contiguous()
        y = filled[:, at].t().contiguous()
        adam.zero_grad()
        with harness.pinned_range(other, False):
            out = other(x, None)
        if gaps:
            v = plane[at - W].to(torch.float32)
            loss = ((out - y) ** 2 * v).sum() / v.sum()
        else:
            loss = torch.nn.functional.mse_loss(out, y, reduction="mean")
        loss.backward()
        adam.step()
        other_losses.append(float(loss.detach()))
    return _distance(model, other, init, losses, other_losses)


def test_three_gappy_steps_against_plain_torch_within_twice_the_finite_distance(gpu_device):
    """The yardstick is no code of the change.  Its bound is not invented: the distance between gaps=False native steps
    and the same torch loop with F.mse_loss on the FINITE series is measured first, here, on this device; the gappy
    steps (gaps=True against the masked mean in torch) may lie twice as far.  DESIGN §3.4c records both."""
    base = _three_steps(_coupled_series(N, T_LEN, 1), gpu_device, gaps=False)
    dist = _three_steps(_gappy_training_series(), gpu_device, gaps=True)
    print(f"native against torch, finite gaps=False: parameters {base[0]:.3e} losses {base[1]:.3e}; "
          f"gappy gaps=True: parameters {dist[0]:.3e} losses {dist[1]:.3e}")
    assert dist[0] <= 2 * base[0] and dist[1] <= 2 * base[1]


def test_validate_series_with_the_plane(gpu_device):
    from gdn_amd import harness
    raw = _gappy_training_series()
    filled_np, valid_np = ref.fill(raw, W)
    filled, plane = torch.from_numpy(filled_np).to(gpu_device), torch.from_numpy(valid_np).to(gpu_device)
    model = _model(5, gpu_device).eval()
    at = torch.cat([torch.arange(ALL_GONE - 30, ALL_GONE + 40), torch.tensor([T_LEN - 1, W])])      # 72 = 2 x 32 + 8
    _plain_loss, want_pred, want_gt = harness.validate_series(model, filled, at, 32)
    val_loss, pred, gt = harness.validate_series(model, filled, at, 32, valid=plane)
    assert torch.equal(pred, want_pred) and torch.equal(gt, want_gt)
    v = valid_np[at.numpy() - W]
    assert 0 < v.sum() < v.size
    _means, _counts, want = ref.masked_batch_means(pred.cpu().numpy(), gt.cpu().numpy(), v, 32)
    print(f"validate_series(valid=): {val_loss!r} against {want!r}; without the plane {_plain_loss!r}")
    np.testing.assert_allclose(val_loss, want, rtol=1e-12, atol=0)
    empty = torch.tensor([ALL_GONE] * 3)                            # no minibatch has a real target
    assert harness.validate_series(model, filled, empty, 2, valid=plane)[0] == 0.0


def test_train_series_with_gaps_runs_to_the_end_and_without_them_yields_nan(gpu_device, tmp_path):
    """Two epochs with a validation block on the gappy series: finite losses and a finite saved state_dict.  The same
    call with gaps=False on the raw series yields NaN losses — why the feature exists."""
    from gdn_amd import harness
    raw = torch.from_numpy(_gappy_training_series()).to(gpu_device)
    val = STARTS[60:100]
    train = torch.cat([STARTS[:60], STARTS[100:]])
    assert ALL_GONE in train.tolist() and bool(torch.isnan(raw[:, val]).any())
    path = str(tmp_path / "best.pt")
    torch.manual_seed(44)
    losses = harness.train_series(_model(22, gpu_device), path, {"epoch": 2, "batch": BATCH}, raw, W, train, val, gaps=True)
    assert len(losses) == 2 * 5 and all(np.isfinite(losses))        # 129 windows: four steps of 32 and a tail of 1
    saved = torch.load(path, weights_only=True)
    assert all(bool(torch.isfinite(t).all()) for t in saved.values() if t.is_floating_point())
    torch.manual_seed(44)
    nan_losses = harness.train_series(_model(22, gpu_device), "", {"epoch": 2, "batch": BATCH}, raw, W, train, val, gaps=False)
    assert len(nan_losses) == 10 and bool(np.isnan(nan_losses).any()) and np.isnan(nan_losses[-1])
    torch.manual_seed(44)
    by_config = harness.train_series(_model(22, gpu_device), "", {"epoch": 2, "batch": BATCH, "train_gaps": True}, raw, W,
                                     train, val)
    assert by_config == losses                                      # gaps=None takes config["train_gaps"]
