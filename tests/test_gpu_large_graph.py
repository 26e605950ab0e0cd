"""GPU suite: graphs beyond the LDS tile (up to 4096 sensors).  Where the window's projected tile does not fit
one CU's LDS, gdn_project_fwd / gdn_attn_aggregate_fwd / gdn_attn_aggregate_bwd run the large-graph kernels
(gather from global memory) and GDN's eval forward takes the staged route; training goes through autograd.
Everything here was refused with GDN_ERR_UNSUPPORTED before those kernels existed (except the head-bound test,
which pins the exact-sum bound of the train-mode head at the largest chunk count)."""
import copy

import numpy as np
import pytest
import torch

from _graph_build_ref import clear_rows
from oracle import gdn_oracle
from test_gpu_forward_parity import random_params
from test_gpu_train_parity import FixedMaskDropout

pytestmark = pytest.mark.gpu

SHAPES = [(700, 15, 30, 64),      # just past the d = 64 tile
          (1024, 30, 64, 128),    # refused by the native training step
          (2500, 10, 20, 16),     # past the d = 16 tile
          (4096, 5, 16, 32)]      # the cap
IDS = ["n{}_w{}_k{}_d{}".format(*s) for s in SHAPES]
F64 = torch.float64


def _model(n, w, k, d, dev, seed=31, out_layer_num=1):
    model = random_params(n, w, k, d, seed=seed, out_layer_num=out_layer_num)
    p = {key: v.detach().clone() for key, v in model.state_dict().items()}
    return model.to(dev), p


def _p64(p):
    return {key: (v.to(F64) if v.is_floating_point() else v) for key, v in p.items()}


_clear_rows = clear_rows      # float64 cosine ranking: rows with a clear k-th / (k+1)-th gap, the top-k sets


def test_predicate_and_native_step_stay_on_the_tile(gpu_device):
    from gdn_amd import _lib, harness
    lib = _lib.load()
    for n, w, k, d in SHAPES:
        assert lib.gdn_tile_fits(n, w, d, k) == 0
        assert lib.gdn_train_supported(n, w, d, k) == 0
    assert lib.gdn_tile_fits(512, 30, 64, 64) == 1
    model, _ = _model(700, 15, 30, 64, gpu_device)
    assert not harness.NativeTrainStep.applicable(model)
    assert not model.eval().fused_keys_supported()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_eval_forward_and_attention_against_float64_oracle(shape, gpu_device):
    n, w, k, d = shape
    b = 2
    model, p = _model(n, w, k, d, gpu_device)
    model.eval()
    x = torch.rand((b, n, w), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        out = model(x.to(gpu_device), None)
    graph = model.learned_graph.cpu()
    clear, sets = _clear_rows(p["embedding.weight"], k)
    assert clear.float().mean() > 0.9
    got = torch.sort(graph, dim=1).values
    want = torch.sort(sets, dim=1).values
    assert torch.equal(got[clear], want[clear])
    ref = gdn_oracle.forward(_p64(p), x.to(F64), k, graph=graph)
    err = float((out.cpu().to(F64) - ref["out"]).abs().max())
    assert err < 2e-5, err
    # attention weights in edge_index_1 order; each target's weights sum to 1
    layer = model.gnn_layers[0]
    att = layer.att_weight_1.view(-1).cpu().to(F64)
    ei = layer.edge_index_1.cpu()
    assert torch.equal(ei, ref["edge_index_1"])
    np.testing.assert_allclose(att.numpy(), ref["att_weight_1"].view(-1).numpy(), atol=2e-6, rtol=0)
    sums = torch.zeros(b * n, dtype=F64).index_add_(0, ei[1], att)
    np.testing.assert_allclose(sums.numpy(), 1.0, atol=1e-5)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=[IDS[0], IDS[2]])
def test_eval_forward_with_mlp_head(shape, gpu_device):
    n, w, k, d = shape
    model, p = _model(n, w, k, d, gpu_device, out_layer_num=2)
    model.eval()
    x = torch.rand((2, n, w), generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        out = model(x.to(gpu_device), None)
    ref = gdn_oracle.forward(_p64(p), x.to(F64), k, 2, graph=model.learned_graph.cpu())
    err = float((out.cpu().to(F64) - ref["out"]).abs().max())
    assert err < 2e-5, err


def test_bf16_windows_are_refused_with_a_reason(gpu_device):
    from gdn_amd import _lib
    model, _ = _model(700, 15, 30, 64, gpu_device)
    model.eval()
    x = torch.rand((2, 700, 15), device=gpu_device).bfloat16()
    with pytest.raises(_lib.GdnHipError, match="LDS tile"):
        with torch.no_grad():
            model(x, None)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_kernels_are_bitwise_reproducible(shape, gpu_device):
    from gdn_amd import ops
    n, w, k, d = shape
    b = 3
    model, _ = _model(n, w, k, d, gpu_device)
    model.train()
    gnn = model.gnn_layers[0].gnn
    g = torch.Generator().manual_seed(8)
    x = torch.rand((b, n, w), generator=g).to(gpu_device)
    y = torch.rand((b, n), generator=g).to(gpu_device)
    mask = ((torch.rand((b, n, d), generator=g) >= 0.2).float() / 0.8).to(gpu_device)
    c = model._constants()
    runs = []
    for _ in range(2):
        xlin, s_i, s_j = ops.project_fwd(x, gnn.lin.weight, c.terms)
        z, alpha = ops.attn_aggregate_fwd(xlin, s_i, s_j, c.graph, gnn.bias, b, want_alpha=True)
        model.dp = FixedMaskDropout([mask])
        model.zero_grad()
        torch.nn.functional.mse_loss(model(x, None), y).backward()
        runs.append([z, alpha] + [prm.grad.clone() for prm in model.parameters()])
    torch.cuda.synchronize()
    for a, bb in zip(*runs):
        assert torch.equal(a, bb)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=[IDS[0], IDS[3]])
def test_series_forward_and_evaluator(shape, gpu_device):
    from gdn_amd import evaluate, harness
    n, w, k, d = shape
    t = 40
    model, _ = _model(n, w, k, d, gpu_device)
    model.eval()
    series = torch.rand((n, t + w), generator=torch.Generator().manual_seed(4)).to(gpu_device)
    xs = series.unfold(1, w, 1)[:, :t].permute(1, 0, 2).contiguous()       # window b = series[:, b : b + w]
    y = series[:, w:].t().contiguous()
    with torch.no_grad():
        eager = model(xs, None)
        fs = model.forward_series(series, 0, t)
        fs2 = model.forward_series(series, 7, t - 7)
    assert torch.equal(fs, eager)
    assert torch.equal(fs2, eager[7:])
    _, want, _ = evaluate.anomaly_scores(eager, y, want_scores=False)
    ev = harness.SeriesEvaluator(model, None, y, batch=16, use_graph=True, series=series)
    got = ev.step()
    torch.cuda.synchronize()
    assert torch.equal(ev.pred, eager)
    assert torch.equal(got, want)
    ev2 = harness.SeriesEvaluator(model, xs, y, batch=16, use_graph=True)
    assert torch.equal(ev2.step(), want)


# seeds with no ReLU / LeakyReLU input of the step within KINK_BAND of 0 (float64: 2.3e-5 and 5.6e-6)
@pytest.mark.parametrize("shape,seed", [(SHAPES[0], 22), (SHAPES[1], 33)], ids=[IDS[0], IDS[1]])
def test_autograd_training_step_against_float64(shape, seed, gpu_device):
    from _grad_check import KINK_BAND, assert_grads_close, oracle_step
    n, w, k, d = shape
    b = 2
    model, p = _model(n, w, k, d, gpu_device, seed=seed)
    model.train()
    g = torch.Generator().manual_seed(seed + 1)
    x, y = torch.rand((b, n, w), generator=g), torch.rand((b, n), generator=g)
    mask = (torch.rand((b, n, d), generator=g) >= 0.2).float() / 0.8
    model.dp = FixedMaskDropout([mask.to(gpu_device)])
    model.zero_grad()
    loss = torch.nn.functional.mse_loss(model(x.to(gpu_device), None), y.to(gpu_device))
    loss.backward()
    got = {name: prm.grad for name, prm in model.named_parameters()}
    ref_loss, want, kink = oracle_step(p, x, y, model.learned_graph.cpu(), 1, mask)
    assert kink > KINK_BAND
    assert abs(float(loss.detach()) - ref_loss) < 2e-6
    assert_grads_close(got, want, what="large graph")


def test_graphed_train_step_equals_eager_steps(gpu_device):
    from gdn_amd import harness
    n, w, k, d, b = 700, 15, 30, 64, 2
    g = torch.Generator().manual_seed(3)
    xs = [torch.rand((b, n, w), generator=g).to(gpu_device) for _ in range(3)]
    ys = [torch.rand((b, n), generator=g).to(gpu_device) for _ in range(3)]
    results = []
    for use_graph in (False, True):
        model, _ = _model(n, w, k, d, gpu_device, seed=21)
        model.dp = torch.nn.Dropout(0.0)
        model.operand_range = "narrow"
        step = harness.GraphedTrainStep(model, b, use_graph=use_graph)
        assert isinstance(step, harness.AutogradTrainStep)
        losses = []
        for x, y in zip(xs, ys):
            step.x.copy_(x)
            step.y.copy_(y)
            step.step()
            losses.append(step.loss.clone())
        torch.cuda.synchronize()
        results.append((losses, [prm.detach().clone() for prm in model.parameters()]))
    (l0, p0), (l1, p1) = results
    for a, bb in zip(l0 + p0, l1 + p1):
        assert torch.equal(a, bb)


def test_train_head_exact_sums_at_the_largest_chunk_count(gpu_device):
    """gdn_head_train_fwd / _bwd at n = 4096, d = 16 (64 sensor chunks per pass) against float64 autograd."""
    from gdn_amd import ops
    n, d, b = 4096, 16, 3
    g = torch.Generator().manual_seed(12)
    z = torch.randn((b * n, d), generator=g)
    emb = torch.rand((n, d), generator=g) + 0.5
    bn1, bn2 = torch.nn.BatchNorm1d(d), torch.nn.BatchNorm1d(d)
    with torch.no_grad():
        for bn in (bn1, bn2):
            bn.weight.copy_(torch.rand(d, generator=g) + 0.5)
            bn.bias.copy_(torch.rand(d, generator=g) * 0.4 - 0.2)
    lin_w, lin_b = torch.rand((1, d), generator=g) - 0.5, torch.rand((1,), generator=g)
    d_out = torch.randn((b, n), generator=g)
    dev = gpu_device
    bn1d, bn2d = copy.deepcopy(bn1).to(dev), copy.deepcopy(bn2).to(dev)
    out, stats = ops.head_train_fwd(z.to(dev), emb.to(dev), bn1d, bn2d, lin_w.to(dev), lin_b.to(dev), None, b)
    grads = ops.head_train_bwd(d_out.to(dev), z.to(dev), emb.to(dev), bn1d.weight.detach(), bn1d.bias.detach(),
                               bn2d.weight.detach(), bn2d.bias.detach(), lin_w.to(dev), None, stats,
                               float(bn1.eps), float(bn2.eps), b)
    # float64 autograd of models/GDN.py:77-79,175-184 in training (no dropout)
    leaves = [t.detach().to(F64).requires_grad_() for t in
              (z, emb, bn1.weight, bn1.bias, bn2.weight, bn2.bias, lin_w, lin_b)]
    zz, ee, w1, b1, w2, b2, lw, lb = leaves
    pre1 = torch.nn.functional.batch_norm(zz, None, None, w1, b1, training=True, eps=bn1.eps)
    h = torch.relu(pre1).view(b, n, d) * ee
    pre2 = torch.nn.functional.batch_norm(h.reshape(b * n, d), None, None, w2, b2, training=True, eps=bn2.eps)
    ref = (torch.relu(pre2) @ lw.t() + lb).view(b, n)
    ref.backward(d_out.to(F64))
    np.testing.assert_allclose(out.cpu().numpy(), ref.detach().numpy(), atol=2e-5, rtol=0)
    kink = (pre1.detach().abs() < 1e-5) | (pre2.detach().abs() < 1e-5)
    names = ["d_z", "d_emb", "d_bn1_w", "d_bn1_b", "d_bn2_w", "d_bn2_b", "d_lin_w", "d_lin_b"]
    for name, got, leaf in zip(names, grads, leaves):
        want = leaf.grad.reshape(-1)
        got = got.detach().cpu().to(F64).reshape(-1)
        if name == "d_z":
            keep = ~kink.reshape(-1)
            got, want = got[keep], want[keep]
        scale = float(want.abs().max())
        err = float((got - want).abs().max())
        assert err <= 1e-4 * scale + 1e-7, (name, err, scale)


def test_command_line_at_1000_sensors(tmp_path, monkeypatch, capsys):
    import os

    import pandas as pd
    from gdn_amd import main as cli
    n, t_train, t_test = 1000, 120, 80
    rng = np.random.default_rng(7)
    phase = rng.uniform(0, 6.28, size=n)

    def series(t0, t):
        tt = np.arange(t0, t0 + t)[:, None]
        return 0.5 + 0.4 * np.sin(0.07 * tt + phase[None, :]) + 0.02 * rng.standard_normal((t, n))
    cols = [f"s{i}" for i in range(n)]
    root = tmp_path / "data" / "big1000"
    os.makedirs(root)
    pd.DataFrame(series(0, t_train), columns=cols).to_csv(root / "train.csv")
    test = pd.DataFrame(series(t_train, t_test), columns=cols)
    attack = np.zeros(t_test, dtype=int)
    attack[40:55] = 1
    test.iloc[40:55, :10] += 0.8
    test["attack"] = attack
    test.to_csv(root / "test.csv")
    (root / "list.txt").write_text("\n".join(cols) + "\n")
    monkeypatch.chdir(tmp_path)
    info = cli.main(["-dataset", "big1000", "-data_root", str(tmp_path / "data"), "-batch", "16", "-slide_win", "10",
                     "-dim", "64", "-slide_stride", "1", "-topk", "20", "-random_seed", "5", "-epoch", "1",
                     "-val_ratio", "0.2", "-save_path_pattern", "big1000"])
    assert all(np.isfinite(v) for v in info[:3]) and 0.0 <= info[0] <= 1.0
    assert "F1 score:" in capsys.readouterr().out
