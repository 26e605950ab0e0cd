"""GPU suite: embedding widths other than 16, 32, 64 and 128 (any 1 <= d <= 256).  Such widths run
gdn_any_width.hip's kernels on the staged route (project -> aggregate -> head) and train through the autograd step.
Every model here raised GdnHipError (GDN_ERR_UNSUPPORTED from gdn_topk_graph or gdn_project_fwd) at its first
forward before those kernels existed."""
import numpy as np
import pytest
import torch

from oracle import gdn_oracle
from test_gpu_forward_parity import _assert_fp32_grade, random_params
from test_gpu_train_parity import FixedMaskDropout

pytestmark = pytest.mark.gpu

SHAPES = [(27, 5, 5, 3),          # odd width: scalar rows
          (51, 10, 5, 50),        # d % 4 == 2: float2 rows
          (127, 15, 30, 48),      # the SWaT shape at d = 48
          (127, 15, 30, 256),     # the cap
          (700, 30, 30, 96),      # beyond the old tile size
          (127, 100, 30, 72)]     # long window
IDS = ["n{}_w{}_k{}_d{}".format(*s) for s in SHAPES]
F64 = torch.float64


def _model(n, w, k, d, dev, seed=31, out_layer_num=1, inter=256):
    model = random_params(n, w, k, d, seed=seed, out_layer_num=out_layer_num, inter=inter)
    p = {key: v.detach().clone() for key, v in model.state_dict().items()}
    return model.to(dev), p


def _p64(p):
    return {key: (v.to(F64) if v.is_floating_point() else v) for key, v in p.items()}


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_eval_forward_and_attention_against_float64_oracle(shape, gpu_device):
    n, w, k, d = shape
    b = 2
    model, p = _model(n, w, k, d, gpu_device)
    model.eval()
    x = torch.rand((b, n, w), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        out = model(x.to(gpu_device), None)
        again = model(x.to(gpu_device), None)
    assert torch.equal(out, again)
    graph = model.learned_graph.cpu()
    ref = gdn_oracle.forward(_p64(p), x.to(F64), k, graph=graph)
    err = float((out.cpu().to(F64) - ref["out"]).abs().max())
    assert err < 2e-5, err
    layer = model.gnn_layers[0]
    att = layer.att_weight_1.view(-1).cpu().to(F64)
    ei = layer.edge_index_1.cpu()
    assert torch.equal(ei, ref["edge_index_1"])
    np.testing.assert_allclose(att.numpy(), ref["att_weight_1"].view(-1).numpy(), atol=2e-6, rtol=0)
    sums = torch.zeros(b * n, dtype=F64).index_add_(0, ei[1], att)
    np.testing.assert_allclose(sums.numpy(), 1.0, atol=1e-5)


@pytest.mark.parametrize("n,d,k", [(27, 3, 5), (51, 50, 5), (127, 48, 30)])
def test_learned_graph_is_a_descending_topk_of_the_cosine_matrix(n, d, k, gpu_device):
    from gdn_amd import ops
    model, p = _model(n, 5, k, d, gpu_device)
    graph = ops.topk_graph(model.embedding.weight, k, want_cos=True)
    topk = graph.topk.cpu()
    emb = p["embedding.weight"].to(F64)
    nrm = emb.norm(dim=1)
    cos = (emb @ emb.T) / (nrm[:, None] * nrm[None, :])
    np.testing.assert_allclose(graph.cos.cpu().to(F64).numpy(), cos.numpy(), atol=1e-6, rtol=0)
    for i in range(n):
        row = topk[i]
        assert len(set(row.tolist())) == k
        vals = cos[i, row]
        assert bool(torch.all(vals[:-1] >= vals[1:] - 1e-6)), i
        rest = torch.ones(n, dtype=torch.bool)
        rest[row] = False
        if bool(rest.any()):
            assert float(vals.min()) >= float(cos[i, rest].max()) - 1e-6, i


@pytest.mark.parametrize("inter", [256, 50])
def test_mlp_head_eval_and_training_against_float64(inter, gpu_device):
    from _grad_check import KINK_BAND, assert_grads_close, oracle_step
    n, w, k, d, b, seed = 40, 8, 6, 24, 2, 23
    model, p = _model(n, w, k, d, gpu_device, seed=seed, out_layer_num=2, inter=inter)
    g = torch.Generator().manual_seed(seed + 1)
    x, y = torch.rand((b, n, w), generator=g), torch.rand((b, n), generator=g)
    model.eval()
    with torch.no_grad():
        out = model(x.to(gpu_device), None)
    ref = gdn_oracle.forward(_p64(p), x.to(F64), k, 2, graph=model.learned_graph.cpu())
    assert float((out.cpu().to(F64) - ref["out"]).abs().max()) < 2e-5
    model.train()
    mask = (torch.rand((b, n, d), generator=g) >= 0.2).float() / 0.8
    model.dp = FixedMaskDropout([mask.to(gpu_device)])
    model.zero_grad()
    loss = torch.nn.functional.mse_loss(model(x.to(gpu_device), None), y.to(gpu_device))
    loss.backward()
    ref_loss, want, kink = oracle_step(p, x, y, model.learned_graph.cpu(), 2, mask)
    assert kink > KINK_BAND
    assert abs(float(loss.detach()) - ref_loss) < 2e-6
    assert_grads_close({name: prm.grad for name, prm in model.named_parameters()}, want, what=f"mlp {inter}")


def test_raw_unit_inputs_equal_float64(gpu_device):
    """The any-width route is fp32 throughout (no 16-bit operands, no range switch): inputs in raw units (x 1e5)
    equal float64 through model(x) and through the evaluator."""
    from gdn_amd import harness
    n, w, k, d, b = 127, 15, 30, 48, 6
    model, p = _model(n, w, k, d, gpu_device)
    model.eval()
    g = torch.Generator().manual_seed(32)
    x = torch.rand((b, n, w), generator=g) * 1.0e5
    with torch.no_grad():
        out = model(x.to(gpu_device), None)
        _assert_fp32_grade(out, p, x, k, model.learned_graph.cpu(), what="raw units, d = 48")
        y = torch.rand((b, n), generator=g).to(gpu_device)
        ev = harness.SeriesEvaluator(model, x.to(gpu_device), y, batch=4, use_graph=False)
        ev.step()
        torch.cuda.synchronize()
        assert torch.equal(ev.pred, out)


def test_bf16_windows_are_refused_naming_the_width(gpu_device):
    from gdn_amd import _lib
    model, _ = _model(127, 15, 30, 48, gpu_device)
    model.eval()
    x = torch.rand((2, 127, 15), device=gpu_device).bfloat16()
    with pytest.raises(_lib.GdnHipError, match="embedding width 48"):
        with torch.no_grad():
            model(x, None)


def test_width_beyond_the_cap_is_refused_naming_it(gpu_device):
    from gdn_amd import _lib
    model, _ = _model(27, 5, 5, 257, gpu_device)
    model.eval()
    with pytest.raises(_lib.GdnHipError, match="257"):
        with torch.no_grad():
            model(torch.rand((2, 27, 5), device=gpu_device), None)


def test_both_projection_addressings_give_the_same_bits(gpu_device):
    from gdn_amd import _lib, ops
    for n, w, k, d in [SHAPES[0], SHAPES[2], SHAPES[5]]:
        t = 9
        model, _ = _model(n, w, k, d, gpu_device)
        gnn = model.gnn_layers[0].gnn
        c = model.eval()._constants()
        series = torch.rand((n, t + w + 3), generator=torch.Generator().manual_seed(2)).to(gpu_device)
        first = 3
        xs = series.unfold(1, w, 1)[:, first:first + t].permute(1, 0, 2).contiguous()
        xlin, s_i, s_j = ops.project_fwd(xs, gnn.lin.weight, c.terms)
        xl2, si2, sj2 = torch.empty_like(xlin), torch.empty_like(s_i), torch.empty_like(s_j)
        _lib.call("gdn_project_fwd_series", series.data_ptr(), series.shape[1], first, gnn.lin.weight.data_ptr(),
                  c.terms.data_ptr(), t, n, w, d, xl2.data_ptr(), si2.data_ptr(), sj2.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(xlin, xl2) and torch.equal(s_i, si2) and torch.equal(s_j, sj2), (n, w, d)
        want = xs.cpu().to(F64).reshape(t * n, w) @ gnn.lin.weight.detach().cpu().to(F64).t()
        np.testing.assert_allclose(xlin.cpu().to(F64).numpy(), want.numpy(), atol=2e-6)


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4]], ids=[IDS[1], IDS[4]])
def test_series_forward_and_evaluator(shape, gpu_device):
    from gdn_amd import evaluate, harness
    n, w, k, d = shape
    t = 40
    model, _ = _model(n, w, k, d, gpu_device)
    model.eval()
    series = torch.rand((n, t + w), generator=torch.Generator().manual_seed(4)).to(gpu_device)
    xs = series.unfold(1, w, 1)[:, :t].permute(1, 0, 2).contiguous()
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


def _bn_running_f64(p, prefix, v, mom=0.1):
    """torch's train-mode running-statistics update of BatchNorm1d over the rows of v [rows, c], in float64."""
    return ((1 - mom) * p[prefix + "running_mean"].to(F64) + mom * v.mean(0),
            (1 - mom) * p[prefix + "running_var"].to(F64) + mom * v.var(0, unbiased=True))


# seeds with no ReLU / LeakyReLU input of the step within KINK_BAND of 0 (screened in float64)
TRAIN = [(SHAPES[0], 40), (SHAPES[0], 41), (SHAPES[1], 40), (SHAPES[1], 41), (SHAPES[2], 40), (SHAPES[2], 41),
         (SHAPES[3], 41), (SHAPES[3], 42), (SHAPES[4], 42), (SHAPES[4], 47), (SHAPES[5], 41), (SHAPES[5], 42)]


@pytest.mark.parametrize("shape,seed", TRAIN, ids=[f"{IDS[SHAPES.index(s)]}_s{q}" for s, q in TRAIN])
def test_autograd_training_step_against_float64(shape, seed, gpu_device):
    from _grad_check import KINK_BAND, assert_grads_close, oracle_step, staged_f64, f64_leaves
    from gdn_amd import harness
    n, w, k, d = shape
    b = 2
    model, p = _model(n, w, k, d, gpu_device, seed=seed)
    assert not harness.NativeTrainStep.applicable(model)
    model.train()
    g = torch.Generator().manual_seed(seed + 1)
    x, y = torch.rand((b, n, w), generator=g), torch.rand((b, n), generator=g)
    mask = (torch.rand((b, n, d), generator=g) >= 0.2).float() / 0.8
    model.dp = FixedMaskDropout([mask.to(gpu_device)] * 2)
    runs = []
    for _ in range(2):
        model.load_state_dict(p)            # both steps from the same BatchNorm buffers
        model.zero_grad()
        loss = torch.nn.functional.mse_loss(model(x.to(gpu_device), None), y.to(gpu_device))
        loss.backward()
        runs.append([loss.detach().clone()] + [prm.grad.clone() for prm in model.parameters()] +
                    [buf.clone() for buf in model.buffers()])
    torch.cuda.synchronize()
    for a, bb in zip(*runs):
        assert torch.equal(a, bb)
    graph = model.learned_graph.cpu()
    got = {name: prm.grad for name, prm in model.named_parameters()}
    ref_loss, want, kink = oracle_step(p, x, y, graph, 1, mask)
    assert kink > KINK_BAND, kink
    assert abs(float(loss.detach()) - ref_loss) < 2e-6
    assert_grads_close(got, want, what=f"d = {d}")
    # the BatchNorm running statistics of the step against float64
    q = f64_leaves(p)
    _, st, _, _ = staged_f64(q, x.to(F64), y.to(F64), graph, 1, mask.to(F64))
    z = st["z"].reshape(b * n, d)
    bn1 = "gnn_layers.0.bn."
    zn = (z - z.mean(0)) / torch.sqrt(z.var(0, unbiased=False) + 1e-5) * q[bn1 + "weight"] + q[bn1 + "bias"]
    h1 = (torch.relu(zn).view(b, n, d) * q["embedding.weight"]).reshape(b * n, d)
    for prefix, v in ((bn1, z), ("bn_outlayer_in.", h1)):
        rm, rv = _bn_running_f64(p, prefix, v.detach())
        sd = model.state_dict()
        np.testing.assert_allclose(sd[prefix + "running_mean"].cpu().to(F64).numpy(), rm.numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(sd[prefix + "running_var"].cpu().to(F64).numpy(), rv.numpy(), rtol=1e-5, atol=1e-6)


def test_graphed_train_step_equals_eager_steps(gpu_device):
    from gdn_amd import harness
    n, w, k, d, b = 127, 15, 30, 48, 2
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


def _dataset(root, n, t_train=400, t_test=220):
    import os

    import pandas as pd
    rng = np.random.default_rng(7)
    phase = rng.uniform(0, 6.28, size=n)

    def series(t0, t):
        tt = np.arange(t0, t0 + t)[:, None]
        return 0.5 + 0.4 * np.sin(0.07 * tt + phase[None, :]) + 0.02 * rng.standard_normal((t, n))
    cols = [f"s{i}" for i in range(n)]
    os.makedirs(root)
    pd.DataFrame(series(0, t_train), columns=cols).to_csv(root / "train.csv")
    test = pd.DataFrame(series(t_train, t_test), columns=cols)
    attack = np.zeros(t_test, dtype=int)
    attack[150:170] = 1
    test.iloc[150:170, :5] += 0.8
    test["attack"] = attack
    test.to_csv(root / "test.csv")
    (root / "list.txt").write_text("\n".join(cols) + "\n")


@pytest.mark.parametrize("dim,win", [(48, 15), (72, 100)])
def test_command_line_at_new_widths(dim, win, tmp_path, monkeypatch, capsys):
    from gdn_amd import main as cli
    name = f"dim{dim}"
    _dataset(tmp_path / "data" / name, 27)
    monkeypatch.chdir(tmp_path)
    info = cli.main(["-dataset", name, "-data_root", str(tmp_path / "data"), "-batch", "16", "-slide_win", str(win),
                     "-dim", str(dim), "-slide_stride", "1", "-topk", "5", "-random_seed", "5", "-epoch", "1",
                     "-val_ratio", "0.2", "-save_path_pattern", name])
    assert all(np.isfinite(v) for v in info[:3]) and 0.0 <= info[0] <= 1.0
    assert "F1 score:" in capsys.readouterr().out
