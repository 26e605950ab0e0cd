"""GPU suite: windows longer than 64 ticks (up to 1024).  The window enters the graph layer only through the
projection, which runs on gdn_long_window.hip's fp32 matrix-core kernel for w > 64; the eval forward takes the
staged route project -> aggregate -> head and training the autograd step.  Every model here raised GdnHipError
(GDN_ERR_UNSUPPORTED from gdn_node_terms) at its first forward before that kernel existed."""
import numpy as np
import pytest
import torch

from oracle import gdn_oracle
from test_gpu_forward_parity import _assert_fp32_grade, random_params
from test_gpu_train_parity import FixedMaskDropout

pytestmark = pytest.mark.gpu

SHAPES = [(27, 65, 5, 64),        # just past the old cap; matrix-core aggregate (n <= 127, d = 64)
          (127, 100, 30, 64),     # the common 100-tick window on the 127-sensor graph
          (127, 256, 30, 128),    # d = 128: tile-form aggregate
          (51, 1024, 5, 16),      # the cap
          (700, 100, 30, 64)]     # long window on a graph beyond the tile
IDS = ["n{}_w{}_k{}_d{}".format(*s) for s in SHAPES]
F64 = torch.float64


def _model(n, w, k, d, dev, seed=31, out_layer_num=1):
    model = random_params(n, w, k, d, seed=seed, out_layer_num=out_layer_num)
    p = {key: v.detach().clone() for key, v in model.state_dict().items()}
    return model.to(dev), p


def _p64(p):
    return {key: (v.to(F64) if v.is_floating_point() else v) for key, v in p.items()}


def _scale(ref, w):
    """Bound scale: 1, or max|xlin| for w >= 256 — a w-term fp32 dot product carries an error that grows with the
    size of its terms' sum, and xlin, which every later stage is linear in, reaches a few units at these windows."""
    return max(1.0, float(ref["xlin"].abs().max())) if w >= 256 else 1.0


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
    ref = gdn_oracle.forward(_p64(p), x.to(F64), k, graph=graph)
    scale = _scale(ref, w)
    err = float((out.cpu().to(F64) - ref["out"]).abs().max())
    assert err < 2e-5 * scale, (err, scale)
    layer = model.gnn_layers[0]
    att = layer.att_weight_1.view(-1).cpu().to(F64)
    ei = layer.edge_index_1.cpu()
    assert torch.equal(ei, ref["edge_index_1"])
    np.testing.assert_allclose(att.numpy(), ref["att_weight_1"].view(-1).numpy(), atol=2e-6 * scale, rtol=0)
    sums = torch.zeros(b * n, dtype=F64).index_add_(0, ei[1], att)
    np.testing.assert_allclose(sums.numpy(), 1.0, atol=1e-5)


def test_eval_forward_with_mlp_head(gpu_device):
    n, w, k, d = SHAPES[1]
    model, p = _model(n, w, k, d, gpu_device, out_layer_num=2)
    model.eval()
    x = torch.rand((2, n, w), generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        out = model(x.to(gpu_device), None)
    ref = gdn_oracle.forward(_p64(p), x.to(F64), k, 2, graph=model.learned_graph.cpu())
    err = float((out.cpu().to(F64) - ref["out"]).abs().max())
    assert err < 2e-5, err


def test_raw_unit_inputs_keep_the_fp32_aggregate(gpu_device):
    """At (127, 100, 30, 64) gdn_attn_aggregate_fwd would pick the matrix-core aggregate, which carries xlin as two
    f16 terms: inputs in raw units (x 1e5) must still equal float64, through model(x) under operand_range 'auto'
    and through the evaluator, which looks at its data once."""
    from gdn_amd import harness
    n, w, k, d, b = 127, 100, 30, 64, 6
    model, p = _model(n, w, k, d, gpu_device)
    model.eval()
    g = torch.Generator().manual_seed(32)
    x = torch.rand((b, n, w), generator=g) * 1.0e5
    with torch.no_grad():
        out = model(x.to(gpu_device), None)
        graph = model.learned_graph.cpu()
        assert model.input_exceeds_limit(x.to(gpu_device))
        _assert_fp32_grade(out, p, x, k, graph, what="raw units, long window")
        y = torch.rand((b, n), generator=g).to(gpu_device)
        ev = harness.SeriesEvaluator(model, x.to(gpu_device), y, batch=4, use_graph=False)
        ev.step()
        torch.cuda.synchronize()
        assert ev.wide
        assert torch.equal(ev.pred, out)


def test_bf16_windows_are_refused_naming_the_window(gpu_device):
    from gdn_amd import _lib
    model, _ = _model(127, 100, 30, 64, gpu_device)
    model.eval()
    x = torch.rand((2, 127, 100), device=gpu_device).bfloat16()
    with pytest.raises(_lib.GdnHipError, match="windows of 100 ticks"):
        with torch.no_grad():
            model(x, None)


def test_window_beyond_the_cap_is_refused(gpu_device):
    from gdn_amd import _lib
    model, _ = _model(27, 1025, 5, 64, gpu_device)
    model.eval()
    with pytest.raises(_lib.GdnHipError):
        with torch.no_grad():
            model(torch.rand((2, 27, 1025), device=gpu_device), None)


def test_both_projection_addressings_give_the_same_bits(gpu_device):
    """gdn_project_fwd on materialised windows (16-byte loads: w % 4 == 0) and gdn_project_fwd_series on the raw
    series (element loads at any offset) run one arithmetic: identical xlin, s_i, s_j."""
    from gdn_amd import _lib, ops
    for n, w, k, d in [SHAPES[1], SHAPES[0], SHAPES[3]]:
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
        # and against float64: xlin = x lin^T, s = x . a + c
        x64 = xs.cpu().to(F64).reshape(t * n, w)
        want = x64 @ gnn.lin.weight.detach().cpu().to(F64).t()
        np.testing.assert_allclose(xlin.cpu().to(F64).numpy(), want.numpy(), atol=2e-6 * max(1.0, float(want.abs().max())))


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4]], ids=[IDS[1], IDS[4]])
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


# seeds with no ReLU / LeakyReLU input of the step within KINK_BAND of 0 (float64: 1.3e-4 and 1.5e-5)
@pytest.mark.parametrize("shape,seed", [(SHAPES[1], 21), (SHAPES[4], 20)], ids=[IDS[1], IDS[4]])
def test_autograd_training_step_against_float64(shape, seed, gpu_device):
    from _grad_check import KINK_BAND, assert_grads_close, oracle_step
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
        model.zero_grad()
        loss = torch.nn.functional.mse_loss(model(x.to(gpu_device), None), y.to(gpu_device))
        loss.backward()
        runs.append([loss.detach().clone()] + [prm.grad.clone() for prm in model.parameters()])
    torch.cuda.synchronize()
    for a, bb in zip(*runs):
        assert torch.equal(a, bb)
    got = {name: prm.grad for name, prm in model.named_parameters()}
    ref_loss, want, kink = oracle_step(p, x, y, model.learned_graph.cpu(), 1, mask)
    assert kink > KINK_BAND
    assert abs(float(loss.detach()) - ref_loss) < 2e-6
    assert_grads_close(got, want, what="long window")


def test_command_line_with_100_tick_windows(tmp_path, monkeypatch, capsys):
    import os

    import pandas as pd
    from gdn_amd import main as cli
    n, t_train, t_test = 27, 400, 220
    rng = np.random.default_rng(7)
    phase = rng.uniform(0, 6.28, size=n)

    def series(t0, t):
        tt = np.arange(t0, t0 + t)[:, None]
        return 0.5 + 0.4 * np.sin(0.07 * tt + phase[None, :]) + 0.02 * rng.standard_normal((t, n))
    cols = [f"s{i}" for i in range(n)]
    root = tmp_path / "data" / "win100"
    os.makedirs(root)
    pd.DataFrame(series(0, t_train), columns=cols).to_csv(root / "train.csv")
    test = pd.DataFrame(series(t_train, t_test), columns=cols)
    attack = np.zeros(t_test, dtype=int)
    attack[150:170] = 1
    test.iloc[150:170, :5] += 0.8
    test["attack"] = attack
    test.to_csv(root / "test.csv")
    (root / "list.txt").write_text("\n".join(cols) + "\n")
    monkeypatch.chdir(tmp_path)
    info = cli.main(["-dataset", "win100", "-data_root", str(tmp_path / "data"), "-batch", "16", "-slide_win", "100",
                     "-dim", "64", "-slide_stride", "1", "-topk", "5", "-random_seed", "5", "-epoch", "1",
                     "-val_ratio", "0.2", "-save_path_pattern", "win100"])
    assert all(np.isfinite(v) for v in info[:3]) and 0.0 <= info[0] <= 1.0
    assert "F1 score:" in capsys.readouterr().out
