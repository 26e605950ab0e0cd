"""GPU suite: MLP-head models (out_layer_num > 1) on the evaluation fast path.  gdn_head_mlp_fwd folds the eval head
into the OutLayer MLP's first matrix operand (no h2 in memory); GDN.forward_into / forward_series run the staged route
project -> aggregate -> MLP tail on cached buffers at every shape, and harness.SeriesEvaluator and the command line
evaluate such a model from the resident series.  Before this, forward_into / forward_series raised RuntimeError for
every model here and the library had no gdn_head_mlp_fwd."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import gdn_oracle
from test_gpu_forward_parity import random_params

pytestmark = pytest.mark.gpu
F64 = torch.float64


def _mlp_model(n, w, k, d, hidden, layers, dev, seed=41):
    """random_params plus non-trivial running statistics in the OutLayer's own BatchNorms."""
    model = random_params(n, w, k, d, seed=seed, out_layer_num=layers, inter=hidden)
    g = torch.Generator().manual_seed(seed + 2)
    with torch.no_grad():
        for mod in model.out_layer.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=g) + 0.5)
                mod.bias.copy_(torch.rand(mod.bias.shape, generator=g) * 0.4 - 0.2)
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) + 0.5)
    p = {key: v.detach().clone() for key, v in model.state_dict().items()}
    return model.to(dev).eval(), p


def _p64(p):
    return {key: (v.to(F64) if v.is_floating_point() else v) for key, v in p.items()}


def _windows(series, w, count):
    """window b = series[:, b : b + w]"""
    return series.unfold(1, w, 1)[:, :count].permute(1, 0, 2).contiguous()


# ---------------------------------------------------------------- 1. the kernel, bit for bit
@pytest.mark.parametrize("d,hidden,layers", [(64, 256, 2), (64, 128, 3), (32, 48, 2), (16, 24, 4), (128, 200, 3)],
                         ids=lambda v: str(v))
def test_head_mlp_kernel_equals_head_then_mlp_bit_for_bit(d, hidden, layers, gpu_device):
    """gdn_head_mlp_fwd(z) == gdn_mlp_fwd(gdn_head_fwd(z).h2) at the five one-launch configurations of
    test_outlayer_mlp_on_the_matrix_cores: a row count that is no multiple of 128 (partial last block) and one above
    2 * CUs * 128 rows (the grid-stride loop is taken)."""
    from gdn_amd import ops
    n = 27
    model, _ = _mlp_model(n, 5, 5, d, hidden, layers, gpu_device)
    c = model._constants()
    plan = ops.mlp_plan(model.out_layer, d)
    assert plan is not None
    emb = model.embedding.weight
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    big = (2 * cus * 128) // n + 3
    zero_w, zero_b = torch.zeros((d,), device=gpu_device), torch.zeros((1,), device=gpu_device)
    for batch in (5, big):
        rows = batch * n
        assert rows % 128 != 0 and (batch == 5 or rows > 2 * cus * 128)
        z = torch.randn((rows, d), generator=torch.Generator().manual_seed(batch)).to(gpu_device)
        _, h2 = ops.head_fwd(z, emb, c.bn1, c.bn2, zero_w, zero_b, batch, want_h2=True)
        want = ops.mlp_fwd(h2, plan)
        got = ops.head_mlp_fwd(z, emb, c.bn1, c.bn2, plan, batch)
        assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
        assert torch.equal(got, want), (batch, float((got - want).abs().max()))
        into = torch.full((rows + 64,), 7.0, device=gpu_device)       # out= is written in place, nothing past its end
        ops.head_mlp_fwd(z, emb, c.bn1, c.bn2, plan, batch, out=into[:rows])
        assert torch.equal(into[:rows], want) and bool((into[rows:] == 7.0).all())


# ---------------------------------------------------------------- 2. + 3. against float64; the two addressings
#          (n,   w,   k,  d,   hidden, layers)
TILE = [(127, 15, 30, 64, 256, 2), (40, 10, 8, 64, 128, 3), (20, 8, 6, 32, 48, 2), (30, 20, 10, 128, 200, 3),
        (127, 15, 30, 64, 512, 2)]
ANY_WIDTH, LONG_WINDOW, LARGE_GRAPH = (127, 15, 30, 48, 256, 2), (127, 100, 30, 64, 256, 2), (700, 15, 30, 64, 256, 2)
SHAPES = TILE + [ANY_WIDTH, LONG_WINDOW, LARGE_GRAPH]
IDS = ["n{}_w{}_k{}_d{}_h{}_L{}".format(*s) for s in SHAPES]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_forward_into_and_forward_series_against_float64(shape, gpu_device):
    """Both entry points against gdn_oracle.forward in float64 on the model's own graph.  Tile shapes: the bar of
    test_outlayer_mlp_on_the_matrix_cores (atol 2e-6, rtol 1e-5).  Any width, long window, beyond the tile: max error
    < 2e-5, the bar of the MLP-head tests of those suites (test_gpu_any_width.py
    test_mlp_head_eval_and_training_against_float64, test_gpu_long_window.py / test_gpu_large_graph.py
    test_eval_forward_with_mlp_head).
    The two addressings of the same windows: bit for bit where gdn_project_fwd and gdn_project_fwd_series share one
    arithmetic (those three shapes); at tile shapes the windowed projection is the matrix-core kernel and both are
    held to the float64 bar.  `first` > 0 and a last window that ends at the series' last tick are covered."""
    n, w, k, d, hidden, layers = shape
    t, first = 9, 3
    model, p = _mlp_model(n, w, k, d, hidden, layers, gpu_device)
    series = torch.rand((n, t + w), generator=torch.Generator().manual_seed(6))
    xs = _windows(series, w, t + 1)                      # t + 1 windows: the last one ends at the last tick
    assert xs.shape[0] == t + 1 and torch.equal(xs[t, :, -1], series[:, -1])
    dev_series, dev_xs = series.to(gpu_device), xs.to(gpu_device)
    into = torch.empty((t + 1, n), device=gpu_device)
    with torch.no_grad():
        assert model.forward_into(dev_xs, into) is into
        fs = model.forward_series(dev_series, 0, t + 1)
        fs_tail = model.forward_series(dev_series, first, t + 1 - first)
    c = model._constants()
    if hidden <= 256 and d in (16, 32, 64, 128):
        assert c.tail == "plan" and c.mlp is not None            # gdn_head_mlp_fwd: no h2 buffer was allocated
        assert all(len(bufs) == 4 for bufs in c.bufs.values())
    else:
        assert c.tail == "wide" and c.mlp is None
    ref = gdn_oracle.forward(_p64(p), xs.to(F64), k, layers, graph=model.learned_graph.cpu())["out"]
    for name, got in (("forward_into", into), ("forward_series", fs)):
        got = got.cpu().to(F64)
        err = float((got - ref).abs().max())
        print(f"{IDS[SHAPES.index(shape)]} {name}: max|hip - float64| = {err:.3e} (max|ref| {float(ref.abs().max()):.3f})")
        if shape in TILE:
            np.testing.assert_allclose(got.numpy(), ref.numpy(), atol=2e-6, rtol=1e-5, err_msg=name)
        else:
            assert err < 2e-5, (name, err)
    assert torch.equal(fs_tail, fs[first:])              # the same windows whatever `first`
    if shape not in TILE:
        assert torch.equal(fs, into)


# ---------------------------------------------------------------- 4. the evaluator
@pytest.mark.parametrize("form", ["windows", "series"])
@pytest.mark.parametrize("shape", [TILE[0], LARGE_GRAPH], ids=[IDS[0], IDS[-1]])
def test_series_evaluator_with_an_mlp_head(shape, form, gpu_device):
    from gdn_amd import evaluate, harness
    n, w, k, d, hidden, layers = shape
    t = 40
    model, _ = _mlp_model(n, w, k, d, hidden, layers, gpu_device)
    series = torch.rand((n, t + w), generator=torch.Generator().manual_seed(4)).to(gpu_device)
    xs = _windows(series, w, t)
    y = series[:, w:].t().contiguous()

    def make(m, use_graph):
        if form == "series":
            return harness.SeriesEvaluator(m, None, y, batch=16, use_graph=use_graph, series=series)
        return harness.SeriesEvaluator(m, xs, y, batch=16, use_graph=use_graph)

    def direct(m):
        with torch.no_grad():
            if form == "series":
                return m.forward_series(series, 0, t)
            return m.forward_into(xs, torch.empty((t, n), device=gpu_device))

    want_pred = direct(model).clone()
    _, want_anomaly, want_mi = evaluate.anomaly_scores(want_pred, y, want_scores=False)
    eager = make(model, False)
    assert eager.wide is False
    got = eager.step()
    torch.cuda.synchronize()
    assert torch.equal(eager.pred, want_pred)
    assert torch.equal(got, want_anomaly) and torch.equal(eager.med_iqr, want_mi)
    # no allocation per step once the buffers of every (stream, span) exist
    eager.step()
    torch.cuda.synchronize()
    after2 = torch.cuda.memory_allocated()
    eager.step()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == after2
    # captured == eager, bit for bit, twice
    graphed = make(model, True)
    for _ in range(2):
        graphed.pred.zero_()
        graphed.anomaly.zero_()
        out = graphed.step()
        torch.cuda.synchronize()
        assert graphed.graph is not None
        assert torch.equal(graphed.pred, want_pred) and torch.equal(out, want_anomaly)
        assert torch.equal(graphed.med_iqr, want_mi)
    # a parameter changes in place: after invalidate_constants() every evaluator follows
    with torch.no_grad():
        model.out_layer.mlp[0].weight.mul_(1.25)
        model.gnn_layers[0].bn.running_mean.add_(0.05)
    model.invalidate_constants()
    fresh = make(model, False)
    want2 = fresh.step().clone()
    torch.cuda.synchronize()
    assert not torch.equal(fresh.pred, want_pred)
    assert torch.equal(fresh.pred, direct(model))
    for ev in (graphed, eager):
        got2 = ev.step()
        torch.cuda.synchronize()
        assert torch.equal(ev.pred, fresh.pred) and torch.equal(got2, want2)


# ---------------------------------------------------------------- 5. raw units
def _assert_fp32_grade(got, p, x, k, graph, layers, what=""):
    """The bound of test_gpu_forward_parity._assert_fp32_grade (used by test_evaluator_and_training_on_raw_unit_series)
    with the oracle evaluating the MLP head: 4 x the op-faithful fp32 oracle's own worst deviation from float64 plus
    2e-5 of the output scale."""
    ref = gdn_oracle.forward(_p64(p), x.to(F64), k, layers, graph=graph)["out"]
    ref32 = gdn_oracle.forward(p, x, k, layers, graph=graph)["out"].double()
    scale = max(1.0, float(ref.abs().max()))
    bound = 4.0 * float((ref32 - ref).abs().max()) + 2e-5 * scale
    err = float((got.cpu().double() - ref).abs().max())
    print(f"{what}: err {err:.3e} bound {bound:.3e} scale {scale:.3e}")
    assert err <= bound, (what, err, bound, scale)


def test_evaluator_on_raw_unit_series_with_an_mlp_head(gpu_device):
    """A series in raw engineering units (x 1e5) under operand_range='auto': the evaluator's one-time range check
    runs for MLP-head models too and selects the fp32 projection / aggregate."""
    from gdn_amd import harness
    n, w, k, d, t = 27, 10, 8, 64, 300
    model, p = _mlp_model(n, w, k, d, 256, 2, gpu_device, seed=33)
    assert model.operand_range == "auto"
    series = torch.rand((n, t + w), generator=torch.Generator().manual_seed(34)) * 1.0e5
    xs = _windows(series, w, t)
    raw = series.to(gpu_device)
    y = raw[:, w:].t().contiguous()
    ev = harness.SeriesEvaluator(model, None, y, batch=64, use_graph=True, series=raw)
    assert ev.wide is True
    ev.step()
    torch.cuda.synchronize()
    graph = model.learned_graph.cpu()
    _assert_fp32_grade(ev.pred, p, xs, k, graph, 2, what="series evaluator, x 1e5")
    ev2 = harness.SeriesEvaluator(model, xs.to(gpu_device), y, batch=64, use_graph=False)
    assert ev2.wide is True
    ev2.step()
    torch.cuda.synchronize()
    _assert_fp32_grade(ev2.pred, p, xs, k, graph, 2, what="window evaluator, x 1e5")


# ---------------------------------------------------------------- 6. refusals
def test_refusals(gpu_device):
    from gdn_amd import _lib
    n, w, k, d = 27, 10, 8, 64
    x = torch.rand((3, n, w), generator=torch.Generator().manual_seed(1)).to(gpu_device)
    series = torch.rand((n, 40), generator=torch.Generator().manual_seed(2)).to(gpu_device)
    out = torch.empty((3, n), device=gpu_device)
    # hidden = 600: no kernel; said so, naming the width, before anything is allocated or launched
    wide, _ = _mlp_model(n, w, k, d, 600, 2, gpu_device)
    wide._constants()
    assert wide.mlp_fast_path_supported() is False
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(_lib.GdnHipError, match="600"):
        wide.forward_into(x, out)
    with pytest.raises(_lib.GdnHipError, match="600"):
        wide.forward_series(series, 0, 3)
    assert torch.cuda.memory_allocated() == before and not wide._constants().bufs
    model, _ = _mlp_model(n, w, k, d, 256, 2, gpu_device)
    assert model.mlp_fast_path_supported() is True and model.fused_keys_supported() is False
    keys = (torch.zeros((3, n), device=gpu_device), torch.zeros((n, 3), dtype=F64, device=gpu_device).data_ptr(), 3)
    with pytest.raises(_lib.GdnHipError, match="scoring keys"):
        model.forward_into(x, out, keys=keys)
    with pytest.raises(_lib.GdnHipError, match="scoring keys"):
        model.forward_series(series, 0, 3, keys=keys)
    with pytest.raises(_lib.GdnHipError, match="bf16"):
        model.forward_series(series.to(torch.bfloat16), 0, 3)
    with pytest.raises(_lib.GdnHipError, match="bf16"):
        model.forward_into(x.to(torch.bfloat16), out)
    model.train()
    with pytest.raises(RuntimeError):
        model.forward_into(x, out)
    with pytest.raises(RuntimeError):
        model.forward_series(series, 0, 3)


# ---------------------------------------------------------------- 7. the command line
def test_command_line_predicts_from_the_resident_series(gpu_device, tmp_path, capsys):
    """`python -m gdn_amd.main -out_layer_num 2 -load_model_path ...` on the demo slice of the existing CLI test:
    the test predictions come from forward_series — the test windows are never materialised — and equal
    per-minibatch model(x) over the same windows within the tile bar (atol 2e-6, rtol 1e-5)."""
    import random

    from gdn_amd import main as cli
    from test_gpu_end_to_end import _write_cli_dataset
    data, _p = load_golden("cli_msl_slice")
    batch, w, dim, stride, topk, seed, inter = (int(v) for v in data["meta_cfg"])
    root = str(tmp_path / "data")
    _write_cli_dataset(data, root)
    n = len(data["features"])
    model, p = _mlp_model(n, w, topk, dim, inter, 2, "cpu", seed=seed)
    ckpt = str(tmp_path / "ckpt_mlp.pt")
    torch.save(p, ckpt)
    random.seed(seed)
    torch.manual_seed(seed)
    m = cli.Main({"batch": batch, "epoch": 1, "slide_win": w, "dim": dim, "slide_stride": stride, "comment": "",
                  "seed": seed, "out_layer_num": 2, "out_layer_inter_dim": inter, "decay": 0,
                  "val_ratio": float(data["val_ratio"]), "topk": topk},
                 {"save_path": "msl", "dataset": "msl", "report": "best", "device": "cuda", "load_model_path": ckpt,
                  "data_root": root})
    calls = {"test": 0}
    inner = m.test_dataset.batch

    def counted(idx):
        calls["test"] += 1
        return inner(idx)
    m.test_dataset.batch = counted
    info = m.run()
    assert calls["test"] == 0
    printed = capsys.readouterr().out
    assert "F1 score:" in printed and all(np.isfinite(v) for v in info[:3]) and 0.0 <= info[0] <= 1.0
    pred = m.test_result[0]
    n_test = m.test_series.shape[1] - w
    assert pred.shape == (n_test, n) and bool(torch.isfinite(pred).all())
    with torch.no_grad():
        want = torch.cat([m.model(inner(torch.arange(s, min(n_test, s + batch)))[0], None)
                          for s in range(0, n_test, batch)])
    np.testing.assert_allclose(pred.cpu().numpy(), want.cpu().numpy(), atol=2e-6, rtol=1e-5)
    assert os.path.exists(ckpt)
