"""The fused dense forward with fp32 storage aggregates the raw window on the matrix cores and projects the
aggregated rows afterwards (gdn_forward_dense.hip, DCfg::XAGG).  Every case here is held against the float64 oracle
at the bar of test_fused_forward_keeps_fp32_grade_against_float64 (2e-7 of the output scale), planned and
plan-less: window lengths around the 16-column operand block, sensor counts around the 32-row wave tile, fully
connected graphs, d = 64 and 128, a model whose C-in (GraphLayer bias, BatchNorm shift) dominates, inputs at the
new x limit, and the raw-series / scoring-keys entry points bit for bit against the plain planned launch."""
import numpy as np
import pytest
import torch

from oracle import gdn_oracle
from test_gpu_forward_parity import _assert_fp32_grade, random_params

pytestmark = pytest.mark.gpu

CASES = [  # (n, w, k, d, batch)
    (127, 1, 30, 64, 9), (127, 15, 30, 64, 33), (127, 16, 30, 64, 9), (127, 17, 30, 64, 9), (127, 32, 30, 64, 9),
    (31, 15, 31, 64, 17), (32, 16, 32, 64, 17), (33, 17, 33, 64, 17), (63, 32, 63, 64, 5),
    (127, 15, 63, 128, 9), (31, 1, 31, 128, 6), (32, 32, 12, 128, 6), (33, 16, 33, 128, 6), (127, 17, 30, 128, 300),
]


def f64_params(p):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in p.items()}


def planned_and_plain(model, x, dev):
    from gdn_amd import ops
    with torch.no_grad():
        planned = model(x.to(dev), None)
    c = model._constants()
    assert c.plans[False] is not None
    gnn, lin = model.gnn_layers[0].gnn, model.out_layer.mlp[0]
    plain = ops.forward_fused(x.to(dev), gnn.lin.weight, c.terms, c.graph, gnn.bias, model.embedding.weight,
                              c.bn1, c.bn2, lin.weight, lin.bias)
    return planned, plain


def assert_fp32_grade(model, p, x, k, dev):
    planned, plain = planned_and_plain(model, x, dev)
    ref = gdn_oracle.forward(f64_params(p), x.double(), k, graph=model.learned_graph.cpu())["out"]
    bound = 2e-7 * max(1.0, float(ref.abs().max()))
    for name, got in (("planned", planned), ("plan-less", plain)):
        err = float((got.cpu().double() - ref).abs().max())
        print(f"{name}: err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("n,w,k,d,b", CASES, ids=lambda v: str(v))
def test_reordered_forward_against_float64(n, w, k, d, b, gpu_device):
    model = random_params(n, w, k, d, seed=71)
    p = {key: v.detach().clone() for key, v in model.state_dict().items()}
    model = model.to(gpu_device).eval()
    x = torch.rand((b, n, w), generator=torch.Generator().manual_seed(72))
    assert_fp32_grade(model, p, x, k, gpu_device)


@pytest.mark.parametrize("d", [64, 128])
def test_c_in_enters_behind_the_aggregation(d, gpu_device):
    """GraphLayer bias and BatchNorm shift several times larger than the projected features (+-3 and +3 against
    features of ~0.5): C-in is the initial value of the projection's accumulator, added once per column, whatever
    the softmax weights sum to.  How large: an fp32 pre-activation of magnitude C carries 2^-24 C whoever computes
    it; with bias x 100 and shift + 10 the fp32 oracle itself is 2.9e-7 of the output scale from float64 on this
    model, beyond the 2e-7 bar for any fp32 arithmetic; at x 30 / + 3 it is 0.96e-7 (d = 64), half the bar."""
    n, w, k, b = 127, 15, 30, 12
    model = random_params(n, w, k, d, seed=73)
    with torch.no_grad():
        model.gnn_layers[0].gnn.bias.mul_(30.0)
        model.gnn_layers[0].bn.bias.add_(3.0)
    p = {key: v.detach().clone() for key, v in model.state_dict().items()}
    model = model.to(gpu_device).eval()
    x = torch.rand((b, n, w), generator=torch.Generator().manual_seed(74))
    assert_fp32_grade(model, p, x, k, gpu_device)


def _planned_launch_with_guard(model, x):
    from gdn_amd import _lib
    c = model._constants()
    plan = model._plan(c, False)
    torch.cuda.synchronize()
    ptrs, n, w, d, k = c.fused_args
    guard = torch.zeros(2, dtype=torch.int32, device=x.device)
    out = torch.empty((x.shape[0], n), dtype=torch.float32, device=x.device)
    _lib.call("gdn_forward_fused_plan", x.data_ptr(), plan.data_ptr(), x.shape[0], n, w, d, k, 0, out.data_ptr(),
              guard.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out, guard.tolist()


@pytest.mark.parametrize("n,w,k,d", [(127, 15, 30, 64), (40, 20, 12, 128)])
def test_inputs_at_the_x_limit(n, w, k, d, gpu_device):
    """The x limit of a plan is 60000 / 2^3 whatever lin' and C-in are (the projected tile no longer exists in 16
    bits).  Just below it the planned launch alone computes the batch and leaves its guard down; just above it
    the launch raises the guard and `model(x)` returns the gated fp32 recompute.  At these scales the logits are
    O(1e3): the bar is the one the raw-unit tests use (the fp32 oracle's own deviation from float64)."""
    b = 21
    model = random_params(n, w, k, d, seed=75)
    p = {key: v.detach().clone() for key, v in model.state_dict().items()}
    model = model.to(gpu_device).eval()
    with torch.no_grad():
        model(torch.rand((1, n, w)).to(gpu_device), None)
    limit = model.operand_limit()
    assert limit == 7500.0
    graph = model.learned_graph.cpu()
    g = torch.Generator().manual_seed(76)
    below = torch.rand((b, n, w), generator=g) * (0.999 * limit)
    below[2, 3, 0] = -0.9999 * limit
    below[b - 1, n - 1, w - 1] = 0.9999 * limit
    out, guard = _planned_launch_with_guard(model, below.to(gpu_device))
    assert guard == [0, 0]
    _assert_fp32_grade(out, p, below, k, graph, what="just below the limit, matrix cores alone")
    above = below.clone()
    above[5, n // 2, w // 2] = 1.0001 * limit
    _out, guard = _planned_launch_with_guard(model, above.to(gpu_device))
    assert guard[0] == 1
    with torch.no_grad():
        redone = model(above.to(gpu_device), None)
    _assert_fp32_grade(redone, p, above, k, graph, what="just above the limit, gated recompute")
    assert next(iter(model._constants().guards.values())).tolist() == [0, 0]


@pytest.mark.parametrize("n,w,k,d", [(127, 15, 30, 64), (33, 17, 20, 128)])
def test_series_and_keys_entries_equal_the_planned_launch_bit_for_bit(n, w, k, d, gpu_device):
    t = 700
    model = random_params(n, w, k, d, seed=77)
    p = {key: v.detach().clone() for key, v in model.state_dict().items()}
    model = model.to(gpu_device).eval()
    raw = torch.rand((n, t + w), generator=torch.Generator().manual_seed(78))
    x = raw.unfold(1, w, 1)[:, :t].permute(1, 0, 2).contiguous()
    dev_raw, dev_x = raw.to(gpu_device), x.to(gpu_device)
    gt = dev_raw[:, w:].t().contiguous()
    with torch.no_grad():
        plain = model.forward_into(dev_x, torch.empty((t, n), device=gpu_device))
        series = model.forward_series(dev_raw, 0, t)
        tail = model.forward_series(dev_raw, 41, t - 41)
        assert model.fused_keys_supported(False)
        keys = torch.zeros((n, t), dtype=torch.float64, device=gpu_device)
        keyed = model.forward_into(dev_x, torch.empty((t, n), device=gpu_device), keys=(gt, keys.data_ptr(), t))
        keys_s = torch.zeros((n, t), dtype=torch.float64, device=gpu_device)
        keyed_s = model.forward_series(dev_raw, 0, t, keys=(gt, keys_s.data_ptr(), t))
    torch.cuda.synchronize()
    assert torch.equal(series, plain) and torch.equal(tail, plain[41:])
    assert torch.equal(keyed, plain) and torch.equal(keyed_s, plain)
    want = (plain.double() - gt.double()).abs().t()
    assert torch.equal(keys, want) and torch.equal(keys_s, want)
    ref = gdn_oracle.forward(f64_params(p), x.double(), k, graph=model.learned_graph.cpu())["out"]
    err = float((plain.cpu().double() - ref).abs().max())
    assert err <= 2e-7 * max(1.0, float(ref.abs().max())), err
