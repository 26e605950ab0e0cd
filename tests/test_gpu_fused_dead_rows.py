"""The fused dense forward with fp32 storage at w <= 16 (gdn_forward_dense.hip, DCfg::XHALF) carries the lo term of
X^T in the product rows that no window column fills and adds them to the live rows in front of the projection
(tests/test_cpu_fused_dead_rows_emulation.py restates the chain).  `GDN.forward`, `forward_into` and `forward_series`
are held against the float64 oracle at the bar of tests/test_gpu_fused_reordered.py (2e-7 of the output scale) on
the smallest shapes that reach every changed path: the headline instantiation, w exactly 16 with three waves and
short lists, one live window column, d = 128; batches of 1, 3 and 769 (beyond two windows per workgroup: a workgroup
loops).  The windows form and the series form of one input are the same bits, and w = 17 (two window k-steps: code
this layout does not touch) still routes, runs, repeats itself and keeps the bar."""
import pytest
import torch

from oracle import gdn_oracle
from test_gpu_forward_parity import random_params

pytestmark = pytest.mark.gpu

SHAPES = [(127, 15, 30, 64), (65, 16, 15, 64), (127, 1, 30, 64), (100, 9, 20, 128)]   # (n, w, k, d)
BATCHES = (1, 3, 769)
T = max(BATCHES)


def f64_params(p):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in p.items()}


def series_case(n, w, k, d, seed, dev):
    """(model, state dict, raw series [n, T + w], its T windows [T, n, w], float64 reference [T, n])."""
    model = random_params(n, w, k, d, seed=seed)
    p = {key: v.detach().clone() for key, v in model.state_dict().items()}
    model = model.to(dev).eval()
    raw = torch.rand((n, T + w), generator=torch.Generator().manual_seed(seed + 1))
    x = raw.unfold(1, w, 1)[:, :T].permute(1, 0, 2).contiguous()
    with torch.no_grad():
        model(x[:1].to(dev), None)                       # the model learns its graph
    ref = gdn_oracle.forward(f64_params(p), x.double(), k, graph=model.learned_graph.cpu())["out"]
    return model, raw, x, ref


def assert_in_bar(got, ref, what):
    err = float((got.cpu().double() - ref).abs().max())
    bound = 2e-7 * max(1.0, float(ref.abs().max()))
    print(f"{what}: err {err:.3e} bound {bound:.3e}")
    assert err <= bound, (what, err, bound)


@pytest.mark.parametrize("n,w,k,d", SHAPES, ids=lambda v: str(v))
def test_every_entry_point_against_float64(n, w, k, d, gpu_device):
    model, raw, x, ref = series_case(n, w, k, d, 93, gpu_device)
    dev_raw, dev_x = raw.to(gpu_device), x.to(gpu_device)
    with torch.no_grad():
        for b in BATCHES:
            fwd = model(dev_x[:b], None)
            into = model.forward_into(dev_x[:b], torch.empty((b, n), device=gpu_device))
            series = model.forward_series(dev_raw, 0, b)
            torch.cuda.synchronize()
            assert_in_bar(fwd, ref[:b], f"forward b={b}")
            assert_in_bar(into, ref[:b], f"forward_into b={b}")
            assert_in_bar(series, ref[:b], f"forward_series b={b}")
            assert torch.equal(into, series) and torch.equal(fwd, into)
        tail = model.forward_series(dev_raw, 41, T - 41)     # a launch that starts inside the series
        torch.cuda.synchronize()
        assert torch.equal(tail, into[41:])


def test_two_window_k_steps_still_route_and_run(gpu_device):
    n, w, k, d = 127, 17, 30, 64
    model, raw, x, ref = series_case(n, w, k, d, 95, gpu_device)
    dev_x = x.to(gpu_device)
    with torch.no_grad():
        first = model.forward_into(dev_x, torch.empty((T, n), device=gpu_device))
        again = model.forward_into(dev_x, torch.empty((T, n), device=gpu_device))
        series = model.forward_series(raw.to(gpu_device), 0, T)
    torch.cuda.synchronize()
    assert torch.equal(first, again) and torch.equal(first, series)
    assert_in_bar(first, ref, "w = 17")
