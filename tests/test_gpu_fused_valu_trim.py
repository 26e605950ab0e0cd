"""The window loop of the fused dense forward (gdn_forward_dense.hip) with the trimmed vector instruction stream:
both 16-bit terms of a pair of values in three instructions (Fmt<FMT_F16>::split2), a one-instruction first ReLU
on the projection accumulator (relu_acc) and packed fp32 arithmetic on register pairs (Pk2).  None of the three
changes a bit of a finite result (tools/probe_fused_bits.py holds the digests of this file's shapes against the
library before the change), so what is asked here is what was asked before: `GDN.forward` against the float64
oracle at 2e-7 of the output scale (the bar of tests/test_gpu_fused_reordered.py), on a covering set of the
instantiations — n = 5 / 33 / 127 (one, two and four waves, each with pad rows), w = 5 / 15 / 16 and 30 (two window
k-steps), top-k 4 / 15 (8 list slots per lane) and 30 (16), d = 64 / 128 — each at batch 3 and at batch 769, which
leaves the workgroups of every instantiation with unequal window counts (768, 512 or 256 resident workgroups).
bf16 STORAGE rounds the windows and the projected tile to bf16, so float64 at 2e-7 is not a bar it can have: those
cases keep the bar of tests/test_gpu_dense_and_bf16.py (the oracle with storage="bf16", 2e-4 absolute).

Three cases aim at what the change touches: BatchNorm shifts that push most first-ReLU inputs below zero, with
columns whose input is exactly zero; attention vectors under which one neighbour takes nearly all the weight, so
that most weights sit near or below the f16 subnormal floor of the hi term and the lo terms carry them; and windows
with a NaN or a value beyond the x limit, where the guarded `GDN.forward` must return the row-gather kernel's bits."""
import pytest
import torch

from oracle import gdn_oracle
from test_gpu_forward_parity import random_params

pytestmark = pytest.mark.gpu

# (n, w, k, d, bf16)
CASES = [
    (127, 15, 30, 64, False),     # the headline instantiation
    (127, 30, 30, 64, False),     # two window k-steps
    (127, 16, 15, 64, True),
    (127, 5, 30, 128, True),
    (33, 15, 15, 64, False),
    (33, 16, 30, 128, False),
    (33, 5, 30, 64, True),
    (33, 30, 15, 128, True),
    (5, 5, 4, 64, False),
    (5, 16, 3, 128, False),
    (5, 30, 4, 64, True),
    (127, 16, 30, 128, False),
]
B_SMALL, B_UNEQUAL = 3, 769


def f64_params(p):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in p.items()}


def run_case(model, x, k, bf16, dev, what):
    """forward at both batch sizes against the oracle (computed once, at the larger batch)."""
    p = {key: v.detach().clone() for key, v in model.state_dict().items()}
    model = model.to(dev).eval()
    xin = x.bfloat16() if bf16 else x
    with torch.no_grad():
        big = model(xin.to(dev), None)
        small = model(xin[:B_SMALL].to(dev), None)
        torch.cuda.synchronize()
    graph = model.learned_graph.cpu()
    if bf16:
        ref = gdn_oracle.forward(f64_params(p), xin.double(), k, graph=graph, storage="bf16")
        bound = 2e-4
    else:
        ref = gdn_oracle.forward(f64_params(p), x.double(), k, graph=graph)
        bound = 2e-7 * max(1.0, float(ref["out"].abs().max()))
    for got, want, b in ((big, ref["out"], B_UNEQUAL), (small, ref["out"][:B_SMALL], B_SMALL)):
        assert got.shape == want.shape
        err = float((got.cpu().double() - want).abs().max())
        print(f"{what} b={b}: err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (what, b, err, bound)
    assert torch.equal(big[:B_SMALL], small)          # a window's result does not depend on the launch it is in
    return ref


@pytest.mark.parametrize("n,w,k,d,bf16", CASES, ids=lambda v: str(v))
def test_shapes_against_float64(n, w, k, d, bf16, gpu_device):
    model = random_params(n, w, k, d, seed=181)
    x = torch.rand((B_UNEQUAL, n, w), generator=torch.Generator().manual_seed(182))
    run_case(model, x, k, bf16, gpu_device, f"n={n} w={w} k={k} d={d} {'bf16' if bf16 else 'fp32'}")


@pytest.mark.parametrize("d", [64, 128])
def test_first_relu_mostly_negative_with_exact_zeros(d, gpu_device):
    n, w, k = 127, 15, 30
    model = random_params(n, w, k, d, seed=183)
    with torch.no_grad():
        gnn, bn = model.gnn_layers[0].gnn, model.gnn_layers[0].bn
        bn.bias.fill_(-1.5)                               # |lin' . Zx| is ~0.5: most columns end below zero
        bn.bias[d // 2:d // 2 + 6] = 0.5                  # ... a few well above
        zero = slice(3, 11)                               # ... and eight whose first-ReLU input is exactly 0
        gnn.lin.weight[zero] = 0.0
        gnn.bias[zero] = 0.0
        bn.bias[zero] = 0.0
        bn.running_mean[zero] = 0.0
    x = torch.rand((B_UNEQUAL, n, w), generator=torch.Generator().manual_seed(184))
    ref = run_case(model, x, k, False, gpu_device, f"negative first ReLU d={d}")
    # the case is what it says: the first ReLU's input is BatchNorm(aggregate), from the oracle's aggregate
    p = f64_params({key: v.detach().cpu() for key, v in model.state_dict().items()})
    pre = ((ref["agg"] - p["gnn_layers.0.bn.running_mean"]) / torch.sqrt(p["gnn_layers.0.bn.running_var"] + bn.eps)
           * p["gnn_layers.0.bn.weight"] + p["gnn_layers.0.bn.bias"])
    assert float((pre < 0).double().mean()) > 0.6 and int((pre == 0).sum()) == 8 * B_UNEQUAL * n


def test_weights_near_the_f16_subnormal_floor(gpu_device):
    n, w, k, d = 127, 15, 30, 64
    model = random_params(n, w, k, d, seed=185)
    with torch.no_grad():
        gnn = model.gnn_layers[0].gnn
        gnn.att_em_j.mul_(150.0)                          # logits spread over tens of units: one neighbour dominates
        gnn.att_j.mul_(20.0)
    x = torch.rand((B_UNEQUAL, n, w), generator=torch.Generator().manual_seed(186))
    ref = run_case(model, x, k, False, gpu_device, "dominant neighbour")
    alpha = ref["att_weight_1"].double().reshape(-1)
    scaled = alpha * 4096.0                               # what the kernel splits (GDN_F16_ALPHA_SCALE)
    near_floor = ((scaled > 1e-9) & (scaled < 6.2e-5)).double().mean()    # below the f16 normal range, above nothing
    print(f"weights: {float(near_floor):.2%} with a subnormal or vanishing hi term, max {float(alpha.max()):.4f}")
    assert float(near_floor) > 0.2 and float(alpha.max()) > 0.99


def test_nan_and_out_of_range_windows_equal_the_row_gather_kernel(gpu_device):
    n, w, k, d, b = 127, 15, 30, 64, 37
    model = random_params(n, w, k, d, seed=187).to(gpu_device).eval()
    g = torch.Generator().manual_seed(188)
    clean = torch.rand((b, n, w), generator=g)
    with torch.no_grad():
        limit = model.operand_limit()
        for what in ("nan", "big", "both"):
            x = clean.clone()
            if what in ("nan", "both"):
                x[5, 17, 3] = float("nan")
            if what in ("big", "both"):
                x[20, 90, 14] = -4.0 * limit
            xd = x.to(gpu_device)
            guarded = model(xd, None)
            gather = model.forward_into(xd, torch.empty((b, n), device=gpu_device), wide=True)
            torch.cuda.synchronize()
            assert torch.equal(guarded.view(torch.int32), gather.view(torch.int32)), what
            rows = [i for i in range(b) if i not in (5, 20)]      # (a window's result depends on that window only)
            assert bool(torch.isfinite(guarded[rows]).all())
        # the guard is down again: a clean batch comes from the matrix-core kernel and holds the bar
        out = model(clean.to(gpu_device), None)
        p = {key: v.detach().cpu().clone() for key, v in model.state_dict().items()}
        ref = gdn_oracle.forward(f64_params(p), clean.double(), k, graph=model.learned_graph.cpu())["out"]
        err = float((out.cpu().double() - ref).abs().max())
        assert err <= 2e-7 * max(1.0, float(ref.abs().max())), err
