"""CPU emulation of the fused dense forward with fp32 storage as it computes the attention scalars on the VALU
(gdn_forward_dense.hip, DCfg::XAGG, phase X): s_i / s_j of a source are fp32 dot products of its window with the
folded coefficients a_i' / a_j' (log2 e included), reduced over the lanes that hold the source's columns in the order
of the kernel's halving butterfly; the softmax runs in the log2 domain; the aggregation of the raw window and the
projection behind it are the split-f16 chain of tests/test_cpu_fused_reordered_emulation.py, unchanged.  Every
rounding is restated in numpy and the result is held against the float64 oracle at the bar the GPU tests hold the
kernel to (2e-7 of the output scale), on the shapes of tests/test_gpu_fused_reordered.py."""
import numpy as np
import pytest
import torch

from oracle import gdn_oracle
from test_cpu_fused_reordered_emulation import (ALPHA_SCALE, LIN_SCALE, LOG2E, X_SCALE, Z_SCALE, f32, prod3, split2)
from test_gpu_forward_parity import random_params
from test_gpu_fused_reordered import CASES

IDS = ["n{}_w{}_k{}_d{}".format(*c[:4]) for c in CASES]


def source_slot(n, w):
    """(lane-low-bits index of every source row, columns per row CW) of the kernel's x staging: a thread holds
    column c of the 8 WK sources  row = 16 s + 4 hh + 16 NT q + 8 (u >> 2) + (u & 3)  of its slot (s, hh); after
    the butterfly the lane with low bits 8 q + u holds the scalar of that source."""
    nt, wk = (n + 1 + 31) // 32, 1 if w <= 16 else 2
    idx = np.zeros(32 * nt, dtype=np.int64)
    for slot in range(64 * nt // (16 * wk)):
        row0 = 16 * (slot >> 1) + 4 * (slot & 1)
        for i in range(8 * wk):
            idx[row0 + 16 * nt * (i >> 3) + 8 * ((i & 7) >> 2) + (i & 3)] = i
    return idx, 16 * wk


def fma32(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in float64, one rounding of the sum to
    float64 in between is far below the final rounding to fp32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def scalars_on_the_valu(x, a, c, kind, n, w):
    """s[b, row] = c[row] + sum_col x[b, row, col] a[col] in fp32, in the kernel's order.  kind 0 = s_i, 1 = s_j."""
    idx, cw = source_slot(n, w)
    half = cw // 2
    xp = np.zeros(x.shape[:2] + (cw,), dtype=f32)
    xp[..., :w] = x
    ap = np.zeros(cw, dtype=f32)
    ap[:w] = a
    # first exchange: the lanes whose column has bit `half` equal to `kind` keep this kind; partner column = own
    # column with every bit flipped (WK = 1, row mirror) or with bit 16 flipped (WK = 2)
    own = kind * half + np.arange(half)
    partner = own ^ (15 if cw == 16 else 16)
    v = fma32(xp[..., partner], ap[partner], (xp[..., own] * ap[own]).astype(f32))      # [b, n, half]
    low = np.arange(half)
    for m in ([15] if cw == 32 else []) + [7, 3, 1]:       # row mirror, half mirror, quad reverse, pair swap
        v = (v + v[..., low ^ m]).astype(f32)
    s = np.take_along_axis(v, np.broadcast_to(idx[:x.shape[1]], x.shape[:2])[..., None], axis=-1)[..., 0]
    return (s + c).astype(f32)


def emulate(p, x, graph):
    """out[b, n] of the fused fp32-storage kernel; `p` fp32 state dict, x [b, n, w], graph [n, k]."""
    g = {k: v.numpy() for k, v in p.items()}
    n, d = g["embedding.weight"].shape
    w = x.shape[2]
    pre = "gnn_layers.0.gnn."
    lin = g[pre + "lin.weight"].astype(f32)                                    # [d, w]
    x = x.numpy().astype(f32)

    def affine(prefix):
        sc = (g[prefix + "weight"] / np.sqrt(g[prefix + "running_var"] + f32(gdn_oracle.BN_EPS))).astype(f32)
        return sc, (g[prefix + "bias"] - g[prefix + "running_mean"] * sc).astype(f32)
    sc1, sh1 = affine("gnn_layers.0.bn.")
    sc2, sh2 = affine("bn_outlayer_in.")
    emb = g["embedding.weight"].astype(f32)
    # X: attention scalars, fp32 on the VALU, log2 domain
    a_i = (g[pre + "att_i"].reshape(-1) @ lin).astype(f32) * LOG2E
    a_j = (g[pre + "att_j"].reshape(-1) @ lin).astype(f32) * LOG2E
    c_i = (emb @ g[pre + "att_em_i"].reshape(-1)).astype(f32) * LOG2E
    c_j = (emb @ g[pre + "att_em_j"].reshape(-1)).astype(f32) * LOG2E
    s_i = scalars_on_the_valu(x, a_i, c_i, 0, n, w)
    s_j = scalars_on_the_valu(x, a_j, c_j, 1, n, w)
    # S: softmax over the list of every target (the top-k row without the target, plus the target)
    mask = np.zeros((n, n), dtype=bool)
    mask[np.arange(n)[:, None], graph.numpy()] = True
    mask[np.arange(n), np.arange(n)] = True
    e = s_i[:, :, None] + s_j[:, None, :]
    e = np.maximum(e, f32(gdn_oracle.NEG_SLOPE) * e).astype(f32)
    e = np.where(mask[None], e, -np.inf).astype(f32)
    e = np.exp2(e - e.max(-1, keepdims=True)).astype(f32)
    inv = (f32(1.0) / (e.sum(-1, keepdims=True, dtype=f32) / f32(ALPHA_SCALE) + f32(gdn_oracle.SOFTMAX_EPS / ALPHA_SCALE)))
    alpha = split2(e * inv.astype(f32))                                        # [b, n, n] x 2^12
    # M: Zx = alpha . x on the raw window (x 2^3), then back to 2^3 by an exact power of two
    zx = prod3(alpha, split2(x * f32(X_SCALE))) * f32(Z_SCALE / (ALPHA_SCALE * X_SCALE))
    # P1: out = Zx . lin'^T + C-in, both in the accumulator's scale
    linp = split2((lin * sc1[:, None] * f32(LIN_SCALE)).T)
    cin = (g[pre + "bias"] * sc1 + sh1).astype(f32) * f32(Z_SCALE * LIN_SCALE)
    acc = prod3(split2(zx), linp, cin)
    # E
    e2 = (emb * sc2).astype(f32) * f32(1.0 / (Z_SCALE * LIN_SCALE))
    h = np.maximum(acc, 0)
    h = np.maximum(h * e2 + sh2, 0).astype(f32)
    ow = g["out_layer.mlp.0.weight"].reshape(-1).astype(f32)
    return (h @ ow).astype(f32) + g["out_layer.mlp.0.bias"].astype(f32)


def check(model, x, k, bound_rel=2e-7):
    p = {key: v.detach().clone() for key, v in model.state_dict().items()}
    graph = gdn_oracle.learned_graph(p["embedding.weight"], k)
    p64 = {key: (v.double() if v.is_floating_point() else v) for key, v in p.items()}
    ref = gdn_oracle.forward(p64, x.double(), k, graph=graph)["out"].numpy()
    got = emulate(p, x, graph).astype(np.float64)
    err = float(np.abs(got - ref).max())
    bound = bound_rel * max(1.0, float(np.abs(ref).max()))
    print(f"emulated scalar path + operand chain vs float64: err {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)


def test_every_source_row_has_one_lane():
    for n, w in ((1, 1), (31, 15), (32, 16), (33, 17), (63, 32), (96, 30), (127, 15), (127, 32)):
        idx, cw = source_slot(n, w)
        nt = (n + 1 + 31) // 32
        # every slot's 8 WK sources are distinct rows and the slots tile the 32 NT rows
        rows = set()
        for slot in range(64 * nt // cw):
            row0 = 16 * (slot >> 1) + 4 * (slot & 1)
            for i in range(cw // 2):
                rows.add(row0 + 16 * nt * (i >> 3) + 8 * ((i & 7) >> 2) + (i & 3))
        assert rows == set(range(32 * nt)) and idx.max() == cw // 2 - 1


def test_butterfly_equals_the_plain_dot_product_in_exact_arithmetic():
    """Integer-valued inputs: every partial sum is exact in fp32, so the butterfly must reproduce x . a + c."""
    rng = np.random.default_rng(0)
    for n, w in ((127, 15), (33, 17), (60, 32), (5, 1), (96, 16)):
        x = rng.integers(-8, 9, size=(3, n, w)).astype(f32)
        a = rng.integers(-8, 9, size=w).astype(f32)
        c = rng.integers(-8, 9, size=n).astype(f32)
        for kind in (0, 1):
            np.testing.assert_array_equal(scalars_on_the_valu(x, a, c, kind, n, w), x @ a + c)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_emulated_scalar_path_keeps_fp32_grade(case):
    n, w, k, d, b = case
    model = random_params(n, w, k, d, seed=71)
    x = torch.rand((min(b, 16), n, w), generator=torch.Generator().manual_seed(72))
    check(model, x, k)


def test_emulated_scalar_path_on_the_bench_model():
    model = random_params(127, 15, 30, 64, seed=0)
    x = torch.rand((8, 127, 15), generator=torch.Generator().manual_seed(0))
    check(model, x, 30)


def test_emulated_scalar_path_with_attention_that_follows_the_window():
    """att_i / att_j four times their initial size: the x-dependent part of the logits outweighs the embedding part
    (tests/test_gpu_fused_three_wg.py runs the same model on the GPU)."""
    model = random_params(127, 15, 30, 64, seed=81)
    with torch.no_grad():
        model.gnn_layers[0].gnn.att_i.mul_(4.0)
        model.gnn_layers[0].gnn.att_j.mul_(4.0)
    x = torch.rand((8, 127, 15), generator=torch.Generator().manual_seed(82))
    check(model, x, 30)
