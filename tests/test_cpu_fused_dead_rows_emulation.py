"""CPU emulation of the aggregation product of the fused dense forward with fp32 storage at w <= 16
(gdn_forward_dense.hip, DCfg::XHALF, phase M).  The product rows 16 .. 31, which no window column fills, carry the lo
term of X^T, so a target's aggregated window is accumulated in TWO fp32 chains over the k-steps of 16 sources and
added once in front of P1:

    rows r       sum_ks Xhi . ahi   then   + sum_ks Xhi . alo      (x 2^3 and alpha 2^12 in two float16 terms each)
    rows 16 + r  sum_ks Xlo . ahi   then   + sum_ks Xlo . alo
    fold         rows r + rows 16 + r, x 2^-12, split again for P1

(the lo pass keeps the hi pass's addressing, so the second chain ends with Xlo . alo: the fourth term of the exact
product, 2^-22 of it).  Every rounding is restated in numpy; the attention scalars, the softmax, P1 and the epilogue
are those of tests/test_cpu_fused_scalar_path_emulation.py, unchanged.  The result is held against the float64 oracle
at the bar of tests/test_gpu_fused_reordered.py (2e-7 of the output scale) on the shapes of
tests/test_gpu_fused_dead_rows.py, unit-scale inputs (torch.rand).

Emulated error / bound per shape (n, w, k, d), 16 windows:
    (127, 15, 30, 64)   1.30e-08 / 2.0e-07
    (65, 16, 15, 64)    2.76e-08 / 2.0e-07
    (127, 1, 30, 64)    9.77e-09 / 2.0e-07
    (100, 9, 20, 128)   1.79e-08 / 2.0e-07
"""
import numpy as np
import pytest
import torch

from oracle import gdn_oracle
from test_cpu_fused_reordered_emulation import (ALPHA_SCALE, LIN_SCALE, LOG2E, X_SCALE, Z_SCALE, f32, prod3, split2)
from test_cpu_fused_scalar_path_emulation import scalars_on_the_valu
from test_gpu_forward_parity import random_params

SHAPES = [(127, 15, 30, 64), (65, 16, 15, 64), (127, 1, 30, 64), (100, 9, 20, 128)]   # tests/test_gpu_fused_dead_rows.py
IDS = ["n{}_w{}_k{}_d{}".format(*s) for s in SHAPES]


def aggregate_two_chains(alpha, x):
    """Zx[b, target, w] x 2^15 as phase M leaves it in registers j and 8 + j, folded: alpha [b, n, n] x 2^12 and
    x [b, n, w] x 2^3 in fp32.  One k-step is one matrix-core product over 16 sources, added to the fp32 accumulator."""
    b, n, w = x.shape
    ks = 2 * ((n + 1 + 31) // 32)
    ap = np.zeros((b, n, 16 * ks), dtype=f32)
    ap[..., :n] = alpha
    xp = np.zeros((b, 16 * ks, w), dtype=f32)
    xp[:, :n] = x
    (ah, al), (xh, xl) = split2(ap), split2(xp)
    rows_lo = np.zeros((b, n, w), dtype=f32)          # accumulator registers 0 .. 7: the hi term of X^T
    rows_hi = np.zeros((b, n, w), dtype=f32)          # accumulator registers 8 .. 15: the lo term of X^T
    for a in (ah, al):                                # the alpha plane holds ahi, then alo
        for s in range(ks):
            k = slice(16 * s, 16 * s + 16)
            rows_lo = (rows_lo + np.matmul(a[..., k], xh[:, k], dtype=f32)).astype(f32)
            rows_hi = (rows_hi + np.matmul(a[..., k], xl[:, k], dtype=f32)).astype(f32)
    return (rows_lo + rows_hi).astype(f32)


def emulate(p, x, graph):
    """out[b, n] of the fused fp32-storage kernel at w <= 16; `p` fp32 state dict, x [b, n, w], graph [n, k]."""
    g = {k: v.numpy() for k, v in p.items()}
    n, d = g["embedding.weight"].shape
    w = x.shape[2]
    assert w <= 16
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
    # M: the two chains and the fold, then back to 2^3 by an exact power of two
    zx = aggregate_two_chains((e * inv.astype(f32)).astype(f32), (x * f32(X_SCALE)).astype(f32))
    zx = zx * f32(Z_SCALE / (ALPHA_SCALE * X_SCALE))
    # P1 as it stands: out = Zx . lin'^T + C-in, both in the accumulator's scale
    linp = split2((lin * sc1[:, None] * f32(LIN_SCALE)).T)
    cin = (g[pre + "bias"] * sc1 + sh1).astype(f32) * f32(Z_SCALE * LIN_SCALE)
    acc = prod3(split2(zx), linp, cin)
    # E
    e2 = (emb * sc2).astype(f32) * f32(1.0 / (Z_SCALE * LIN_SCALE))
    h = np.maximum(acc, 0)
    h = np.maximum(h * e2 + sh2, 0).astype(f32)
    ow = g["out_layer.mlp.0.weight"].reshape(-1).astype(f32)
    return (h @ ow).astype(f32) + g["out_layer.mlp.0.bias"].astype(f32)


def test_two_chains_and_fold_equal_the_plain_product_in_exact_arithmetic():
    """Integer-valued factors below 2^11 are their own hi term (lo = 0) and every partial sum is exact in fp32: the
    two chains and the fold must reproduce alpha . x, with the lo chain identically zero."""
    rng = np.random.default_rng(0)
    for n, w in ((127, 15), (65, 16), (127, 1), (100, 9), (5, 3)):
        alpha = rng.integers(0, 9, size=(2, n, n)).astype(f32)
        x = rng.integers(-8, 9, size=(2, n, w)).astype(f32)
        np.testing.assert_array_equal(aggregate_two_chains(alpha, x), alpha @ x)


def test_lo_term_of_x_is_added_exactly_once():
    """alpha a power of two on one source (its own hi term), x with a non-zero lo term: the fold returns hi + lo of
    that source's window, which is x to 2^-22: neither dropped (error 2^-12) nor added twice."""
    n, w = 65, 16
    rng = np.random.default_rng(1)
    x = (rng.random((1, n, w)) + 1.0).astype(f32)                    # [1, 2): hi carries 11 bits, lo the next 11
    alpha = np.zeros((1, n, n), dtype=f32)
    alpha[0, np.arange(n), (np.arange(n) * 7 + 3) % n] = 4096.0
    got = aggregate_two_chains(alpha, x) / f32(4096.0)
    want = x[:, (np.arange(n) * 7 + 3) % n]
    hi, lo = split2(x)
    assert float(np.abs(lo).max()) > 2.0 ** -13                      # the case has something to lose
    assert float(np.abs(got - want).max()) <= 2.0 ** -21


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_emulated_two_chain_aggregation_keeps_fp32_grade(shape):
    n, w, k, d = shape
    model = random_params(n, w, k, d, seed=91)
    x = torch.rand((16, n, w), generator=torch.Generator().manual_seed(92))
    p = {key: v.detach().clone() for key, v in model.state_dict().items()}
    graph = gdn_oracle.learned_graph(p["embedding.weight"], k)
    p64 = {key: (v.double() if v.is_floating_point() else v) for key, v in p.items()}
    ref = gdn_oracle.forward(p64, x.double(), k, graph=graph)["out"].numpy()
    err = float(np.abs(emulate(p, x, graph).astype(np.float64) - ref).max())
    bound = 2e-7 * max(1.0, float(np.abs(ref).max()))
    print(f"emulated two-chain aggregation vs float64: err {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)
