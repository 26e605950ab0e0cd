"""CPU emulation of the operand chain of the fused dense forward with fp32 storage (gdn_forward_dense.hip,
DCfg::XAGG): the raw window is aggregated first and projected afterwards, every matrix-core operand is two float16
terms of an fp32 value times a power of two, every product accumulates in fp32.  The emulation restates exactly
those roundings in numpy (float16 terms, float32 sums) and is compared with the float64 oracle at the bar the GPU
test holds the kernel to (2e-7 of the output scale): the scales below are the kernel's, so a change of scales that
loses accuracy shows here, without a GPU."""
import numpy as np
import pytest
import torch

from oracle import gdn_oracle
from test_gpu_forward_parity import random_params

X_SCALE = 8.0          # GDN_F16_XT_SCALE: x operand of the aggregation
ALPHA_SCALE = 4096.0   # GDN_F16_ALPHA_SCALE
Z_SCALE = 8.0          # GDN_F16_Z_SCALE: the aggregated row, operand of the projection
LIN_SCALE = 8.0        # GDN_F16_X_SCALE: lin' operand
LOG2E = np.float32(1.44269504088896340736)
f32 = np.float32

SHAPES = [dict(b=16, n=127, w=15, k=30), dict(b=64, n=27, w=5, k=5), dict(b=8, n=64, w=15, k=63),
          dict(b=5, n=100, w=30, k=40), dict(b=3, n=33, w=12, k=1), dict(b=700, n=51, w=15, k=15),
          dict(b=9, n=60, w=32, k=20), dict(b=4, n=127, w=17, k=63)]        # as tests/test_gpu_dense_and_bf16.py
IDS = ["b{b}_n{n}_w{w}_k{k}".format(**s) for s in SHAPES]


def split2(v):
    """fp32 -> two float16 terms (round to nearest even; the residual is exact in fp32), returned as fp32."""
    v = v.astype(f32)
    hi = v.astype(np.float16).astype(f32)
    lo = (v - hi).astype(np.float16).astype(f32)
    return hi, lo


def prod3(a, b, c=None):
    """hi*hi + lo*hi + hi*lo of two split factors, fp32 accumulate: a [.., m, k] @ b [.., k, n] (+ c)."""
    (ah, al), (bh, bl) = a, b
    acc = np.matmul(ah, bh, dtype=f32) + np.matmul(al, bh, dtype=f32) + np.matmul(ah, bl, dtype=f32)
    return acc if c is None else (acc + c).astype(f32)


def emulate(p, x, graph):
    """out[b, n] of the reordered fp32-storage kernel; `p` fp32 state dict, x [b, n, w], graph [n, k]."""
    g = {k: v.numpy() for k, v in p.items()}
    n, d = g["embedding.weight"].shape
    pre = "gnn_layers.0.gnn."
    lin = g[pre + "lin.weight"].astype(f32)                                    # [d, w]
    x = x.numpy().astype(f32)

    def affine(prefix):
        sc = (g[prefix + "weight"] / np.sqrt(g[prefix + "running_var"] + f32(gdn_oracle.BN_EPS))).astype(f32)
        return sc, (g[prefix + "bias"] - g[prefix + "running_mean"] * sc).astype(f32)
    sc1, sh1 = affine("gnn_layers.0.bn.")
    sc2, sh2 = affine("bn_outlayer_in.")
    emb = g["embedding.weight"].astype(f32)
    # P0: attention scalars from x itself (unscaled terms), log2 domain
    a_i = (g[pre + "att_i"].reshape(-1) @ lin).astype(f32) * LOG2E
    a_j = (g[pre + "att_j"].reshape(-1) @ lin).astype(f32) * LOG2E
    c_i = (emb @ g[pre + "att_em_i"].reshape(-1)).astype(f32) * LOG2E
    c_j = (emb @ g[pre + "att_em_j"].reshape(-1)).astype(f32) * LOG2E
    xs = split2(x)
    s_i = prod3(xs, tuple(t[:, None] for t in split2(a_i)))[..., 0] + c_i
    s_j = prod3(xs, tuple(t[:, None] for t in split2(a_j)))[..., 0] + c_j
    # S: softmax over the list of every target (the top-k row without the target, plus the target)
    mask = np.zeros((n, n), dtype=bool)
    mask[np.arange(n)[:, None], graph.numpy()] = True
    mask[np.arange(n), np.arange(n)] = True
    e = s_i[:, :, None] + s_j[:, None, :]
    e = np.where(e > 0, e, f32(gdn_oracle.NEG_SLOPE) * e).astype(f32)
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
    print(f"emulated operand chain vs float64: err {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_emulated_operand_chain_keeps_fp32_grade(shape):
    model = random_params(shape["n"], shape["w"], shape["k"], 64, seed=5)
    x = torch.rand((min(shape["b"], 16), shape["n"], shape["w"]), generator=torch.Generator().manual_seed(6))
    check(model, x, shape["k"])


def test_emulated_operand_chain_on_the_bench_model():
    model = random_params(127, 15, 30, 64, seed=0)
    x = torch.rand((8, 127, 15), generator=torch.Generator().manual_seed(0))
    check(model, x, 30)


def test_emulated_operand_chain_with_large_bias_and_inputs_near_the_limit():
    """C-in enters behind the aggregation (no reliance on the weights summing to 1), and inputs just below the
    x limit (60000 / 2^3) keep every 16-bit term finite."""
    model = random_params(127, 15, 30, 64, seed=9)
    with torch.no_grad():
        model.gnn_layers[0].gnn.bias.mul_(30.0)
        model.gnn_layers[0].bn.bias.add_(3.0)
    x = torch.rand((4, 127, 15), generator=torch.Generator().manual_seed(10))
    check(model, x, 30)
    model = random_params(64, 15, 20, 64, seed=11)
    x = torch.rand((4, 64, 15), generator=torch.Generator().manual_seed(12)) * 7400.0
    p = {key: v.detach().clone() for key, v in model.state_dict().items()}
    graph = gdn_oracle.learned_graph(p["embedding.weight"], 20)
    got = emulate(p, x, graph)
    assert np.isfinite(got).all()
    # at this scale the logits are O(1e3) and fp32 softmax itself is the error: the fp32 oracle's own deviation
    p64 = {key: (v.double() if v.is_floating_point() else v) for key, v in p.items()}
    ref = gdn_oracle.forward(p64, x.double(), 20, graph=graph)["out"].numpy()
    ref32 = gdn_oracle.forward(p, x, 20, graph=graph)["out"].double().numpy()
    scale = max(1.0, float(np.abs(ref).max()))
    bound = 4.0 * float(np.abs(ref32 - ref).max()) + 2e-5 * scale
    assert float(np.abs(got - ref).max()) <= bound
