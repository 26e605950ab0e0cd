"""GPU suite: the matrix-core ("dense") kernels of gdn_amd/csrc/gdn_forward_dense.hip — fused forward,
staged projection and gather-aggregate — and the bf16-STORAGE variants BASELINE.json configs[2] / configs[4]
name, against the oracle.

fp32 storage: north_star's bar is 1e-4; the dense kernels split both factors of every product into two f16
terms (fp32-grade) and are held to the same 2e-5 / 2e-6-vs-float64 bars as the VALU kernels.

bf16 storage (include/gdn_hip.h "bf16 STORAGE variants"): the oracle is fed the same bf16 inputs and rounds
xlin (and, staged, z) to bf16 where the kernels store them.  TOLERANCE, stated here because neither the
reference nor north_star defines one for bf16: stored tensors must equal the oracle's bf16 values except for
<= 0.2 % of the elements, which may differ by ONE bf16 ulp (the fp32 value behind a stored number sits on a
rounding boundary, and the kernels' fp32 summation order is not the oracle's); final predictions within 2e-4
absolute (observed <= 5e-5; the bf16 storage itself moves predictions by ~3e-5 relative to the fp32 path)."""
import numpy as np
import pytest
import torch

from conftest import load_golden, meta
from oracle import gdn_oracle
from test_gpu_forward_parity import build_model, random_params

pytestmark = pytest.mark.gpu

SHAPES = [dict(b=16, n=127, w=15, k=30), dict(b=64, n=27, w=5, k=5), dict(b=8, n=64, w=15, k=63),
          dict(b=5, n=100, w=30, k=40), dict(b=3, n=33, w=12, k=1), dict(b=700, n=51, w=15, k=15),
          dict(b=9, n=60, w=32, k=20), dict(b=4, n=127, w=17, k=63)]
IDS = ["b{b}_n{n}_w{w}_k{k}".format(**s) for s in SHAPES]


def f64_params(p):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in p.items()}


def setup(shape, device, seed=5):
    model = random_params(shape["n"], shape["w"], shape["k"], 64, seed=seed)
    p = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(device).eval()
    x = torch.rand((shape["b"], shape["n"], shape["w"]), generator=torch.Generator().manual_seed(seed + 1))
    return model, p, x


def bf16_ulp(t):
    """One unit in the last place of the bf16 numbers nearest to t (8 significant bits)."""
    return torch.exp2(torch.floor(torch.log2(t.abs().clamp_min(1e-30))) - 7)


def assert_bf16_stored(got, want, name, fp32_floor=0.0):
    """`fp32_floor`: absolute error the fp32 computation behind the stored value may carry (a sum whose terms
    cancel has an error set by its TERMS, which can exceed one ulp of a small result)."""
    got, want = got.float().cpu().double(), want.double()
    diff = (got - want).abs()
    bad = diff > 0
    assert bad.double().mean() <= 2e-3, f"{name}: {bad.double().mean():.2e} of the stored bf16 values differ"
    allowed = torch.clamp_min(1.01 * bf16_ulp(want[bad]), fp32_floor)
    assert bool((diff[bad] <= allowed).all()), f"{name}: a stored value is off by more than one bf16 ulp"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_dense_staged_kernels_fp32_against_float64_oracle(shape, gpu_device):
    """gdn_project_fwd / gdn_attn_aggregate_fwd / gdn_head_fwd on the matrix-core path (these shapes all
    take it) against the float64 oracle, intermediate by intermediate."""
    from gdn_amd import ops
    model, p, x = setup(shape, gpu_device)
    c = model._constants()
    gnn, lin = model.gnn_layers[0].gnn, model.out_layer.mlp[0]
    ref = gdn_oracle.forward(f64_params(p), x.double(), shape["k"], graph=c.graph.topk.cpu())
    xlin, s_i, s_j = ops.project_fwd(x.to(gpu_device), gnn.lin.weight, c.terms)
    np.testing.assert_allclose(xlin.cpu().double().numpy(), ref["xlin"].numpy(), atol=2e-6, rtol=1e-5)
    z, alpha = ops.attn_aggregate_fwd(xlin, s_i, s_j, c.graph, gnn.bias, shape["b"], want_alpha=True)
    np.testing.assert_allclose(z.cpu().double().numpy(), ref["agg"].numpy(), atol=2e-6, rtol=1e-5)
    layer = model.gnn_layers[0]
    layer._set_dense((alpha, c.graph, shape["b"]))
    np.testing.assert_allclose(layer.att_weight_1.cpu().double().numpy(), ref["att_weight_1"].numpy(), atol=2e-6, rtol=0)
    a = alpha.cpu()
    np.testing.assert_allclose(a.sum(1).numpy(), 1.0, atol=1e-5)
    pad = torch.arange(c.graph.pitch).view(1, -1) >= c.graph.deg.cpu().view(-1, 1)
    assert float(a.view(shape["b"], shape["n"], -1)[:, pad].abs().max()) == 0.0      # padding slots exactly 0
    out, _ = ops.head_fwd(z, model.embedding.weight, c.bn1, c.bn2, lin.weight, lin.bias, shape["b"])
    np.testing.assert_allclose(out.cpu().double().numpy(), ref["out"].numpy(), atol=2e-6, rtol=1e-5)


@pytest.mark.parametrize("shape", SHAPES[:3], ids=IDS[:3])
def test_dense_kernels_are_deterministic_and_alpha_does_not_change_z(shape, gpu_device):
    """Same launch twice = same bits; asking for the attention weights does not change z (to rounding);
    the fused kernel gives the same bits for a window whatever launch it is part of."""
    from gdn_amd import ops
    model, _p, x = setup(shape, gpu_device)
    c = model._constants()
    gnn = model.gnn_layers[0].gnn
    xd = x.to(gpu_device)
    xlin, s_i, s_j = ops.project_fwd(xd, gnn.lin.weight, c.terms)
    xlin2, s_i2, s_j2 = ops.project_fwd(xd, gnn.lin.weight, c.terms)
    assert torch.equal(xlin, xlin2) and torch.equal(s_i, s_i2) and torch.equal(s_j, s_j2)
    z0, _ = ops.attn_aggregate_fwd(xlin, s_i, s_j, c.graph, gnn.bias, shape["b"], want_alpha=False)
    z1, _ = ops.attn_aggregate_fwd(xlin, s_i, s_j, c.graph, gnn.bias, shape["b"], want_alpha=False)
    z2, _ = ops.attn_aggregate_fwd(xlin, s_i, s_j, c.graph, gnn.bias, shape["b"], want_alpha=True)
    assert torch.equal(z0, z1)
    # the two variants are separate instantiations, and without alpha the launch reads the bank-ordered lists (the
    # softmax denominator is then summed in another order): equal to the last few bits, not bit for bit.  (An
    # earlier build, with the 16-bit split written as inline asm, failed here by 3e-5 in ONE target row of ONE
    # window: hipcc pads no hazards around asm.)
    np.testing.assert_allclose(z0.cpu().numpy(), z2.cpu().numpy(), atol=1e-6, rtol=0)
    with torch.no_grad():
        o0, o1 = model(xd, None), model(xd, None)
        o2 = model(xd[1:3].contiguous(), None)
    assert torch.equal(o0, o1) and torch.equal(o0[1:3], o2)


@pytest.mark.parametrize("bf16", [False, True])
def test_planned_launch_equals_the_plain_entry_point(bf16, gpu_device):
    """gdn_forward_fused_plan (constants precomputed by gdn_fused_plan_build, what GDN.forward uses) against
    gdn_forward_fused / gdn_forward_fused_bf16 (constants computed in every workgroup's prologue): the same
    results up to the summation order of the softmax denominator (the plan also reorders each lane's list
    slots to spread LDS banks); and the plan follows the parameters (rebuilt after an update)."""
    from gdn_amd import ops
    shape = dict(b=300, n=127, w=15, k=30)
    model, _p, x = setup(shape, gpu_device)
    xd = (x.bfloat16() if bf16 else x).to(gpu_device)
    c = model._constants()
    gnn, lin = model.gnn_layers[0].gnn, model.out_layer.mlp[0]
    with torch.no_grad():
        planned = model(xd, None)
    assert c.plans[bf16] is not None
    plain = ops.forward_fused(xd, gnn.lin.weight, c.terms, c.graph, gnn.bias, model.embedding.weight, c.bn1, c.bn2,
                              lin.weight, lin.bias)
    np.testing.assert_allclose(planned.cpu().numpy(), plain.cpu().numpy(), atol=2e-7, rtol=0)
    with torch.no_grad():
        gnn.lin.weight.mul_(1.25)                      # version bump -> constants and plan are rebuilt
        again = model(xd, None)
    assert not torch.equal(again, planned)
    c2 = model._constants()
    plain2 = ops.forward_fused(xd, gnn.lin.weight, c2.terms, c2.graph, gnn.bias, model.embedding.weight, c2.bn1,
                               c2.bn2, lin.weight, lin.bias)
    np.testing.assert_allclose(again.cpu().numpy(), plain2.cpu().numpy(), atol=2e-7, rtol=0)


def test_valu_and_dense_fused_paths_agree(gpu_device, tmp_path):
    """The fp32 VALU row-gather kernel (GDN_FUSED_PATH=valu, also the path of every shape the dense kernels
    do not take) and the matrix-core kernel on the same inputs, in two processes (the choice is read once)."""
    import os
    import subprocess
    import sys
    code = ("import sys, torch; sys.path.insert(0, %r); sys.path.insert(0, %r + '/tests');"
            "from test_gpu_forward_parity import random_params;"
            "m = random_params(127, 15, 30, 64, seed=2).to('cuda:0').eval();"
            "x = torch.rand((64, 127, 15), generator=torch.Generator().manual_seed(3)).to('cuda:0');"
            "torch.save(m(x, None).cpu(), sys.argv[1])")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for path in ("dense", "valu"):
        f = str(tmp_path / f"gdn_path_{path}.pt")
        subprocess.run([sys.executable, "-c", code % (root, root), f], check=True,
                       env=dict(os.environ, GDN_FUSED_PATH=path))
        outs.append(torch.load(f, weights_only=True))
    assert not torch.equal(outs[0], outs[1])             # really two implementations
    np.testing.assert_allclose(outs[0].numpy(), outs[1].numpy(), atol=4e-6, rtol=0)


def test_valu_staged_aggregate_gets_rank_ordered_lists(gpu_device, tmp_path):
    """Under GDN_FUSED_PATH=valu the staged aggregate routes to the row-gather kernel, which walks ceil(deg / 16)
    rounds of a RANK-ordered list: ops.attn_aggregate_fwd asks the library's route (gdn_kernel_family) and must not
    hand it the bank-ordered copy.  n = 40, k = 32 with every sensor in its own top-k: pitch 48, deg 32 — the smallest
    shape where the bank permutation moves a valid entry past round 2.  z without alpha must equal, bit for bit, z of
    the want_alpha call (always rank-ordered) in the same process."""
    import os
    import subprocess
    import sys
    code = ("import sys, torch; sys.path.insert(0, %r);"
            "from gdn_amd import ops;"
            "g = torch.Generator().manual_seed(5); n, w, d, k, b = 40, 8, 64, 32, 3;"
            "r = lambda *s: (torch.rand(s, generator=g) * 2 - 1).to('cuda:0');"
            "emb, lin_w, bias, x = r(n, d), r(d, w) * 0.3, r(d) * 0.1, r(b, n, w);"
            "graph = ops.topk_graph(emb, k);"
            "terms = ops.node_terms(lin_w, r(d) * 0.3, r(d) * 0.3, r(d) * 0.3, r(d) * 0.3, emb);"
            "xlin, s_i, s_j = ops.project_fwd(x, lin_w, terms);"
            "za, _ = ops.attn_aggregate_fwd(xlin, s_i, s_j, graph, bias, b, want_alpha=True);"
            "zb, _ = ops.attn_aggregate_fwd(xlin, s_i, s_j, graph, bias, b, want_alpha=False);"
            "torch.save((za.cpu(), zb.cpu(), graph.deg.cpu(), graph.pitch), sys.argv[1])")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    f = str(tmp_path / "valu_aggregate.pt")
    subprocess.run([sys.executable, "-c", code % root, f], check=True, env=dict(os.environ, GDN_FUSED_PATH="valu"))
    za, zb, deg, pitch = torch.load(f, weights_only=True)
    assert pitch == 48 and bool((deg == 32).all())
    assert bool(za.abs().sum() > 0) and torch.equal(za, zb)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bf16_storage_fused_forward(shape, gpu_device):
    """GDN.forward on bfloat16 windows (bf16 storage of x and of the LDS-resident projected tile)."""
    model, p, x = setup(shape, gpu_device)
    xb = x.bfloat16()
    with torch.no_grad():
        out = model(xb.to(gpu_device), None)
    assert out.dtype == torch.float32
    graph = model.learned_graph.cpu()
    ref = gdn_oracle.forward(f64_params(p), xb.double(), shape["k"], graph=graph, storage="bf16")
    np.testing.assert_allclose(out.cpu().double().numpy(), ref["out"].numpy(), atol=2e-4, rtol=0)
    fp32 = gdn_oracle.forward(f64_params(p), x.double(), shape["k"], graph=graph)
    assert float((out.cpu().double() - fp32["out"]).abs().max()) < 5e-3   # storage precision, not garbage


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bf16_storage_staged_pipeline(shape, gpu_device):
    """gdn_project_fwd_bf16 -> gdn_attn_aggregate_fwd_bf16 -> gdn_head_fwd_bf16, every stored tensor."""
    from gdn_amd import ops
    model, p, x = setup(shape, gpu_device)
    c = model._constants()
    gnn, lin = model.gnn_layers[0].gnn, model.out_layer.mlp[0]
    xb = x.bfloat16()
    ref = gdn_oracle.forward(f64_params(p), xb.double(), shape["k"], graph=c.graph.topk.cpu(), storage="bf16",
                             round_agg=True)
    xlin, s_i, s_j = ops.project_fwd(xb.to(gpu_device), gnn.lin.weight, c.terms)
    assert xlin.dtype == torch.bfloat16
    assert_bf16_stored(xlin, ref["xlin"], "xlin")
    # the scalars come from the unrounded projection: s = x.a + c (graph_layer.py:94-104 folded)
    p64 = f64_params(p)
    d = 64
    full = xb.double().view(-1, shape["w"]) @ p64["gnn_layers.0.gnn.lin.weight"].T
    emb = p64["embedding.weight"]
    want_si = (full @ p64["gnn_layers.0.gnn.att_i"].view(d)).view(shape["b"], -1) + emb @ p64["gnn_layers.0.gnn.att_em_i"].view(d)
    np.testing.assert_allclose(s_i.cpu().double().numpy(), want_si.reshape(-1).numpy(), atol=2e-6, rtol=1e-5)
    z, alpha = ops.attn_aggregate_fwd(xlin, s_i, s_j, c.graph, gnn.bias, shape["b"], want_alpha=True)
    assert z.dtype == torch.bfloat16
    # z against the aggregate of THE STORED xlin (a one-ulp difference in xlin moves z by more than an ulp
    # of a small z): sum over the list slots in float64 with the oracle's attention weights, rounded once
    b, n = shape["b"], shape["n"]
    nbr = c.graph.nbr.cpu().long()
    xl = torch.cat((xlin.float().cpu().double().view(b, n, d), torch.zeros((b, 1, d), dtype=torch.float64)), 1)
    layer = model.gnn_layers[0]
    layer._set_dense((alpha, c.graph, b))
    np.testing.assert_allclose(layer.att_weight_1.cpu().double().numpy(), ref["att_weight_1"].numpy(), atol=2e-6, rtol=0)
    a64 = alpha.cpu().double().view(b, n, -1)
    want_z = (a64.unsqueeze(-1) * xl[:, nbr]).sum(2) + p64["gnn_layers.0.gnn.bias"]
    # alpha enters the product as two bf16 terms (2^-17 relative): 1e-5 of the largest feature
    assert_bf16_stored(z, gdn_oracle.round_bf16(want_z).view(b * n, d), "z", fp32_floor=1e-5 * float(xl.abs().max()))
    out, _ = ops.head_fwd(z, model.embedding.weight, c.bn1, c.bn2, lin.weight, lin.bias, shape["b"])
    np.testing.assert_allclose(out.cpu().double().numpy(), ref["out"].numpy(), atol=2e-4, rtol=0)


def test_bf16_storage_at_baseline_config2_batch_512(gpu_device):
    """BASELINE configs[2] as worded: 127 sensors, top-k 30, W=15, batch 512, bf16 — on the fixture's
    parameters; the fp32 reference output bounds how far bf16 storage may move a prediction."""
    from test_oracle_golden import full_batch_input
    data, p = load_golden("cfg2_swat127_w15_k30_b512")
    m = meta(data)
    model = build_model(p, m, gpu_device)
    xb = full_batch_input(data).bfloat16()
    with torch.no_grad():
        out = model(xb.to(gpu_device), None)
    ref = gdn_oracle.forward(f64_params(p), xb.double(), m["k"], graph=model.learned_graph.cpu(), storage="bf16")
    np.testing.assert_allclose(out.cpu().double().numpy(), ref["out"].numpy(), atol=2e-4, rtol=0)
    np.testing.assert_allclose(out.cpu().numpy(), data["eval_out"], atol=2e-3, rtol=0)


@pytest.mark.parametrize("n,w,k,d,b", [(512, 30, 64, 64, 6), (300, 12, 20, 64, 5), (127, 15, 30, 32, 9),
                                       (200, 40, 90, 32, 4)],
                         ids=["config4_n512_k64_w30", "n300_w12_k20", "n127_d32", "n200_w40_k90_d32"])
def test_bf16_storage_fused_forward_on_the_gather_path(n, w, k, d, b, gpu_device):
    """Shapes the matrix-core kernels do not take (n > 127, d not 64 / 128, w > 32): the fp32 row-gather kernel reads
    bf16 windows and rounds the LDS-resident projected tile to bf16 — the same storage semantics, the
    oracle's rounding point exactly.  First case = BASELINE configs[4] as worded (512 sensors, top-k 64,
    W=30, bf16)."""
    model = random_params(n, w, k, d, seed=4)
    p = {kk: v.detach().clone() for kk, v in model.state_dict().items()}
    model = model.to(gpu_device).eval()
    xb = torch.rand((b, n, w), generator=torch.Generator().manual_seed(8)).bfloat16()
    with torch.no_grad():
        out = model(xb.to(gpu_device), None)
        out32 = model(xb.float().to(gpu_device), None)
    graph = model.learned_graph.cpu()
    ref = gdn_oracle.forward(f64_params(p), xb.double(), k, graph=graph, storage="bf16")
    np.testing.assert_allclose(out.cpu().double().numpy(), ref["out"].numpy(), atol=2e-4, rtol=0)
    assert not torch.equal(out, out32)                       # the tile really was rounded
    assert float((out - out32).abs().max()) < 5e-3


@pytest.mark.parametrize("n,w,k,b", [(127, 15, 30, 9), (40, 30, 16, 33), (64, 5, 63, 4), (100, 17, 40, 700)])
@pytest.mark.parametrize("bf16", [False, True])
def test_dense_fused_forward_at_d128(n, w, k, b, bf16, gpu_device):
    """d = 128 (the paper's WADI width): the fused matrix-core kernel with four 32-column blocks
    (gdn_forward_dense_d128.hip) — planned launch (GDN.forward), plain entry point, float64 oracle, and the
    fp32 row-gather kernel on the same inputs."""
    from gdn_amd import ops
    model = random_params(n, w, k, 128, seed=6)
    p = {kk: v.detach().clone() for kk, v in model.state_dict().items()}
    model = model.to(gpu_device).eval()
    x = torch.rand((b, n, w), generator=torch.Generator().manual_seed(2))
    xin = (x.bfloat16() if bf16 else x).to(gpu_device)
    with torch.no_grad():
        out = model(xin, None)
    c = model._constants()
    assert c.plans[bf16] is not None                       # the matrix-core path took it
    gnn, lin = model.gnn_layers[0].gnn, model.out_layer.mlp[0]
    plain = ops.forward_fused(xin, gnn.lin.weight, c.terms, c.graph, gnn.bias, model.embedding.weight, c.bn1, c.bn2,
                              lin.weight, lin.bias)
    np.testing.assert_allclose(out.cpu().numpy(), plain.cpu().numpy(), atol=3e-7, rtol=0)
    ref = gdn_oracle.forward(f64_params(p), xin.cpu().double(), k, graph=model.learned_graph.cpu(),
                             storage="bf16" if bf16 else "fp32")
    np.testing.assert_allclose(out.cpu().double().numpy(), ref["out"].numpy(), atol=2e-4 if bf16 else 2e-6, rtol=0)


def test_bf16_staged_kernels_refuse_shapes_outside_the_matrix_core_path(gpu_device):
    """The staged bf16 entry points (bf16 xlin / z in HBM) exist for the matrix-core shapes only."""
    from gdn_amd import ops
    from gdn_amd._lib import GdnHipError
    model = random_params(300, 12, 20, 64, seed=1).to(gpu_device).eval()
    c = model._constants()
    with pytest.raises(GdnHipError, match="UNSUPPORTED"):
        ops.project_fwd(torch.rand((2, 300, 12), device=gpu_device).bfloat16(), model.gnn_layers[0].gnn.lin.weight, c.terms)


@pytest.mark.parametrize("cfg", [dict(n=127, w=15, k=30, d=64, hidden=256, layers=2, b=9),
                                 dict(n=40, w=10, k=8, d=64, hidden=128, layers=3, b=33),
                                 dict(n=20, w=8, k=6, d=32, hidden=48, layers=2, b=5),
                                 dict(n=12, w=4, k=3, d=16, hidden=24, layers=4, b=70),
                                 dict(n=30, w=20, k=10, d=128, hidden=200, layers=3, b=6),
                                 # beyond the one-launch chain (hidden > 256): gdn_mlp_eval_fwd, fp32 matrix-core GEMMs;
                                 # 512 = the default inter_num of the reference's OutLayer class (models/GDN.py:28)
                                 dict(n=127, w=15, k=30, d=64, hidden=512, layers=2, b=9),
                                 dict(n=27, w=10, k=8, d=64, hidden=384, layers=3, b=21),
                                 # widths that are not a multiple of 4 (element-wise operand staging)
                                 dict(n=27, w=10, k=8, d=64, hidden=50, layers=3, b=21),
                                 dict(n=27, w=10, k=8, d=32, hidden=301, layers=3, b=21)],
                         ids=lambda c: "n{n}_d{d}_h{hidden}_L{layers}".format(**c))
def test_outlayer_mlp_on_the_matrix_cores(cfg, gpu_device):
    """out_layer_num > 1 in eval mode: gdn_mlp_fwd (one launch, activations in registers, BatchNorm folded into
    the plan) against the float64 oracle's OutLayer (models/GDN.py:27-56) — non-trivial running statistics."""
    from gdn_amd import GDN
    torch.manual_seed(7)
    model = GDN([torch.zeros((2, 1), dtype=torch.long)], cfg["n"], dim=cfg["d"], out_layer_inter_dim=cfg["hidden"],
                input_dim=cfg["w"], out_layer_num=cfg["layers"], topk=cfg["k"])
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=g) + 0.5)
                mod.bias.copy_(torch.rand(mod.bias.shape, generator=g) * 0.4 - 0.2)
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) + 0.5)
    p = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(gpu_device).eval()
    x = torch.rand((cfg["b"], cfg["n"], cfg["w"]), generator=g)
    with torch.no_grad():
        out = model(x.to(gpu_device), None)
    # a HIP kernel ran, not the library GEMMs: the one-launch chain up to 256 hidden units, gdn_mlp_eval_fwd beyond
    from gdn_amd import ops
    if cfg["hidden"] <= 256:
        assert model._constants().mlp is not None
    else:
        assert model._constants().mlp is None and ops.mlp_eval_wide_supported(model.out_layer, cfg["d"])
    ref = gdn_oracle.forward(f64_params(p), x.double(), cfg["k"], cfg["layers"], graph=model.learned_graph.cpu())
    np.testing.assert_allclose(out.cpu().double().numpy(), ref["out"].numpy(), atol=2e-6, rtol=1e-5)


def test_matrix_core_kernels_over_random_shapes(gpu_device):
    """A seeded sweep over the whole shape family of the matrix-core kernels (n 2..127, w 1..32, k 1..min(n, 63),
    d 64 / 128, batch 1..40): fused forward (planned, fp32 and bf16 storage) and the staged fp32 kernels against
    the float64 oracle.  Catches tile-edge cases the hand-picked shapes miss (n = 32 m and 32 m - 1, k = n,
    pitch boundaries 15/16, 31/32, 47/48, w = 16/17)."""
    from gdn_amd import ops
    rng = np.random.default_rng(20260)
    shapes = [(31, 16, 15, 64), (32, 17, 16, 64), (33, 1, 31, 64), (63, 32, 47, 64), (64, 8, 48, 64), (65, 15, 63, 64),
              (95, 3, 32, 128), (96, 16, 1, 128), (97, 17, 30, 64), (2, 5, 1, 64), (2, 5, 2, 128), (127, 32, 63, 128)]
    while len(shapes) < 44:
        n = int(rng.integers(2, 128))
        shapes.append((n, int(rng.integers(1, 33)), int(rng.integers(1, min(n, 63) + 1)), int(rng.choice([64, 64, 128]))))
    worst = 0.0
    for idx, (n, w, k, d) in enumerate(shapes):
        b = int(rng.integers(1, 41))
        model = random_params(n, w, k, d, seed=100 + idx)
        p = {kk: v.detach().clone() for kk, v in model.state_dict().items()}
        model = model.to(gpu_device).eval()
        x = torch.rand((b, n, w), generator=torch.Generator().manual_seed(idx))
        with torch.no_grad():
            out = model(x.to(gpu_device), None)
            out_b = model(x.bfloat16().to(gpu_device), None)
        c = model._constants()
        assert c.plans[False] is not None and c.plans[True] is not None, (n, w, k, d)
        graph = model.learned_graph.cpu()
        ref = gdn_oracle.forward(f64_params(p), x.double(), k, graph=graph)
        err = float((out.cpu().double() - ref["out"]).abs().max())
        worst = max(worst, err)
        assert err < 2e-6, (n, w, k, d, b, err)
        ref_b = gdn_oracle.forward(f64_params(p), x.bfloat16().double(), k, graph=graph, storage="bf16")
        assert float((out_b.cpu().double() - ref_b["out"]).abs().max()) < 2e-4, (n, w, k, d, b)
        if d == 64:
            gnn = model.gnn_layers[0].gnn
            xlin, s_i, s_j = ops.project_fwd(x.to(gpu_device), gnn.lin.weight, c.terms)
            z, alpha = ops.attn_aggregate_fwd(xlin, s_i, s_j, c.graph, gnn.bias, b, want_alpha=True)
            np.testing.assert_allclose(z.cpu().double().numpy(), ref["agg"].numpy(), atol=2e-6, rtol=1e-5, err_msg=str((n, w, k)))
            np.testing.assert_allclose(alpha.cpu().sum(1).numpy(), 1.0, atol=1e-5)
    assert worst < 2e-6


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fused_forward_keeps_fp32_grade_against_float64(shape, gpu_device):
    """The planned fused forward (what GDN.forward launches) and the plan-less entry point against float64 at
    2e-7 of the output scale — ten times tighter than the parity bar, on purpose: every factor of every product is
    split into two f16 terms whose sum must reproduce the fp32 value EXACTLY.  Round 3 found the split silently
    broken for one value in ~2^13 (hi rounded from the exact product by a contracted v_fma_mixlo_f16, lo taken
    against the fp32-rounded one: an f16 ulp lost), which put the forward at 1.2e-6 — invisible at 2e-5."""
    from gdn_amd import ops
    model, p, x = setup(shape, gpu_device)
    with torch.no_grad():
        planned = model(x.to(gpu_device), None)
    c = model._constants()
    gnn, lin = model.gnn_layers[0].gnn, model.out_layer.mlp[0]
    plain = ops.forward_fused(x.to(gpu_device), gnn.lin.weight, c.terms, c.graph, gnn.bias, model.embedding.weight,
                              c.bn1, c.bn2, lin.weight, lin.bias)
    ref = gdn_oracle.forward(f64_params(p), x.double(), shape["k"], graph=model.learned_graph.cpu())["out"]
    bound = 2e-7 * max(1.0, float(ref.abs().max()))
    for name, got in (("planned", planned), ("plan-less", plain)):
        err = float((got.cpu().double() - ref).abs().max())
        assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("shape", SHAPES[:4] + SHAPES[5:], ids=IDS[:4] + IDS[5:])
def test_bank_ordered_lists_are_a_permutation_and_give_the_same_aggregate(shape, gpu_device):
    """gdn_graph_bank_order: every row holds the same entries, permuted inside its two halves only; the staged
    gather-aggregate fed the ordered table returns the z of the rank-ordered one (the softmax denominator is
    summed in another order: 1e-6 of the scale), for fp32 and bf16 storage."""
    from gdn_amd import ops
    model, p, x = setup(shape, gpu_device)
    c = model._constants()
    gnn = model.gnn_layers[0].gnn
    nbr, ordn = c.graph.nbr.cpu().view(torch.int16).long(), c.graph.nbr_ordered().cpu().view(torch.int16).long()
    assert not torch.equal(nbr, ordn) or shape["k"] <= 1
    half = c.graph.pitch // 2
    for lo in (0, half):
        assert torch.equal(nbr[:, lo:lo + half].sort(dim=1).values, ordn[:, lo:lo + half].sort(dim=1).values)
    for xin in (x.to(gpu_device), x.to(gpu_device).bfloat16()):
        xlin, s_i, s_j = ops.project_fwd(xin, gnn.lin.weight, c.terms)
        z_rank, _alpha = ops.attn_aggregate_fwd(xlin, s_i, s_j, c.graph, gnn.bias, shape["b"], want_alpha=xin.dtype == torch.float32)
        z_ord, _ = ops.attn_aggregate_fwd(xlin, s_i, s_j, c.graph, gnn.bias, shape["b"], want_alpha=False)
        if xin.dtype == torch.bfloat16:     # bf16 storage has no alpha output: run the rank-ordered table by hand
            from gdn_amd import _lib
            z_rank = torch.empty_like(xlin)
            _lib.call("gdn_attn_aggregate_fwd_bf16", xlin.data_ptr(), s_i.data_ptr(), s_j.data_ptr(),
                      c.graph.nbr.data_ptr(), c.graph.deg.data_ptr(), gnn.bias.data_ptr(), shape["b"], shape["n"], 64,
                      shape["k"], z_rank.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
            assert_bf16_stored(z_ord, z_rank.float().cpu(), "z (ordered vs rank)", fp32_floor=1e-6)
        else:
            scale = max(1.0, float(z_rank.abs().max()))
            assert float((z_ord - z_rank).abs().max()) <= 1e-6 * scale
