"""The graph-layer backward stage by stage, every kernel family against a float64 reference of the same stage
(tests/_graph_layer_bwd_ref.py): gdn_attn_aggregate_bwd[_wide] (TILE in its three sub-forms at 256 / 512 threads,
LARGE, ANY), gdn_graph_reverse, gdn_project_bwd (TILE, LONG, ANY), gdn_terms_bwd[_acc], and the bit claims of
include/gdn_hip.h (sliced = unsliced, `_wide` = plain where both are TILE, run to run).

A stage takes s_i / s_j as INPUTS: fp32 `s_i + s_j[j]` has the sign of the exact sum, so there is no kink problem and
the bound of the dense stage test (test_matrix_core_backward_of_the_aggregate_over_random_shapes) applies as it is:
  d_xlin, d_si, d_sj   per window, max|got - want| / max(1, max|want|) on values divided by the window's scale < 3e-6;
  d_bias               rtol 2e-5, atol 2e-6 * max scale * sqrt(b n);
  project / terms      max|got - want| <= 3e-6 * max|want| per tensor.
The tables below name the cell every case is there for; tests/test_cpu_backward_stages_ref.py holds them to
gdn_kernel_family, so they cannot drift when the routing changes.  Every candidate shape landed in its cell as given.

MEASURED on the MI355X (worst ratio over a family's cases, learned and hub graphs, zero-logit and per-window-scale
runs included; every test prints its own with -s; the whole file takes 12 s, 4.4 s of them the two child processes):
  gdn_attn_aggregate_bwd   TILE/lds/256 1.35e-6   TILE/lds/512 3.1e-7   TILE/global/512 6.5e-7   TILE/sliced/512 6.4e-7
                           LARGE 7.0e-7           ANY 3.3e-7
  gdn_project_bwd          TILE 4.3e-7 (batch-over-grid: grid 1024 at batch 3000)   LONG 1.8e-7   ANY 1.4e-7
  gdn_terms_bwd[_acc]      TILE 1.8e-7   LONG 8.8e-8   ANY 1.6e-7
TILE/lds/256 is the one family above a quarter of 3e-6: d_sj at (n, d, k) = (17, 32, 15), 1.35e-6.  torch float32
autograd of the same stage on the CPU, same inputs and graph, is 6.3e-7 from float64 there (d_sj = a sum of
alpha (d_alpha - sum alpha d_alpha) terms, each a difference of numbers ~10 times the result): fp32's own error, so
the family's bound is 4 x that = 2.5e-6 (the factor covers the summation order), below the 3e-6 it started from.
FOUND: sliced and unsliced d = 128 gave different bits in d_bias (alone): the sliced kernel summed the columns of d_z
per target in pass 1 over 32 lane groups, the unsliced one over 16.  Fixed in gdn_backward.hip (the sliced kernel now
sums them from its pass-2 tile in the unsliced order); test_sliced_and_unsliced_d128_backward_give_the_same_bits is
the regression case.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _graph_layer_bwd_ref as ref
from gdn_amd import _lib, ops

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, DENSE, TILE, LARGE, LONG, ANY = range(6)
TABLES_LDS, TABLES_GLOBAL, SLICED = range(3)
BOUND = 3e-6                 # the dense stage test's bound (set for the 16-bit operand split; fp32 VALU sits below)
BOUNDS = {"TILE/lds/256": 2.5e-6}   # 4 x the CPU-fp32 error of the family's worst case (module docstring)


def _agg(name, n, d, k, family, form=0, threads=0, wide=False, hub=False):
    return dict(id=name, n=n, d=d, k=k, family=family, form=form, threads=threads, wide=wide, hub=hub)


# (n, d, k) of gdn_attn_aggregate_bwd: the family, for TILE the GDN_BWD_* sub-form and the launch's thread count
AGG_CASES = [
    _agg("tile-lds-256-rpitch16", 12, 16, 3, TILE, TABLES_LDS, 256, hub=True),          # rpitch 16: second prefetch = first
    _agg("tile-lds-256-wide", 40, 64, 6, TILE, TABLES_LDS, 256, wide=True),             # a dense shape: `_wide` only
    _agg("tile-lds-512", 100, 16, 5, TILE, TABLES_LDS, 512, hub=True),
    _agg("tile-lds-512-wide", 127, 64, 30, TILE, TABLES_LDS, 512, wide=True, hub=True),
    _agg("tile-lds-512-d128", 40, 128, 16, TILE, TABLES_LDS, 512),                       # two lane groups per row
    _agg("tile-global", 300, 64, 30, TILE, TABLES_GLOBAL, 512, hub=True),               # n > 256: the reverse kernel's block
    _agg("tile-global-d128", 200, 128, 63, TILE, TABLES_GLOBAL, 512),
    _agg("tile-sliced", 330, 128, 8, TILE, SLICED, 512, hub=True),
    _agg("large", 650, 64, 5, LARGE, hub=True),
    _agg("any-d24", 12, 24, 3, ANY),
    _agg("any-d3", 70, 3, 5, ANY, hub=True),                                            # d % 4 != 0
    _agg("any-d200", 33, 200, 8, ANY),                                                  # padded to 256
    _agg("k1", 2, 16, 1, TILE, TABLES_LDS, 256),
    _agg("k-equals-n", 20, 32, 20, TILE, TABLES_LDS, 256),
    _agg("pitch16-full", 17, 32, 15, TILE, TABLES_LDS, 256),
    _agg("pitch32", 40, 32, 16, TILE, TABLES_LDS, 256),
]
AGG = {c["id"]: c for c in AGG_CASES}

# (b, n, w, d) of gdn_project_bwd: family, the padded window wp of the TILE kernel, what the case is there for
PROJECT_CASES = [
    dict(id="wp8", shape=(3, 27, 5, 64), family=TILE, wp=8),
    dict(id="wp8-w1", shape=(3, 5, 1, 16), family=TILE, wp=8),
    dict(id="one-pass", shape=(3, 27, 16, 32), family=TILE, wp=16),
    dict(id="two-passes", shape=(3, 27, 17, 64), family=TILE, wp=32),
    dict(id="four-passes", shape=(2, 40, 64, 128), family=TILE, wp=64),
    dict(id="chunked", shape=(2, 200, 64, 128), family=TILE, wp=64, chunked=True),        # rc = 124 < n
    dict(id="batch-over-grid", shape=(3000, 2, 3, 16), family=TILE, wp=8),
    dict(id="long-w65", shape=(2, 12, 65, 64), family=LONG),
    dict(id="long-w200", shape=(2, 5, 200, 32), family=LONG),
    dict(id="any-d24", shape=(3, 12, 4, 24), family=ANY),
    dict(id="any-d50-w70", shape=(2, 9, 70, 50), family=ANY),
]
PROJECT = {c["id"]: c for c in PROJECT_CASES}

# (n, w, d) of gdn_terms_bwd[_acc]: the TERMS family and the number of workgroups of the TILE kernel
TERMS_CASES = [
    dict(id="tile", shape=(27, 5, 64), family=TILE, groups=1),
    dict(id="tile-d128", shape=(40, 64, 128), family=TILE, groups=3),
    dict(id="tile-many-workgroups", shape=(300, 15, 16), family=TILE, groups=3),         # n d > 2048
    dict(id="any-d24", shape=(12, 4, 24), family=ANY),
    dict(id="long-w65", shape=(12, 65, 64), family=LONG),
]

WORST = {}                   # family / stage -> worst ratio seen in this session (printed by every test)


def _note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"[bwd-stages] {key:28s} ratio {ratio:9.2e}   worst so far {WORST[key]:9.2e}")


def _family_name(case):
    if case["family"] != TILE:
        return ("NONE", "DENSE", "TILE", "LARGE", "LONG", "ANY")[case["family"]]
    return "TILE/" + ("lds", "global", "sliced")[case["form"]] + f"/{case['threads']}"


# ---- inputs (seeded CPU generators) and the comparison ---------------------------------------------------------

def _seed(case):
    return 1000 + [c["id"] for c in AGG_CASES].index(case["id"])


def _batch(case):
    return 2 + _seed(case) % 4


def agg_inputs(case, scaled=False):
    """xlin, d_z ~ randn; s_i, s_j ~ 2 randn (attention far from uniform, both signs of the logit); bias ~ 0.1 randn;
    `scaled`: d_z of window b times 10^u, u ~ U(-9, 3).  CPU fp32."""
    n, d, b = case["n"], case["d"], 5 if scaled else _batch(case)
    g = torch.Generator().manual_seed(_seed(case))
    t = dict(xlin=torch.randn((b, n, d), generator=g), s_i=2 * torch.randn((b, n), generator=g),
             s_j=2 * torch.randn((b, n), generator=g), bias=0.1 * torch.randn((d,), generator=g),
             d_z=torch.randn((b, n, d), generator=g), emb=torch.randn((n, d), generator=g))
    t["mags"] = torch.ones((b,))
    if scaled:
        t["mags"] = 10.0 ** (torch.rand((b,), generator=g) * 12 - 9)
        t["d_z"] = t["d_z"] * t["mags"].view(b, 1, 1)
    return t


def make_graph(case, kind, t, device):
    if kind == "hub":
        return ops.graph_from_topk(ref.hub_topk(case["n"], case["k"], _seed(case)).to(device))
    return ops.topk_graph(t["emb"].to(device), case["k"])


def run_aggregate(case, t, graph, device, wide=None):
    """Forward (alpha on the same route) and backward on the GPU; everything back on the CPU."""
    b, n, d = t["xlin"].shape
    wide = case["wide"] if wide is None else wide
    dev = lambda v: v.reshape(b * n, *v.shape[2:]).to(device)
    xlin, s_i, s_j, d_z = dev(t["xlin"]), dev(t["s_i"]), dev(t["s_j"]), dev(t["d_z"])
    z, alpha = ops.attn_aggregate_fwd(xlin, s_i, s_j, graph, t["bias"].to(device), b, want_alpha=True, wide=wide)
    d_xlin, d_si, d_sj, d_bias = ops.attn_aggregate_bwd(d_z, xlin, alpha, s_i, s_j, graph, b, wide=wide)
    torch.cuda.synchronize()
    return dict(z=z.cpu().view(b, n, d), alpha=alpha.cpu().view(b, n, -1), d_xlin=d_xlin.cpu().view(b, n, d),
                d_si=d_si.cpu().view(b, n), d_sj=d_sj.cpu().view(b, n), d_bias=d_bias.cpu())


def window_ratio(got, want, mags):
    """The dense stage test's measure, window by window: max|got - want| / max(1, max|want|) on values divided by the
    window's scale; the worst window."""
    b = want.shape[0]
    scale = mags.double().view(b, *([1] * (want.dim() - 1)))
    diff = ((got.double() - want) / scale).abs().reshape(b, -1).max(dim=1).values
    top = (want / scale).abs().reshape(b, -1).max(dim=1).values.clamp_min(1.0)
    return float((diff / top).max())


def check_aggregate(case, got, t, nbr, what):
    want = dict(zip(("z", "alpha", "d_xlin", "d_si", "d_sj", "d_bias"),
                    ref.aggregate_ref(t["xlin"], t["s_i"], t["s_j"], t["bias"], nbr, t["d_z"])))
    b, n, d = t["xlin"].shape
    for name in ("z", "alpha"):
        np.testing.assert_allclose(got[name].double().numpy(), want[name].numpy(), atol=3e-6, rtol=1e-5,
                                   err_msg=f"{what}: {name}")
    worst = 0.0
    for name in ("d_xlin", "d_si", "d_sj"):
        ratio = window_ratio(got[name], want[name], t["mags"])
        worst = max(worst, ratio)
        print(f"[bwd-stages]   {what:44s} {name:7s} {ratio:9.2e}")
        assert ratio < BOUNDS.get(_family_name(case), BOUND), (what, name, ratio)
    _note(_family_name(case), worst)
    np.testing.assert_allclose(got["d_bias"].double().numpy(), want["d_bias"].numpy(), rtol=2e-5,
                               atol=2e-6 * float(t["mags"].max()) * (b * n) ** 0.5, err_msg=f"{what}: d_bias")
    return want


# ---- (a) gdn_attn_aggregate_bwd[_wide] ---------------------------------------------------------------------------

AGG_RUNS = [(c["id"], "learned") for c in AGG_CASES] + [(c["id"], "hub") for c in AGG_CASES if c["hub"]]


@pytest.mark.parametrize("name,kind", AGG_RUNS, ids=[f"{a}-{b}" for a, b in AGG_RUNS])
def test_aggregate_backward_against_float64(name, kind, gpu_device):
    """Every family of gdn_attn_aggregate_bwd on a learned graph (in-degree ~ k) and, where marked, on the hub graph:
    sensor 0 is named by every target (rlen = n: reverse-list entries beyond the 32 prefetched ones, beyond the
    reverse kernel's block of 256 at n = 300 / 330 / 650), sensor n - 1 by itself only (rlen = 1)."""
    case = AGG[name]
    fam = _lib.load().gdn_kernel_family(_lib.STAGE_ATTN_BWD, case["n"], 1, case["d"], case["k"], int(case["wide"]))
    assert (fam & 0xff, fam >> 8 if case["family"] == TILE else 0) == (case["family"], case["form"])
    t = agg_inputs(case)
    graph = make_graph(case, kind, t, gpu_device)
    if kind == "hub":
        rlen = graph.reverse()[1].cpu()
        assert int(rlen[0]) == case["n"] and int(rlen[-1]) == 1
    got = run_aggregate(case, t, graph, gpu_device)
    check_aggregate(case, got, t, graph.nbr.cpu().long(), f"{name} {kind} b={_batch(case)}")


@pytest.mark.parametrize("name", ["tile-lds-512", "large"])
def test_aggregate_backward_with_logits_that_are_exactly_zero(name, gpu_device):
    """s_i[b, i] = -s_j[b, j] for a handful of (target i, listed source j) pairs: those logits are exactly 0.0 in fp32
    and in float64.  The LeakyReLU derivative there is the slope (`pi > 0.f ? 1 : slope`, torch's convention), and the
    d_s_i shortcut — (0.2 - 1) times the sum over the slots with a non-positive logit — must count them."""
    case = AGG[name]
    t = agg_inputs(case)
    graph = make_graph(case, "hub", t, gpu_device)
    nbr, deg = graph.nbr.cpu().long(), graph.deg.cpu()
    b, n = t["s_i"].shape
    hit = 0
    for w in range(b):
        for q in range(6):
            i = (7 + 13 * w + 37 * q) % n
            j = int(nbr[i, (w + 3 * q) % int(deg[i])])
            t["s_i"][w, i] = -t["s_j"][w, j]
            hit += int(float(t["s_i"][w, i] + t["s_j"][w, j]) == 0.0)
    assert hit == 6 * b
    got = run_aggregate(case, t, graph, gpu_device)
    check_aggregate(case, got, t, nbr, f"{name} zero-logit")


@pytest.mark.parametrize("name", ["tile-global", "large"])
def test_aggregate_backward_with_a_scale_per_window(name, gpu_device):
    """d_z of window b times 10^u, u ~ U(-9, 3), as in the dense stage test: every window judged relative to its own
    scale (fp32 kernels carry no shared scale between the windows of a launch)."""
    case = AGG[name]
    t = agg_inputs(case, scaled=True)
    assert float(t["mags"].max() / t["mags"].min()) > 100
    graph = make_graph(case, "learned", t, gpu_device)
    got = run_aggregate(case, t, graph, gpu_device)
    check_aggregate(case, got, t, graph.nbr.cpu().long(), f"{name} per-window scale")


# ---- (b) gdn_graph_reverse -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,k,kind", [(12, 3, "hub"), (300, 30, "hub"), (650, 5, "hub"), (127, 30, "learned")])
def test_reverse_lists_against_the_reference(n, k, kind, gpu_device):
    """rlen and the first rlen[j] entries of every row, as integers (what lies beyond rlen is unspecified)."""
    if kind == "hub":
        graph = ops.graph_from_topk(ref.hub_topk(n, k, n).to(gpu_device))
    else:
        graph = ops.topk_graph(torch.randn((n, 64), generator=torch.Generator().manual_seed(n)).to(gpu_device), k)
    rent, rlen = graph.reverse()
    assert rent.shape == (n, (n + 15) & ~15)
    rent, rlen = rent.cpu().long() & 0xffffffff, rlen.cpu()
    want = ref.reverse_ref(graph.nbr.cpu().long(), graph.deg.cpu())
    assert rlen.tolist() == [len(r) for r in want]
    if kind == "hub":
        assert len(want[0]) == n and len(want[n - 1]) == 1
    for j in range(n):
        assert rent[j, :len(want[j])].tolist() == want[j], j


# ---- (c) gdn_project_bwd ---------------------------------------------------------------------------------------------

def project_inputs(shape, seed):
    b, n, w, d = shape
    g = torch.Generator().manual_seed(seed)
    return dict(x=torch.rand((b, n, w), generator=g), d_xlin=torch.randn((b, n, d), generator=g),
                d_si=torch.randn((b, n), generator=g), d_sj=torch.randn((b, n), generator=g))


def run_project(t, device):
    b, n, w = t["x"].shape
    d = t["d_xlin"].shape[-1]
    out = ops.project_bwd(t["x"].to(device), t["d_xlin"].reshape(b * n, d).to(device),
                          t["d_si"].reshape(-1).to(device), t["d_sj"].reshape(-1).to(device), d)
    torch.cuda.synchronize()
    return out


def tensor_ratio(got, want):
    return float((got.detach().cpu().double() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("name", [c["id"] for c in PROJECT_CASES])
def test_project_backward_against_float64(name, gpu_device):
    """gdn_project_bwd at the edges of its kernels: wp = 8 and its clamped float4 reads, one pass against several, a
    window staged in chunks, a workgroup looping over windows, the long-window and any-width forms.
    batch-over-grid: the launch's grid is min(batch, CUs x workgroups per CU, GDN_PBWD_MAX_ROWS = 1024) — recorded on
    the MI355X: 1024 (the cap), read back from gdn_project_bwd_partials and asserted below the batch of 3000."""
    case = PROJECT[name]
    b, n, w, d = case["shape"]
    t = project_inputs(case["shape"], 50 + len(name))
    if name == "batch-over-grid":
        rows = ctypes.c_int(0)
        ws = torch.empty((_lib.load().gdn_project_bwd_workspace_bytes(n, w, d) // 4,), device=gpu_device)
        dev = [t[key].reshape(b * n, -1).to(gpu_device) for key in ("x", "d_xlin", "d_si", "d_sj")]
        _lib.call("gdn_project_bwd_partials", *[v.data_ptr() for v in dev], b, n, w, d, ws.data_ptr(),
                  ctypes.byref(rows), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        print(f"[bwd-stages]   gdn_project_bwd grid at batch {b}: {rows.value}")
        assert 0 < rows.value <= 1024 < b
    d_lin_w, d_a, d_c = run_project(t, gpu_device)
    want = ref.project_bwd_ref(t["x"], t["d_xlin"], t["d_si"], t["d_sj"])
    assert d_a.shape == (2, ref.terms_pitch(w)) and d_lin_w.shape == (d, w) and d_c.shape == (2, n)
    assert bool((d_a[:, w:] == 0).all())                       # the padding of d_a is exactly 0
    worst = 0.0
    for tag, got, ww in zip(("d_lin_w", "d_a", "d_c"), (d_lin_w, d_a, d_c), want):
        ratio = tensor_ratio(got, ww)
        worst = max(worst, ratio)
        print(f"[bwd-stages]   project {name:18s} {tag:8s} {ratio:9.2e}")
        assert ratio <= BOUND, (name, tag, ratio)
    _note("PROJECT_BWD/" + ("NONE", "DENSE", "TILE", "LARGE", "LONG", "ANY")[case["family"]], worst)


# ---- (d) gdn_terms_bwd / gdn_terms_bwd_acc ------------------------------------------------------------------------

@pytest.mark.parametrize("case", TERMS_CASES, ids=[c["id"] for c in TERMS_CASES])
def test_terms_backward_against_float64(case, gpu_device):
    """The six formulas of gdn_terms_bwd on gdn_project_bwd's own outputs: d_lin_w is in/out (the direct term stays and
    is added to); gdn_terms_bwd_acc adds the graph layer's share of d_emb to what d_emb holds (accumulate_emb = 1) or
    overwrites it (0)."""
    n, w, d = case["shape"]
    t = project_inputs((2, n, w, d), 70 + n)
    g = torch.Generator().manual_seed(90 + n)
    lin_w, emb = torch.randn((d, w), generator=g), torch.randn((n, d), generator=g)
    att = [torch.randn((d,), generator=g) for _ in range(4)]
    prior = torch.randn((n, d), generator=g)
    direct, d_a, d_c = run_project(t, gpu_device)
    dev = lambda v: v.to(gpu_device)
    names = ("d_lin_w", "d_att_i", "d_att_j", "d_att_em_i", "d_att_em_j", "d_emb")
    want = ref.terms_bwd_ref(lin_w, *att, emb, direct.cpu(), d_a.cpu(), d_c.cpu())
    want_acc = ref.terms_bwd_ref(lin_w, *att, emb, direct.cpu(), d_a.cpu(), d_c.cpu(), d_emb_in=prior)
    assert float(direct.abs().max()) > 0
    worst = 0.0

    def judge(tag, got, ww):
        nonlocal worst
        for nm, gt, wt in zip(names, got, ww):
            ratio = tensor_ratio(gt.reshape(wt.shape), wt)
            worst = max(worst, ratio)
            print(f"[bwd-stages]   terms {case['id']:22s} {tag:10s} {nm:11s} {ratio:9.2e}")
            assert ratio <= BOUND, (case["id"], tag, nm, ratio)

    args = [dev(lin_w)] + [dev(a) for a in att] + [dev(emb)]
    judge("plain", ops.terms_bwd(*args, direct.clone(), d_a, d_c), want)
    for accumulate, ww in ((1, want_acc), (0, want)):
        d_lin = direct.clone()
        small = torch.empty((4, d), device=gpu_device)
        d_emb = dev(prior).clone()
        _lib.call("gdn_terms_bwd_acc", *[v.data_ptr() for v in args], d_a.data_ptr(), d_c.data_ptr(), n, d, w,
                  d_lin.data_ptr(), *[small[q].data_ptr() for q in range(4)], d_emb.data_ptr(), accumulate,
                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        judge(f"acc={accumulate}", (d_lin, small[0], small[1], small[2], small[3], d_emb), ww)
    _note("TERMS/" + ("NONE", "DENSE", "TILE", "LARGE", "LONG", "ANY")[case["family"]], worst)


# ---- (e) bit claims ----------------------------------------------------------------------------------------------------

BIT_OUTPUTS = ("d_xlin", "d_si", "d_sj", "d_bias")


def child_d128_backward(path):
    """Runs in a fresh process (GDN_BWD_SLICED is read once): the d = 128 backward at n = 40, k = 16 and the sub-form
    the route chose."""
    case = AGG["tile-lds-512-d128"]
    t = agg_inputs(case)
    device = torch.device("cuda:0")
    got = run_aggregate(case, t, make_graph(case, "learned", t, device), device)
    form = _lib.load().gdn_kernel_family(_lib.STAGE_ATTN_BWD, case["n"], 1, case["d"], case["k"], 0)
    torch.save(([got[key] for key in BIT_OUTPUTS], form), path)


def test_sliced_and_unsliced_d128_backward_give_the_same_bits(gpu_device, tmp_path):
    """include/gdn_hip.h / gdn_backward.hip: "the sum of two slices is the sum the unsliced kernel forms with its two
    lane groups, so both give the same bits" — n = 40, k = 16, d = 128, with GDN_BWD_SLICED=1 and without, each in a
    fresh child process."""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r + '/tests');"
            "import test_gpu_backward_stages as t; t.child_d128_backward(sys.argv[1])") % (ROOT, ROOT)
    env = {key: v for key, v in os.environ.items() if key != "GDN_BWD_SLICED"}
    outs = {}
    for tag, extra in (("unsliced", {}), ("sliced", {"GDN_BWD_SLICED": "1"})):
        f = str(tmp_path / f"bwd_{tag}.pt")
        subprocess.run([sys.executable, "-c", code, f], check=True, timeout=120, env=dict(env, **extra))
        outs[tag] = torch.load(f, weights_only=True)
    assert outs["unsliced"][1] == (TILE | TABLES_LDS << 8) and outs["sliced"][1] == (TILE | SLICED << 8)
    differ = [nm for nm, a, b in zip(BIT_OUTPUTS, outs["unsliced"][0], outs["sliced"][0]) if not torch.equal(a, b)]
    assert not differ, differ


def test_wide_and_plain_entry_points_give_the_same_bits_on_the_tile(gpu_device):
    """(100, 16, 5) is no dense shape: gdn_attn_aggregate_bwd and `_wide` route to the same TILE kernel."""
    case = AGG["tile-lds-512"]
    fams = [_lib.load().gdn_kernel_family(_lib.STAGE_ATTN_BWD, case["n"], 1, case["d"], case["k"], f) for f in (0, 1)]
    assert fams[0] == fams[1] == TILE
    t = agg_inputs(case)
    graph = make_graph(case, "hub", t, gpu_device)
    plain, wide = (run_aggregate(case, t, graph, gpu_device, wide=wd) for wd in (False, True))
    assert all(torch.equal(plain[key], wide[key]) for key in BIT_OUTPUTS + ("z", "alpha"))


@pytest.mark.parametrize("name", ["large", "tile-global"])
def test_two_calls_give_the_same_bits(name, gpu_device):
    """No floating-point atomics anywhere in the backward: the same inputs give the same bits (d_bias included, whose
    rows meet in the order of the ticket's last workgroup)."""
    case = AGG[name]
    t = agg_inputs(case)
    graph = make_graph(case, "hub", t, gpu_device)
    first, second = (run_aggregate(case, t, graph, gpu_device) for _ in range(2))
    assert float(first["d_xlin"].abs().max()) > 0
    assert all(torch.equal(first[key], second[key]) for key in BIT_OUTPUTS)
