"""The float64 stage references of tests/_graph_layer_bwd_ref.py pinned to the oracle the gradient tests already trust
(_grad_check.staged_f64, itself pinned to oracle.gdn_oracle at 1e-10), the properties of the hub graph, and the shape
tables of tests/test_gpu_backward_stages.py held to the route (gdn_kernel_family).  Host only: no GPU, no launch."""
import pytest
import torch

import _graph_layer_bwd_ref as ref
import test_gpu_backward_stages as stages
from _grad_check import f64_leaves, lists_of, staged_f64
from conftest import load_golden, meta
from gdn_amd import _lib

NONE, DENSE, TILE, LARGE, LONG, ANY = range(6)
TOL = 1e-12


def close(got, want, what):
    top = float(want.abs().max())
    assert float((got.reshape(want.shape) - want).abs().max()) <= TOL * top, (what, top)


@pytest.mark.parametrize("case", ["msl_demo_w5_k5", "mlp2_n20_w8_k6", "wadi_stress_small_n40_w30_k16_d128"])
def test_stage_references_equal_the_staged_float64_oracle(case):
    """staged_f64's gradient at z, pushed through aggregate_ref -> project_bwd_ref -> terms_bwd_ref, gives staged_f64's
    gradient at every stage boundary and the parameter gradients of the graph layer, to 1e-12 relative."""
    data, p = load_golden(case)
    m = meta(data)
    x, y = torch.from_numpy(data["x"]).double(), torch.from_numpy(data["y"]).double()
    mask, graph = torch.from_numpy(data["dropout_mask"]).double(), torch.from_numpy(data["learned_graph"])
    leaf = f64_leaves(p)
    _loss, st, sg, grads = staged_f64(leaf, x, y, graph, m["out_layer_num"], mask)
    b, n, d, w = m["b"], m["n"], m["d"], m["w"]
    nbr, deg = ref.nbr_of(graph)
    lst, valid = lists_of(graph)
    assert torch.equal(nbr[:, :m["k"] + 1], lst.masked_fill(~valid, n)) and torch.equal(deg, valid.sum(1))
    pre = "gnn_layers.0.gnn."

    z, alpha, d_xlin, d_si, d_sj, d_bias = ref.aggregate_ref(st["xlin"], st["s_i"], st["s_j"], leaf[pre + "bias"], nbr, sg["z"])
    close(z, st["z"], "z")
    close(alpha[:, :, :m["k"] + 1], st["alpha"], "alpha")
    assert float(alpha[:, :, m["k"] + 1:].abs().max() if alpha.shape[2] > m["k"] + 1 else 0.0) == 0.0
    close(d_xlin, sg["xlin"], "d_xlin")
    close(d_si, sg["s_i"], "d_si")
    close(d_sj, sg["s_j"], "d_sj")
    # a bias in front of a train-mode BatchNorm: both sides hold float64 rounding noise (the column sums of d_z)
    assert float((d_bias - grads[pre + "bias"]).abs().max()) <= TOL * float(sg["z"].abs().max()) * b * n

    d_lin_direct, d_a, d_c = ref.project_bwd_ref(x, d_xlin, d_si, d_sj)
    assert d_a.shape == (2, ref.terms_pitch(w)) and float(d_a[:, w:].abs().max()) == 0.0
    close(d_lin_direct, sg["lin_direct"], "d_lin_w direct")
    close(d_a[:, :w], sg["a_vec"], "d_a")
    close(d_c, sg["c_vec"], "d_c")

    att = [leaf[pre + name] for name in ("att_i", "att_j", "att_em_i", "att_em_j")]
    emb = leaf["embedding.weight"]
    out = ref.terms_bwd_ref(leaf[pre + "lin.weight"], *att, emb, d_lin_direct, d_a, d_c)
    for got, name in zip(out[:5], ("lin.weight", "att_i", "att_j", "att_em_i", "att_em_j")):
        close(got, grads[pre + name], name)
    # the graph layer's share of d_emb: autograd of c = emb . att_em alone, seeded with staged_f64's d_c
    e = emb.detach().clone().requires_grad_(True)
    c_vec = torch.stack((e @ att[2].detach().view(d), e @ att[3].detach().view(d)))
    (share,) = torch.autograd.grad(c_vec, e, sg["c_vec"])
    close(out[5], share, "d_emb share")
    prior = torch.randn((n, d), dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    acc = ref.terms_bwd_ref(leaf[pre + "lin.weight"], *att, emb, d_lin_direct, d_a, d_c, d_emb_in=prior)
    close(acc[5], prior + share, "d_emb accumulated")


@pytest.mark.parametrize("n,k", [(12, 3), (70, 5), (100, 5), (127, 30), (300, 30), (330, 8), (650, 5), (5, 1)])
def test_hub_graph_properties(n, k):
    topk = ref.hub_topk(n, k, seed=n)
    assert topk.shape == (n, k) and topk.dtype == torch.int64 and torch.equal(topk, ref.hub_topk(n, k, seed=n))
    assert int(topk.min()) >= 0 and int(topk.max()) < n and bool((topk[:, 0] == 0).all())
    assert all(len(set(row.tolist())) == k for row in topk)                        # distinct entries per row
    nbr, deg = ref.nbr_of(topk)
    own = (topk == torch.arange(n).view(n, 1)).any(1)
    assert torch.equal(deg, torch.where(own, k, k + 1))
    if k >= 2:
        assert 0.4 * n <= int(own.sum()) <= 0.6 * n + 1                            # mixed degrees, about half each
    rev = ref.reverse_ref(nbr, deg)
    rlen = [len(r) for r in rev]
    assert rlen[0] == n and rlen[n - 1] == 1 and sum(rlen) == int(deg.sum())
    assert rev[0] == sorted(rev[0]) and [e >> 16 for e in rev[0]] == list(range(n))
    for j, row in enumerate(rev):                                                   # every entry names its source
        assert all(int(nbr[e >> 16, e & 0xffff]) == j for e in row)


def fam(stage, n, w, d, k, flags=0):
    return _lib.load().gdn_kernel_family(stage, n, w, d, k, flags)


def test_aggregate_cases_land_in_the_cells_they_claim():
    """Family, and for the TILE backward the GDN_BWD_* sub-form (bits 8 and up) and the thread count of the launch
    (gdn_backward.hip: 512 threads with the tables in the workspace or more than 64 tile rows of 64 columns)."""
    cells = set()
    for c in stages.AGG_CASES:
        n, d, k, flags = c["n"], c["d"], c["k"], int(c["wide"])
        got = fam(_lib.STAGE_ATTN_BWD, n, 1, d, k, flags)
        assert got & 0xff == c["family"], (c["id"], got)
        assert fam(_lib.STAGE_ATTN_BWD, n, 1, d, k, 0) & 0xff != DENSE or c["wide"], c["id"]     # never the dense test's cell
        if c["family"] == TILE:
            assert got >> 8 == c["form"], (c["id"], got >> 8)
            threads = 512 if c["form"] != stages.TABLES_LDS or n * max(d // 64, 1) > 64 else 256
            assert threads == c["threads"], c["id"]
        assert k <= n and (not c["hub"] or k <= n - 2)
        cells.add((c["family"], c["form"], c["threads"]))
    assert {(TILE, 0, 256), (TILE, 0, 512), (TILE, 1, 512), (TILE, 2, 512), (LARGE, 0, 0), (ANY, 0, 0)} <= cells
    by = stages.AGG
    assert (by["tile-lds-256-rpitch16"]["n"] + 15) // 16 * 16 == 16                  # rpitch 16
    assert all(by[name]["n"] > 256 for name in ("tile-global", "tile-sliced", "large"))   # beyond the reverse kernel's block
    assert by["any-d3"]["d"] % 4 != 0 and by["any-d200"]["d"] > 128
    assert ref.nbr_pitch(by["pitch16-full"]["k"]) == 16 == by["pitch16-full"]["k"] + 1
    assert ref.nbr_pitch(by["pitch32"]["k"]) == 32 and by["k-equals-n"]["k"] == by["k-equals-n"]["n"]
    # the zero-logit / per-window-scale / bit-claim tests name their cases: one TILE and the LARGE shape each
    assert by["tile-lds-512"]["hub"] and by["large"]["hub"] and by["tile-global"]["hub"]
    assert fam(_lib.STAGE_ATTN_BWD, 100, 1, 16, 5, 1) == fam(_lib.STAGE_ATTN_BWD, 100, 1, 16, 5, 0) == TILE


def test_project_and_terms_cases_land_in_the_cells_they_claim():
    for c in stages.PROJECT_CASES:
        b, n, w, d = c["shape"]
        assert fam(_lib.STAGE_PROJECT_BWD, n, w, d, 1) & 0xff == c["family"], c["id"]
        if c["family"] != TILE:
            continue
        wp = 8 if w <= 8 else (w + 15) & ~15
        rc = min(n, (24576 - 2 * n) // (wp + d + 2))               # gdn_backward.hip: pbwd_chunk_rows
        assert wp == c["wp"], c["id"]
        assert (rc < n) == bool(c.get("chunked")), (c["id"], rc)
    by = stages.PROJECT
    assert by["one-pass"]["wp"] == 16 and by["two-passes"]["wp"] == 32 and by["four-passes"]["wp"] == 64
    assert by["batch-over-grid"]["shape"][0] > 1024                # GDN_PBWD_MAX_ROWS caps the grid
    assert {c["family"] for c in stages.PROJECT_CASES} == {TILE, LONG, ANY}
    for c in stages.TERMS_CASES:
        n, w, d = c["shape"]
        assert fam(_lib.STAGE_TERMS, n, w, d, 1) & 0xff == c["family"], c["id"]
        assert fam(_lib.STAGE_PROJECT_BWD, n, w, d, 1) & 0xff != NONE       # its inputs come from gdn_project_bwd
        if c["family"] == TILE:
            assert (n * d + 2047) // 2048 == c["groups"], c["id"]           # gdn_terms_bwd_acc's grid
    assert {c["family"] for c in stages.TERMS_CASES} == {TILE, LONG, ANY}
    assert any(c["family"] == TILE and c["groups"] > 1 and c["shape"][2] == 16 for c in stages.TERMS_CASES)
