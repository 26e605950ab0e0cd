"""The float64 stage references of tests/_graph_layer_fwd_ref.py pinned to oracle/gdn_oracle.py, the case tables of
tests/test_gpu_forward_stages.py held to the route (gdn_kernel_family) and to the tile kernel's form
(gdn_tile_forward_form), the coverage of those tables asserted, and the CPU-float32 yardsticks its bounds come from.
Host only: no GPU, no launch."""
import pytest
import torch

import _graph_layer_fwd_ref as ref
import test_gpu_forward_stages as stages
from conftest import load_golden, meta
from gdn_amd import _lib
from oracle import gdn_oracle

NONE, DENSE, TILE, LARGE, LONG, ANY = range(6)
TOL = 1e-12


def close(got, want, what):
    top = float(want.abs().max())
    assert float((got.reshape(want.shape) - want).abs().max()) <= TOL * top, (what, top)


@pytest.mark.parametrize("case", ["msl_demo_w5_k5", "wadi_stress_small_n40_w30_k16_d128"])
def test_stage_references_chained_equal_the_oracle(case):
    """bn_fold_ref, node_terms_ref -> project_ref -> aggregate_ref -> head_ref on a golden fixture, in float64, against
    the edge-list oracle's xlin, agg, att_weight_1 and out, to 1e-12 relative."""
    data, p = load_golden(case)
    m = meta(data)
    assert m["out_layer_num"] == 1
    p = {key: v.double() if v.is_floating_point() else v for key, v in p.items()}
    x, graph = torch.from_numpy(data["x"]).double(), torch.from_numpy(data["learned_graph"])
    b, n, d, k = x.shape[0], m["n"], m["d"], m["k"]
    want = gdn_oracle.forward(p, x, k, graph=graph)
    pre = "gnn_layers.0.gnn."
    terms = ref.node_terms_ref(p[pre + "lin.weight"], p[pre + "att_i"], p[pre + "att_j"], p[pre + "att_em_i"],
                               p[pre + "att_em_j"], p["embedding.weight"])
    xlin, s_i, s_j = ref.project_ref(x, p[pre + "lin.weight"], terms)
    close(xlin, want["xlin"], "xlin")
    nbr, deg = ref.nbr_of(graph)
    z, alpha = ref.aggregate_ref(xlin, s_i, s_j, p[pre + "bias"], nbr)
    close(z, want["agg"], "agg")
    # the oracle's attention weights are per edge (source, target): into list form through the slot of every source
    slot = torch.full((n, n + 1), -1, dtype=torch.long)
    rows = torch.arange(n).view(n, 1).expand_as(nbr)
    slot[rows[nbr < n], nbr[nbr < n]] = torch.arange(nbr.shape[1]).expand_as(nbr)[nbr < n]
    src, tgt = want["edge_index_1"]
    dense = torch.zeros_like(alpha)
    dense[tgt // n, tgt % n, slot[tgt % n, src % n]] = want["att_weight_1"].reshape(-1)
    assert int(slot[tgt % n, src % n].min()) >= 0 and src.numel() == b * int(deg.sum())
    close(alpha, dense, "att_weight_1")
    assert bool((alpha[:, nbr >= n] == 0.0).all())
    affine = [ref.bn_fold_ref(*(p[bn + key] for key in ("weight", "bias", "running_mean", "running_var")), 1e-5)
              for bn in ("gnn_layers.0.bn.", "bn_outlayer_in.")]
    out, h2 = ref.head_ref(z, p["embedding.weight"], *affine, p["out_layer.mlp.0.weight"], p["out_layer.mlp.0.bias"])
    assert h2.shape == (b, n, d) and float(h2.min()) >= 0.0
    # eps reaches gdn_bn_fold as an fp32 number (1e-5 rounded): its distance from the oracle's double 1e-5 is the
    # only difference, 3.6e-13 relative in var + eps, so the head is compared at 1e-11
    assert float((out - want["out"]).abs().max()) <= 1e-11 * float(want["out"].abs().max().clamp_min(1.0))


def unpack(form):
    return dict(proj=form & 15, lst=form >> 4 & 15, threads=(form >> 8 & 15) * 256, slices=1 + (form >> 12 & 1),
                lists_lds=form >> 13 & 1, wl=form >> 14 & 1, chunked=form >> 15 & 1, xrows=form >> 16)


def test_projection_cases_land_in_the_cells_they_claim():
    lib = _lib.load()
    forms = []
    for c in stages.PROJECT_CASES:
        n, w, d = c["n"], c["w"], c["d"]
        flags = {"plain": 0, "wide": _lib.ROUTE_WIDE, "series": _lib.ROUTE_SERIES}[c["entry"]]
        assert lib.gdn_kernel_family(_lib.STAGE_PROJECT, n, w, d, 1, flags) & 0xff == c["family"], c["id"]
        if c["entry"] == "wide":       # `_wide` cases are the dense shapes: the plain entry point never runs TILE there
            assert lib.gdn_kernel_family(_lib.STAGE_PROJECT, n, w, d, 1, 0) & 0xff == DENSE, c["id"]
        form = lib.gdn_tile_forward_form(_lib.STAGE_PROJECT, n, w, d, 0)
        if c["family"] != TILE:
            assert form == -1 or c["family"] == DENSE or c["entry"] == "series", c["id"]
            continue
        f = unpack(form)
        forms.append(f)
        for key in ("proj", "threads", "slices", "wl", "chunked"):
            assert f[key] == c[key], (c["id"], key, f)
        assert f["lst"] == 0 and f["lists_lds"] == 0 and (f["xrows"] < n) == bool(c["chunked"]), (c["id"], f)
        assert c["xrows"] is None or f["xrows"] == c["xrows"], (c["id"], f)
    # the coverage: every PROJ value, both thread counts, both slice counts, weights in LDS and not, a chunked x tile
    assert {f["proj"] for f in forms} == {0, 1, 2, 3, 4, 5}
    assert {f["threads"] for f in forms} == {256, 512} and {f["slices"] for f in forms} == {1, 2}
    assert {f["wl"] for f in forms} == {0, 1} and {f["chunked"] for f in forms} == {0, 1}
    assert all(any(f["chunked"] and f["proj"] == p for f in forms) for p in (0, 1, 5))
    assert {c["family"] for c in stages.PROJECT_CASES} == {DENSE, TILE, LARGE, LONG, ANY}
    by = stages.PROJECT
    assert by["proj0-w1"]["w"] == 1 and by["proj1-w40"]["w"] > 32 and by["large-series"]["entry"] == "series"
    assert all(by[name]["family"] != DENSE for name in stages.PROJECT_SCALED)
    assert {by[name]["family"] for name in stages.PROJECT_SCALED} == {TILE, LARGE, LONG, ANY}


def test_aggregate_cases_land_in_the_cells_they_claim():
    lib = _lib.load()
    forms = []
    for c in stages.AGG_CASES:
        n, d, k = c["n"], c["d"], c["k"]
        assert lib.gdn_kernel_family(_lib.STAGE_AGGREGATE, n, 1, d, k, int(c["wide"])) & 0xff == c["family"], c["id"]
        if c["wide"]:
            assert lib.gdn_kernel_family(_lib.STAGE_AGGREGATE, n, 1, d, k, 0) & 0xff == DENSE, c["id"]
        assert k <= n and (not c["hub"] or k <= n - 2)
        form = lib.gdn_tile_forward_form(_lib.STAGE_AGGREGATE, n, 1, d, k)
        if c["family"] != TILE:
            assert form == -1 or c["family"] == DENSE, c["id"]
            continue
        f = unpack(form)
        forms.append(f)
        for key in ("lst", "threads", "slices", "lists_lds"):
            assert f[key] == c[key], (c["id"], key, f)
        assert f["proj"] == 1 and f["wl"] == 0 and f["chunked"] == 0 and f["xrows"] == 0, (c["id"], f)
    assert {f["lst"] for f in forms} == {0, 1, 2, 5, 6}
    assert {f["threads"] for f in forms} == {256, 512} and {f["slices"] for f in forms} == {1, 2}
    assert {(f["lst"], f["lists_lds"]) for f in forms} >= {(0, 0), (0, 1), (6, 0), (1, 1)}
    assert any(f["slices"] == 2 and not f["lists_lds"] for f in forms)       # the sliced d = 128 aggregate, global lists
    assert {c["family"] for c in stages.AGG_CASES} == {DENSE, TILE, LARGE, ANY}
    by = stages.AGG
    assert by["lst1-k1"]["k"] == 1 and by["lst2-k-equals-n"]["k"] == by["lst2-k-equals-n"]["n"]
    assert by["lst0-lists-lds"]["k"] + 1 > 80 and by["lst5-d128"]["d"] == 128 and by["lst5-d128"]["slices"] == 1
    # the extreme-logit runs: one TILE case per LST value, and LARGE, ANY, DENSE; per-window scale: no DENSE case
    extreme = [by[name] for name in stages.AGG_EXTREME]
    assert {c["lst"] for c in extreme if c["family"] == TILE} == {0, 1, 2, 5, 6}
    assert {c["family"] for c in extreme} == {TILE, LARGE, ANY, DENSE}
    assert {by[name]["family"] for name in stages.AGG_SCALED} == {TILE, LARGE, ANY}
    assert {by[name]["family"] for name in stages.AGG_EQUAL} == {TILE, LARGE, ANY, DENSE}
    assert {by[name]["lst"] for name in stages.ALPHA_NULL if by[name]["family"] == TILE} == {0, 1, 2, 5, 6}
    for stage, name in (("p", "proj0-n50"), ("a", "lst2-512")):               # `_wide` = plain: both must be TILE
        c = stages.PROJECT[name] if stage == "p" else by[name]
        args = (_lib.STAGE_PROJECT, c["n"], c["w"], c["d"], 1) if stage == "p" else \
            (_lib.STAGE_AGGREGATE, c["n"], 1, c["d"], c["k"])
        assert lib.gdn_kernel_family(*args, 0) == lib.gdn_kernel_family(*args, _lib.ROUTE_WIDE) == TILE
    assert lib.gdn_tile_forward_form(_lib.STAGE_FUSED, 27, 5, 64, 5) == -1       # FUSED is not reported
    assert lib.gdn_tile_forward_form(_lib.STAGE_PROJECT, 27, 65, 64, 5) == -1    # make_plan refuses w > 64


def test_head_terms_and_fold_cases():
    lib = _lib.load()
    for c in stages.HEAD_CASES:
        b, n, d = c["shape"]
        assert lib.gdn_kernel_family(_lib.STAGE_HEAD, n, 1, d, 1, 0) & 0xff == c["family"], c["id"]
        assert (b * n) % stages.HEAD_ROWS_PER_WORKGROUP != 0
    assert {c["shape"][2] for c in stages.HEAD_CASES} == {16, 32, 64, 128, 3, 24, 200}
    assert {1, 650} <= {c["shape"][1] for c in stages.HEAD_CASES}
    for c in stages.TERMS_CASES:
        n, w, d = c["shape"]
        assert lib.gdn_kernel_family(_lib.STAGE_TERMS, n, w, d, 1, 0) & 0xff == c["family"], c["id"]
        assert ref.terms_pitch(w) == lib.gdn_terms_pitch(w)
    assert sorted(c["family"] for c in stages.TERMS_CASES) == [TILE, TILE, LONG, LONG, LONG, ANY, ANY]
    assert stages.BN_FOLD_CHANNELS == (3, 16, 200, 256)


def test_inputs_are_what_the_cases_need():
    """Mixed degrees on the learned-style graph, the hub graph's hub, the all-equal targets, underflow in the extreme
    run, both signs under both ReLUs of the head."""
    for name, kind in stages.AGG_RUNS:
        c = stages.AGG[name]
        nbr, deg = stages.agg_lists(name, kind)
        t = stages.agg_inputs(name, kind)
        if kind == "learned" and c["k"] < c["n"]:
            assert {int(v) for v in deg.unique()} == {c["k"], c["k"] + 1}, name
        if kind == "extreme":
            alpha = stages.agg_reference(name, kind)[0]["alpha"]
            assert bool((alpha[nbr.expand_as(alpha) < c["n"]] < 1e-45).any()), name
        if kind == "equal":
            alpha = stages.agg_reference(name, kind)[0]["alpha"]
            assert len(t["targets"]) == 3
            for i in t["targets"]:
                assert float((alpha[:, i, :int(deg[i])] - 1.0 / int(deg[i])).abs().max()) < 1e-15, (name, i)
    for c in stages.HEAD_CASES:
        t = stages.head_inputs(c["id"])
        d = c["shape"][2]
        h1 = t["z"] * t["bn1"][:d] + t["bn1"][d:]
        assert d < 16 or 0.25 < float((h1 < 0).float().mean()) < 0.75
        h2 = stages.head_reference(c["id"])[0]["h2"]
        assert d < 16 or 0.2 < float((h2 == 0).double().mean()) < 0.9          # (three channels: too few to count)


def test_yardsticks_are_the_cpu_float32_error_of_the_cases():
    """Every case's stage in torch float32 on the CPU against float64, in the measure of the GPU tests: the recorded
    YARDSTICK of a cell (bound = 4 x it) is the worst over the cell's runs.  The recorded number may not exceed twice what
    this machine measures (CPU kernels may sum in another order; the bound cannot drift up unnoticed)."""
    measured = stages.measured_yardsticks()
    for key in sorted(measured):
        print(f"[fwd-stages] yardstick {key:26s} measured {measured[key]:9.2e}   recorded "
              f"{stages.YARDSTICK.get(key, float('nan')):9.2e}")
    assert set(measured) == set(stages.YARDSTICK)
    # the runs on which float32 on the CPU misses the suite's element-wise bar itself (the GPU file judges them by their
    # cell's bound alone): randn windows (sums of up to 200 products of size 1, results near 0 among results of size
    # 30) and extreme logits (a logit of size 100 carries an fp32 ulp of 7.6e-6 into alpha); never a plain run
    beyond = [(name, kind) for name, kind in stages.PROJECT_RUNS if not stages.project_reference(name, kind)[2]] + \
             [(name, kind) for name, kind in stages.AGG_RUNS if not stages.agg_reference(name, kind)[2]]
    print("[fwd-stages] CPU float32 misses the suite's bar on:", beyond)
    assert all(kind in ("randn", "extreme") for _name, kind in beyond), beyond
    for key, value in measured.items():
        assert 0 < stages.YARDSTICK[key] <= 2 * value, (key, value, stages.YARDSTICK[key])
        # the bars the suite already had (3e-6 for z / alpha, 2e-6 elsewhere) stay on top of every cell but the
        # extreme-logit ones, whose own fp32 error is at the bar (judge() in the GPU file); no other cell needs them lifted
        assert key.endswith("/extreme") or stages.FACTOR * stages.YARDSTICK[key] <= 3e-6, key
