"""The staged forward stage by stage, every kernel form against a float64 reference of the same stage
(tests/_graph_layer_fwd_ref.py): gdn_project_fwd[_wide|_series], gdn_attn_aggregate_fwd[_wide], gdn_head_fwd,
gdn_node_terms, gdn_bn_fold, and the bit claims of include/gdn_hip.h.

A stage takes its inputs as given (a given node_terms; given s_i / s_j; given affine tables), so a stage is judged alone.
Measure, as in tests/test_gpu_backward_stages.py: per window and tensor max|got - want| / max(1, max|want|) on values
divided by the window's scale; a test's ratio is the worst of its tensors and windows, printed with -s.
Bound of a cell = 4 x its YARDSTICK, the worst error of torch float32 on the CPU against float64 over the cell's own
runs (the factor covers the summation order; tests/test_cpu_forward_stages_ref.py measures the yardsticks again without
a GPU).  On top of it the bars the suite already had hold element by element: atol 3e-6 / rtol 1e-5 for z and alpha,
atol 2e-6 / rtol 1e-5 for xlin, s_i, s_j, out — on every run on which float32 on the CPU meets them itself.  It does not
on the randn windows of proj1-chunked, proj1-sliced, large-n600 and long-w200 (sums of 64 to 200 products of size 1:
results near 0 among results of size 30) nor on the extreme-logit runs but lst1 / ANY / DENSE (a logit of size 100
carries an fp32 ulp of 7.6e-6 into alpha; float32 on the CPU is 1.8e-6 to 2.9e-6 from float64 there): those runs demand
more than fp32 gives and are held to their cell's bound alone, the extreme-logit runs as cells of their own.
DENSE keeps the bar of tests/test_gpu_dense_and_bf16.py (atol 2e-6, rtol 1e-5) on every run: its 16-bit operand split is
not fp32's error.  Every output is cut from the middle of a buffer filled with a bit pattern: the 64 floats in front
of and behind it must keep their bits and every element in between must have been written; alpha is exactly 0.0 in
the padding and its rows sum to 1 within the cell's bound.
The tables below name the cell every case is there for; tests/test_cpu_forward_stages_ref.py holds them to
gdn_kernel_family and gdn_tile_forward_form and asserts the coverage, so they cannot drift when the routing changes.
Every candidate shape of the issue landed in its cell, but (9, 70, 50) of gdn_node_terms: TERMS is LONG at w > 64
whatever the width, so it stays as a LONG case and (9, 40, 50) is the ANY one.

MEASURED on the MI355X (cell: cases; yardstick; bound; worst ratio over the cell's runs — uniform and randn windows,
mixed-degree and hub graphs, all-equal logits, per-window scale, alpha = NULL; the whole file takes 9.1 s, no case more
than 0.3 s):
  gdn_project_fwd[_wide|_series]
    TILE/proj0   proj0-w1, proj0-n50, proj0-512-chunked                         1.27e-7   5.1e-7   1.27e-7
    TILE/proj1   proj1-weights-lds, -w40, -512-weights-global, -chunked, -sliced 4.36e-7   1.7e-6   4.36e-7
    TILE/proj2   proj2-d32, proj2-wide-n27, proj2-wide-n127                      1.77e-7   7.1e-7   1.91e-7
    TILE/proj3   proj3-d32, proj3-n129                                           2.14e-7   8.6e-7   2.62e-7
    TILE/proj4   proj4-d128, proj4-n128                                          2.65e-7   1.1e-6   2.65e-7
    TILE/proj5   proj5, proj5-sliced-chunked, proj5-chunked-d32                  2.68e-7   1.1e-6   2.68e-7
    DENSE        dense-n27, dense-n127-w32                                       -         the bar  2.32e-7
    LARGE        large-n600, large-series                                        4.25e-7   1.7e-6   4.25e-7
    LONG         long-w65, long-w200                                             7.01e-7   2.8e-6   7.01e-7
    ANY          any-d24, any-d50-w70, any-d200                                  3.23e-7   1.3e-6   4.11e-7
  (where the worst ratio equals the yardstick the kernel adds the products of a row in the order torch's CPU matmul
  does: the same bits)
  gdn_attn_aggregate_fwd[_wide]                                                             plain / extreme logits
    TILE/lst1    lst1-n12, lst1-k1, lst1-sliced               2.66e-7 / 1.74e-7   1.1e-6 / 7.0e-7   2.39e-7 / 1.74e-7
    TILE/lst2    lst2-k-equals-n, lst2-wide, lst2-512         4.72e-7 / 1.95e-6   1.9e-6 / 7.8e-6   4.51e-7 / 1.97e-6
    TILE/lst5    lst5-d128, lst5-512                          4.37e-7 / 1.94e-6   1.7e-6 / 7.8e-6   5.86e-7 / 1.99e-6
    TILE/lst6    lst6, lst6-sliced, lst6-n2000                4.75e-7 / 2.86e-6   1.9e-6 / 1.1e-5   6.06e-7 / 2.86e-6
    TILE/lst0    lst0-lists-lds, lst0-lists-global, lst0-n128 4.57e-7 / 2.00e-6   1.8e-6 / 8.0e-6   5.53e-7 / 2.04e-6
    DENSE        dense-n40, dense-n127-k62                    -                   the bar           6.44e-7 / 2.99e-7
    LARGE        large                                        2.92e-7 / 1.83e-6   1.2e-6 / 7.3e-6   3.19e-7 / 1.83e-6
    ANY          any-d24, any-d3, any-d200                    3.09e-7 / 8.21e-7   1.2e-6 / 3.3e-6   2.09e-7 / 8.42e-7
    rows of alpha sum to 1 within 2.8e-7 everywhere
  gdn_head_fwd   TILE  tile-d16, -d32-n1, -d64-n650, -d128    2.11e-7   8.4e-7   2.16e-7
                 ANY   any-d3, any-d24, any-d200              2.74e-7   1.1e-6   1.32e-7
  gdn_node_terms TILE 1.47e-7 / 5.9e-7, LONG 1.36e-7 / 5.4e-7, ANY 1.49e-7 / 6.0e-7; gdn_bn_fold 5.33e-8 / 2.1e-7: under
                 their bounds (every test prints its ratio)
  bit claims     alpha = NULL: the same z bits on TILE (every LST), LARGE, ANY; DENSE within 1e-6.  `_wide` = plain on
                 the tile, `_series` = plain beyond it, two calls, and 3 windows alone against the same 3 inside a
                 3000-window launch: the same bits.
FOUND: nothing.  No case failed on the kernels; the four projection runs and five extreme-logit runs named above missed
the suite's element-wise bar exactly where float32 on the CPU misses it.
"""
import functools

import numpy as np
import pytest
import torch

import _graph_layer_fwd_ref as ref
from gdn_amd import _lib, ops

pytestmark = pytest.mark.gpu

NONE, DENSE, TILE, LARGE, LONG, ANY = range(6)
FAMILY_NAMES = ("NONE", "DENSE", "TILE", "LARGE", "LONG", "ANY")
FACTOR = 4.0                                   # bound = FACTOR x the CPU-float32 error (covers the summation order)
BAR_Z = dict(atol=3e-6, rtol=1e-5)             # z, alpha: the bar of tests/test_gpu_backward_stages.py
BAR_S = dict(atol=2e-6, rtol=1e-5)             # xlin, s_i, s_j, out (and DENSE): tests/test_gpu_dense_and_bf16.py
GUARD = 64                                     # floats in front of and behind every output
PATTERN = 0x7fc5a5a5                           # as int32; as a float a quiet NaN with a payload no kernel produces

# cell -> the worst CPU-float32 ratio over the cell's runs (tests/test_cpu_forward_stages_ref.py measures them again and
# holds these numbers to what it finds); a cell's bound is FACTOR x its yardstick
YARDSTICK = {
    "PROJECT/TILE/proj0": 1.27e-07, "PROJECT/TILE/proj1": 4.36e-07, "PROJECT/TILE/proj2": 1.77e-07,
    "PROJECT/TILE/proj3": 2.14e-07, "PROJECT/TILE/proj4": 2.65e-07, "PROJECT/TILE/proj5": 2.68e-07,
    "PROJECT/LARGE": 4.25e-07, "PROJECT/LONG": 7.01e-07, "PROJECT/ANY": 3.23e-07,
    "AGGREGATE/TILE/lst0": 4.57e-07, "AGGREGATE/TILE/lst1": 2.66e-07, "AGGREGATE/TILE/lst2": 4.72e-07,
    "AGGREGATE/TILE/lst5": 4.37e-07, "AGGREGATE/TILE/lst6": 4.75e-07, "AGGREGATE/LARGE": 2.92e-07,
    "AGGREGATE/ANY": 3.09e-07,
    "AGGREGATE/TILE/lst0/extreme": 2.00e-06, "AGGREGATE/TILE/lst1/extreme": 1.74e-07,
    "AGGREGATE/TILE/lst2/extreme": 1.95e-06, "AGGREGATE/TILE/lst5/extreme": 1.94e-06,
    "AGGREGATE/TILE/lst6/extreme": 2.86e-06, "AGGREGATE/LARGE/extreme": 1.83e-06, "AGGREGATE/ANY/extreme": 8.21e-07,
    "HEAD/TILE": 2.11e-07, "HEAD/ANY": 2.74e-07, "TERMS/TILE": 1.47e-07, "TERMS/LONG": 1.36e-07, "TERMS/ANY": 1.49e-07,
    "BN_FOLD": 5.33e-08,
}


def _proj(name, n, w, d, family, entry="plain", proj=-1, threads=0, slices=1, wl=0, chunked=0, xrows=None):
    return dict(id=name, n=n, w=w, d=d, family=family, entry=entry, proj=proj, threads=threads, slices=slices, wl=wl,
                chunked=chunked, xrows=xrows)


# (n, w, d) of gdn_project_fwd ("plain"), `_wide` or `_series`: the family, and for TILE the fields of
# gdn_tile_forward_form (PROJ, threads, slices, lin weights in LDS, x tile chunked, its rows where the issue names them)
PROJECT_CASES = [
    _proj("proj0-w1", 5, 1, 16, TILE, proj=0, threads=256, wl=1),
    _proj("proj0-n50", 50, 7, 16, TILE, proj=0, threads=256, wl=1),
    _proj("proj1-weights-lds", 40, 12, 16, TILE, proj=1, threads=256, wl=1),
    _proj("proj1-w40", 90, 40, 64, TILE, proj=1, threads=256, wl=1),                         # w > 32: in w-chunks
    _proj("proj1-512-weights-global", 260, 33, 64, TILE, proj=1, threads=512),
    _proj("proj1-chunked", 500, 64, 64, TILE, proj=1, threads=512, chunked=1, xrows=112),
    _proj("proj0-512-chunked", 2000, 8, 16, TILE, proj=0, threads=512, chunked=1),
    _proj("proj1-sliced", 300, 64, 128, TILE, proj=1, threads=512, slices=2),
    _proj("proj2-d32", 33, 5, 32, TILE, proj=2, threads=256),
    _proj("proj2-wide-n27", 27, 5, 64, TILE, entry="wide", proj=2, threads=256),
    _proj("proj2-wide-n127", 127, 15, 64, TILE, entry="wide", proj=2, threads=256),
    _proj("proj3-d32", 200, 12, 32, TILE, proj=3, threads=256),
    _proj("proj3-n129", 129, 16, 64, TILE, proj=3, threads=256),
    _proj("proj4-d128", 40, 30, 128, TILE, proj=4, threads=256),
    _proj("proj4-n128", 128, 20, 64, TILE, proj=4, threads=256),
    _proj("proj5", 300, 30, 64, TILE, proj=5, threads=512),
    _proj("proj5-sliced-chunked", 512, 30, 128, TILE, proj=5, threads=512, slices=2, chunked=1, xrows=192),
    _proj("proj5-chunked-d32", 1100, 8, 32, TILE, proj=5, threads=512, chunked=1, xrows=64),
    _proj("dense-n27", 27, 5, 64, DENSE),
    _proj("dense-n127-w32", 127, 32, 64, DENSE),
    _proj("large-n600", 600, 64, 64, LARGE),
    _proj("large-series", 129, 16, 64, LARGE, entry="series"),                             # a TILE shape: `_series` is LARGE
    _proj("long-w65", 12, 65, 64, LONG),
    _proj("long-w200", 5, 200, 32, LONG),
    _proj("any-d24", 12, 4, 24, ANY),
    _proj("any-d50-w70", 9, 70, 50, ANY),
    _proj("any-d200", 33, 8, 200, ANY),
]
PROJECT = {c["id"]: c for c in PROJECT_CASES}


def _agg(name, n, d, k, family, wide=False, hub=False, lst=-1, threads=0, slices=1, lists_lds=0):
    return dict(id=name, n=n, d=d, k=k, family=family, wide=wide, hub=hub, lst=lst, threads=threads, slices=slices,
                lists_lds=lists_lds)


# (n, d, k) of gdn_attn_aggregate_fwd[_wide]: the family, and for TILE LST, threads, slices, lists in LDS
AGG_CASES = [
    _agg("lst1-n12", 12, 16, 3, TILE, lst=1, threads=256, lists_lds=1),
    _agg("lst1-k1", 33, 32, 1, TILE, lst=1, threads=256, lists_lds=1),
    _agg("lst2-k-equals-n", 20, 32, 20, TILE, lst=2, threads=256, lists_lds=1),
    _agg("lst2-wide", 127, 64, 30, TILE, wide=True, lst=2, threads=256, lists_lds=1),
    _agg("lst2-512", 300, 64, 30, TILE, hub=True, lst=2, threads=512, lists_lds=1),
    _agg("lst5-d128", 200, 128, 63, TILE, lst=5, threads=512, lists_lds=1),                  # d = 128 unsliced
    _agg("lst5-512", 600, 16, 70, TILE, lst=5, threads=512, lists_lds=1),
    _agg("lst6", 512, 64, 64, TILE, hub=True, lst=6, threads=512),
    _agg("lst6-sliced", 512, 128, 64, TILE, lst=6, threads=512, slices=2),
    _agg("lst6-n2000", 2000, 16, 5, TILE, lst=6, threads=512),
    _agg("lst1-sliced", 330, 128, 8, TILE, lst=1, threads=512, slices=2, lists_lds=1),
    _agg("lst0-lists-lds", 200, 32, 100, TILE, lst=0, threads=256, lists_lds=1),
    _agg("lst0-lists-global", 512, 64, 100, TILE, hub=True, lst=0, threads=512),
    _agg("lst0-n128", 128, 16, 90, TILE, lst=0, threads=256, lists_lds=1),
    _agg("dense-n40", 40, 64, 6, DENSE),
    _agg("dense-n127-k62", 127, 64, 62, DENSE),
    _agg("large", 650, 64, 5, LARGE, hub=True),
    _agg("any-d24", 12, 24, 3, ANY),
    _agg("any-d3", 70, 3, 5, ANY),
    _agg("any-d200", 33, 200, 8, ANY),
]
AGG = {c["id"]: c for c in AGG_CASES}

# (batch, n, d) of gdn_head_fwd: TILE at the four widths, ANY at three, n = 1, n = 650; no row count is a multiple of
# the 64 rows a workgroup takes per pass (16 row groups x 4 rows in flight, both kernels)
HEAD_ROWS_PER_WORKGROUP = 64
HEAD_CASES = [
    dict(id="tile-d16", shape=(3, 27, 16), family=TILE), dict(id="tile-d32-n1", shape=(5, 1, 32), family=TILE),
    dict(id="tile-d64-n650", shape=(2, 650, 64), family=TILE), dict(id="tile-d128", shape=(3, 40, 128), family=TILE),
    dict(id="any-d3", shape=(3, 7, 3), family=ANY), dict(id="any-d24", shape=(2, 70, 24), family=ANY),
    dict(id="any-d200", shape=(3, 33, 200), family=ANY),
]
# (n, w, d) of gdn_node_terms (STAGE_TERMS family)
TERMS_CASES = [
    dict(id="tile", shape=(27, 5, 64), family=TILE), dict(id="tile-d128", shape=(40, 64, 128), family=TILE),
    dict(id="long-w65", shape=(12, 65, 64), family=LONG), dict(id="long-w200", shape=(5, 200, 32), family=LONG),
    dict(id="any-d24", shape=(12, 4, 24), family=ANY), dict(id="any-d50", shape=(9, 40, 50), family=ANY),
    dict(id="long-w70-d50", shape=(9, 70, 50), family=LONG),        # the route puts w > 64 in front of the width: LONG
]
BN_FOLD_CHANNELS = (3, 16, 200, 256)

# the runs of every case: what the GPU tests execute and what the yardstick is measured over
PROJECT_SCALED = ("proj0-n50", "proj3-n129", "large-n600", "long-w65", "any-d24")          # one (two) per fp32 family
PROJECT_RUNS = ([(c["id"], kind) for c in PROJECT_CASES for kind in ("uniform", "randn")]
                + [(name, "scaled") for name in PROJECT_SCALED])
AGG_EXTREME = ("lst1-n12", "lst2-512", "lst5-d128", "lst6", "lst0-lists-lds", "large", "any-d24", "dense-n40")
AGG_EQUAL = ("lst2-512", "lst0-n128", "large", "any-d3", "dense-n40")
AGG_SCALED = ("lst6", "lst1-sliced", "large", "any-d24")
AGG_RUNS = ([(c["id"], "learned") for c in AGG_CASES] + [(c["id"], "hub") for c in AGG_CASES if c["hub"]]
            + [(name, "extreme") for name in AGG_EXTREME] + [(name, "equal") for name in AGG_EQUAL]
            + [(name, "scaled") for name in AGG_SCALED])
DENSE_X_LIMIT = 7500.0      # include/gdn_hip.h "range guard": 8 |value| must stay below the f16 maximum

WORST = {}                   # cell -> worst ratio seen in this session (printed by every test)


def cell(stage, case, kind=""):
    """The cell of the docstring's tables a case belongs to: the yardstick, the bound and the worst ratio are per cell.
    The extreme-logit runs of a cell are a cell of their own (module docstring)."""
    name = f"{stage}/{FAMILY_NAMES[case['family']]}"
    if kind == "extreme":
        return cell(stage, case) + "/extreme"
    if case["family"] == TILE and stage == "PROJECT":
        name += f"/proj{case['proj']}"
    if case["family"] == TILE and stage == "AGGREGATE":
        name += f"/lst{case['lst']}"
    return name


def bound(key):
    return FACTOR * YARDSTICK[key]


def _note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"[fwd-stages] {key:26s} ratio {ratio:9.2e}   bound {bound(key) if key in YARDSTICK else float('nan'):9.2e}"
          f"   worst so far {WORST[key]:9.2e}")


# ---- inputs (seeded CPU generators) and references --------------------------------------------------------------

def _seed(table, name, kind):
    return 7000 + 37 * [c["id"] for c in table].index(name) + sum(map(ord, kind))


def mixed_topk(n, k, seed):
    """[n, k] int64 table as a learned graph gives it (distinct entries, the sensor itself at rank 0) for the odd rows;
    the even rows do not name themselves (unless k = n), so deg = k and deg = k + 1 both occur."""
    g = torch.Generator().manual_seed(seed)
    score = torch.rand((n, n), generator=g)
    idx = torch.arange(n)
    score[idx, idx] = torch.where(idx % 2 == 1, 2.0, -1.0)
    return score.topk(k, dim=1).indices


@functools.lru_cache(maxsize=None)
def project_inputs(name, kind):
    """x ~ U(0, 1) ("uniform") or randn; lin_w, node_terms ~ randn (the padding of a_i / a_j zero, as gdn_node_terms
    leaves it); "scaled": window b times 10^u, u ~ U(-6, 4).  `_series` cases: the windows are cut from a series."""
    c = PROJECT[name]
    n, w, d = c["n"], c["w"], c["d"]
    seed = _seed(PROJECT_CASES, name, kind)
    g = torch.Generator().manual_seed(seed)
    b = 5 if kind == "scaled" else 2 + seed % 4
    p = ref.terms_pitch(w)
    terms = torch.randn((2 * p + 2 * n,), generator=g)
    terms[:2 * p].view(2, p)[:, w:] = 0.0
    t = dict(lin_w=torch.randn((d, w), generator=g), terms=terms, mags=torch.ones((b,)), first=2)
    draw = torch.randn if kind == "randn" else torch.rand
    if c["entry"] == "series":
        t["series"] = draw((n, t["first"] + b - 1 + w + 3), generator=g)
        t["x"] = torch.stack([t["series"][:, t["first"] + q:t["first"] + q + w] for q in range(b)]).contiguous()
    else:
        t["x"] = draw((b, n, w), generator=g)
    if kind == "scaled":
        t["mags"] = 10.0 ** (torch.rand((b,), generator=g) * 10 - 6)
        t["x"] = t["x"] * t["mags"].view(b, 1, 1)
    return t


@functools.lru_cache(maxsize=None)
def project_reference(name, kind):
    """(float64 xlin / s_i / s_j, the CPU-float32 ratio of the run, whether CPU float32 meets the suite's bar on it)."""
    t = project_inputs(name, kind)
    want = dict(zip(("xlin", "s_i", "s_j"), ref.project_ref(t["x"], t["lin_w"], t["terms"])))
    f32 = dict(zip(("xlin", "s_i", "s_j"), ref.project_ref(t["x"], t["lin_w"], t["terms"], dtype=torch.float32)))
    return (want, max(window_ratio(f32[key], want[key], t["mags"]) for key in want),
            all(meets_bar(f32[key], want[key], t["mags"], BAR_S) for key in want))


@functools.lru_cache(maxsize=None)
def agg_topk(name, kind):
    c = AGG[name]
    if kind == "hub":
        return ref.hub_topk(c["n"], c["k"], _seed(AGG_CASES, name, kind))
    return mixed_topk(c["n"], c["k"], _seed(AGG_CASES, name, "learned"))


@functools.lru_cache(maxsize=None)
def agg_lists(name, kind):
    return ref.nbr_of(agg_topk(name, kind))


@functools.lru_cache(maxsize=None)
def agg_inputs(name, kind):
    """xlin ~ randn; s_i, s_j ~ 2 randn (attention far from uniform, both signs of the logit); bias ~ 0.1 randn.
    "extreme": s_i, s_j ~ 30 randn; "equal": the sources of a few targets share one s_j, so those targets' logits are
    all equal; "scaled": xlin of window b times 10^u, u ~ U(-6, 4)."""
    c = AGG[name]
    n, d = c["n"], c["d"]
    seed = _seed(AGG_CASES, name, kind)
    g = torch.Generator().manual_seed(seed)
    b = 2 if n * ref.nbr_pitch(c["k"]) * d > 2_000_000 else 5 if kind == "scaled" else 2 + seed % 4
    amp = 30.0 if kind == "extreme" else 2.0
    t = dict(xlin=torch.randn((b, n, d), generator=g), s_i=amp * torch.randn((b, n), generator=g),
             s_j=amp * torch.randn((b, n), generator=g), bias=0.1 * torch.randn((d,), generator=g),
             mags=torch.ones((b,)), targets=[])
    if kind == "equal":
        nbr, deg = agg_lists(name, kind)
        shared = t["s_j"][:, int(nbr[3 % n, 0])].unsqueeze(1).clone()          # one value per window for all of them
        for q in range(3):
            i = (3 + 11 * q) % n
            t["s_j"][:, nbr[i, :int(deg[i])]] = shared
            t["targets"].append(i)
    if kind == "scaled":
        t["mags"] = 10.0 ** (torch.rand((b,), generator=g) * 10 - 6)
        t["xlin"] = t["xlin"] * t["mags"].view(b, 1, 1)
    return t


@functools.lru_cache(maxsize=None)
def agg_reference(name, kind):
    """(float64 z / alpha, the CPU-float32 ratio of the run, whether CPU float32 meets the suite's bar on it)."""
    t = agg_inputs(name, kind)
    nbr = agg_lists(name, kind)[0]
    args = (t["xlin"], t["s_i"], t["s_j"], t["bias"], nbr)
    want = dict(zip(("z", "alpha"), ref.aggregate_ref(*args)))
    f32 = dict(zip(("z", "alpha"), ref.aggregate_ref(*args, dtype=torch.float32)))
    ones = torch.ones_like(t["mags"])
    return (want, max(window_ratio(f32["z"], want["z"], t["mags"]), window_ratio(f32["alpha"], want["alpha"], ones)),
            meets_bar(f32["z"], want["z"], t["mags"], BAR_Z) and meets_bar(f32["alpha"], want["alpha"], ones, BAR_Z))


@functools.lru_cache(maxsize=None)
def head_inputs(name):
    """z ~ randn; embedding ~ randn; BatchNorm scales of both signs (about half of each ReLU's inputs negative)."""
    b, n, d = next(c for c in HEAD_CASES if c["id"] == name)["shape"]
    g = torch.Generator().manual_seed(300 + b * n + d)
    return dict(z=torch.randn((b, n, d), generator=g), emb=torch.randn((n, d), generator=g),
                bn1=torch.randn((2 * d,), generator=g), bn2=torch.randn((2 * d,), generator=g),
                out_w=torch.randn((d,), generator=g), out_b=torch.randn((1,), generator=g))


HEAD_KEYS = ("z", "emb", "bn1", "bn2", "out_w", "out_b")


@functools.lru_cache(maxsize=None)
def head_reference(name):
    t = head_inputs(name)
    args = [t[key] for key in HEAD_KEYS]
    want = dict(zip(("out", "h2"), ref.head_ref(*args)))
    f32 = dict(zip(("out", "h2"), ref.head_ref(*args, dtype=torch.float32)))
    ones = torch.ones((t["z"].shape[0],))
    return want, max(window_ratio(f32[key], want[key], ones) for key in want)


@functools.lru_cache(maxsize=None)
def terms_inputs(name):
    n, w, d = next(c for c in TERMS_CASES if c["id"] == name)["shape"]
    g = torch.Generator().manual_seed(500 + n + w + d)
    return [torch.randn((d, w), generator=g)] + [torch.randn((d,), generator=g) for _ in range(4)] + \
           [torch.randn((n, d), generator=g)]


@functools.lru_cache(maxsize=None)
def terms_reference(name):
    args = terms_inputs(name)
    want = ref.node_terms_ref(*args)
    return want, tensor_ratio(ref.node_terms_ref(*args, dtype=torch.float32), want)


@functools.lru_cache(maxsize=None)
def bn_fold_inputs(c):
    """weight of both signs, running variances from 1e-12 (channel 1) to ~4."""
    g = torch.Generator().manual_seed(900 + c)
    var = torch.rand((c,), generator=g) * 4 + 1e-3
    var[1] = 1e-12
    return torch.randn((c,), generator=g), torch.randn((c,), generator=g), torch.randn((c,), generator=g), var, 1e-5


@functools.lru_cache(maxsize=None)
def bn_fold_reference(c):
    args = bn_fold_inputs(c)
    want = ref.bn_fold_ref(*args)
    return want, tensor_ratio(ref.bn_fold_ref(*args, dtype=torch.float32), want)


def window_ratio(got, want, mags):
    """The measure of tests/test_gpu_backward_stages.py, window by window: max|got - want| / max(1, max|want|) on values
    divided by the window's scale; the worst window."""
    b = want.shape[0]
    scale = mags.double().view(b, *([1] * (want.dim() - 1)))
    diff = ((got.double() - want) / scale).abs().reshape(b, -1).max(dim=1).values
    top = (want / scale).abs().reshape(b, -1).max(dim=1).values.clamp_min(1.0)
    return float((diff / top).max())


def meets_bar(got, want, mags, bar):
    """Element by element on values divided by the window's scale: |got - want| <= atol + rtol |want|."""
    b = want.shape[0]
    scale = mags.double().view(b, *([1] * (want.dim() - 1)))
    return bool((((got.double() - want) / scale).abs() <= bar["atol"] + bar["rtol"] * (want / scale).abs()).all())


def tensor_ratio(got, want):
    return float((got.double() - want).abs().max() / want.abs().max().clamp_min(1.0))


def measured_yardsticks():
    """cell -> the worst CPU-float32 ratio over the cell's runs (tests/test_cpu_forward_stages_ref.py holds YARDSTICK
    to it).  DENSE has none: its bar is the existing one."""
    out = {}

    def note(key, value):
        out[key] = max(out.get(key, 0.0), value)

    for name, kind in PROJECT_RUNS:
        if PROJECT[name]["family"] != DENSE:
            note(cell("PROJECT", PROJECT[name]), project_reference(name, kind)[1])
    for name, kind in AGG_RUNS:
        if AGG[name]["family"] != DENSE:
            note(cell("AGGREGATE", AGG[name], kind), agg_reference(name, kind)[1])
    for c in HEAD_CASES:
        note(cell("HEAD", c), head_reference(c["id"])[1])
    for c in TERMS_CASES:
        note(cell("TERMS", c), terms_reference(c["id"])[1])
    for c in BN_FOLD_CHANNELS:
        note("BN_FOLD", bn_fold_reference(c)[1])
    return out


# ---- guarded launches --------------------------------------------------------------------------------------------

class Guarded:
    """An output tensor cut from the middle of a buffer filled with PATTERN: GUARD floats in front, GUARD behind."""

    def __init__(self, shape, device):
        numel = int(np.prod(shape))
        self.buf = torch.full((numel + 2 * GUARD,), PATTERN, dtype=torch.int32, device=device)
        self.out = self.buf[GUARD:GUARD + numel].view(torch.float32).view(shape)

    def intact(self):
        edge = torch.cat((self.buf[:GUARD], self.buf[-GUARD:]))
        return bool((edge == PATTERN).all())

    def written(self):
        return bool((self.out.reshape(-1).view(torch.int32) != PATTERN).all())


def _finish(outs, what):
    torch.cuda.synchronize()
    for key, g in outs.items():
        assert g.intact(), f"{what}: {key} wrote outside its rows"
        assert g.written(), f"{what}: {key} has rows nobody wrote"
    return {key: g.out.cpu() for key, g in outs.items()}


def run_project(name, t, device, entry=None):
    c = PROJECT[name]
    entry = entry or c["entry"]
    b, n, w = t["x"].shape
    d = c["d"]
    lin, terms = t["lin_w"].to(device), t["terms"].to(device)
    outs = dict(xlin=Guarded((b, n, d), device), s_i=Guarded((b, n), device), s_j=Guarded((b, n), device))
    ptrs = [outs[key].out.data_ptr() for key in ("xlin", "s_i", "s_j")]
    stream = torch.cuda.current_stream().cuda_stream
    if entry == "series":
        series = t["series"].to(device)
        _lib.call("gdn_project_fwd_series", series.data_ptr(), series.shape[1], t["first"], lin.data_ptr(),
                  terms.data_ptr(), b, n, w, d, *ptrs, stream)
    else:
        x = t["x"].to(device)
        _lib.call("gdn_project_fwd" + ("_wide" if entry == "wide" else ""), x.data_ptr(), lin.data_ptr(),
                  terms.data_ptr(), b, n, w, d, *ptrs, stream)
    return _finish(outs, f"project {name} {entry}")


def make_graph(name, kind, device):
    return ops.graph_from_topk(agg_topk(name, kind).to(device))


def run_aggregate(name, t, graph, device, want_alpha=True, wide=None):
    c = AGG[name]
    wide = c["wide"] if wide is None else wide
    b, n, d = t["xlin"].shape
    xlin, s_i, s_j, bias = (t[key].to(device) for key in ("xlin", "s_i", "s_j", "bias"))
    outs = dict(z=Guarded((b, n, d), device))
    if want_alpha:
        outs["alpha"] = Guarded((b, n, graph.pitch), device)
    dense = _lib.family(_lib.STAGE_AGGREGATE, n, 1, d, graph.k, int(wide)) == DENSE
    nbr = graph.nbr_ordered() if dense and not want_alpha else graph.nbr        # as ops.attn_aggregate_fwd
    _lib.call("gdn_attn_aggregate_fwd" + ("_wide" if wide else ""), xlin.data_ptr(), s_i.data_ptr(), s_j.data_ptr(),
              nbr.data_ptr(), graph.deg.data_ptr(), bias.data_ptr(), b, n, d, graph.k, outs["z"].out.data_ptr(),
              outs["alpha"].out.data_ptr() if want_alpha else None, torch.cuda.current_stream().cuda_stream)
    return _finish(outs, f"aggregate {name}")


def judge(key, case, got, want, mags, what, bar):
    """One tensor: the ratio under the cell's bound (fp32 families) and, element by element on values divided by the
    window's scale, under the bar the suite already had (bar = None: a run on which torch float32 on the CPU misses
    that bar itself — the cell's bound alone, module docstring); DENSE: that bar alone, always."""
    b = want.shape[0]
    scale = mags.double().view(b, *([1] * (want.dim() - 1)))
    assert bool(torch.isfinite(got).all()), (what, "not finite")
    ratio = window_ratio(got, want, mags)
    print(f"[fwd-stages]   {what:50s} {ratio:9.2e}")
    if bar is not None:
        np.testing.assert_allclose((got.double() / scale).numpy(), (want / scale).numpy(), err_msg=what,
                                   **(BAR_S if case["family"] == DENSE else bar))
    if case["family"] != DENSE:
        assert ratio <= bound(key), (what, ratio, bound(key))
    return ratio


# ---- (a) gdn_project_fwd[_wide|_series] ---------------------------------------------------------------------------

def check_form(stage, case, n, w, d, k):
    lib = _lib.load()
    flags = _lib.ROUTE_WIDE if case.get("entry") == "wide" or case.get("wide") else \
        _lib.ROUTE_SERIES if case.get("entry") == "series" else 0
    assert lib.gdn_kernel_family(stage, n, w, d, k, flags) & 0xff == case["family"], case["id"]
    if case["family"] == TILE:
        form = lib.gdn_tile_forward_form(stage, n, w, d, k)
        assert form >= 0 and (form & 15 if stage == _lib.STAGE_PROJECT else form >> 4 & 15) == \
            (case["proj"] if stage == _lib.STAGE_PROJECT else case["lst"]), (case["id"], hex(form))


@pytest.mark.parametrize("name,kind", PROJECT_RUNS, ids=[f"{a}-{b}" for a, b in PROJECT_RUNS])
def test_projection_against_float64(name, kind, gpu_device):
    """Every form of the projection on x ~ U(0, 1), on randn, and (one case per fp32 family) with a scale per window."""
    case = PROJECT[name]
    check_form(_lib.STAGE_PROJECT, case, case["n"], case["w"], case["d"], 1)
    t = project_inputs(name, kind)
    if kind == "scaled":
        assert float(t["mags"].max() / t["mags"].min()) > 100
    got = run_project(name, t, gpu_device)
    want, _, fp32_meets_bar = project_reference(name, kind)
    key = cell("PROJECT", case)
    bar = BAR_S if fp32_meets_bar or case["family"] == DENSE else None
    worst = max(judge(key, case, got[tag], want[tag], t["mags"], f"project {name} {kind} {tag}", bar)
                for tag in ("xlin", "s_i", "s_j"))
    _note(key, worst)


# ---- (b) gdn_attn_aggregate_fwd[_wide] ------------------------------------------------------------------------------

def check_aggregate(name, kind, got, what):
    case = AGG[name]
    t = agg_inputs(name, kind)
    want, _, fp32_meets_bar = agg_reference(name, kind)
    nbr, deg = agg_lists(name, kind)
    key = cell("AGGREGATE", case, kind)
    ones = torch.ones_like(t["mags"])
    bar = BAR_Z if fp32_meets_bar or case["family"] == DENSE else None
    worst = judge(key, case, got["z"], want["z"], t["mags"], f"{what} z", bar)
    if "alpha" in got:
        worst = max(worst, judge(key, case, got["alpha"], want["alpha"], ones, f"{what} alpha", bar))
        assert bool((got["alpha"][:, nbr >= case["n"]] == 0.0).all()), f"{what}: alpha is not 0 in the padding"
        rows = float((got["alpha"].double().sum(-1) - 1.0).abs().max())
        print(f"[fwd-stages]   {what:50s} {rows:9.2e}  (rows of alpha sum to 1)")
        assert rows <= (1e-5 if case["family"] == DENSE else bound(key)), (what, rows)      # DENSE: its existing bar
    _note(key, worst)
    return want


@pytest.mark.parametrize("name,kind", AGG_RUNS, ids=[f"{a}-{b}" for a, b in AGG_RUNS])
def test_aggregate_against_float64(name, kind, gpu_device):
    """Every form of the aggregate: on a graph of mixed degree ("learned": deg = k and k + 1), on the hub graph, with
    extreme logits (s ~ 30 randn: the exp of every slot but the largest underflows; the result stays finite and within
    the same bound), with targets whose logits are all equal (alpha uniform over deg), with a scale per window."""
    case = AGG[name]
    check_form(_lib.STAGE_AGGREGATE, case, case["n"], 1, case["d"], case["k"])
    t = agg_inputs(name, kind)
    nbr, deg = agg_lists(name, kind)
    if kind == "learned" and case["k"] < case["n"]:
        assert {int(v) for v in deg.unique()} == {case["k"], case["k"] + 1}
    if case["family"] == DENSE:
        assert float(t["xlin"].abs().max()) < DENSE_X_LIMIT            # the range note of include/gdn_hip.h
    got = run_aggregate(name, t, make_graph(name, kind, gpu_device), gpu_device)
    check_aggregate(name, kind, got, f"aggregate {name} {kind}")
    if kind == "extreme":
        want = agg_reference(name, kind)[0]["alpha"]
        assert bool((want[nbr.expand_as(want) < case["n"]] < 1e-45).any())      # below fp32's smallest number: exp gives 0
    key = cell("AGGREGATE", case, kind)
    for i in t["targets"]:
        uniform = 1.0 / int(deg[i])
        off = float((got["alpha"][:, i, :int(deg[i])].double() - uniform).abs().max())
        assert off <= (BAR_S["atol"] if case["family"] == DENSE else bound(key)), (name, i, off)


# ---- (c) gdn_head_fwd ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [c["id"] for c in HEAD_CASES])
def test_head_against_float64(name, gpu_device):
    """gdn_head_fwd with h2 requested and with h2 = NULL (the same `out` bits), the rows around both outputs intact."""
    case = next(c for c in HEAD_CASES if c["id"] == name)
    b, n, d = case["shape"]
    assert _lib.load().gdn_kernel_family(_lib.STAGE_HEAD, n, 1, d, 1, 0) & 0xff == case["family"]
    assert (b * n) % HEAD_ROWS_PER_WORKGROUP != 0
    t = head_inputs(name)
    dev = [t[key].to(gpu_device) for key in HEAD_KEYS]
    results = []
    for want_h2 in (True, False):
        outs = dict(out=Guarded((b, n), gpu_device))
        if want_h2:
            outs["h2"] = Guarded((b, n, d), gpu_device)
        _lib.call("gdn_head_fwd", *[v.data_ptr() for v in dev], b, n, d, outs["out"].out.data_ptr(),
                  outs["h2"].out.data_ptr() if want_h2 else None, torch.cuda.current_stream().cuda_stream)
        results.append(_finish(outs, f"head {name} h2={want_h2}"))
    assert torch.equal(results[0]["out"], results[1]["out"])
    want, _ = head_reference(name)
    key = cell("HEAD", case)
    ones = torch.ones((b,))
    worst = max(judge(key, case, results[0][tag], want[tag], ones, f"head {name} {tag}", BAR_S) for tag in ("out", "h2"))
    _note(key, worst)


# ---- (d) gdn_node_terms, gdn_bn_fold --------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [c["id"] for c in TERMS_CASES])
def test_node_terms_against_float64(name, gpu_device):
    case = next(c for c in TERMS_CASES if c["id"] == name)
    n, w, d = case["shape"]
    assert _lib.load().gdn_kernel_family(_lib.STAGE_TERMS, n, w, d, 1, 0) & 0xff == case["family"]
    p = ref.terms_pitch(w)
    assert p == ops.terms_pitch(w)
    dev = [v.to(gpu_device) for v in terms_inputs(name)]
    outs = dict(terms=Guarded((2 * p + 2 * n,), gpu_device))
    _lib.call("gdn_node_terms", *[v.data_ptr() for v in dev], n, d, w, outs["terms"].out.data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    got = _finish(outs, f"node_terms {name}")["terms"]
    assert bool((got[:2 * p].view(2, p)[:, w:] == 0.0).all())            # the padding of a_i / a_j is exactly 0.0
    want, _ = terms_reference(name)
    key = cell("TERMS", case)
    ratio = tensor_ratio(got, want)
    np.testing.assert_allclose(got.double().numpy(), want.numpy(), **BAR_S)
    assert ratio <= bound(key), (name, ratio, bound(key))
    _note(key, ratio)


@pytest.mark.parametrize("c", BN_FOLD_CHANNELS)
def test_bn_fold_against_float64(c, gpu_device):
    """[scale | shift] with a running variance of 1e-12 among the channels (scale = weight / sqrt(1e-12 + eps))."""
    weight, bias, mean, var, eps = bn_fold_inputs(c)
    assert float(var.min()) < 2e-12
    dev = [v.to(gpu_device) for v in (weight, bias, mean, var)]
    outs = dict(affine=Guarded((2 * c,), gpu_device))
    _lib.call("gdn_bn_fold", *[v.data_ptr() for v in dev], eps, c, outs["affine"].out.data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    got = _finish(outs, f"bn_fold {c}")["affine"]
    want, _ = bn_fold_reference(c)
    ratio = tensor_ratio(got, want)
    assert ratio <= bound("BN_FOLD"), (c, ratio)
    _note("BN_FOLD", ratio)


# ---- (e) bit claims ------------------------------------------------------------------------------------------------------

def same_bits(a, b):
    return all(torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)) for key in a if key in b)


ALPHA_NULL = ("lst1-n12", "lst2-512", "lst5-512", "lst6-sliced", "lst0-lists-global", "large", "any-d200")


@pytest.mark.parametrize("name", ALPHA_NULL + ("dense-n40",))
def test_alpha_null_gives_the_same_z(name, gpu_device):
    """include/gdn_hip.h: alpha is optional.  The fp32 families give the same z bits with and without it; DENSE reads
    the bank-ordered lists without it and keeps the bar of tests/test_gpu_dense_and_bf16.py (atol 1e-6)."""
    t = agg_inputs(name, "learned")
    graph = make_graph(name, "learned", gpu_device)
    with_alpha = run_aggregate(name, t, graph, gpu_device)
    without = run_aggregate(name, t, graph, gpu_device, want_alpha=False)
    if AGG[name]["family"] == DENSE:
        np.testing.assert_allclose(without["z"].numpy(), with_alpha["z"].numpy(), atol=1e-6, rtol=0)
    else:
        assert same_bits(without, with_alpha)
    check_aggregate(name, "learned", without, f"aggregate {name} alpha=NULL")


def test_wide_and_plain_entry_points_give_the_same_bits_on_the_tile(gpu_device):
    """Neither (50, 7, 16) nor (300, 64, 30) is a dense shape: plain and `_wide` run the same TILE kernel."""
    t = project_inputs("proj0-n50", "uniform")
    assert same_bits(run_project("proj0-n50", t, gpu_device, "plain"), run_project("proj0-n50", t, gpu_device, "wide"))
    t = agg_inputs("lst2-512", "hub")
    graph = make_graph("lst2-512", "hub", gpu_device)
    assert same_bits(run_aggregate("lst2-512", t, graph, gpu_device, wide=False),
                     run_aggregate("lst2-512", t, graph, gpu_device, wide=True))


def test_series_entry_point_gives_the_plain_bits_beyond_the_tile(gpu_device):
    """include/gdn_hip.h: gdn_project_fwd_series gives "the same bits gdn_project_fwd gives on the same windows where the
    tile form refuses" — (600, 64, 64), windows cut from one series."""
    name = "large-n600"
    c = PROJECT[name]
    g = torch.Generator().manual_seed(11)
    b, first = 3, 5
    series = torch.rand((c["n"], first + b - 1 + c["w"] + 2), generator=g)
    t = dict(project_inputs(name, "uniform"), series=series, first=first)
    t["x"] = torch.stack([series[:, first + q:first + q + c["w"]] for q in range(b)]).contiguous()
    assert same_bits(run_project(name, t, gpu_device, "plain"), run_project(name, t, gpu_device, "series"))


@pytest.mark.parametrize("stage,name", [("project", "proj5-sliced-chunked"), ("project", "large-n600"),
                                        ("project", "dense-n27"), ("aggregate", "lst6"), ("aggregate", "lst0-lists-lds"),
                                        ("aggregate", "large"), ("aggregate", "dense-n127-k62")])
def test_two_calls_give_the_same_bits(stage, name, gpu_device):
    if stage == "project":
        t = project_inputs(name, "randn")
        first, second = (run_project(name, t, gpu_device) for _ in range(2))
    else:
        t = agg_inputs(name, "learned")
        graph = make_graph(name, "learned", gpu_device)
        first, second = (run_aggregate(name, t, graph, gpu_device) for _ in range(2))
    assert same_bits(first, second) and float(first["xlin" if stage == "project" else "z"].abs().max()) > 0


BIG_LAUNCH = 3000           # windows: more than the resident workgroups of any launch (256 CUs x 8 at the most)


def test_a_window_does_not_depend_on_the_launch_it_is_in(gpu_device):
    """The same 3 windows alone and as the first, middle and last of a 3000-window launch of a tiny shape (workgroups
    loop over windows there): projection (5, 3, 16) and aggregate (5, 16, 2), the same bits."""
    n, w, d, k = 5, 3, 16, 2
    lib = _lib.load()
    assert lib.gdn_kernel_family(_lib.STAGE_PROJECT, n, w, d, 1, 0) == TILE
    assert lib.gdn_kernel_family(_lib.STAGE_AGGREGATE, n, 1, d, k, 0) == TILE
    g = torch.Generator().manual_seed(77)
    pick = [0, BIG_LAUNCH // 2, BIG_LAUNCH - 1]
    stream = torch.cuda.current_stream().cuda_stream
    p = ref.terms_pitch(w)
    terms = torch.randn((2 * p + 2 * n,), generator=g)
    terms[:2 * p].view(2, p)[:, w:] = 0.0
    x, lin = torch.rand((BIG_LAUNCH, n, w), generator=g), torch.randn((d, w), generator=g)
    xlin, s_i, s_j = (torch.randn((BIG_LAUNCH, n, d), generator=g), 2 * torch.randn((BIG_LAUNCH, n), generator=g),
                      2 * torch.randn((BIG_LAUNCH, n), generator=g))
    bias = torch.randn((d,), generator=g)
    graph = ops.graph_from_topk(mixed_topk(n, k, 5).to(gpu_device))
    lin_d, terms_d, bias_d = lin.to(gpu_device), terms.to(gpu_device), bias.to(gpu_device)

    def project(xs):
        b = xs.shape[0]
        xd = xs.contiguous().to(gpu_device)
        outs = dict(xlin=Guarded((b, n, d), gpu_device), s_i=Guarded((b, n), gpu_device), s_j=Guarded((b, n), gpu_device))
        _lib.call("gdn_project_fwd", xd.data_ptr(), lin_d.data_ptr(), terms_d.data_ptr(), b, n, w, d,
                  *[outs[key].out.data_ptr() for key in ("xlin", "s_i", "s_j")], stream)
        return _finish(outs, f"project batch {b}")

    def aggregate(sel):
        b = len(sel) if sel is not None else BIG_LAUNCH
        take = (lambda v: v[sel]) if sel is not None else (lambda v: v)
        ins = [take(v).contiguous().to(gpu_device) for v in (xlin, s_i, s_j)]
        outs = dict(z=Guarded((b, n, d), gpu_device), alpha=Guarded((b, n, graph.pitch), gpu_device))
        _lib.call("gdn_attn_aggregate_fwd", *[v.data_ptr() for v in ins], graph.nbr.data_ptr(), graph.deg.data_ptr(),
                  bias_d.data_ptr(), b, n, d, k, outs["z"].out.data_ptr(), outs["alpha"].out.data_ptr(), stream)
        return _finish(outs, f"aggregate batch {b}")

    for alone, whole in ((project(x[pick]), project(x)), (aggregate(pick), aggregate(None))):
        assert all(float(v.abs().max()) > 0 for v in alone.values())
        assert same_bits(alone, {key: v[pick] for key, v in whole.items()})
