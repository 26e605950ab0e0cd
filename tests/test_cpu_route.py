"""The route table (include/gdn_hip.h): gdn_kernel_family against an independent restatement of the header over the
shapes of tools/route_grid.py, the host queries against the families they are defined from, and the Python callers
that ask the route instead of guessing.  Host only: no GPU, no launch."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import route_grid  # noqa: E402

from gdn_amd import _lib, ops  # noqa: E402

NONE, DENSE, TILE, LARGE, LONG, ANY = range(6)
PROJECT, AGGREGATE, ATTN_BWD, PROJECT_BWD, TERMS, HEAD, FUSED = range(7)
WIDE, BF16, SERIES = 1, 2, 4
TABLES_LDS = 0
SHAPES = route_grid.shapes()
LDS = 160 * 1024


def fam(stage, n, w, d, k, flags=0):
    return _lib.load().gdn_kernel_family(stage, n, w, d, k, flags) & 0xff


def bwd_form(n, d, k, flags=0):
    return _lib.load().gdn_kernel_family(ATTN_BWD, n, 1, d, k, flags) >> 8


def expected(stage, n, w, d, k, flags, lib):
    """The header's table, rule by rule; where it says "where the tile fits" the set of families the LDS budget may
    leave, bounded on both sides: gdn_tile_fits (the fused forward, which holds more than either staged kernel) fits
    => TILE, an xlin tile beyond 160 KB on its own => LARGE."""
    four, dense_shape = d in (16, 32, 64, 128), n <= 127 and d == 64 and k <= 63
    wide, bf16, series = flags & WIDE, flags & BF16, flags & SERIES
    tile_cols = 64 if d == 128 else d

    def tile_or(other):
        if lib.gdn_tile_fits(n, min(w, 64), d, k) == 1:
            return {TILE}
        return {other} if (n + 1) * tile_cols * 4 > LDS else {TILE, other}

    if stage in (PROJECT, AGGREGATE):
        with_w = stage == PROJECT
        dense_shape = n <= 127 and d == 64 and (w <= 32 if with_w else k <= 63)
        if bf16:
            return {DENSE} if dense_shape else {NONE}
        if not four:
            return {ANY}
        if with_w and w > 64:
            return {LONG}
        if with_w and series:
            return {LARGE}
        if dense_shape and not wide:
            return {DENSE}
        return tile_or(LARGE)
    if stage == ATTN_BWD:
        if not four:
            return {ANY}
        if dense_shape and not wide:
            return {DENSE}
        return {TILE, LARGE} if (n + 1) * tile_cols * 4 <= LDS else {LARGE}
    if stage == PROJECT_BWD:
        return {ANY} if not four else {LONG} if w > 64 else {TILE}
    if stage == TERMS:
        return {LONG} if w > 64 else {ANY} if not four else {TILE}
    if stage == HEAD:
        return {ANY} if not four else {TILE}
    if not four or w > 64:
        return {NONE}
    if n <= 127 and w <= 32 and k <= 63 and d in (64, 128) and not wide:
        return {DENSE}
    if lib.gdn_tile_fits(n, w, d, k) == 0:
        return {NONE}
    return {NONE, TILE} if series else {TILE}      # (SERIES: only with the projection on the matrix cores)


def test_abi_has_the_query():
    header = open(os.path.join(ROOT, "include", "gdn_hip.h")).read()
    assert "#define GDN_ABI_VERSION 23" in header and _lib.ABI_VERSION == 23 and _lib.load().gdn_abi_version() == 23
    for i, name in enumerate(("NONE", "DENSE", "TILE", "LARGE", "LONG", "ANY")):
        assert f"#define GDN_FAMILY_{name} {i}" in header and getattr(_lib, "FAMILY_" + name) == i
    for i, name in enumerate(("PROJECT", "AGGREGATE", "ATTN_BWD", "PROJECT_BWD", "TERMS", "HEAD", "FUSED")):
        assert f"#define GDN_STAGE_{name} {i}" in header and getattr(_lib, "STAGE_" + name) == i
    assert (_lib.ROUTE_WIDE, _lib.ROUTE_BF16, _lib.ROUTE_SERIES) == (WIDE, BF16, SERIES)


@pytest.mark.parametrize("flags", [0, WIDE, BF16, SERIES], ids=["plain", "wide", "bf16", "series"])
def test_kernel_family_is_the_headers_table(flags):
    lib = _lib.load()
    for n, w, d, k in SHAPES:
        for stage in range(7):
            got = fam(stage, n, w, d, k, flags)
            assert got in expected(stage, n, w, d, k, flags, lib), (stage, n, w, d, k, flags, got)


def test_outside_the_supported_shapes_is_none():
    for stage in range(7):
        for n, w, d, k in ((0, 8, 64, 1), (4097, 8, 64, 1), (20, 8, 0, 1), (20, 8, 257, 1)):
            assert fam(stage, n, w, d, k) == NONE, (stage, n, w, d, k)
    for n, w, d, k in ((20, 0, 64, 5), (20, 1025, 64, 5)):
        assert fam(PROJECT, n, w, d, k) == fam(PROJECT_BWD, n, w, d, k) == fam(TERMS, n, w, d, k) == NONE
        assert fam(AGGREGATE, n, w, d, k) == DENSE          # (does not depend on w)
    for n, w, d, k in ((20, 8, 64, 0), (20, 8, 64, 21), (4096, 8, 64, 1024)):
        assert fam(AGGREGATE, n, w, d, k) == fam(ATTN_BWD, n, w, d, k) == fam(FUSED, n, w, d, k) == NONE
        assert fam(PROJECT, n, w, d, k) != NONE             # (does not depend on k)


def test_host_queries_are_reads_of_the_route():
    lib = _lib.load()
    for n, w, d, k in SHAPES:
        assert lib.gdn_tile_fits(n, w, d, k) == (fam(FUSED, n, w, d, k, WIDE) == TILE), (n, w, d, k)
        tile_step = all(fam(s, n, w, d, k, WIDE) == TILE for s in (PROJECT, AGGREGATE, ATTN_BWD, PROJECT_BWD))
        assert lib.gdn_train_supported(n, w, d, k) == tile_step, (n, w, d, k)
        assert lib.gdn_attn_aggregate_bwd_uses_reverse(n, d, k) == (fam(ATTN_BWD, n, w, d, k) != DENSE), (n, d, k)
        assert (lib.gdn_project_bwd_workspace_bytes(n, w, d) > 0) == (fam(PROJECT_BWD, n, w, d, k) != NONE)


def test_backward_workspace_holds_the_table_exactly_beyond_lds():
    """[ticket + 1024 rows of d_bias] and, unless the TILE backward keeps its tables in LDS, d_pi[batch*n, pitch]."""
    lib, batch = _lib.load(), 3
    forms = set()
    for n, w, d, k in SHAPES:
        family, form = fam(ATTN_BWD, n, w, d, k, WIDE), bwd_form(n, d, k, WIDE)
        in_lds = family == TILE and form == TABLES_LDS
        want = 4 * (4 + 1024 * d + (0 if in_lds else batch * n * ops.nbr_pitch(k)))
        assert lib.gdn_attn_aggregate_bwd_workspace_bytes(batch, n, d, k) == want, (n, d, k, family, form)
        assert form == bwd_form(n, d, k, 0) or fam(ATTN_BWD, n, w, d, k) == DENSE       # one layout, `_wide` or not
        forms.add((family, form))
    assert {(TILE, 0), (TILE, 1), (TILE, 2), (LARGE, 0), (ANY, 0)} <= forms            # every layout is in the grid


def test_nbr_ordered_is_built_exactly_where_the_aggregate_routes_dense(monkeypatch):
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append(name))
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    for n, k in sorted({(n, k) for n, _, _, k in SHAPES}):
        nbr = torch.zeros((n, ops.nbr_pitch(k)), dtype=torch.int16)
        graph = ops.SensorGraph(torch.zeros((n, k), dtype=torch.int64), nbr, torch.zeros((n,), dtype=torch.int32))
        del calls[:]
        got = graph.nbr_ordered()
        dense = fam(AGGREGATE, n, 1, 64, k) == DENSE
        assert dense == (n <= 127 and k <= 63)
        assert calls == (["gdn_graph_bank_order"] if dense else []) and (got is not nbr) == dense, (n, k)
        assert graph.nbr_ordered() is got and len(calls) == int(dense)                 # once per graph


def test_valu_override_leaves_no_dense_cell():
    """GDN_FUSED_PATH=valu (read once per process: a child): no stage routes to the matrix-core kernels, and
    ops.fused_plan / SensorGraph.nbr_ordered, which ask the route, follow.  bf16 storage of the staged stages exists
    on the matrix cores only and is not part of the A/B."""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r + '/tools');"
            "import route_grid; from gdn_amd import _lib; lib = _lib.load();"
            "bad = [(s, f) + sh for sh in route_grid.shapes() for s in range(7) for f in (0, 1, 4, 6)"
            " if not (f == 6 and s != 6) and lib.gdn_kernel_family(s, *sh, f) & 0xff == 1];"
            "rev = [sh for sh in route_grid.shapes() if not lib.gdn_attn_aggregate_bwd_uses_reverse(sh[0], sh[2], sh[3])];"
            "print(len(bad), len(rev), lib.gdn_kernel_family(1, 20, 1, 64, 6, 0) & 0xff)")
    out = subprocess.run([sys.executable, "-c", code % (ROOT, ROOT)], check=True, capture_output=True, text=True,
                         env=dict(os.environ, GDN_FUSED_PATH="valu")).stdout.split()
    assert out == ["0", "0", str(TILE)], out
    assert fam(AGGREGATE, 20, 1, 64, 6) == DENSE            # (this process: no override)
