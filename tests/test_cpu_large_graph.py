"""CPU suite: the C-ABI surface of graphs beyond the LDS tile (host-only calls, no launch)."""
import os
import re

from conftest import ROOT


def test_large_graph_symbols_declared_and_exported():
    from gdn_amd import _lib
    header = open(os.path.join(ROOT, "include", "gdn_hip.h")).read()
    for name in ("gdn_project_fwd_series", "gdn_tile_fits"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    assert "#define GDN_ABI_VERSION 23" in header and _lib.ABI_VERSION == 23


def test_tile_predicate_follows_the_lds_budget():
    from gdn_amd import _lib
    lib = _lib.load()
    # inside the tile: the fused forward's shapes of the suite and of BASELINE
    for n, w, d, k in [(127, 15, 64, 30), (512, 30, 64, 64), (512, 30, 128, 64), (600, 15, 64, 30),
                       (1100, 5, 32, 16), (2100, 10, 16, 20), (51, 5, 16, 5)]:
        assert lib.gdn_tile_fits(n, w, d, k) == 1, (n, w, d, k)
    # beyond it, up to the 4096-sensor cap
    for n, w, d, k in [(700, 15, 64, 30), (1024, 30, 128, 64), (2500, 10, 16, 20), (4096, 5, 32, 16),
                       (4096, 64, 128, 1023)]:
        assert lib.gdn_tile_fits(n, w, d, k) == 0, (n, w, d, k)
        assert lib.gdn_train_supported(n, w, d, k) == 0, (n, w, d, k)
    # the boundary is monotone in n
    fits = [lib.gdn_tile_fits(n, 15, 64, 30) for n in range(400, 800)]
    assert fits == sorted(fits, reverse=True) and 0 in fits and 1 in fits
    # invalid arguments
    assert lib.gdn_tile_fits(0, 15, 64, 30) == 0 and lib.gdn_tile_fits(127, 15, 48, 30) == 0
    assert lib.gdn_tile_fits(5000, 15, 16, 30) == 0


def test_backward_workspace_covers_the_large_form():
    from gdn_amd import _lib
    lib = _lib.load()
    for b, n, d, k in [(2, 700, 64, 30), (3, 4096, 32, 16), (2, 1024, 128, 64)]:
        pitch = lib.gdn_nbr_pitch(k)
        need = (4 + 1024 * d + b * n * pitch) * 4      # d_bias ticket + rows, then the [B*n, pitch] d_pi table
        assert lib.gdn_attn_aggregate_bwd_workspace_bytes(b, n, d, k) >= need
