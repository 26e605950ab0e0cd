"""CPU suite: the C-ABI surface of windows longer than 64 ticks (host-only calls, no launch)."""
import os
import re

from conftest import ROOT


def test_terms_pitch_declared_and_exported():
    from gdn_amd import _lib
    header = open(os.path.join(ROOT, "include", "gdn_hip.h")).read()
    assert re.search(r"\bint gdn_terms_pitch\(", header)
    assert "gdn_terms_pitch" in _lib.SIGNATURES
    assert hasattr(_lib.load(), "gdn_terms_pitch")
    assert "#define GDN_ABI_VERSION 23" in header and _lib.ABI_VERSION == 23
    assert "1 <= w <= 1024" in header


def test_terms_pitch_is_64_then_rounded_up_and_capped_at_1024():
    from gdn_amd import _lib
    lib = _lib.load()
    for w in (1, 5, 15, 32, 63, 64):
        assert lib.gdn_terms_pitch(w) == 64, w
    for w, p in [(65, 128), (100, 128), (128, 128), (129, 192), (256, 256), (1000, 1024), (1024, 1024)]:
        assert lib.gdn_terms_pitch(w) == p, w
    for w in (0, -3, 1025, 4096):
        assert lib.gdn_terms_pitch(w) == 0, w


def test_long_windows_stay_off_the_tile_the_plans_and_the_native_step():
    from gdn_amd import _lib
    lib = _lib.load()
    for n, w, d, k in [(27, 65, 64, 5), (127, 100, 64, 30), (127, 256, 128, 30), (51, 1024, 16, 5),
                       (700, 100, 64, 30)]:
        assert lib.gdn_tile_fits(n, w, d, k) == 0, (n, w, d, k)
        assert lib.gdn_train_supported(n, w, d, k) == 0, (n, w, d, k)
        assert lib.gdn_fused_plan_bytes(n, w, d, k, 0) == 0, (n, w, d, k)
    # w <= 64 keeps its answers
    assert lib.gdn_tile_fits(127, 64, 64, 30) == 1
    assert lib.gdn_tile_fits(127, 15, 64, 30) == 1


def test_projection_backward_workspace_covers_long_windows():
    from gdn_amd import _lib
    lib = _lib.load()
    for n, w, d in [(127, 100, 64), (700, 100, 64), (51, 1024, 16), (127, 256, 128)]:
        assert lib.gdn_project_bwd_workspace_bytes(n, w, d) >= (d + 2) * w * 4, (n, w, d)
    assert lib.gdn_project_bwd_workspace_bytes(127, 1025, 64) == 0


def test_node_terms_size_follows_the_pitch():
    import pytest
    from gdn_amd import ops
    assert ops.terms_pitch(15) == 64 and ops.terms_pitch(100) == 128
    with pytest.raises(ops._lib.GdnHipError, match="1025"):
        ops.terms_pitch(1025)
