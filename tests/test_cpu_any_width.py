"""CPU suite: the C-ABI surface of embedding widths other than 16, 32, 64 and 128 (host-only calls, no launch)."""
import os

import pytest

from conftest import ROOT

NEW = [(127, 15, 48, 30), (27, 5, 3, 5), (51, 10, 50, 5), (127, 15, 256, 30), (700, 30, 96, 30),
       (127, 100, 72, 30), (40, 8, 24, 6)]      # (n, w, d, k)


def test_header_documents_any_width_and_the_abi_stays():
    from gdn_amd import _lib
    header = open(os.path.join(ROOT, "include", "gdn_hip.h")).read()
    assert "1 <= d <= 256" in header
    assert "#define GDN_ABI_VERSION 23" in header and _lib.ABI_VERSION == 23


def test_new_widths_stay_off_the_tile_the_plans_and_the_native_step():
    from gdn_amd import _lib
    lib = _lib.load()
    for n, w, d, k in NEW:
        assert lib.gdn_tile_fits(n, w, d, k) == 0, (n, w, d, k)
        assert lib.gdn_train_supported(n, w, d, k) == 0, (n, w, d, k)
        assert lib.gdn_fused_plan_bytes(n, w, d, k, 0) == 0, (n, w, d, k)
        assert lib.gdn_fused_plan_bytes(n, w, d, k, 1) == 0, (n, w, d, k)
    # the four tile widths keep their answers
    assert lib.gdn_tile_fits(127, 15, 64, 30) == 1
    assert lib.gdn_tile_fits(127, 15, 32, 30) == 1


def test_workspace_queries_cover_new_widths():
    from gdn_amd import _lib
    lib = _lib.load()
    for n, w, d, k in NEW:
        # one partial [d + 2, w] block per row range
        assert lib.gdn_project_bwd_workspace_bytes(n, w, d) >= (d + 2) * w * 4, (n, w, d)
        # ticket + d_bias rows + the [B*n, pitch] d_pi table
        need = (1024 * d + 2 * n * lib.gdn_nbr_pitch(k)) * 4
        assert lib.gdn_attn_aggregate_bwd_workspace_bytes(2, n, d, k) >= need, (n, d, k)
        assert lib.gdn_head_train_stats_bytes(d) > 0 and lib.gdn_head_train_workspace_bytes(n, d) > 0
    assert lib.gdn_project_bwd_workspace_bytes(127, 1025, 48) == 0


def test_python_width_check_names_the_width():
    from gdn_amd import _lib, ops
    for d in (1, 3, 48, 50, 96, 256):
        assert ops.check_width(d) == d
    with pytest.raises(_lib.GdnHipError, match="257"):
        ops.check_width(257)
    with pytest.raises(_lib.GdnHipError, match="embedding width 0"):
        ops.check_width(0)


def test_cpu_model_constructs_at_any_width():
    import torch
    from gdn_amd import GDN
    for d in (3, 50, 257, 300):
        model = GDN([torch.zeros((2, 1), dtype=torch.long)], 9, dim=d, input_dim=5, topk=3)
        assert model.embedding.weight.shape == (9, d)
