"""CPU suite: the C-ABI surface of gdn_head_mlp_fwd, the eval head folded into the OutLayer MLP's first operand
(host-only calls: every refusal below is decided before any launch, so no device is needed)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

GDN_ERR_ARG, GDN_ERR_UNSUPPORTED = -1, -3
FAKE = 4096          # a non-null, 16-byte aligned address that is never dereferenced on the host


def test_header_declares_the_entry_point_and_the_abi_stays():
    from gdn_amd import _lib
    header = open(os.path.join(ROOT, "include", "gdn_hip.h")).read()
    assert re.search(r"\bint gdn_head_mlp_fwd\(const float\* z, const float\* emb,", header)
    assert "#define GDN_ABI_VERSION 23" in header and _lib.ABI_VERSION == 23


def test_library_exports_and_binding():
    from gdn_amd import _lib, ops
    lib = _lib.load()
    assert lib.gdn_abi_version() == 23
    fn = lib.gdn_head_mlp_fwd                    # AttributeError: the symbol is missing
    # z, emb, bn1, bn2, plan | batch, n, d, hidden, layers | out, stream
    assert _lib.SIGNATURES["gdn_head_mlp_fwd"] == [ctypes.c_void_p] * 5 + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 2
    assert fn.argtypes == _lib.SIGNATURES["gdn_head_mlp_fwd"] and fn.restype is ctypes.c_int
    assert callable(ops.head_mlp_fwd)


@pytest.mark.parametrize("null", [0, 1, 2, 3, 4, 10], ids=["z", "emb", "bn1", "bn2", "plan", "out"])
def test_null_pointer_is_an_argument_error(null):
    from gdn_amd import _lib
    args = [FAKE] * 5 + [2, 27, 64, 256, 2] + [FAKE, None]
    args[null] = None
    assert _lib.load().gdn_head_mlp_fwd(*args) == GDN_ERR_ARG


@pytest.mark.parametrize("batch,n", [(0, 27), (-1, 27), (2, 0)])
def test_non_positive_sizes_are_argument_errors(batch, n):
    from gdn_amd import _lib
    assert _lib.load().gdn_head_mlp_fwd(*([FAKE] * 5), batch, n, 64, 256, 2, FAKE, None) == GDN_ERR_ARG


@pytest.mark.parametrize("d,hidden,layers", [(48, 256, 2), (64, 300, 2), (64, 256, 1)])
def test_configurations_outside_the_plan_are_unsupported(d, hidden, layers):
    """The supported set is gdn_mlp_fwd's: gdn_mlp_plan_bytes(d, hidden, layers) != 0."""
    from gdn_amd import _lib
    lib = _lib.load()
    assert lib.gdn_mlp_plan_bytes(d, hidden, layers) == 0
    assert lib.gdn_head_mlp_fwd(*([FAKE] * 5), 2, 27, d, hidden, layers, FAKE, None) == GDN_ERR_UNSUPPORTED
    with pytest.raises(_lib.GdnHipError, match="GDN_ERR_UNSUPPORTED"):
        _lib.call("gdn_head_mlp_fwd", *([FAKE] * 5), 2, 27, d, hidden, layers, FAKE, None)


def test_misaligned_rows_are_refused_before_any_launch():
    from gdn_amd import _lib
    lib = _lib.load()
    assert lib.gdn_mlp_plan_bytes(64, 256, 2) > 0
    assert lib.gdn_head_mlp_fwd(FAKE + 4, *([FAKE] * 4), 2, 27, 64, 256, 2, FAKE, None) == GDN_ERR_ARG
    assert lib.gdn_head_mlp_fwd(FAKE, FAKE + 8, *([FAKE] * 3), 2, 27, 64, 256, 2, FAKE, None) == GDN_ERR_ARG


def test_training_mode_keeps_its_runtime_error():
    import torch
    from gdn_amd import GDN
    model = GDN([torch.zeros((2, 1), dtype=torch.long)], 9, dim=16, input_dim=5, topk=3, out_layer_num=2,
                out_layer_inter_dim=24).train()
    with pytest.raises(RuntimeError):
        model.forward_into(torch.zeros((1, 9, 5)), torch.zeros((1, 9)))
    with pytest.raises(RuntimeError):
        model.forward_series(torch.zeros((9, 20)), 0, 4)
    assert model.mlp_fast_path_supported() is False
