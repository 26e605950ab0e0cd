"""CPU suite of the localisation entry points (gdn_score_smooth_topm, gdn_attention_mean, gdn_attention_at): the C-ABI
surface and the host-side refusals (decided before any launch, so no device is needed), and the float64 yardstick
of the GPU tests (tests/_localise_ref.py) pinned to the oracle."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _localise_ref as ref
from conftest import ROOT, SCORE_CASES, load_golden, meta

GDN_ERR_ARG, GDN_ERR_UNSUPPORTED = -1, -3
FAKE = 4096          # a non-null, 16-byte aligned address that is never dereferenced on the host
NEW = ["gdn_score_smooth_topm", "gdn_attention_workspace_bytes", "gdn_attention_mean", "gdn_attention_at"]


def test_header_signatures_and_exports_agree_and_the_abi_stays():
    from gdn_amd import _lib
    header = open(os.path.join(ROOT, "include", "gdn_hip.h")).read()
    declared = dict((name, ret) for ret, name in re.findall(r"^(int|long long)\s+(gdn_\w+)\s*\(", header, flags=re.M))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES
        fn = getattr(lib, name)                      # AttributeError: the symbol is missing
        assert fn.argtypes == _lib.SIGNATURES[name]
        assert fn.restype is (ctypes.c_longlong if declared[name] == "long long" else ctypes.c_int)
    assert declared["gdn_attention_workspace_bytes"] == "long long"
    assert [declared[n] for n in NEW if n != "gdn_attention_workspace_bytes"] == ["int"] * 3
    assert "#define GDN_ABI_VERSION 23" in header and _lib.ABI_VERSION == 23 and lib.gdn_abi_version() == 23
    p, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert _lib.SIGNATURES["gdn_score_smooth_topm"] == [p, p, p, i, i, i, p, p, i, p, p, p]
    assert _lib.SIGNATURES["gdn_attention_mean"] == [p, ll, ll, p, p, p, p, i, i, i, i, p, p, p]
    assert _lib.SIGNATURES["gdn_attention_at"] == [p, ll, p, p, i, p, p, p, i, i, i, p, p]
    from gdn_amd import GDN, harness, ops
    assert all(callable(getattr(ops, f)) for f in ("score_smooth_topm", "attention_mean", "attention_at"))
    assert all(callable(getattr(GDN, f)) for f in ("attention_series", "attention_windows", "attention_at"))
    assert callable(harness.localise)


def _topm(m, n, t=100, **kw):
    from gdn_amd import _lib
    args = dict(pred=FAKE, gt=FAKE, med=FAKE, scores=FAKE, sensors=FAKE)
    args.update(kw)
    return _lib.load().gdn_score_smooth_topm(args["pred"], args["gt"], args["med"], t, n, 0, None, None, m,
                                             args["scores"], args["sensors"], None)


@pytest.mark.parametrize("m,n", [(0, 27), (9, 27), (4, 3), (-1, 27)])
def test_topm_refuses_m_outside_one_to_eight_and_beyond_n(m, n):
    assert _topm(m, n) == GDN_ERR_UNSUPPORTED


def test_topm_argument_errors():
    from gdn_amd import _lib
    for null in ("pred", "gt", "med", "scores", "sensors"):
        assert _topm(3, 27, **{null: None}) == GDN_ERR_ARG
    assert _topm(3, 27, t=0) == GDN_ERR_ARG
    # first_tick > 0 needs the halo
    assert _lib.load().gdn_score_smooth_topm(FAKE, FAKE, FAKE, 10, 27, 5, None, None, 3, FAKE, FAKE, None) == GDN_ERR_ARG


def _mean(n=127, w=15, k=30, batch=64, t_raw=1000, first=0):
    from gdn_amd import _lib
    return _lib.load().gdn_attention_mean(FAKE, t_raw, first, None, FAKE, FAKE, FAKE, batch, n, w, k, FAKE, FAKE, None)


def _at(n=127, w=15, k=30, q=4, t_raw=1000):
    from gdn_amd import _lib
    return _lib.load().gdn_attention_at(FAKE, t_raw, FAKE, FAKE, q, FAKE, FAKE, FAKE, n, w, k, FAKE, None)


@pytest.mark.parametrize("shape", [dict(n=4097), dict(w=1025), dict(w=0), dict(n=2000, k=1024), dict(n=20, k=21),
                                   dict(k=0)],
                         ids=["n4097", "w1025", "w0", "k1024", "k_gt_n", "k0"])
def test_attention_refuses_shapes_outside_the_envelope(shape):
    from gdn_amd import _lib
    assert _mean(**shape) == GDN_ERR_UNSUPPORTED
    assert _at(**shape) == GDN_ERR_UNSUPPORTED
    full = dict(n=127, w=15, k=30)
    full.update(shape)
    assert _lib.load().gdn_attention_workspace_bytes(64, full["n"], full["w"], full["k"]) == 0
    with pytest.raises(_lib.GdnHipError, match="GDN_ERR_UNSUPPORTED"):
        _lib.call("gdn_attention_at", FAKE, 1000, FAKE, FAKE, 4, FAKE, FAKE, FAKE, full["n"], full["w"], full["k"],
                  FAKE, None)


def test_attention_mean_refuses_windows_that_do_not_fit():
    assert _mean(t_raw=0, first=3) == GDN_ERR_ARG                       # windows addressing has no `first`
    assert _mean(t_raw=1000, first=1000 - 64 - 15 + 2, batch=64, w=15) == GDN_ERR_ARG     # last window one past the end
    assert _mean(t_raw=1000, first=-1) == GDN_ERR_ARG
    assert _mean(batch=0) == GDN_ERR_ARG


def test_attention_workspace_is_bounded_and_covers_the_partials():
    from gdn_amd import _lib
    lib = _lib.load()
    assert lib.gdn_nbr_pitch(30) == 32
    one = 127 * 32 * 8
    assert lib.gdn_attention_workspace_bytes(1, 127, 15, 30) == one
    big = lib.gdn_attention_workspace_bytes(32768, 127, 15, 30)
    assert big % one == 0 and one < big <= 64 << 20
    # 4096 sensors at the widest list: one block is 32 MB, the workspace stays at a few blocks
    assert lib.gdn_attention_workspace_bytes(32768, 4096, 15, 1023) <= 64 << 20


def test_python_entry_points_refuse_cpu_and_training_by_name():
    from gdn_amd import GDN, _lib
    model = GDN([torch.zeros((2, 1), dtype=torch.long)], 9, dim=16, input_dim=5, topk=3)
    with pytest.raises(RuntimeError, match="eval"):
        model.train().attention_series(torch.zeros((9, 40)), 0, 4)
    from gdn_amd import ops
    with pytest.raises(_lib.GdnHipError, match="HIP device"):
        ops._attention_source(torch.zeros((9, 40)), "series")


# ------------------------------------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("case", SCORE_CASES + ["perf_T1000_N27", "perf_T777_N5_ties"])
def test_score_helper_equals_the_score_oracle(case):
    from oracle import score_oracle
    data, _ = load_golden(case)
    want = score_oracle.full_err_scores(data["pred"], data["gt"])
    np.testing.assert_allclose(ref.scores_f64(data["pred"], data["gt"]), want, rtol=1e-13, atol=1e-14)
    np.testing.assert_allclose(want, data["scores"], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("m", [1, 3, 8])
def test_topm_helper_orders_by_score_then_sensor(m):
    data, _ = load_golden("score_T1000_N27")
    s = data["scores"]
    vals, idx = ref.topm(s, m)
    np.testing.assert_array_equal(vals[:, 0], s.max(axis=0))
    np.testing.assert_array_equal(idx[:3], np.tile(np.arange(m), (3, 1)))        # all-zero ticks: sensors 0 .. m-1
    assert (np.diff(vals, axis=1) <= 0).all()
    tie = np.diff(vals, axis=1) == 0
    assert (np.diff(idx, axis=1)[tie] > 0).all()
    np.testing.assert_array_equal(np.sort(vals, axis=1)[:, ::-1], np.sort(s, axis=0)[::-1][:m].T)
    tied = np.array([[1.0, 1.0, 0.5, 1.0], [2.0, 2.0, 2.0, 2.0]]).T                # [4 sensors, 2 ticks]
    np.testing.assert_array_equal(ref.topm(tied, 3)[1], [[0, 1, 3], [0, 1, 2]])


@pytest.mark.parametrize("t,n", [(32768, 127), (1000, 27), (2048, 4096)])
@pytest.mark.parametrize("m", [1, 3, 8])
def test_seeded_inputs_keep_the_oracle_within_the_skip_cap(t, n, m):
    pred, gt = ref.seeded_scores(t, n, seed=t + n)
    skip = ref.skippable_ticks(ref.scores_f64(pred, gt), m)
    assert ref.skipped_share(skip) <= ref.SKIP_CAP


@pytest.mark.parametrize("case", SCORE_CASES)
@pytest.mark.parametrize("m", [1, 3])
def test_score_fixtures_keep_the_oracle_within_the_skip_cap(case, m):
    data, _ = load_golden(case)
    m = min(m, data["scores"].shape[0])
    assert ref.skipped_share(ref.skippable_ticks(data["scores"], m)) <= ref.SKIP_CAP


@pytest.mark.parametrize("case", ["swat127_w15_k30", "msl_demo_w5_k5", "dupemb_n10_k3"])
def test_attention_helper_equals_the_oracle_in_float64(case):
    from oracle import gdn_oracle
    data, p = load_golden(case)
    m = meta(data)
    p64 = {key: (v.double() if v.is_floating_point() else v) for key, v in p.items()}
    x = torch.from_numpy(data["x"])
    graph = torch.from_numpy(data["learned_graph"])
    r = gdn_oracle.forward(p64, x.double(), m["k"], m["out_layer_num"], graph=graph)
    alpha, nb = ref.attention_rows(p, x, graph)
    _, deg = ref.neighbours(graph)
    np.testing.assert_allclose(ref.edge_order(alpha, deg), r["att_weight_1"].numpy().reshape(-1), atol=1e-10, rtol=0)
    np.testing.assert_allclose(ref.edge_order(alpha, deg), data["att_weight_1"].reshape(-1), atol=2e-6, rtol=1e-5)
    # the slot order is the reference's edge order: sources of window 0's non-self edges, target by target
    ei = r["edge_index_1"].numpy()
    e_nonself = int((deg - 1).sum())
    np.testing.assert_array_equal(np.concatenate([nb[i, :deg[i] - 1] for i in range(m["n"])]), ei[0, :e_nonself])
    np.testing.assert_array_equal(nb[np.arange(m["n"]), deg - 1], np.arange(m["n"]))
    np.testing.assert_allclose(alpha.sum(axis=-1), 1.0, atol=1e-12)
    wt = np.arange(m["b"], dtype=np.float64)
    np.testing.assert_allclose(ref.attention_mean(alpha, wt), (alpha * wt[:, None, None]).sum(0) / wt.sum(), atol=1e-15)
    assert not ref.attention_mean(alpha, np.zeros(m["b"])).any()
