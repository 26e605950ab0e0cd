"""CPU suite of the streaming fleet (gdn_fleet_* entry points, harness.StreamFleet): the C-ABI surface and the host-side
refusals, all decided before any launch, so no device is needed."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

GDN_ERR_ARG, GDN_ERR_UNSUPPORTED = -1, -3
FAKE = 4096          # a non-null, 16-byte aligned address that is never dereferenced on the host
NEW = ["gdn_fleet_state_bytes", "gdn_fleet_init", "gdn_fleet_windows", "gdn_fleet_score", "gdn_fleet_advance"]


def _lib():
    from gdn_amd import _lib as binding
    return binding.load()


def test_header_signatures_and_exports_agree_and_the_abi_stays():
    from gdn_amd import _lib as binding
    header = open(os.path.join(ROOT, "include", "gdn_hip.h")).read()
    declared = dict((name, ret) for ret, name in re.findall(r"^(int|long long)\s+(gdn_\w+)\s*\(", header, flags=re.M))
    lib = binding.load()
    for name in NEW:
        assert name in declared and name in binding.SIGNATURES
        fn = getattr(lib, name)                      # AttributeError: the symbol is missing
        assert fn.argtypes == binding.SIGNATURES[name]
        assert fn.restype is (ctypes.c_longlong if declared[name] == "long long" else ctypes.c_int)
        params = re.search(name + r"\s*\(([^)]*)\)\s*;", header).group(1)
        assert len(params.split(",")) == len(binding.SIGNATURES[name]), name
    assert declared["gdn_fleet_state_bytes"] == "long long"
    assert [declared[n] for n in NEW[1:]] == ["int"] * 4
    assert "#define GDN_ABI_VERSION 23" in header and binding.ABI_VERSION == 23 and lib.gdn_abi_version() == 23
    p, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert binding.SIGNATURES["gdn_fleet_state_bytes"] == [i, i, i]
    assert binding.SIGNATURES["gdn_fleet_init"] == [p, p, ll, i, i, i, p]
    assert binding.SIGNATURES["gdn_fleet_windows"] == [p, p, p, i, i, i, i, p, p]
    assert binding.SIGNATURES["gdn_fleet_score"] == [p, p, p, p, p, p, i, i, i, i, i, p, p, p, p]
    assert binding.SIGNATURES["gdn_fleet_advance"] == [p, p, p, p, p, p, p, i, i, i, i, i, p, p, ll, p]
    from gdn_amd import harness, ops
    assert all(callable(getattr(ops, f)) for f in ("fleet_state", "fleet_state_views", "fleet_windows", "fleet_score",
                                                   "fleet_advance"))
    assert callable(harness.StreamFleet) and callable(harness.StreamFleet.from_calibration)


def test_fleet_state_bytes_are_units_times_a_stream_state():
    lib = _lib()
    for units, n, w in [(1, 1, 1), (3, 5, 4), (16, 127, 15), (256, 127, 15), (7, 130, 65), (2, 4096, 1024), (4096, 3, 1)]:
        assert lib.gdn_fleet_state_bytes(units, n, w) == units * lib.gdn_stream_state_bytes(n, w) > 0
    for units, n, w in [(0, 127, 15), (-1, 127, 15), (3, 4097, 15), (3, 127, 1025), (3, 0, 15), (3, 127, 0)]:
        assert lib.gdn_fleet_state_bytes(units, n, w) <= 0


def _init(h=20, units=3, n=127, w=15, state=FAKE, history=FAKE):
    return _lib().gdn_fleet_init(state, history, h, units, n, w, None)


def _windows(units=3, c=16, n=127, w=15, state=FAKE, chunk=FAKE, counts=FAKE, x=FAKE):
    return _lib().gdn_fleet_windows(state, chunk, counts, units, c, n, w, x, None)


def _score(units=3, c=16, n=127, w=15, m=3, **kw):
    a = dict(state=FAKE, pred=FAKE, chunk=FAKE, med=FAKE, thr=FAKE, counts=FAKE, scores=FAKE, sensors=FAKE, alarm=FAKE)
    a.update(kw)
    return _lib().gdn_fleet_score(a["state"], a["pred"], a["chunk"], a["med"], a["thr"], a["counts"], units, c, n, w, m,
                                  a["scores"], a["sensors"], a["alarm"], None)


def _advance(units=3, c=16, n=127, w=15, m=3, log_len=8, **kw):
    a = dict(state=FAKE, chunk=FAKE, pred=FAKE, med=FAKE, alarm=FAKE, sensors=FAKE, counts=FAKE, log_ticks=FAKE,
             log_sensors=FAKE)
    a.update(kw)
    return _lib().gdn_fleet_advance(a["state"], a["chunk"], a["pred"], a["med"], a["alarm"], a["sensors"], a["counts"],
                                    units, c, n, w, m, a["log_ticks"], a["log_sensors"], log_len, None)


def test_every_null_pointer_is_an_argument_error():
    assert _init(state=None) == GDN_ERR_ARG and _init(history=None) == GDN_ERR_ARG
    assert _init(h=14, w=15) == GDN_ERR_ARG                 # a cold start
    for null in ("state", "chunk", "counts", "x"):
        assert _windows(**{null: None}) == GDN_ERR_ARG, null
    for null in ("state", "pred", "chunk", "med", "thr", "counts", "scores", "sensors", "alarm"):
        assert _score(**{null: None}) == GDN_ERR_ARG, null
    for null in ("state", "chunk", "pred", "med", "alarm", "sensors", "counts"):
        assert _advance(**{null: None}) == GDN_ERR_ARG, null
    assert _advance(log_ticks=None) == GDN_ERR_ARG and _advance(log_sensors=None) == GDN_ERR_ARG
    assert _advance(log_len=-1) == GDN_ERR_ARG
    # L = 0 needs neither table (checked: it passes on to the shape refusals)
    assert _advance(log_len=0, log_ticks=None, log_sensors=None, n=4097) == GDN_ERR_UNSUPPORTED


@pytest.mark.parametrize("shape", [dict(units=4097, c=1), dict(units=1, c=4097), dict(units=17, c=241), dict(units=0),
                                   dict(c=0), dict(n=4097), dict(n=0), dict(w=0), dict(w=1025)],
                         ids=["u4097", "c4097", "17x241", "u0", "c0", "n4097", "n0", "w0", "w1025"])
def test_shapes_outside_the_limits_are_refused_without_a_device(shape):
    assert _windows(**shape) == GDN_ERR_UNSUPPORTED
    assert _score(**shape) == GDN_ERR_UNSUPPORTED
    assert _advance(**shape) == GDN_ERR_UNSUPPORTED
    if "c" not in shape:
        assert _init(h=2000, **shape) == GDN_ERR_UNSUPPORTED
    from gdn_amd import _lib as binding
    full = dict(units=3, c=16, n=127, w=15)
    full.update(shape)
    with pytest.raises(binding.GdnHipError, match="GDN_ERR_UNSUPPORTED"):
        binding.call("gdn_fleet_windows", FAKE, FAKE, FAKE, full["units"], full["c"], full["n"], full["w"], FAKE, None)


@pytest.mark.parametrize("m,n", [(0, 27), (9, 27), (4, 3), (-1, 27)], ids=["m0", "m9", "m_gt_n", "m_neg"])
def test_score_and_advance_refuse_m_outside_one_to_eight_and_beyond_n(m, n):
    assert _score(m=m, n=n) == GDN_ERR_UNSUPPORTED
    assert _advance(m=m, n=n) == GDN_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------- StreamFleet, host side
def _cpu_model(n=9, w=5, **kw):
    from gdn_amd import GDN
    return GDN([torch.zeros((2, 1), dtype=torch.long)], n, dim=16, input_dim=w, topk=3, **kw)


def _fleet(model, units=3, n=9, w=5, **kw):
    from gdn_amd import harness
    args = dict(med_iqr=torch.zeros((units, n, 2), dtype=torch.float64), threshold=1.0,
                history=torch.zeros((units, n, w)), chunk=4)
    args.update(kw)
    return harness.StreamFleet(model, args.pop("med_iqr"), args.pop("threshold"), args.pop("history"),
                               args.pop("chunk"), **args)


@pytest.mark.parametrize("units,chunk", [(3, 0), (3, -2), (3, 1366), (1, 4097), (4097, 1)])
def test_fleet_refuses_units_times_chunk_outside_one_to_4096(units, chunk):
    from gdn_amd import harness
    with pytest.raises(ValueError, match="units \\* chunk"):
        _fleet(_cpu_model(), units=units, chunk=chunk)
    with pytest.raises(ValueError, match="units \\* chunk"):
        harness.fleet_check_shape(units, chunk, 9, 5)
    harness.fleet_check_shape(3, 1365, 9, 5)                # 4095 windows: fine
    with pytest.raises(ValueError, match="at least one unit"):
        harness.fleet_check_shape(0, 4, 9, 5)


def test_fleet_refuses_a_window_buffer_beyond_256_mb():
    from gdn_amd import harness
    n, w = 4096, 64                                          # 1 MB of windows per tick: 256 fit, 3 * 86 = 258 do not
    harness.fleet_check_shape(4, 64, n, w)
    with pytest.raises(ValueError, match="256 MB"):
        harness.fleet_check_shape(3, 86, n, w)
    with pytest.raises(ValueError, match="256 MB"):
        _fleet(_cpu_model(n=n, w=w), n=n, w=w, chunk=86)


def test_fleet_refuses_wrong_shapes_top_m_and_log_by_name():
    model = _cpu_model()
    with pytest.raises(ValueError, match="history"):
        _fleet(model, history=torch.zeros((9, 5)))                        # a single stream's history
    with pytest.raises(ValueError, match="history"):
        _fleet(model, history=torch.zeros((3, 8, 5)))                     # another sensor count
    with pytest.raises(ValueError, match="med_iqr"):
        _fleet(model, med_iqr=torch.zeros((9, 2), dtype=torch.float64))   # one table for all units
    with pytest.raises(ValueError, match="threshold"):
        _fleet(model, threshold=torch.ones(2))
    for top_m in (0, 9, 10):
        with pytest.raises(ValueError, match="top_m"):
            _fleet(model, top_m=top_m)
    with pytest.raises(ValueError, match="log"):
        _fleet(model, log=-1)


def test_fleet_refuses_an_mlp_head_without_a_fast_path_and_host_tensors_by_name():
    from gdn_amd import _lib as binding, ops
    with pytest.raises(binding.GdnHipError, match="OutLayer"):
        _fleet(_cpu_model(out_layer_num=2, out_layer_inter_dim=600))      # hidden 600: neither eval tail takes it
    with pytest.raises(binding.GdnHipError, match="HIP device"):
        _fleet(_cpu_model())                                               # history on the host
    with pytest.raises(binding.GdnHipError, match="HIP device"):
        ops.fleet_state(torch.zeros((3, 9, 5)), 5)
    with pytest.raises(binding.GdnHipError, match="HIP device"):
        ops.fleet_windows(torch.zeros((3, 16), dtype=torch.int64), torch.zeros((3, 4, 9)),
                          torch.zeros(3, dtype=torch.int32), 5, torch.zeros((3, 4, 9, 5)))


def test_push_checks_ticks_and_host_counts_before_any_device_work():
    from gdn_amd import harness
    check = harness.fleet_check_push
    ticks = torch.zeros((3, 4, 9))
    assert check(ticks, None, 3, 9) is None
    assert check(ticks, [4, 0, 2], 3, 9).tolist() == [4, 0, 2]
    assert check(ticks, torch.tensor([0, 4, 1], dtype=torch.int32), 3, 9).tolist() == [0, 4, 1]
    for bad in ([5, 0, 2], [4, -1, 2], [4, 0], [4, 0, 2, 1], [[4, 0, 2]], [1.0, 2.0, 3.0], [True, False, True]):
        with pytest.raises(ValueError, match="counts"):
            check(ticks, bad, 3, 9)
    for shape in [(4, 9), (3, 4, 8), (2, 4, 9), (3, 4, 9, 1)]:
        with pytest.raises(ValueError, match="ticks"):
            check(torch.zeros(shape), None, 3, 9)
    with pytest.raises(ValueError, match="at least one tick"):
        check(torch.zeros((3, 0, 9)), None, 3, 9)
    with pytest.raises(TypeError, match="float32"):
        check(torch.zeros((3, 4, 9), dtype=torch.float64), None, 3, 9)
