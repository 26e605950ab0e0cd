"""CPU suite of the fleet's missing readings and alarm episodes (gdn_fleet_fill / _score_gaps / _advance_gaps / _events,
harness.StreamFleet(gaps=, events=)): the C-ABI surface and the host-side refusals, all decided before any launch, so no
device is needed."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

GDN_ERR_ARG, GDN_ERR_UNSUPPORTED = -1, -3
FAKE = 4096          # a non-null, 16-byte aligned address that is never dereferenced on the host
NEW = ["gdn_fleet_fill", "gdn_fleet_score_gaps", "gdn_fleet_advance_gaps", "gdn_fleet_events_bytes", "gdn_fleet_events"]


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
        params = re.search(r"^(?:int|long long)\s+" + name + r"\s*\(([^)]*)\)\s*;", header, flags=re.M).group(1)
        assert len(params.split(",")) == len(binding.SIGNATURES[name]), name
    assert [declared[n] for n in NEW] == ["int", "int", "int", "long long", "int"]
    assert "#define GDN_ABI_VERSION 23" in header and binding.ABI_VERSION == 23 and lib.gdn_abi_version() == 23
    p, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert binding.SIGNATURES["gdn_fleet_fill"] == [p, p, p, i, i, i, i, p, p, p, p]
    assert binding.SIGNATURES["gdn_fleet_score_gaps"] == [p, p, p, p, p, p, p, i, i, i, i, i, p, p, p, p]
    assert binding.SIGNATURES["gdn_fleet_advance_gaps"] == [p, p, p, p, p, p, p, p, p, i, i, i, i, i, p, p, ll, p, p]
    assert binding.SIGNATURES["gdn_fleet_events_bytes"] == [i, i, ll]
    assert binding.SIGNATURES["gdn_fleet_events"] == [p, p, p, p, p, p, i, i, i, i, i, i, i, ll, p, p]
    # the gaps forms mirror the single stream's, with (counts, units) in the place of count and the fleet's w
    assert binding.SIGNATURES["gdn_fleet_score_gaps"].count(p) == binding.SIGNATURES["gdn_stream_score_gaps"].count(p) + 1
    assert (binding.SIGNATURES["gdn_fleet_advance_gaps"].count(p)
            == binding.SIGNATURES["gdn_stream_advance_gaps"].count(p) + 1)
    from gdn_amd import harness, ops
    assert all(callable(getattr(ops, f)) for f in ("fleet_fill", "fleet_score", "fleet_advance", "fleet_events",
                                                   "fleet_events_alloc"))
    assert callable(harness.StreamFleet.status_gaps) and callable(harness.StreamFleet.episodes)
    assert callable(harness.fleet_clear_levels)


def test_fleet_events_bytes_are_units_times_a_stream_events_allocation():
    lib = _lib()
    for units, m, E in [(1, 1, 0), (3, 3, 2), (16, 8, 64), (256, 3, 4096), (4096, 1, 1), (2, 8, 1 << 20)]:
        assert lib.gdn_fleet_events_bytes(units, m, E) == units * lib.gdn_stream_events_bytes(m, E) > 0
    for units, m, E in [(0, 3, 64), (-1, 3, 64), (4097, 3, 64), (3, 0, 64), (3, 9, 64), (3, 3, -1), (3, 3, (1 << 20) + 1)]:
        assert lib.gdn_fleet_events_bytes(units, m, E) == 0


def _fill(units=3, c=16, n=127, w=15, **kw):
    a = dict(state=FAKE, raw=FAKE, counts=FAKE, filled=FAKE, valid=FAKE, gap_chunk=FAKE)
    a.update(kw)
    return _lib().gdn_fleet_fill(a["state"], a["raw"], a["counts"], units, c, n, w, a["filled"], a["valid"],
                                 a["gap_chunk"], None)


def _score(units=3, c=16, n=127, w=15, m=3, **kw):
    a = dict(state=FAKE, pred=FAKE, chunk=FAKE, valid=FAKE, med=FAKE, thr=FAKE, counts=FAKE, scores=FAKE, sensors=FAKE,
             alarm=FAKE)
    a.update(kw)
    return _lib().gdn_fleet_score_gaps(a["state"], a["pred"], a["chunk"], a["valid"], a["med"], a["thr"], a["counts"],
                                       units, c, n, w, m, a["scores"], a["sensors"], a["alarm"], None)


def _advance(units=3, c=16, n=127, w=15, m=3, log_len=8, **kw):
    a = dict(state=FAKE, chunk=FAKE, pred=FAKE, valid=FAKE, gap_chunk=FAKE, med=FAKE, alarm=FAKE, sensors=FAKE,
             counts=FAKE, log_ticks=FAKE, log_sensors=FAKE, gaps=FAKE)
    a.update(kw)
    return _lib().gdn_fleet_advance_gaps(a["state"], a["chunk"], a["pred"], a["valid"], a["gap_chunk"], a["med"],
                                         a["alarm"], a["sensors"], a["counts"], units, c, n, w, m, a["log_ticks"],
                                         a["log_sensors"], log_len, a["gaps"], None)


def _events(units=3, c=16, n=127, w=15, m=3, on=2, off=3, E=64, **kw):
    a = dict(state=FAKE, scores=FAKE, sensors=FAKE, thr=FAKE, clear=FAKE, counts=FAKE, events=FAKE)
    a.update(kw)
    return _lib().gdn_fleet_events(a["state"], a["scores"], a["sensors"], a["thr"], a["clear"], a["counts"], units, c, n,
                                   w, m, on, off, E, a["events"], None)


def test_every_null_pointer_is_an_argument_error():
    for null in ("state", "raw", "counts", "filled", "valid", "gap_chunk"):
        assert _fill(**{null: None}) == GDN_ERR_ARG, null
    for null in ("state", "pred", "chunk", "valid", "med", "thr", "counts", "scores", "sensors", "alarm"):
        assert _score(**{null: None}) == GDN_ERR_ARG, null
    for null in ("state", "chunk", "pred", "valid", "gap_chunk", "med", "alarm", "sensors", "counts", "gaps"):
        assert _advance(**{null: None}) == GDN_ERR_ARG, null
    assert _advance(log_ticks=None) == GDN_ERR_ARG and _advance(log_sensors=None) == GDN_ERR_ARG
    assert _advance(log_len=-1) == GDN_ERR_ARG
    assert _advance(log_len=0, log_ticks=None, log_sensors=None, n=4097) == GDN_ERR_UNSUPPORTED
    for null in ("state", "scores", "sensors", "thr", "clear", "counts", "events"):
        assert _events(**{null: None}) == GDN_ERR_ARG, null
    assert _events(state=None, n=4097) == GDN_ERR_ARG          # a null pointer is looked at first


@pytest.mark.parametrize("shape", [dict(units=4097, c=1), dict(units=1, c=4097), dict(units=17, c=241), dict(units=0),
                                   dict(c=0), dict(n=4097), dict(n=0), dict(w=0), dict(w=1025)],
                         ids=["u4097", "c4097", "17x241", "u0", "c0", "n4097", "n0", "w0", "w1025"])
def test_shapes_outside_the_limits_are_refused_without_a_device(shape):
    assert _fill(**shape) == GDN_ERR_UNSUPPORTED
    assert _score(**shape) == GDN_ERR_UNSUPPORTED
    assert _advance(**shape) == GDN_ERR_UNSUPPORTED
    assert _events(**shape) == GDN_ERR_UNSUPPORTED


@pytest.mark.parametrize("m,n", [(0, 27), (9, 27), (4, 3), (-1, 27)], ids=["m0", "m9", "m_gt_n", "m_neg"])
def test_score_and_advance_refuse_m_outside_one_to_eight_and_beyond_n(m, n):
    assert _score(m=m, n=n) == GDN_ERR_UNSUPPORTED
    assert _advance(m=m, n=n) == GDN_ERR_UNSUPPORTED


@pytest.mark.parametrize("bad", [dict(m=0), dict(m=9), dict(on=0), dict(on=4097), dict(off=0), dict(off=4097),
                                 dict(E=-1), dict(E=(1 << 20) + 1)],
                         ids=["m0", "m9", "on0", "on4097", "off0", "off4097", "E_neg", "E_big"])
def test_events_refuse_the_limits_of_the_single_stream_launch(bad):
    assert _events(**bad) == GDN_ERR_UNSUPPORTED
    stream = dict(m=3, on=2, off=3, E=64)
    stream.update(bad)
    assert _lib().gdn_stream_events(FAKE, FAKE, FAKE, FAKE, FAKE, 16, 16, stream["m"], stream["on"], stream["off"],
                                    stream["E"], FAKE, None) == GDN_ERR_UNSUPPORTED


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


def test_the_options_are_off_by_default_and_reach_the_device_check_when_the_host_facts_hold():
    from gdn_amd import _lib as binding
    model = _cpu_model()
    for kw in (dict(), dict(gaps=True), dict(events=dict(on=2, off=3, lo=0.5, cap=8)),
               dict(gaps=True, events=dict(lo=[0.5, 1.0, 0.0]))):
        with pytest.raises(binding.GdnHipError, match="HIP device"):        # history on the host: the last host check
            _fleet(model, **kw)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_gaps_refuse_a_history_whose_last_w_ticks_of_any_unit_are_not_finite(bad):
    from gdn_amd import _lib as binding
    model = _cpu_model()
    history = torch.zeros((3, 9, 7))
    history[1, 4, 6] = bad                                   # unit 1's last tick
    with pytest.raises(ValueError, match="history"):
        _fleet(model, history=history, gaps=True)
    history = torch.zeros((3, 9, 7))
    history[2, 0, 1] = bad                                   # before the last w = 5 ticks: not looked at
    with pytest.raises(binding.GdnHipError, match="HIP device"):
        _fleet(model, history=history, gaps=True)
    history[1, 4, 6] = bad
    with pytest.raises(binding.GdnHipError, match="HIP device"):            # gaps=False never looks
        _fleet(model, history=history)


def test_events_are_checked_by_events_config_and_lo_per_unit_by_name():
    from gdn_amd import harness
    model = _cpu_model()
    for events, what in ((dict(on=0), "on"), (dict(off=4097), "off"), (dict(cap=-1), "cap"), (dict(hi=1.0), "hi"),
                         (dict(cap=(1 << 20) + 1), "cap")):
        with pytest.raises(ValueError, match=what):
            _fleet(model, events=events)
    with pytest.raises(ValueError, match=r"lo\[0\]"):
        _fleet(model, events=dict(lo=1.5))                                  # one number above the one threshold
    with pytest.raises(ValueError, match=r"lo\[1\]"):
        _fleet(model, threshold=torch.tensor([1.0, 0.5, 2.0]), events=dict(lo=[1.0, 0.75, 2.0]))
    with pytest.raises(ValueError, match=r"lo\[2\]"):
        _fleet(model, threshold=torch.tensor([1.0, 0.5, 0.25]), events=dict(lo=0.5))
    with pytest.raises(ValueError, match="lo"):
        _fleet(model, events=dict(lo=[0.5, 0.5]))                           # neither 1 nor U levels
    with pytest.raises(ValueError, match="lo"):
        _fleet(model, events=dict(lo=[[0.5, 0.5, 0.5]]))
    with pytest.raises(ValueError, match="NaN"):
        _fleet(model, events=dict(lo=[0.5, float("nan"), 0.5]))
    levels = harness.fleet_clear_levels
    assert levels(None, torch.tensor([1.0, 0.5, 2.0]), 3).tolist() == [1.0, 0.5, 2.0]
    assert levels(0.25, 1.0, 3).tolist() == [0.25] * 3 and levels(None, 1.0, 3).tolist() == [1.0] * 3
    got = levels([1.0, -1.0, 2.0], torch.tensor([1.0, 0.5, 2.0]), 3)        # lo == hi: no hysteresis, allowed
    assert got.dtype == torch.float64 and got.tolist() == [1.0, -1.0, 2.0]


def test_status_gaps_and_episodes_need_their_option():
    from gdn_amd import harness
    plain = harness.StreamFleet.__new__(harness.StreamFleet)
    plain.with_gaps, plain.events = False, None
    with pytest.raises(ValueError, match="gaps=False"):
        plain.status_gaps()
    with pytest.raises(ValueError, match="events=None"):
        plain.episodes(0)


def test_from_calibration_with_gaps_refuses_a_series_that_is_not_finite():
    from gdn_amd import _lib as binding, harness
    model = _cpu_model()
    series = torch.rand((3, 9, 40))
    series[2, 3, 7] = float("nan")
    with pytest.raises(ValueError, match="calibration period"):
        harness.StreamFleet.from_calibration(model, series, 4, gaps=True)
    with pytest.raises(binding.GdnHipError, match="HIP device"):            # gaps=False: as before
        harness.StreamFleet.from_calibration(model, series, 4)
    with pytest.raises(binding.GdnHipError, match="HIP device"):            # finite: on to the device check
        harness.StreamFleet.from_calibration(model, torch.rand((3, 9, 40)), 4, gaps=True, events=dict(on=2))


def test_the_fleet_wrappers_refuse_host_tensors_and_partial_gap_arguments_by_name():
    from gdn_amd import _lib as binding, ops
    state, counts = torch.zeros((3, 16), dtype=torch.int64), torch.zeros(3, dtype=torch.int32)
    chunk = torch.zeros((3, 4, 9))
    with pytest.raises(binding.GdnHipError, match="HIP device"):
        ops.fleet_fill(state, chunk, counts, 5, torch.zeros((3, 4, 9)), torch.zeros((3, 4, 9), dtype=torch.uint8),
                       torch.zeros((3, 2, 9), dtype=torch.int32))
    with pytest.raises(ValueError, match="all of valid, gap_chunk and gaps"):
        ops.fleet_advance(state, chunk, chunk, None, None, None, counts, 5, 1, valid=torch.zeros((3, 4, 9), dtype=torch.uint8))
    with pytest.raises(binding.GdnHipError, match="fleet events"):
        ops.fleet_events_alloc(0, 3, 64, "cpu")
    with pytest.raises(binding.GdnHipError, match="fleet events"):
        ops.fleet_events_alloc(3, 9, 64, "cpu")
    assert ops.fleet_events_alloc(3, 2, 5, "cpu").shape == (3, (160 + 32 * 5 + 4 * 5 * 2) // 8)
