"""CPU suite of the threshold from the ring (gdn_fleet_ring_threshold_bytes / gdn_fleet_ring_threshold,
harness.StreamDetector / StreamFleet(recal_threshold=), recalibrate(threshold=)): the C-ABI surface, the
refusals decided before any launch, and the numpy yardstick on hand-made rings with the answer written out.  No device
is needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _ring_threshold_ref as ref
from conftest import ROOT

GDN_OK, GDN_ERR_ARG, GDN_ERR_UNSUPPORTED = 0, -1, -3
FAKE = 4096          # a non-null, 16-byte aligned address that is never dereferenced on the host
NEW = ["gdn_fleet_ring_threshold_bytes", "gdn_fleet_ring_threshold"]


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
    assert [declared[n] for n in NEW] == ["long long", "int"]
    assert "#define GDN_ABI_VERSION 23" in header and binding.ABI_VERSION == 23 and lib.gdn_abi_version() == 23
    p, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    assert binding.SIGNATURES["gdn_fleet_ring_threshold_bytes"] == [i, i]
    assert binding.SIGNATURES["gdn_fleet_ring_threshold"] == [p] * 5 + [i] * 5 + [d, i] + [p] * 8
    from gdn_amd import harness, ops
    assert callable(ops.fleet_ring_threshold) and callable(ops.fleet_ring_threshold_workspace)
    assert callable(harness.checkpoint_recal_threshold)


def test_workspace_bytes_are_positive_inside_the_ring_limits_and_zero_outside():
    lib = _lib()
    for units, n, R in [(1, 1, 64), (3, 9, 130), (6, 129, 64), (16, 127, 1024), (256, 127, 1024), (4096, 17, 64),
                        (2, 3, 1 << 20), (4096, 1, 65536)]:
        assert lib.gdn_fleet_calib_bytes(units, n, R) > 0
        assert lib.gdn_fleet_ring_threshold_bytes(units, R) == 16 * units * ((R + 60) // 61) > 0
    for units, R in [(0, 64), (-1, 64), (4097, 64), (3, 63), (3, (1 << 20) + 1), (3, 0)]:
        assert lib.gdn_fleet_ring_threshold_bytes(units, R) == 0, (units, R)


def _call(units=3, n=9, w=5, R=130, mode=0, margin=1.0, min_eligible=1, **kw):
    a = dict(state=FAKE, keys=FAKE, keep=FAKE, med_iqr=FAKE, select=None, ws=FAKE, threshold=FAKE, clear_frac=None,
             clear=None, peak=FAKE, eligible=FAKE, peak_slot=FAKE)
    a.update(kw)
    return _lib().gdn_fleet_ring_threshold(a["state"], a["keys"], a["keep"], a["med_iqr"], a["select"], units, n, w, R,
                                           mode, margin, min_eligible, a["ws"], a["threshold"], a["clear_frac"],
                                           a["clear"], a["peak"], a["eligible"], a["peak_slot"], None)


def test_null_pointers_are_argument_errors():
    for null in ["state", "keys", "keep", "med_iqr", "ws", "threshold", "peak", "eligible", "peak_slot"]:
        assert _call(**{null: None}) == GDN_ERR_ARG, null
        assert _call(mode=2, **{null: None}) == GDN_ERR_ARG, null
    assert _call(clear_frac=FAKE) == GDN_ERR_ARG                      # one of the pair without the other
    assert _call(clear=FAKE) == GDN_ERR_ARG
    assert _call(state=None, n=4097) == GDN_ERR_ARG                   # a null pointer is looked at first


@pytest.mark.parametrize("margin", [0.0, -1.0, float("nan"), float("inf"), float("-inf")])
def test_a_margin_that_is_not_finite_and_positive_is_an_argument_error(margin):
    assert _call(margin=margin) == GDN_ERR_ARG
    assert _call(margin=margin, mode=2, select=FAKE, clear_frac=FAKE, clear=FAKE) == GDN_ERR_ARG


def test_min_eligible_below_one_and_an_unknown_mode_are_argument_errors():
    assert _call(min_eligible=0) == GDN_ERR_ARG
    assert _call(min_eligible=-5) == GDN_ERR_ARG
    assert _call(mode=3) == GDN_ERR_ARG
    assert _call(mode=-1) == GDN_ERR_ARG


@pytest.mark.parametrize("shape", [dict(units=4097), dict(units=0), dict(n=4097), dict(n=0), dict(w=0), dict(w=1025),
                                   dict(R=63), dict(R=(1 << 20) + 1), dict(units=4096, n=65, R=1024),
                                   dict(units=2, n=4096, R=65536)],
                         ids=["u4097", "u0", "n4097", "n0", "w0", "w1025", "R63", "R_big", "fleet_2GiB", "fleet_2GiB_b"])
def test_shapes_outside_the_limits_are_refused_without_a_device(shape):
    assert _call(**shape) == GDN_ERR_UNSUPPORTED
    assert _call(mode=2, **shape) == GDN_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------- host side of the harness
def _cpu_model(n=9, w=5, **kw):
    from gdn_amd import GDN
    return GDN([torch.zeros((2, 1), dtype=torch.long)], n, dim=16, input_dim=w, topk=3, **kw)


def _detector(model, n=9, w=5, **kw):
    from gdn_amd import harness
    return harness.StreamDetector(model, torch.zeros((n, 2), dtype=torch.float64), 1.0, torch.zeros((n, w)), 4, **kw)


def _fleet(model, units=3, n=9, w=5, **kw):
    from gdn_amd import harness
    return harness.StreamFleet(model, torch.zeros((units, n, 2), dtype=torch.float64), 1.0,
                               torch.zeros((units, n, w)), 4, **kw)


@pytest.mark.parametrize("build", [_detector, _fleet], ids=["detector", "fleet"])
def test_the_constructors_refuse_by_name_before_any_device_work(build):
    from gdn_amd import _lib as binding
    model = _cpu_model()
    with pytest.raises(ValueError, match="recal_threshold"):
        build(model, recal_threshold=1.05)                                  # no ring
    for bad in (0.0, -1.0, float("nan"), float("inf"), "wide"):
        with pytest.raises(ValueError, match="recal_threshold"):
            build(model, recal=64, recal_threshold=bad)
    for kw in (dict(recal=64, recal_threshold=1.0), dict(recal=64, recal_threshold=1.05, events=dict(on=2)),
               dict(recal=130, gaps=True, calib="sensor", recal_threshold=2)):
        with pytest.raises(binding.GdnHipError, match="HIP device"):        # history on the host: the last host check
            build(model, **kw)


@pytest.mark.parametrize("cls", ["StreamDetector", "StreamFleet"])
def test_recalibrate_refuses_a_bad_margin_by_name_before_any_device_work(cls):
    from gdn_amd import harness
    obj = getattr(harness, cls).__new__(getattr(harness, cls))
    obj.recal, obj.recal_threshold = 64, None
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="threshold = "):
            obj.recalibrate(threshold=bad)
    obj.recal = 0
    with pytest.raises(ValueError, match="recal=0"):
        obj.recalibrate(threshold=1.0)


def test_the_margin_of_recalibrate_resolves_on_the_host():
    from gdn_amd import harness
    core = harness._StreamCore()
    core.recal_threshold = 1.25
    assert core._margin(None) == 1.25 and core._margin(False) is None and core._margin(2) == 2.0
    core.recal_threshold = None
    assert core._margin(None) is None and core._margin(1.5) == 1.5


def test_the_checkpoint_checkers_know_the_optional_keys_and_refuse_a_mismatch_by_name():
    from gdn_amd import harness
    assert harness.checkpoint_recal_threshold({}) is None
    assert harness.checkpoint_recal_threshold({"recal_threshold": np.array(1.05)}) == 1.05
    for bad in (np.array(0.0), np.array(float("nan")), np.array([1.0]), np.array(1, dtype=np.int64)):
        with pytest.raises(ValueError, match="recal_threshold"):
            harness.checkpoint_recal_threshold({"recal_threshold": bad})
    sd = {"recal_threshold": np.array(1.05)}
    harness._check_recal_threshold(sd, {}, 64, None, "stream checkpoint")                         # load(): nothing to compare
    harness._check_recal_threshold(sd, {"recal_threshold": 1.05}, 64, None, "stream checkpoint")
    harness._check_recal_threshold({}, {"recal_threshold": None}, 64, None, "stream checkpoint")  # an older file
    with pytest.raises(ValueError, match="recal_threshold = 1.05"):
        harness._check_recal_threshold(sd, {"recal_threshold": None}, 64, None, "stream checkpoint")
    with pytest.raises(ValueError, match="recal_threshold = None"):
        harness._check_recal_threshold({}, {"recal_threshold": 1.05}, 64, None, "stream checkpoint")
    with pytest.raises(ValueError, match="recal_threshold = 1.05"):
        harness._check_recal_threshold(sd, {"recal_threshold": 1.1}, 64, None, "fleet checkpoint")
    with pytest.raises(ValueError, match="without a calibration ring"):
        harness._check_recal_threshold(sd, {}, 0, None, "stream checkpoint")
    with pytest.raises(ValueError, match="clear_frac"):
        harness._check_recal_threshold({"clear_frac": np.ones(1)}, {}, 64, {"on": 1}, "stream checkpoint")
    with pytest.raises(ValueError, match="clear_frac"):
        harness._check_recal_threshold(dict(sd, clear_frac=np.ones(1)), {}, 64, None, "stream checkpoint")


def test_the_command_line_takes_the_margin():
    from gdn_amd import main
    args = main.build_parser().parse_args(["-stream", "64", "-stream_recal", "256", "-stream_recal_threshold", "1.05"])
    assert args.stream_recal == 256 and args.stream_recal_threshold == 1.05
    assert main.build_parser().parse_args([]).stream_recal_threshold is None


# ------------------------------------------------------------------------------------------- the yardstick, by hand
# One sensor, median 0 and IQR 0.99: inv_den = 1 / (0.99 + 0.01) = 1, so an error is its key and a score is the mean of
# four keys (exact in float64 for the small integers used here).
UNIT = np.array([[0.0, 0.99]])
R = 64


def _ring(values=None, keep=None):
    keys = np.zeros((1, R)) if values is None else np.asarray(values, dtype=np.float64).reshape(1, R)
    return keys, (np.ones(R, np.uint8) if keep is None else np.asarray(keep, dtype=np.uint8))


def test_the_seam_leaves_out_the_three_oldest_ticks():
    keys, keep = _ring()
    keys[0, 10] = 400.0                               # the largest key sits in the oldest tick of a ring with base 10
    ok = ref.ring_eligible(keep, 10)
    assert not ok[10] and not ok[11] and not ok[12] and ok[13] and ok[9] and int(ok.sum()) == R - 3
    # slots 10 .. 12 see it but straddle the seam; slot 13 is the first whose window holds it whole
    assert ref.ring_peak(keys, keep, UNIT, 10) == (100.0, R - 3, 13)
    # with base 11 the key is the NEWEST tick: slot 10 itself is eligible, 11 .. 13 are not
    assert ref.ring_peak(keys, keep, UNIT, 11) == (100.0, R - 3, 10)
    # base 0: the seam sits at the ring's end and no window wraps
    assert ref.ring_peak(keys, keep, UNIT, 0) == (100.0, R - 3, 10)


def test_the_predecessors_wrap_around_the_ring():
    keys, keep = _ring()
    keys[0, R - 1], keys[0, 0] = 8.0, 4.0             # slot 1 smooths over slots R-2, R-1, 0, 1
    peak, eligible, slot = ref.ring_peak(keys, keep, UNIT, 30)
    assert (peak, eligible, slot) == (3.0, R - 3, 0)  # slots 0, 1 and 2 all reach (8 + 4) / 4: the smallest slot wins
    score = ref.ring_scores(keys, UNIT, False)
    assert score[R - 1] == 2.0 and score[0] == 3.0 and score[1] == 3.0 and score[2] == 3.0 and score[3] == 1.0


def test_a_keep_run_of_three_has_no_eligible_slot_and_a_run_of_four_has_one():
    keys, keep = _ring(np.arange(R, dtype=np.float64), np.zeros(R, np.uint8))
    keep[20:23] = 1
    assert ref.ring_peak(keys, keep, UNIT, 0) == (-np.inf, 0, -1)
    keep[20:24] = 1
    assert ref.ring_peak(keys, keep, UNIT, 0) == ((20 + 21 + 22 + 23) / 4.0, 1, 23)
    # ... unless the seam cuts that one window
    assert ref.ring_peak(keys, keep, UNIT, 22) == (-np.inf, 0, -1)
    # a single zero in an otherwise full ring takes out its slot and the three after it (and the seam three more)
    keep = np.ones(R, np.uint8)
    keep[40] = 0
    ok = ref.ring_eligible(keep, 0)
    assert not ok[40:44].any() and ok[44] and ok[39] and int(ok.sum()) == R - 3 - 4


def test_the_filler_is_a_neutral_reading_in_sensor_mode_only():
    keys, keep = _ring(np.full(R, 2.0))
    keys.view(np.uint64)[0, 7] = ref.FILLER
    err = ref.ring_errors(keys, UNIT, True)
    assert err[0, 7] == 0.0 and err[0, 6] == 2.0
    peak, eligible, slot = ref.ring_peak(keys, keep, UNIT, 0, by_sensor=True)
    assert (peak, eligible, slot) == (2.0, R - 3, 3)  # slots 7 .. 10 score 1.5, every other eligible slot 2.0
    score = ref.ring_scores(keys, UNIT, True)
    assert (score[7:11] == 1.5).all() and score[11] == 2.0
    # tick mode never reads a filler in an eligible window: such a tick has keep 0; read all the same it is a NaN error
    # that never wins the maximum
    assert np.isnan(ref.ring_errors(keys, UNIT, False)[0, 7])
    assert ref.ring_scores(keys, UNIT, False)[7] == -np.inf
    keep[7] = 0
    assert ref.ring_peak(keys, keep, UNIT, 0) == (2.0, R - 3 - 4, 3)


def test_the_rule_of_the_rewrite():
    keys, keep = _ring(np.full(R, 2.0), np.zeros(R, np.uint8))
    peak, eligible, slot = ref.ring_peak(keys, keep, UNIT, 5)
    assert (peak, eligible, slot) == (-np.inf, 0, -1)
    assert ref.ring_threshold(7.0, peak, eligible, 1.05, 1) == 7.0                  # no eligible slot: kept
    assert ref.ring_threshold(7.0, 2.0, 61, 1.05, 61) == 2.0 * 1.05
    assert ref.ring_threshold(7.0, 2.0, 60, 1.05, 61) == 7.0                        # below min_eligible
    assert ref.ring_threshold(7.0, 2.0, 61, 1.05, 61, selected=False) == 7.0
    assert ref.ring_threshold(7.0, 0.0, 61, 1.05, 1) == 7.0                         # peak must be > 0
    assert ref.ring_threshold(7.0, -3.0, 61, 1.05, 1) == 7.0
    assert ref.ring_threshold(7.0, np.inf, 61, 1.05, 1) == 7.0                      # ... and finite
    # the scale is the scorer's: (key - median) * (1 / (|iqr| + 1e-2)), a negative IQR by its magnitude
    table = np.array([[1.0, -0.49], [0.5, 0.24]])
    two = np.stack([np.full(R, 3.0), np.full(R, 1.0)])
    peak, _, _ = ref.ring_peak(two, np.ones(R, np.uint8), table, 0)
    e0, e1 = (3.0 - 1.0) * (1.0 / (0.49 + 1e-2)), (1.0 - 0.5) * (1.0 / (0.24 + 1e-2))
    assert peak == max((((e0 + e0) + e0) + e0) / 4.0, (((e1 + e1) + e1) + e1) / 4.0)
