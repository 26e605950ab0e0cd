"""CPU suite of the fleet archive evaluator: the additive entry points in header, bindings and library,
the refusals that harness.FleetEvaluator decides from host facts alone (no device is touched), and the seam rule of the
per-unit smoothing restated in NumPy float64."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from _fleet_case import MSL, _cpu_model
from conftest import ROOT

NEW = ("gdn_fleet_series_keys", "gdn_fleet_series_smooth_max", "gdn_fleet_series_smooth_topm",
       "gdn_fleet_series_smooth_max_gaps", "gdn_fleet_series_smooth_topm_gaps")


def test_the_symbols_are_declared_bound_and_exported_and_the_abi_stays():
    from gdn_amd import _lib as binding
    header = open(os.path.join(ROOT, "include", "gdn_hip.h")).read()
    declared = dict((name, ret) for ret, name in re.findall(r"^(int|long long)\s+(gdn_\w+)\s*\(", header, flags=re.M))
    lib = binding.load()
    for name in NEW:
        assert declared.get(name) == "int" and name in binding.SIGNATURES, name
        fn = getattr(lib, name)                      # AttributeError: the symbol is missing
        assert fn.argtypes == binding.SIGNATURES[name] and fn.restype is ctypes.c_int
        params = re.search(name + r"\s*\(([^)]*)\)\s*;", header).group(1)
        assert len(params.split(",")) == len(binding.SIGNATURES[name]), name
    assert "#define GDN_ABI_VERSION 23" in header and binding.ABI_VERSION == 23 and lib.gdn_abi_version() == 23
    p, i = ctypes.c_void_p, ctypes.c_int
    # (pred, gt, keep, valid, units, t, n, pitch, keys, stream)
    assert binding.SIGNATURES["gdn_fleet_series_keys"] == [p, p, p, p, i, i, i, i, p, p]
    assert binding.SIGNATURES["gdn_fleet_series_smooth_max"] == [p, p, p, i, i, i, p, p, p]
    assert binding.SIGNATURES["gdn_fleet_series_smooth_topm"] == [p, p, p, i, i, i, i, p, p, p]
    for plain in ("gdn_fleet_series_smooth_max", "gdn_fleet_series_smooth_topm"):       # `valid` before the stream
        assert binding.SIGNATURES[plain + "_gaps"] == binding.SIGNATURES[plain][:-1] + [p, p]
    from gdn_amd import harness, ops
    for f in ("fleet_series_keys", "fleet_series_smooth_max", "fleet_series_smooth_topm"):
        assert "valid" in inspect.signature(getattr(ops, f)).parameters, f
    sig = inspect.signature(harness.FleetEvaluator.__init__).parameters
    assert list(sig)[1:] == ["model", "series", "batch", "use_graph", "want_scores", "top_m", "gaps", "min_kept", "calib",
                             "streams"]
    assert (sig["use_graph"].default, sig["top_m"].default, sig["min_kept"].default, sig["calib"].default,
            sig["streams"].default) == (True, 0, 64, "tick", 3)
    for name in ("step", "thresholds", "status_gaps", "unit", "fleet"):
        assert callable(getattr(harness.FleetEvaluator, name)), name


def test_the_limits_are_host_arithmetic():
    from gdn_amd import _lib, ops
    ops.fleet_series_check(1, 1, 1)
    ops.fleet_series_check(4096, 16, 4096)                           # 8 * 2^12 * 2^12 * 2^4 = 2 GiB exactly
    ops.fleet_series_check(32, 2048, 4096)
    for units, t, n, pitch in ((0, 5, 5, None), (4097, 5, 5, None), (3, 0, 5, None), (3, 5, 0, None), (3, 5, 4097, None),
                               (3, 5, 5, 4), (4096, 17, 4096, None), (32, 2048, 4096, 2049)):
        with pytest.raises(_lib.GdnHipError, match="fleet series"):
            ops.fleet_series_check(units, t, n, pitch)


def test_the_constructor_refuses_by_name_without_a_device():
    from gdn_amd import _lib, harness
    model = _cpu_model(MSL)
    n, w = MSL[:2]
    fine = torch.zeros((3, n, w + 45))
    with pytest.raises(ValueError, match=r"\[U, n, T_raw\]"):
        harness.FleetEvaluator(model, fine[0], batch=16)             # a 2-D series
    for t_raw in (w, w - 1):
        with pytest.raises(ValueError, match="no tick to score"):
            harness.FleetEvaluator(model, fine[:, :, :t_raw], batch=16)
    with pytest.raises(ValueError, match="needs gaps=True"):
        harness.FleetEvaluator(model, fine, batch=16, calib="sensor")
    with pytest.raises(ValueError, match="one of want_scores and top_m"):
        harness.FleetEvaluator(model, fine, batch=16, top_m=3, want_scores=True)
    with pytest.raises(ValueError, match="top_m = 9"):
        harness.FleetEvaluator(model, fine, batch=16, top_m=9)
    with pytest.raises(_lib.GdnHipError, match="bfloat16"):
        harness.FleetEvaluator(model, fine.to(torch.bfloat16), batch=16)
    big = torch.empty((64, n, w + 200000), device="meta")            # 8 * 64 * 27 * 200000 bytes of keys: 2.6 GiB
    with pytest.raises(_lib.GdnHipError, match="2 GiB"):
        harness.FleetEvaluator(model, big, batch=16)
    with pytest.raises(_lib.GdnHipError, match="units = 4097"):
        harness.FleetEvaluator(model, torch.empty((4097, n, w + 1), device="meta"), batch=16)
    with pytest.raises(_lib.GdnHipError, match="HIP device"):        # what is left is the device itself
        harness.FleetEvaluator(model, fine, batch=16)


def _smooth(e):
    """The 4-tap causal mean of e [t, n] float64 with the scorer's rule: ticks 0 - 2 are 0.0, the sum runs left to
    right."""
    out = np.zeros_like(e)
    for i in range(3, e.shape[0]):
        out[i] = (((e[i - 3] + e[i - 2]) + e[i - 1]) + e[i]) / 4.0
    return out


def test_the_seam_rule_every_unit_is_a_series_of_its_own():
    """What gdn_fleet_series_smooth_* must NOT do: smooth the concatenation of the units.  Per unit the first three
    ticks are 0.0 and no predecessor comes from the unit before; on the concatenated series exactly the first three
    ticks of units 1 .. U-1 differ (they mix in the tail of the previous unit), every other tick agrees bit for bit."""
    rng = np.random.default_rng(8)
    units, t, n = 3, 21, 5
    e = rng.random((units, t, n))                                    # normalised errors, float64
    per_unit = np.stack([_smooth(e[u]) for u in range(units)])
    flat = _smooth(e.reshape(units * t, n)).reshape(units, t, n)
    assert (per_unit[:, :3] == 0.0).all()
    np.testing.assert_array_equal(per_unit[0], flat[0])              # the first unit has no seam before it
    np.testing.assert_array_equal(per_unit[:, 3:], flat[:, 3:])      # ticks whose window lies inside one unit
    assert (flat[1:, :3] != 0.0).all() and (flat[1:, :3] != per_unit[1:, :3]).all()    # the leak the kernel must not have
    # the maximum over sensors, the anomaly score, differs there too
    assert (flat.max(axis=2)[1:, :3] > per_unit.max(axis=2)[1:, :3]).all()
    # a partial last run (t = 21 = 2 * 8 + 5) and a unit shorter than the window: every score is 0
    assert (_smooth(e[0, :2]) == 0.0).all()
