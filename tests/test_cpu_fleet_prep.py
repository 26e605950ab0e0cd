"""CPU suite of a fleet's raw-readings front end (gdn_fleet_prep_bytes / gdn_fleet_prep_ticks, harness.StreamFleet(prep=)):
the C-ABI surface and the host-side refusals and arithmetic, all decided before any launch, so no device is needed."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

GDN_ERR_ARG, GDN_ERR_UNSUPPORTED = -1, -3
FAKE = 4096          # a non-null, 16-byte aligned address that is never dereferenced on the host
NEW = ["gdn_fleet_prep_bytes", "gdn_fleet_prep_ticks"]


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
    assert declared["gdn_fleet_prep_bytes"] == "long long" and declared["gdn_fleet_prep_ticks"] == "int"
    assert "#define GDN_ABI_VERSION 23" in header and binding.ABI_VERSION == 23 and lib.gdn_abi_version() == 23
    p, i = ctypes.c_void_p, ctypes.c_int
    assert binding.SIGNATURES["gdn_fleet_prep_bytes"] == [i, i, i]
    assert binding.SIGNATURES["gdn_fleet_prep_ticks"] == [p, i, i, p, p, i, i, i, i, p, p, p, p]
    from gdn_amd import harness, ops
    assert all(callable(getattr(ops, f)) for f in ("fleet_prep_state", "fleet_prep_ticks", "fleet_prep_views"))
    assert all(callable(getattr(harness, f)) for f in ("fleet_check_prep", "fleet_raw_cuts", "fleet_raw_hand"))


def test_prep_bytes_are_the_ticks_and_one_count_word_per_tile_and_zero_outside_the_limits():
    lib = _lib()
    for units, n, down in [(1, 1, 1), (3, 65, 10), (3, 130, 17), (256, 127, 10), (4096, 4096, 64), (2, 64, 64)]:
        tiles = (n + 63) // 64
        want = 8 * units * down * n + ((4 * units * tiles + 7) & ~7)
        assert lib.gdn_fleet_prep_bytes(units, n, down) == want > 0
        assert want % 8 == 0
    for units, n, down in [(0, 127, 10), (-1, 127, 10), (4097, 127, 10), (3, 0, 10), (3, 4097, 10), (3, 127, 0),
                           (3, 127, 65), (3, 127, -1)]:
        assert lib.gdn_fleet_prep_bytes(units, n, down) <= 0


def _ticks(rows=40, f64=0, units=3, c=4, n=127, down=10, **kw):
    a = dict(raw=FAKE, raw_counts=FAKE, pend=FAKE, table=FAKE, out=FAKE, counts=FAKE)
    a.update(kw)
    return _lib().gdn_fleet_prep_ticks(a["raw"], rows, f64, a["raw_counts"], a["pend"], units, c, n, down, a["table"],
                                       a["out"], a["counts"], None)


def test_every_null_pointer_and_a_row_count_outside_one_to_c_down_is_an_argument_error():
    for null in ("raw", "raw_counts", "pend", "table", "out", "counts"):
        for f64 in (0, 1):
            assert _ticks(f64=f64, **{null: None}) == GDN_ERR_ARG, null
    for rows in (0, -1, 41, 1 << 30):
        assert _ticks(rows=rows) == GDN_ERR_ARG, rows
    assert _ticks(rows=2, c=1, down=1) == GDN_ERR_ARG


@pytest.mark.parametrize("shape", [dict(units=4097, c=1), dict(units=1, c=4097), dict(units=17, c=241), dict(units=0),
                                   dict(c=0), dict(n=4097), dict(n=0), dict(down=0), dict(down=65), dict(down=-3)],
                         ids=["u4097", "c4097", "17x241", "u0", "c0", "n4097", "n0", "down0", "down65", "down_neg"])
def test_shapes_outside_the_limits_are_refused_without_a_device(shape):
    assert _ticks(rows=1, **shape) == GDN_ERR_UNSUPPORTED
    from gdn_amd import _lib as binding
    full = dict(units=3, c=4, n=127, down=10)
    full.update(shape)
    with pytest.raises(binding.GdnHipError, match="GDN_ERR_UNSUPPORTED"):
        binding.call("gdn_fleet_prep_ticks", FAKE, 1, 0, FAKE, FAKE, full["units"], full["c"], full["n"], full["down"],
                     FAKE, FAKE, FAKE, None)


# ------------------------------------------------------------------------------------------- StreamFleet, host side
def _cpu_model(n=9, w=5, **kw):
    from gdn_amd import GDN
    return GDN([torch.zeros((2, 1), dtype=torch.long)], n, dim=16, input_dim=w, topk=3, **kw)


def _prep(n=9, down=4):
    from gdn_amd.prep import Prep
    table = torch.stack([torch.ones(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)], dim=1)
    return Prep(table, torch.zeros((n, 4), dtype=torch.float64), down)


def _fleet(model, units=3, n=9, w=5, **kw):
    from gdn_amd import harness
    args = dict(med_iqr=torch.zeros((units, n, 2), dtype=torch.float64), threshold=1.0,
                history=torch.zeros((units, n, w)), chunk=4)
    args.update(kw)
    return harness.StreamFleet(model, args.pop("med_iqr"), args.pop("threshold"), args.pop("history"),
                               args.pop("chunk"), **args)


def test_the_constructor_takes_prep_and_refuses_another_sensor_count_and_a_staging_buffer_beyond_256_mb():
    from gdn_amd import _lib as binding, harness
    with pytest.raises(ValueError, match="prep: fitted on 8 sensors"):
        _fleet(_cpu_model(), prep=_prep(n=8))
    # a prep that fits passes on to the first device need: the history on the host (prep= is a known keyword)
    with pytest.raises(binding.GdnHipError, match="HIP device"):
        _fleet(_cpu_model(), prep=_prep())
    # [3, 64 * 64, 4096] fp32 = 192 MB fits, float64 = 384 MB does not; [6, 64 * 64, 4096] fp32 does not either
    big = _prep(n=4096, down=64)
    harness.fleet_check_prep(big, 3, 64, 4096)
    with pytest.raises(ValueError, match="staging buffer.*256 MB"):
        harness.fleet_check_prep(big, 3, 64, 4096, itemsize=8)
    with pytest.raises(ValueError, match="staging buffer.*256 MB"):
        harness.fleet_check_prep(big, 6, 64, 4096)
    with pytest.raises(ValueError, match="staging buffer.*256 MB"):
        _fleet(_cpu_model(n=4096, w=1), n=4096, w=1, units=6, chunk=64, prep=big)


def test_push_checks_raw_ticks_and_host_counts_before_any_device_work():
    from gdn_amd import harness
    check = harness.fleet_check_push
    for dtype in (torch.float32, torch.float64):
        ticks = torch.zeros((3, 11, 9), dtype=dtype)
        assert check(ticks, None, 3, 9, raw=True) is None
        assert check(ticks, [11, 0, 3], 3, 9, raw=True).tolist() == [11, 0, 3]
        for bad in ([12, 0, 2], [4, -1, 2], [4, 0], [1.0, 2.0, 3.0]):
            with pytest.raises(ValueError, match="counts"):
                check(ticks, bad, 3, 9, raw=True)
    for dtype in (torch.float16, torch.int32, torch.bfloat16):
        with pytest.raises(TypeError, match="float32 or torch.float64"):
            check(torch.zeros((3, 4, 9), dtype=dtype), None, 3, 9, raw=True)
    with pytest.raises(TypeError, match="float32"):                  # without prep: fp32 only, as ever
        check(torch.zeros((3, 4, 9), dtype=torch.float64), None, 3, 9)
    with pytest.raises(ValueError, match="ticks"):
        check(torch.zeros((3, 4, 8)), None, 3, 9, raw=True)
    with pytest.raises(ValueError, match="at least one tick"):
        check(torch.zeros((3, 0, 9)), None, 3, 9, raw=True)


def test_the_wrappers_refuse_host_tensors_and_wrong_shapes_by_name():
    from gdn_amd import _lib as binding, ops
    with pytest.raises(binding.GdnHipError, match="HIP device"):
        ops.fleet_prep_ticks(torch.zeros((3, 8, 9)), torch.zeros(3, dtype=torch.int32), torch.zeros(64, dtype=torch.int64),
                             4, torch.zeros((9, 2), dtype=torch.float64), torch.zeros((3, 2, 9)),
                             torch.zeros(3, dtype=torch.int32))
    with pytest.raises(binding.GdnHipError, match="fleet prep state"):
        ops.fleet_prep_state(3, 9, 65, "cpu")
    pend = ops.fleet_prep_state(3, 130, 10, "cpu")                   # (zeros on the host: the layout needs no device)
    ticks, pending = ops.fleet_prep_views(pend, 3, 130, 10)
    assert ticks.shape == (3, 10, 130) and ticks.dtype == torch.float64
    assert pending.shape == (3, 3) and pending.dtype == torch.int32
    assert pend.numel() * 8 == _lib().gdn_fleet_prep_bytes(3, 130, 10)
    assert pending.data_ptr() == pend.data_ptr() + 8 * 3 * 10 * 130 and ticks.data_ptr() == pend.data_ptr()


def test_raw_cuts_carry_at_most_chunk_down_rows_and_the_views_cover_what_a_unit_can_complete():
    from gdn_amd import harness
    cuts = harness.fleet_raw_cuts
    assert cuts(37, 4, 4) == [(0, 16, 4), (16, 16, 4), (32, 5, 2)]
    assert cuts(1, 10, 1) == [(0, 1, 1)]                             # one raw tick may close a group of ten
    assert cuts(10, 10, 1) == [(0, 10, 1)] and cuts(11, 10, 1) == [(0, 10, 1), (10, 1, 1)]
    assert cuts(3, 1, 2) == [(0, 2, 2), (2, 1, 1)]
    for down in (1, 3, 10, 64):
        for chunk in (1, 4):
            for r in (1, down - 1, down, chunk * down, chunk * down + 1, 3 * chunk * down + 2):
                if r < 1:
                    continue
                got = cuts(r, down, chunk)
                assert sum(rows for _, rows, _ in got) == r and [s for s, _, _ in got] == \
                    list(range(0, r, chunk * down))
                for _, rows, views in got:
                    assert 1 <= rows <= chunk * down
                    # the most a unit completes: an open group of down - 1 raw ticks plus all the rows
                    assert views == max((p + rows) // down for p in range(down)) <= chunk
    with pytest.raises(ValueError):
        cuts(4, 0, 1)


def test_the_recal_clock_counts_model_ticks_as_raw_rows_handed_floor_down():
    from gdn_amd import harness
    hand = harness.fleet_raw_hand
    assert hand(0, 9, 10) == 0 and hand(9, 1, 10) == 1 and hand(7, 5, 4) == 2 and hand(0, 40, 10) == 4
    for down in (1, 3, 10):
        raw = model = 0
        for rows in (1, 2, down, 7, 3 * down + 1, 1, 1, 5):
            model += hand(raw, rows, down)
            raw += rows
            assert model == raw // down

    # _hand() under that clock: recalibrate() exactly when the model ticks cross a multiple of recal_every
    class Clock(harness._StreamCore):
        def __init__(self, every):
            self.recal_every, self._handed, self.calls = every, 0, []

        def recalibrate(self):
            self.calls.append(self._handed)
    clock, raw = Clock(3), 0
    for rows in (5, 5, 5, 16, 1, 30):                                # down = 4: model ticks 1, 2, 3, 7, 8, 15
        clock._hand(hand(raw, rows, 4))
        raw += rows
    assert clock._handed == raw // 4 == 15 and clock.calls == [3, 7, 15]
