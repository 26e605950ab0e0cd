"""CPU suite of the fleet's rolling calibration (gdn_fleet_calib_bytes / _calib_write* / _ring_counts,
harness.StreamFleet(recal=, recal_every=, recal_min=, calib=)): the C-ABI surface, the host-side refusals and the row
split of the select, all decided before any launch, so no device is needed."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

GDN_OK, GDN_ERR_ARG, GDN_ERR_UNSUPPORTED = 0, -1, -3
FAKE = 4096          # a non-null, 16-byte aligned address that is never dereferenced on the host
NEW = ["gdn_fleet_calib_bytes", "gdn_fleet_calib_write", "gdn_fleet_calib_write_gaps", "gdn_fleet_calib_write_sensor",
       "gdn_fleet_ring_counts"]


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
    assert [declared[n] for n in NEW] == ["long long", "int", "int", "int", "int"]
    assert "#define GDN_ABI_VERSION 23" in header and binding.ABI_VERSION == 23 and lib.gdn_abi_version() == 23
    p, i = ctypes.c_void_p, ctypes.c_int
    assert binding.SIGNATURES["gdn_fleet_calib_bytes"] == [i, i, i]
    assert binding.SIGNATURES["gdn_fleet_calib_write"] == [p, p, p, p, p, i, i, i, i, i, i, p, p, p]
    assert binding.SIGNATURES["gdn_fleet_calib_write_gaps"] == [p, p, p, p, p, p, i, i, i, i, i, i, p, p, p]
    assert binding.SIGNATURES["gdn_fleet_calib_write_sensor"] == binding.SIGNATURES["gdn_fleet_calib_write_gaps"]
    assert binding.SIGNATURES["gdn_fleet_ring_counts"] == [p, p, i, i, i, p, p, p]
    # the fleet forms mirror the single stream's, with (counts, units) in the place of count and the fleet's w
    for tail in ("", "_gaps", "_sensor"):
        assert (binding.SIGNATURES["gdn_fleet_calib_write" + tail].count(p)
                == binding.SIGNATURES["gdn_stream_calib_write" + tail].count(p) + 1)
    from gdn_amd import harness, ops
    assert all(callable(getattr(ops, f)) for f in ("fleet_calib_ring", "fleet_calib_write", "fleet_ring_counts",
                                                   "fleet_select_spans", "fleet_select_counts"))
    assert callable(harness.StreamFleet.recalibrate) and callable(harness.StreamFleet.calibration)


def test_fleet_calib_bytes_are_units_times_a_stream_ring():
    lib = _lib()
    for units, n, R in [(1, 1, 64), (3, 9, 130), (6, 129, 64), (16, 127, 1024), (256, 127, 1024), (4096, 17, 64),
                        (2, 3, 1 << 20), (4096, 1, 65536)]:
        assert lib.gdn_fleet_calib_bytes(units, n, R) == units * lib.gdn_stream_calib_bytes(n, R) > 0
    assert lib.gdn_fleet_calib_bytes(4096, 64, 1024) == 4096 * lib.gdn_stream_calib_bytes(64, 1024)   # exactly 2 GiB
    for units, n, R in [(0, 9, 64), (-1, 9, 64), (4097, 9, 64), (3, 0, 64), (3, 4097, 64), (3, 9, 63),
                        (3, 9, (1 << 20) + 1), (3, 4096, 1 << 17),      # one unit beyond the single stream's 2 GiB
                        (4096, 65, 1024), (2, 4096, 65536)]:           # every unit fits, the fleet does not
        assert lib.gdn_fleet_calib_bytes(units, n, R) == 0, (units, n, R)


def _write(name="gdn_fleet_calib_write", units=3, c=16, n=127, w=15, R=256, **kw):
    a = dict(state=FAKE, pred=FAKE, chunk=FAKE, alarm=FAKE, valid=FAKE, counts=FAKE, keys=FAKE, keep=FAKE)
    a.update(kw)
    head = [a["state"], a["pred"], a["chunk"], a["alarm"]] + ([] if name == "gdn_fleet_calib_write" else [a["valid"]])
    return getattr(_lib(), name)(*head, a["counts"], units, c, n, w, R, 1, a["keys"], a["keep"], None)


FORMS = ["gdn_fleet_calib_write", "gdn_fleet_calib_write_gaps", "gdn_fleet_calib_write_sensor"]


@pytest.mark.parametrize("name", FORMS)
def test_every_null_pointer_and_a_push_longer_than_the_ring_are_argument_errors(name):
    nulls = ["state", "pred", "chunk", "alarm", "counts", "keys", "keep"] + ([] if name == FORMS[0] else ["valid"])
    for null in nulls:
        assert _write(name, **{null: None}) == GDN_ERR_ARG, null
        assert _write(name, c=64, **{null: None}) == GDN_ERR_ARG, null          # the tile form's side of the border
    assert _write(name, state=None, n=4097) == GDN_ERR_ARG                      # a null pointer is looked at first
    assert _write(name, c=65, R=64) == GDN_ERR_ARG
    assert _write(name, c=257, R=256) == GDN_ERR_ARG


@pytest.mark.parametrize("name", FORMS)
@pytest.mark.parametrize("shape", [dict(units=4097, c=1), dict(units=1, c=4097, R=8192), dict(units=17, c=241),
                                   dict(units=0), dict(c=0), dict(n=4097), dict(n=0), dict(w=0), dict(w=1025),
                                   dict(R=63, c=1), dict(R=(1 << 20) + 1), dict(units=4096, c=1, n=65, R=1024)],
                         ids=["u4097", "c4097", "17x241", "u0", "c0", "n4097", "n0", "w0", "w1025", "R63", "R_big",
                              "fleet_2GiB"])
def test_shapes_outside_the_limits_are_refused_without_a_device(name, shape):
    assert _write(name, **shape) == GDN_ERR_UNSUPPORTED


def test_ring_counts_refusals():
    lib = _lib()
    assert lib.gdn_fleet_ring_counts(FAKE, FAKE, 3, 9, 64, None, FAKE, None) == GDN_ERR_ARG
    assert lib.gdn_fleet_ring_counts(FAKE, None, 3, 9, 64, FAKE, None, None) == GDN_ERR_ARG     # tick mode needs kept
    assert lib.gdn_fleet_ring_counts(FAKE, None, 3, 9, 63, FAKE, FAKE, None) == GDN_ERR_UNSUPPORTED
    assert lib.gdn_fleet_ring_counts(FAKE, None, 4097, 9, 64, FAKE, FAKE, None) == GDN_ERR_UNSUPPORTED
    assert lib.gdn_fleet_ring_counts(None, None, 3, 9, 64, FAKE, None, None) == GDN_OK          # sensor, no mask: no launch


# ------------------------------------------------------------------------------------------- the row split
@pytest.mark.parametrize("units,n", [(1, 4096), (16, 4096), (4096, 17), (3, 9)])
def test_the_select_rows_are_cut_at_whole_units_with_at_most_65535_rows_a_call(units, n):
    from gdn_amd import ops
    spans = ops.fleet_select_spans(units, n)
    assert spans[0][0] == 0 and sum(k for _, k in spans) == units
    for (u0, k), nxt in zip(spans, spans[1:] + [(units, 0)]):
        assert k >= 1 and u0 + k == nxt[0] and k * n <= 65535
    # as few calls as whole units allow: every span but the last is full
    assert all((k + 1) * n > 65535 for _, k in spans[:-1])
    want = {(1, 4096): [(0, 1)], (16, 4096): [(0, 15), (15, 1)], (4096, 17): [(0, 3855), (3855, 241)],
            (3, 9): [(0, 3)]}[(units, n)]
    assert spans == want


def test_the_row_split_refuses_what_it_cannot_cut():
    from gdn_amd import ops
    for units, n in [(0, 9), (3, 0), (3, 65536)]:
        with pytest.raises(ValueError, match="units"):
            ops.fleet_select_spans(units, n)


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


def test_the_ring_is_off_by_default_and_reaches_the_device_check_when_the_host_facts_hold():
    from gdn_amd import _lib as binding
    model = _cpu_model()
    for kw in (dict(), dict(recal=64), dict(recal=64, recal_min=1, recal_every=7, exclude_alarms=False),
               dict(recal=130, gaps=True, calib="sensor"), dict(recal=64, recal_min=64, events=dict(on=2))):
        with pytest.raises(binding.GdnHipError, match="HIP device"):        # history on the host: the last host check
            _fleet(model, **kw)


def test_the_host_refusals_name_their_argument():
    model = _cpu_model()
    with pytest.raises(ValueError, match="recal = 64"):
        _fleet(model, chunk=65, recal=64)                                   # recal < chunk
    with pytest.raises(ValueError, match="recal = 63"):
        _fleet(model, recal=63)                                             # below the ring's smallest
    with pytest.raises(ValueError, match="recal = "):
        _fleet(model, recal=(1 << 20) + 1)
    with pytest.raises(ValueError, match="recal_every"):
        _fleet(model, recal_every=16)                                       # no ring
    with pytest.raises(ValueError, match="recal_every"):
        _fleet(model, recal=64, recal_every=-1)
    for bad in (0, 65, -3):
        with pytest.raises(ValueError, match="recal_min"):
            _fleet(model, recal=64, recal_min=bad)
    with pytest.raises(ValueError, match="recal_min"):
        _fleet(model, recal_min=8)                                          # given with recal=0
    with pytest.raises(ValueError, match="calib='sensor'"):
        _fleet(model, recal=64, calib="sensor")                             # no gaps
    with pytest.raises(ValueError, match="calib='sensor'"):
        _fleet(model, gaps=True, calib="sensor")                            # no ring
    with pytest.raises(ValueError, match="calib"):
        _fleet(model, recal=64, calib="row")


def test_recalibrate_and_calibration_need_a_ring():
    from gdn_amd import harness
    plain = harness.StreamFleet.__new__(harness.StreamFleet)
    plain.recal = 0
    with pytest.raises(ValueError, match="recal=0"):
        plain.recalibrate()
    with pytest.raises(ValueError, match="recal=0"):
        plain.calibration()


def test_from_calibration_refuses_the_new_keywords_by_name():
    from gdn_amd import _lib as binding, harness
    model = _cpu_model()
    series = torch.rand((3, 9, 40))
    with pytest.raises(ValueError, match="calib_gaps=True"):
        harness.StreamFleet.from_calibration(model, series, 4, gaps=True, recal=64, calib="sensor")
    with pytest.raises(ValueError, match="gaps=True"):
        harness.StreamFleet.from_calibration(model, series, 4, calib_gaps=True)
    series[1, 2, 3] = float("nan")
    with pytest.raises(binding.GdnHipError, match="HIP device"):            # calib_gaps takes a period with gaps
        harness.StreamFleet.from_calibration(model, series, 4, gaps=True, calib_gaps=True, recal=64)


def test_the_wrappers_refuse_host_tensors_and_partial_gap_arguments_by_name():
    from gdn_amd import _lib as binding, ops
    state, counts = torch.zeros((3, 16), dtype=torch.int64), torch.zeros(3, dtype=torch.int32)
    chunk, alarm = torch.zeros((3, 4, 9)), torch.zeros((3, 4), dtype=torch.int32)
    keys, keep = torch.zeros((3, 9, 64), dtype=torch.float64), torch.zeros((3, 64), dtype=torch.uint8)
    with pytest.raises(binding.GdnHipError, match="HIP device"):
        ops.fleet_calib_write(state, chunk, chunk, alarm, counts, 5, keys, keep)
    with pytest.raises(ValueError, match="by_sensor needs the validity plane"):
        ops.fleet_calib_write(state, chunk, chunk, alarm, counts, 5, keys, keep, by_sensor=True)
    with pytest.raises(binding.GdnHipError, match="ring_keys is on cpu"):
        ops.fleet_ring_counts(keys, keep, torch.zeros((3, 9), dtype=torch.int32), torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="ring_keys"):
        ops.fleet_ring_counts(keys[0], keep, None)
    for units, n, R in [(0, 9, 64), (3, 9, 63), (4097, 9, 64)]:
        with pytest.raises(binding.GdnHipError, match="fleet calibration ring"):
            ops.fleet_calib_ring(units, n, R, "cpu")
    ring_keys, ring_keep = ops.fleet_calib_ring(3, 9, 130, "cpu")           # views of ONE allocation, created empty
    assert ring_keys.shape == (3, 9, 130) and ring_keep.shape == (3, 130)
    assert bool((ring_keys.view(torch.int64) == -1).all()) and int(ring_keep.sum()) == 0
    one_keys, one_keep = ops.stream_calib_ring(9, 130, "cpu")
    assert torch.equal(ring_keys[1].view(torch.int64), one_keys.view(torch.int64)) and torch.equal(ring_keep[2], one_keep)
    base = ring_keys.untyped_storage().data_ptr()
    assert ring_keys.data_ptr() == base and ring_keep.data_ptr() == base + 8 * 3 * 9 * 130
