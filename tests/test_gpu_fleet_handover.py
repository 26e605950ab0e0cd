"""GPU suite of unit hand-over and of StreamFleet.localise: a unit leaves a running fleet as a detector
(`unit_state_dict`), a detector enters one (`load_unit`), a unit is re-seeded (`reset_unit`) — unit u against a
StreamDetector that runs alone, every other unit against a twin fleet that was left alone — and `localise(u)` against
the detector's.  Every comparison is on bit patterns."""
import numpy as np
import pytest
import torch

from _fleet_case import CHUNK, DOWN, N, UNITS, W, assert_same_memory, gen, memory, raw_ticks, same, tables
from _fleet_units_case import ALL, assert_unit_is, build, detector, detectors, make_prep_units, push_both, unit_memory

pytestmark = pytest.mark.gpu

U = 1                                                # the unit that moves; it contributes every tick (the clocks agree)
CASES = {"plain": (dict(), False), "all": (ALL, True)}


def _ticks(g, r, fleet, dev):
    """r ticks per unit: raw float64 ticks under prep=, else model ticks; under gaps=True with missing readings."""
    ticks = raw_ticks(g, r, torch.float64, dev) if fleet.prep is not None else torch.rand((UNITS, r, N), generator=g).to(dev)
    if fleet.with_gaps:
        ticks[0, :, 3] = float("nan")
        ticks[U, r // 2, 5] = float("inf")
    return ticks


def _graphs(fleet):
    return fleet.graph, dict(fleet._prep_graphs)


def _same_graphs(fleet, before):
    graph, prep_graphs = _graphs(fleet)
    assert graph is before[0] and list(prep_graphs) == list(before[1])
    assert all(prep_graphs[k] is before[1][k] for k in prep_graphs)
    assert graph is not None or prep_graphs                          # (one was captured: the test means something)


def _others_equal(fleet, twin):
    a, b = memory(fleet), memory(twin)
    for u in range(UNITS):
        if u != U:
            assert_same_memory(unit_memory(a, u), unit_memory(b, u))


def _pair(dev, case):
    """Two fleets built alike (the second is the twin that is left alone)."""
    kw, with_prep = CASES[case]
    prep = make_prep_units(dev) if with_prep else None
    model, fleet, seeds = build(dev, kw, prep)
    _, twin, _ = build(dev, kw, prep)
    return model, fleet, twin, seeds, kw


BEFORE = [(16, None), (7, [3, 7, 0]), (9, [9, 9, 4]), (32, None)]    # 64 rows of the time axis, unit U all of them
AFTER = [(5, None), (16, [16, 16, 2]), (37, None), (6, [0, 6, 6])]


@pytest.mark.parametrize("case", list(CASES))
def test_export_the_detector_built_from_unit_state_dict_goes_on_as_the_unit_in_the_fleet(case, gpu_device, tmp_path):
    from gdn_amd import harness
    dev = gpu_device
    model, fleet, _, _, _ = _pair(dev, case)
    g = gen(31)
    for r, counts in BEFORE:
        fleet.push(_ticks(g, r, fleet, dev), counts)
    before = _graphs(fleet)
    mem = memory(fleet)
    sd = fleet.unit_state_dict(U)
    assert_same_memory(memory(fleet), mem)                           # read-only
    _same_graphs(fleet, before)
    path = str(tmp_path / "unit.npz")
    harness.write_stream_checkpoint(path, sd)
    det = harness.StreamDetector.load(path, model, prep=fleet.unit_prep(U), device=dev, use_graph=False)
    assert det.chunk == CHUNK and det._handed == fleet._handed and det.recal_every == fleet.recal_every
    if fleet.prep is not None:
        assert same(det.prep.table, fleet.prep.tables[U])
    assert_unit_is(fleet, U, det, "at export")
    for r, counts in AFTER:
        push_both(fleet, {U: det}, _ticks(g, r, fleet, dev), counts)
    assert int(fleet.status()[1][U]) > 0
    assert_unit_is(fleet, U, det, "after export")
    if fleet.events is not None:
        for a, b in zip(fleet.episodes(U), det.episodes()):
            assert same(a, b)
    with pytest.raises(ValueError, match=r"unit_state_dict\(3\)"):
        fleet.unit_state_dict(UNITS)


@pytest.mark.parametrize("case", list(CASES))
def test_adopt_load_unit_continues_the_detector_in_place_and_moves_no_other_unit(case, gpu_device):
    dev = gpu_device
    model, fleet, twin, _, kw = _pair(dev, case)
    g = gen(32)
    # a detector that ran alone, on a table, a threshold and a history of its own, as many ticks as the fleet
    own = torch.rand((N, W + 2), generator=gen(33)).to(dev)
    det = detector(model, tables(dev, gen(34), units=1)[0], 0.75, own, kw, fleet.unit_prep(U))
    for r, counts in BEFORE:
        ticks = _ticks(g, r, fleet, dev)
        fleet.push(ticks, counts)
        twin.push(ticks, counts)
        alone = _ticks(g, r, fleet, dev)[U]
        for s in range(0, r, CHUNK * (DOWN if fleet.prep is not None else 1)):
            det.push(alone[s:s + CHUNK * (DOWN if fleet.prep is not None else 1)].contiguous())
    assert det._handed == fleet._handed
    before = _graphs(fleet)
    fleet.load_unit(U, det.state_dict())
    _same_graphs(fleet, before)
    assert_unit_is(fleet, U, det, "at adoption")
    _others_equal(fleet, twin)
    assert fleet.localise(U).ticks.numel() == 0                      # the unit has no rows in the last push's buffers
    for r, counts in AFTER:
        ticks = _ticks(g, r, fleet, dev)
        push_both(fleet, {U: det}, ticks, counts)
        twin.push(ticks, counts)
    _same_graphs(fleet, before)
    assert_unit_is(fleet, U, det, "after adoption")
    _others_equal(fleet, twin)
    # refused by the name of the field, before any device write
    mem = memory(fleet)
    sd = det.state_dict()
    with pytest.raises(ValueError, match="unit hand-over: wide = 1, the fleet was built with wide = 0"):
        fleet.load_unit(U, dict(sd, wide=np.array(1, dtype=np.int64)))
    with pytest.raises(ValueError, match="unit hand-over: top_m = 2"):
        fleet.load_unit(U, dict(sd, top_m=np.array(2, dtype=np.int64)))
    with pytest.raises(ValueError, match="model_sha256 differs"):
        fleet.load_unit(U, dict(sd, model_sha256=np.array("00" * 32)))
    with pytest.raises(ValueError, match=r"load_unit\(-1\)"):
        fleet.load_unit(-1, sd)
    other = detector(model, tables(dev, gen(34), units=1)[0], 0.75, own, {} if kw else dict(gaps=True))
    with pytest.raises(ValueError, match="unit hand-over: with_gaps"):
        fleet.load_unit(U, other.state_dict())
    assert_same_memory(memory(fleet), mem)


@pytest.mark.parametrize("case", list(CASES))
def test_reset_unit_gives_a_fresh_detector_and_leaves_the_others_alone(case, gpu_device):
    dev = gpu_device
    model, fleet, twin, _, kw = _pair(dev, case)
    g = gen(35)
    for r, counts in BEFORE:                                         # 64 rows: recal_every's clock stands on a multiple
        ticks = _ticks(g, r, fleet, dev)
        fleet.push(ticks, counts)
        twin.push(ticks, counts)
    assert int(fleet.status()[0][U]) > 0
    before = _graphs(fleet)
    table, history = tables(dev, gen(36), units=1)[0], torch.rand((N, W + 3), generator=gen(37)).to(dev)
    fleet.reset_unit(U, table, 0.6, history)
    det = detector(model, table, 0.6, history, kw, fleet.unit_prep(U))
    _same_graphs(fleet, before)
    assert_unit_is(fleet, U, det, "at reset")
    assert fleet.status()[0][U] == 0 and fleet.localise(U).ticks.numel() == 0
    _others_equal(fleet, twin)
    for r, counts in AFTER:
        ticks = _ticks(g, r, fleet, dev)
        push_both(fleet, {U: det}, ticks, counts)
        twin.push(ticks, counts)
    _same_graphs(fleet, before)
    assert_unit_is(fleet, U, det, "after reset")
    _others_equal(fleet, twin)
    mem = memory(fleet)
    with pytest.raises(ValueError, match=r"history of shape \[70, h\]"):
        fleet.reset_unit(U, table, 0.6, history[:-1])
    with pytest.raises(ValueError, match="shorter than the window"):
        fleet.reset_unit(U, table, 0.6, history[:, :W - 1].contiguous())
    if fleet.with_gaps:
        bad = history.clone()
        bad[4, -1] = float("nan")
        with pytest.raises(ValueError, match="history: its last 5 ticks hold a value that is not finite"):
            fleet.reset_unit(U, table, 0.6, bad)
        with pytest.raises(ValueError, match=r"lo\[0\] = 0.9 lies above the raise level"):
            fleet.reset_unit(U, table, 0.6, history, lo=0.9)
    else:
        with pytest.raises(ValueError, match="lo = 0.1: the fleet was built with events=None"):
            fleet.reset_unit(U, table, 0.6, history, lo=0.1)
        with pytest.raises(ValueError, match="seed: the fleet was built with recal=0"):
            fleet.reset_unit(U, table, 0.6, history, seed=(None, None, None, None))
    assert_same_memory(memory(fleet), mem)


def test_reset_unit_seeds_the_ring_as_from_calibration_seeds_it(gpu_device):
    from gdn_amd import harness
    from _fleet_case import MSL, model_on
    dev = gpu_device
    model, n = model_on(dev, MSL), MSL[0]
    series = torch.rand((UNITS, n, 120), generator=gen(38)).to(dev)
    kw = dict(top_m=2, wide=False, recal=64, recal_min=8)
    fleet = harness.StreamFleet.from_calibration(model, series, CHUNK, **kw)
    other = torch.rand((n, 150), generator=gen(39)).to(dev)
    w = MSL[1]
    table, threshold, tail, _, _, rows = harness._calibrate_period(model, other, w, 8192, False, 64, "tick", True)
    det = harness.StreamDetector.from_calibration(model, other, CHUNK, use_graph=False, **kw)
    keys0, keep0 = fleet.ring_keys[0].clone(), fleet.ring_keep[0].clone()
    fleet.reset_unit(U, table, threshold, tail, seed=rows)
    assert same(fleet.ring_keys[U], det.ring_keys) and torch.equal(fleet.ring_keep[U], det.ring_keep)
    assert torch.equal(fleet.unit_state(U), det.state) and same(fleet.med_iqr[U], det.med_iqr)
    assert same(fleet.threshold[U:U + 1], det.threshold.view(1))
    assert same(fleet.ring_keys[0], keys0) and torch.equal(fleet.ring_keep[0], keep0)
    fleet.reset_unit(U, table, threshold, tail)                      # without a seed: an empty ring
    empty = harness.StreamDetector(model, table, threshold, tail, CHUNK, use_graph=False, **kw)
    assert same(fleet.ring_keys[U], empty.ring_keys) and not fleet.ring_keep[U].any()


# --------------------------------------------------------------------------------------------------- localise(u)
@pytest.mark.parametrize("case", ["plain", "prep_gaps"])
def test_localise_equals_the_detectors_of_that_unit_field_by_field(case, gpu_device):
    dev = gpu_device
    kw = dict(gaps=True) if case == "prep_gaps" else dict()
    prep = make_prep_units(dev) if case == "prep_gaps" else None
    model, fleet, seeds = build(dev, kw, prep)
    dets = detectors(model, fleet, seeds, kw)
    g = gen(40)
    scale = DOWN if prep is not None else 1
    for r, counts in [(4 * scale, None), (3 * scale, [3 * scale, 0, 2 * scale])]:
        push_both(fleet, dets, _ticks(g, r, fleet, dev), counts)
        real = fleet.counts.tolist()
        assert real == ([r // scale] * UNITS if counts is None else [c // scale for c in counts])
        for u in range(UNITS):
            got = fleet.localise(u)
            if real[u] == 0:                                         # silent: an empty result
                assert got.ticks.numel() == 0 and got.attention.shape[0] == 0
                continue
            want = dets[u].localise()
            assert torch.equal(torch.nonzero(fleet.alarm[u, :real[u]]).view(-1) + int(dets[u].state[0]) - real[u], got.ticks)
            for name in want._fields:
                assert same(getattr(got, name), getattr(want, name)), (u, name)
            rows = [real[u] - 1, 0]
            got, want = fleet.localise(u, rows), dets[u].localise(rows)
            assert got.ticks.numel() == 2
            for name in want._fields:
                assert same(getattr(got, name), getattr(want, name)), (u, name)
            with pytest.raises(ValueError, match=rf"rows outside \[0, {real[u]}\)"):
                fleet.localise(u, [real[u]])
            with pytest.raises(ValueError, match="rows outside"):
                fleet.localise(u, [-1])
    assert int(fleet.status()[1].sum()) > 0                          # some default rows were alarm rows
    with pytest.raises(ValueError, match=r"localise\(3\)"):
        fleet.localise(UNITS)
