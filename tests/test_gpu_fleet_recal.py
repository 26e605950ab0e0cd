"""GPU suite of the fleet's rolling calibration: gdn_fleet_calib_write / _gaps / _sensor, gdn_fleet_ring_counts and
harness.StreamFleet(recal=, recal_every=, recal_min=, calib=).  The yardstick is never the code under test: the ring write
is compared with the single-stream ops.stream_calib_write on each unit's slice, the tables with ops.score_select /
score_select_counts on each unit's ring, and StreamFleet with U StreamDetectors pushed each unit's real rows in the same
cuts and recalibrated at the same point.  The arithmetic and its order per unit are the same, so every comparison is
exact: torch.equal, float64 on its bit patterns.  No tolerance."""
import pytest
import torch

from test_gpu_fleet import SHAPES, _bits, _gen, _i32, _model, _real_rows_of_last_cut, _same, _staged_fleet, _tables

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
MODES = {"plain": (False, False), "gaps": (True, False), "sensor": (True, True)}      # -> (valid given, by_sensor)


def _clamped(counts, c):
    return [min(max(int(v), 0), c) for v in counts]


# ------------------------------------------------------------------------------------------------ the ring write
# c = 63 | 64: the border between the direct form and the tile form; 65: a ragged second tile; n = 64 | 65 | 129: one
# sensor tile, a second one of one lane, a third.  R = 64 is the smallest ring (c = 64 fills it), 130 an odd pitch.
@pytest.mark.parametrize("c,R", [(c, R) for c in (1, 9, 63, 64, 65) for R in (64, 130) if c <= R])
@pytest.mark.parametrize("n", [1, 64, 65, 129])
def test_ring_write_equals_the_single_stream_launch_per_unit_and_a_silent_ring_is_untouched(n, c, R, gpu_device):
    from gdn_amd import ops
    dev, w, units = gpu_device, 4, 6
    g = _gen(n, c, R)
    # some units wrap the ring's end inside the push (R - 1, 2 R - (c + 1) // 2 with c > 1), some do not (0, 3 R + 7 ..)
    ticks = [0, R - 1, 2 * R - (c + 1) // 2, 1000, 5, 3 * R + 7]
    state, _med_iqr, _thr, chunk, pred = _staged_fleet(n, w, c, dev, g, ticks)
    alarm = (torch.rand((units, c), generator=g) < 0.3).to(torch.int32)
    alarm[0, 0], alarm[1, c - 1], alarm[3, 0] = 1, 0, 0
    valid = (torch.rand((units, c, n), generator=g) > 0.2).to(torch.uint8)
    valid[3, 0], valid[2, 0, 0] = 1, 0                               # a complete tick that did not alarm; a broken one
    alarm, valid = alarm.to(dev), valid.to(dev)
    before = state.clone()
    wrote_keep, wrote_filler = 0, 0
    for counts in ([c, c - 1, (c + 1) // 2, 1, 0, c], [c + 5, -3, c, 0, 1, c]):
        real = _clamped(counts, c)
        for mode, (with_valid, by_sensor) in MODES.items():
            for exclude in (True, False):
                keys = torch.full((units, n, R), 123.0, dtype=torch.float64, device=dev)
                keep = torch.full((units, R), 9, dtype=torch.uint8, device=dev)
                want_keys, want_keep = keys.clone(), keep.clone()
                ops.fleet_calib_write(state, pred, chunk, alarm, _i32(counts, dev), w, keys, keep, exclude,
                                      valid=valid if with_valid else None, by_sensor=by_sensor)
                for u, cnt in enumerate(real):
                    if cnt:
                        ops.stream_calib_write(state[u], pred[u], chunk[u], alarm[u], want_keys[u], want_keep[u],
                                               exclude, count=cnt, valid=valid[u] if with_valid else None,
                                               by_sensor=by_sensor)
                what = (mode, exclude, counts)
                assert _same(keys, want_keys), what
                assert torch.equal(keep, want_keep), what
                for u, cnt in enumerate(real):
                    written = int((keep[u] != 9).sum())
                    assert written == cnt, (u, what)                 # one slot per real row, no other byte of the flags
                    if cnt == 0:                                     # a silent unit: byte for byte the sentinel
                        assert bool((keys[u] == 123.0).all()) and bool((keep[u] == 9).all()), (u, what)
                wrote_keep += int((keep == 1).sum())
                wrote_filler += int((keys.view(torch.int64) == -1).sum())
    assert wrote_keep > 0 and wrote_filler > 0                       # both kinds of tick were met
    assert torch.equal(state, before)                                # the launch reads the states


# ------------------------------------------------------------------------------------------------ the counts
def _random_rings(units, n, R, dev, g, kept):
    """Rings as the tick-mode writer leaves them: unit u keeps kept[u] of its ticks, anywhere in the ring; a tick that
    is not kept holds the filler in all n keys."""
    from gdn_amd import ops
    ring_keys, ring_keep = ops.fleet_calib_ring(units, n, R, dev)
    keep = torch.zeros((units, R), dtype=torch.uint8)
    for u, k in enumerate(kept):
        keep[u, torch.randperm(R, generator=g)[:k]] = 1
    values = torch.rand((units, n, R), generator=g, dtype=torch.float64)
    values[:, :, ::7] = values[:, :, 3:4]                            # repeated keys: ties at the ranks
    ring_keys.copy_(values.to(dev))
    ring_keep.copy_(keep.to(dev))
    ring_keys.view(torch.int64)[(ring_keep == 0)[:, None, :].expand(units, n, R)] = -1
    return ring_keys, ring_keep


def test_ring_counts_are_the_keep_sums_per_unit_and_masked_units_get_zero(gpu_device):
    from gdn_amd import ops
    dev, units, n, R = gpu_device, 5, 9, 130
    g = _gen(units, n, R)
    ring_keys, ring_keep = _random_rings(units, n, R, dev, g, [R, 65, 13, 0, 91])
    sums = ring_keep.sum(1).to(torch.int32)
    counts = torch.full((units, n), -7, dtype=torch.int32, device=dev)
    kept = torch.full((units,), -7, dtype=torch.int32, device=dev)
    ops.fleet_ring_counts(ring_keys, ring_keep, counts, kept)
    assert torch.equal(kept, sums) and torch.equal(counts, sums[:, None].expand(units, n))
    assert kept.tolist()[0] == R and kept.tolist()[3] == 0
    mask = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8, device=dev)
    for select in (mask, mask.bool()):
        kept.fill_(-7)
        ops.fleet_ring_counts(ring_keys, ring_keep, counts, kept, select=select)
        assert torch.equal(counts, (sums * mask)[:, None].expand(units, n))
        assert kept.tolist() == [R, -7, int(sums[2]), 0, -7]         # a unit left out keeps its entry
    # per-sensor calibration: every row's own real keys
    ring_keys.view(torch.int64)[1, 2, :50] = -1                      # sensor 2 of unit 1 lost 50 more (some twice)
    ring_keys.view(torch.int64)[4, 0] = -1                           # a dead sensor
    want = torch.stack([ops.score_key_counts(ring_keys[u], 1, n, R) for u in range(units)])
    counts.fill_(-7)
    ops.fleet_ring_counts(ring_keys, None, counts, by_sensor=True)
    assert torch.equal(counts, want) and int(counts[4, 0]) == 0 and int(counts[1, 2]) < int(counts[1, 1])
    ops.fleet_ring_counts(ring_keys, None, counts, select=mask, by_sensor=True)
    assert torch.equal(counts, want * mask[:, None])


# ------------------------------------------------------------------------------------------------ recalibrate
def _bare_fleet(ring_keys, ring_keep, calib, recal_min):
    """A StreamFleet with nothing but what recalibrate() touches: the rings, the counts, the workspace and a table."""
    from gdn_amd import harness, ops
    units, n, R = ring_keys.shape
    dev = ring_keys.device
    fleet = harness.StreamFleet.__new__(harness.StreamFleet)
    fleet.units, fleet.n, fleet.recal, fleet.calib, fleet.recal_min, fleet.recals = units, n, R, calib, recal_min, 0
    fleet.ring_keys, fleet.ring_keep = ring_keys, ring_keep
    fleet.state = torch.zeros((units, 1), dtype=torch.int64, device=dev)
    fleet._recal_ws = ops.fleet_select_workspace(units, n, R, dev)
    fleet.recal_kept = torch.zeros((units,), dtype=torch.int32, device=dev) if calib == "tick" else None
    fleet.recal_counts = torch.zeros((units, n), dtype=torch.int32, device=dev)
    fleet.med_iqr = _tables(units, n, dev, _gen(units, n, R, 3))
    return fleet


# R = 64 and 2048: the select's single slice; 4096: one workgroup; 34816: digit passes
@pytest.mark.parametrize("R", [64, 2048, 4096, 34816])
def test_recalibrate_writes_the_detectors_select_per_unit_and_keeps_the_other_rows(R, gpu_device):
    from gdn_amd import ops
    dev, units, n = gpu_device, 5, 3
    recal_min = max(8, R // 4)
    g = _gen(R, 1)
    # unit 2 keeps fewer than recal_min ticks, unit 3 none at all; unit 4 is left out through units=
    totals = [R, recal_min, recal_min - 1, 0, R - 3]
    ring_keys, ring_keep = _random_rings(units, n, R, dev, g, totals)
    assert ring_keep.sum(1).tolist() == totals
    fleet = _bare_fleet(ring_keys, ring_keep, "tick", recal_min)
    before = fleet.med_iqr.clone()
    table = fleet.med_iqr
    fleet.recalibrate(units=[0, 1, 2, 3])
    assert fleet.med_iqr is table                                    # in place: the captured graph's pointer
    for u in (0, 1):
        want = ops.score_select(ring_keys[u], 1, n, R, totals[u])
        assert _same(fleet.med_iqr[u], want), u
        assert not _same(want, before[u])
    for u in (2, 3, 4):
        assert _same(fleet.med_iqr[u], before[u]), u                 # too few kept ticks / left out: bit for bit
    tables, kept = fleet.calibration()
    assert _same(tables, fleet.med_iqr) and kept.tolist() == totals[:4] + [0] and not kept.is_cuda
    assert fleet.recal_counts[:, 0].tolist() == totals[:4] + [0]
    fleet.recalibrate(units=torch.tensor([0, 0, 0, 0, 1], dtype=torch.bool, device=dev))
    assert _same(fleet.med_iqr[4], ops.score_select(ring_keys[4], 1, n, R, totals[4]))
    assert fleet.recal_kept.tolist() == totals
    fleet.med_iqr.copy_(before)
    fleet.recalibrate()                                              # everyone
    for u in (0, 1, 4):
        assert _same(fleet.med_iqr[u], ops.score_select(ring_keys[u], 1, n, R, totals[u])), u
    assert _same(fleet.med_iqr[2:4], before[2:4])


@pytest.mark.parametrize("R", [64, 2048, 4096, 34816])
def test_recalibrate_per_sensor_equals_the_counting_select_per_unit(R, gpu_device):
    from gdn_amd import ops
    dev, units, n = gpu_device, 4, 3
    recal_min = max(8, R // 4)
    g = _gen(R, 2)
    ring_keys, ring_keep = ops.fleet_calib_ring(units, n, R, dev)
    values = torch.rand((units, n, R), generator=g, dtype=torch.float64)
    share = torch.tensor([[1.0, 0.7, 0.5], [0.9, 0.0, 0.6], [0.1, 0.05, 0.12], [0.8, 0.8, 0.02]])   # [1, 1]: a dead sensor
    real = torch.rand((units, n, R), generator=g) < share[:, :, None]                  # unit 2: all below recal_min
    ring_keys.copy_(values.to(dev))
    ring_keys.view(torch.int64)[~real.to(dev)] = -1
    ring_keep.fill_(1)
    fleet = _bare_fleet(ring_keys, ring_keep, "sensor", recal_min)
    before = fleet.med_iqr.clone()
    fleet.recalibrate(units=[0, 1, 2])
    for u in range(units):
        want = before[u].clone()
        if u < 3:
            ops.score_select_counts(ring_keys[u], 1, n, R, ops.score_key_counts(ring_keys[u], 1, n, R), recal_min,
                                    out=want)
        assert _same(fleet.med_iqr[u], want), u
    assert _same(fleet.med_iqr[1, 1], before[1, 1]) and _same(fleet.med_iqr[2], before[2])
    assert not _same(fleet.med_iqr[0], before[0]) and not _same(fleet.med_iqr[1, 0], before[1, 0])
    tables, counts = fleet.calibration()
    assert counts.shape == (units, n) and counts[3].tolist() == [0, 0, 0] and int(counts[1, 1]) == 0
    assert torch.equal(counts[:3], real[:3].sum(2).to(torch.int32))


def test_a_fleet_of_4096_units_is_written_and_selected_in_two_spans(gpu_device):
    from gdn_amd import ops
    dev, units, n, R, w = gpu_device, 4096, 17, 64, 4
    assert ops.fleet_select_spans(units, n) == [(0, 3855), (3855, 241)]              # 69632 rows
    g = _gen(units, n)
    ring_keys, ring_keep = ops.fleet_calib_ring(units, n, R, dev)
    ring_keys.copy_(torch.rand((units, n, R), generator=g, dtype=torch.float64).to(dev))
    ring_keep.fill_(1)
    state = ops.fleet_state(torch.rand((units, n, w), generator=g).to(dev), w)
    ops.fleet_state_views(state, units, n, w)[0][:, 0] = torch.arange(units, device=dev) * 3
    chunk, pred = torch.rand((units, 1, n), generator=g).to(dev), torch.rand((units, 1, n), generator=g).to(dev)
    alarm = (torch.arange(units, device=dev) % 5 == 0).to(torch.int32).view(units, 1)
    counts = (torch.arange(units, device=dev) % 3 != 1).to(torch.int32)              # every third unit is silent
    look = [0, 3854, 3855, 4095]
    want = [(ring_keys[u].clone(), ring_keep[u].clone()) for u in look]
    ops.fleet_calib_write(state, pred, chunk, alarm, counts, w, ring_keys, ring_keep)
    fleet = _bare_fleet(ring_keys, ring_keep, "tick", 8)
    fleet.recalibrate()
    for u, (keys, keep) in zip(look, want):
        if int(counts[u]):
            ops.stream_calib_write(state[u], pred[u], chunk[u], alarm[u], keys, keep, count=1)
        assert _same(ring_keys[u], keys) and torch.equal(ring_keep[u], keep), u
        assert _same(fleet.med_iqr[u], ops.score_select(keys, 1, n, R, int(keep.sum()))), u
    # all four wrote a tick; units 0, 3855 and 4095 (multiples of 5) alarmed in it: excluded
    assert [int(ring_keep[u].sum()) for u in look] == [R - 1, R, R - 1, R - 1]


# ------------------------------------------------------------------------------------------------ StreamFleet
UNITS, TOP_M, LOG, RING, RECAL_MIN = 5, 2, 8, 64, 8
OPTIONS = {"plain": dict(), "gaps": dict(gaps=True), "sensor": dict(gaps=True, calib="sensor"),
           "events": dict(events=dict(on=2, off=2, cap=16))}


def _ticks(units, r, n, g, missing):
    ticks = torch.rand((units, r, n), generator=g)
    if missing:
        hit = torch.rand(ticks.shape, generator=g) < 0.02
        ticks[hit] = NAN
        ticks[(torch.rand(ticks.shape, generator=g) < 0.005)] = INF
    return ticks


def _pair(dev, options, chunk, g, use_graph=True, **kw):
    """A fleet and one detector per unit with the same options; thresholds from 'alarms most ticks' to 'never'."""
    from gdn_amd import harness
    n, w = SHAPES["msl"][:2]
    model = _model(dev, SHAPES["msl"])
    history = torch.rand((UNITS, n, w + 2), generator=g).to(dev)
    med_iqr = _tables(UNITS, n, dev, g)
    threshold = torch.tensor([0.0, 4.0, 6.0, 50.0, 5.0], dtype=torch.float64)
    common = dict(top_m=TOP_M, log=LOG, wide=False, recal=RING, recal_min=RECAL_MIN, **options, **kw)
    fleet = harness.StreamFleet(model, med_iqr, threshold, history, chunk, use_graph=use_graph, **common)
    dets = [harness.StreamDetector(model, med_iqr[u], float(threshold[u]), history[u].contiguous(), chunk,
                                   use_graph=False, **common) for u in range(UNITS)]
    return fleet, dets, n, w


def _push_both(fleet, dets, ticks, counts, chunk, step):
    r = ticks.shape[1]
    each = [r] * len(dets) if counts is None else list(counts)
    got = fleet.push(ticks, counts)
    for u, cnt in enumerate(each):
        if cnt == 0:
            continue                                                 # a silent unit: its detector is not pushed
        want = dets[u].push(ticks[u, :cnt])
        real = _real_rows_of_last_cut(cnt, r, chunk)
        if real:
            for a, b, what in zip(got, want, ("top_scores", "top_sensors", "alarm")):
                assert _same(a[u, :real], b), (step, u, what)


def _assert_units_equal(fleet, dets, at):
    for u, det in enumerate(dets):
        assert _same(fleet.ring_keys[u], det.ring_keys), (at, u)
        assert torch.equal(fleet.ring_keep[u], det.ring_keep), (at, u)
        assert _same(fleet.med_iqr[u], det.med_iqr), (at, u)
        assert torch.equal(fleet.unit_state(u), det.state), (at, u)
        assert torch.equal(fleet.log_ticks[u], det.log_ticks) and torch.equal(fleet.log_sensors[u], det.log_sensors)
        if fleet.events is not None:
            assert torch.equal(fleet.events[u], det.events), (at, u)
        if fleet.with_gaps:
            assert torch.equal(fleet.gaps[u], det.gaps), (at, u)


@pytest.mark.parametrize("chunk", [1, 8])
@pytest.mark.parametrize("options", list(OPTIONS))
def test_fleet_with_a_ring_writes_the_bits_of_one_detector_per_unit(options, chunk, gpu_device):
    dev = gpu_device
    g = _gen(chunk, len(options))
    fleet, dets, n, w = _pair(dev, OPTIONS[options], chunk, g)
    missing = fleet.with_gaps
    script = [(8, None), (3, None), (8, [8, 0, 5, 8, 1]), (5, [0, 5, 5, 2, 5]), (8, None), (8, [8, 8, 0, 8, 8])]
    first_graph = None
    for step, (r, counts) in enumerate(script):
        _push_both(fleet, dets, _ticks(UNITS, r, n, g, missing).to(dev), counts, chunk, step)
        first_graph = fleet.graph if first_graph is None else first_graph
        assert fleet.graph is not None and fleet.graph is first_graph            # one graph: full, short, silent
    _assert_units_equal(fleet, dets, "before")
    table, before = fleet.med_iqr, fleet.med_iqr.clone()
    fleet.recalibrate()
    done = [det.recalibrate() for det in dets]
    assert fleet.graph is first_graph and fleet.med_iqr is table                 # the graph and its pointer stay
    _assert_units_equal(fleet, dets, "recalibrated")
    assert done[0] == 0 and _same(fleet.med_iqr[0], before[0])                   # unit 0 alarms: too few kept ticks
    assert done[3] > 0 and not _same(fleet.med_iqr[3], before[3])                # unit 3 never alarms: a new table
    if fleet.calib == "tick":
        assert [k for k in fleet.calibration()[1].tolist()][3] == done[3]
    for step, (r, counts) in enumerate([(8, None), (2, [2, 1, 0, 2, 2]), (11, None)]):
        _push_both(fleet, dets, _ticks(UNITS, r, n, g, missing).to(dev), counts, chunk, 100 + step)
        assert fleet.graph is first_graph
    _assert_units_equal(fleet, dets, "after")
    assert fleet.status()[0].tolist() == [det.status()[0] for det in dets]


@pytest.mark.parametrize("options", ["plain", "sensor"])
def test_the_ring_adds_exactly_one_launch_to_a_push(options, gpu_device, monkeypatch):
    from gdn_amd import _lib as binding
    dev = gpu_device
    names = []
    real_call = binding.call

    def spy(name, *args):
        names.append(name)
        return real_call(name, *args)
    fleet, _dets, n, _w = _pair(dev, OPTIONS[options], 4, _gen(4), use_graph=False)
    kw = {k: v for k, v in OPTIONS[options].items() if k != "calib"}
    from gdn_amd import harness
    plain = harness.StreamFleet(fleet.model, fleet.med_iqr, fleet.threshold.cpu(), torch.rand((UNITS, n, _w)).to(dev), 4,
                                top_m=TOP_M, log=LOG, wide=False, use_graph=False, **kw)
    ticks = torch.rand((UNITS, 4, n)).to(dev)
    plain.push(ticks)                                                # (whatever a model's first forward folds: done)
    fleet.push(ticks)
    monkeypatch.setattr(binding, "call", spy)
    plain.push(ticks)
    without, names[:] = list(names), []
    fleet.push(ticks, [4, 0, 2, 4, 1])
    added = "gdn_fleet_calib_write" + ("_sensor" if options == "sensor" else "")
    at = names.index(added)
    assert names[:at] + names[at + 1:] == without                    # the launches of a plain push, and one more
    assert names[at + 1] in ("gdn_fleet_advance", "gdn_fleet_advance_gaps") and names[at - 1].startswith("gdn_fleet_score")


def test_recal_every_recalibrates_on_the_fleets_clock_as_the_detectors_do_on_theirs(gpu_device):
    dev = gpu_device
    g = _gen(16)
    fleet, dets, n, w = _pair(dev, dict(), 8, g, recal_every=16)
    for step, r in enumerate([8, 3, 8, 13, 1, 8, 8, 20]):            # every unit contributes every tick
        _push_both(fleet, dets, _ticks(UNITS, r, n, g, False).to(dev), None, 8, step)
        _assert_units_equal(fleet, dets, step)
    assert fleet.recals == (8 + 3 + 8 + 13 + 1 + 8 + 8 + 20) // 16 and dets[3].recals >= 1


@pytest.mark.parametrize("calib", ["tick", "sensor"])
def test_from_calibration_seeds_every_unit_as_the_detector_is_seeded(calib, gpu_device):
    from gdn_amd import harness, ops
    dev = gpu_device
    shape = SHAPES["msl"]
    n, w = shape[:2]
    model = _model(dev, shape)
    units, t = 3, 120
    g = _gen(t, len(calib))
    series = torch.rand((units, n, t), generator=g)
    hit = torch.rand(series.shape, generator=g) < 0.01
    hit[:, :, :w] = False                                            # every unit begins on real readings
    series[hit] = NAN
    series[1, 4, -2:] = NAN                                          # a period that ends inside a run
    series = series.to(dev)
    kw = dict(top_m=TOP_M, wide=False, gaps=True, calib_gaps=True, min_kept=8, recal=RING, recal_min=RECAL_MIN,
              calib=calib)
    fleet = harness.StreamFleet.from_calibration(model, series, 4, **kw)
    assert fleet.calib == calib and fleet.recal == RING
    for u in range(units):
        det = harness.StreamDetector.from_calibration(model, series[u].contiguous(), 4, use_graph=False, **kw)
        assert _same(fleet.ring_keys[u], det.ring_keys) and torch.equal(fleet.ring_keep[u], det.ring_keep), u
        assert _same(fleet.med_iqr[u], det.med_iqr) and _same(fleet.threshold[u:u + 1], det.threshold), u
        assert torch.equal(fleet.unit_state(u), det.state), u
        hist = ops.stream_state_views(fleet.unit_state(u), n, w)[2]
        assert bool(torch.isfinite(hist).all())                     # the FILLED period's last w ticks
        assert int(fleet.calib_kept[u]) == det.calib_kept
        if calib == "sensor":
            assert torch.equal(fleet.calib_counts[u], det.calib_counts)
        else:
            assert fleet.calib_counts is None and int(fleet.ring_keep[u].sum()) < RING       # broken ticks: not kept
    # the stream goes on from the seeded rings exactly as the detectors' do
    dets = [harness.StreamDetector.from_calibration(model, series[u].contiguous(), 4, use_graph=False, **kw)
            for u in range(units)]
    ticks = _ticks(units, 6, n, g, True).to(dev)
    got = fleet.push(ticks, [6, 0, 3])
    dets[0].push(ticks[0])
    dets[2].push(ticks[2, :3])
    fleet.recalibrate()
    for u, det in enumerate(dets):
        det.recalibrate()
        assert _same(fleet.ring_keys[u], det.ring_keys) and _same(fleet.med_iqr[u], det.med_iqr), u
    assert got[0].shape == (units, 2, TOP_M)
    # with none of the new keywords: what it did before
    clean = torch.rand((units, n, t), generator=g).to(dev)
    old = harness.StreamFleet.from_calibration(model, clean, 4, top_m=TOP_M, wide=False)
    assert old.recal == 0 and old.ring_keys is None and old.calib_kept is None and old.calib_counts is None
