"""GPU suite of the threshold from the ring (gdn_fleet_ring_threshold, harness.StreamDetector / StreamFleet
(recal_threshold=), recalibrate(threshold=)).  The yardstick is tests/_ring_threshold_ref.py (numpy, the
rule stated slot by slot) for the entry point, the project's own scorer for the bits of the peak, from_calibration for
the seeding identity, and one StreamDetector per unit for the fleet.

Tolerances: `eligible` and `peak_slot` are integers and exact.  `peak` and `threshold` against numpy: relative 1e-12,
the bar of the scoring parity tests — the device multiplies by a reciprocal that is specified to an ulp only (2e-16
relative per error, four errors and a mean: below 1e-15).  Every planted maximum stands at least 1e-6 relative above
the runner-up (asserted on the yardstick's own scores), so `peak_slot` cannot flip within that bar.  Everything that is
computed by the same device code on both sides is compared bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _ring_threshold_ref as ref
from _fleet_case import MSL, gen, model_on, same, tables

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
W = 4
PATTERNS = ("all", "rand90", "zeros", "runs", "none")
PLANTS = ("slot0", "last", "base+3", "base+1")          # base + 1 is never eligible (the seam)
BIG = (1000.0, 1001.0, 1002.0, 1003.0)                  # keys of the planted window, oldest first


def _bases(R):
    return (0, 1, 2, 3, R - 1, R // 2)


def _keep(pattern, R, rng):
    keep = np.ones(R, np.uint8)
    if pattern == "rand90":
        keep = (rng.random(R) < 0.9).astype(np.uint8)
    elif pattern == "zeros":
        keep[rng.choice(R, 3, replace=False)] = 0
    elif pattern == "runs":                             # a run of exactly 3 and two of exactly 4
        keep[:] = 0
        keep[5:8] = keep[20:24] = keep[40:44] = 1
    elif pattern == "none":
        keep[:] = 0
    return keep


def _gap_ok(keys, keep, table, base, by_sensor):
    """Does the largest eligible score lead the runner-up by 1e-6 relative (or is there nothing to confuse)?"""
    score, ok = ref.ring_scores(keys, table, by_sensor), ref.ring_eligible(keep, base)
    top = np.sort(score[ok])[-2:]
    return top.size < 2 or top[1] - top[0] >= 1e-6 * abs(top[1])


def _scenarios(n, R, by_sensor, seed, table):
    """Every base x keep pattern x plant as one unit: (keys [S, n, R], keep [S, R], ticks [S], planted slot [S]).  A
    unit whose two largest eligible scores came out closer than 1e-6 relative is drawn again."""
    rng = np.random.default_rng(seed)
    combos = [(b, p, q) for b in _bases(R) for p in PATTERNS for q in PLANTS]
    S = len(combos)
    keys, keep = np.empty((S, n, R)), np.empty((S, R), np.uint8)
    ticks = np.array([b + 7 * R for b, _, _ in combos], dtype=np.int64)
    planted = np.array([{"slot0": 0, "last": R - 1, "base+3": (b + 3) % R, "base+1": (b + 1) % R}[q]
                        for b, _, q in combos])
    for u, (base, pattern, _plant) in enumerate(combos):
        while True:
            keys[u], keep[u] = rng.random((n, R)), _keep(pattern, R, rng)
            if by_sensor:                               # missing readings anywhere, kept ticks included
                keys[u].view(np.uint64)[rng.random((n, R)) < 0.03] = ref.FILLER
            for j, big in enumerate(BIG):               # the window q - 3 .. q of sensor 0, growing: no two windows tie
                keys[u, 0, (planted[u] - 3 + j) % R] = big
            if not by_sensor:                           # a tick that is not kept holds the filler in every key
                keys[u].view(np.uint64)[np.broadcast_to((keep[u] == 0)[None, :], (n, R))] = ref.FILLER
            if _gap_ok(keys[u], keep[u], table[u], base, by_sensor):
                break
    return combos, keys, keep, ticks, planted


def _expect(keys, keep, table, ticks, by_sensor):
    """The yardstick per unit, with the precondition that the largest eligible score leads by 1e-6 relative."""
    out = []
    R = keep.shape[1]
    for u in range(keys.shape[0]):
        base = int(ticks[u] % R)
        peak, eligible, slot = ref.ring_peak(keys[u], keep[u], table[u], base, by_sensor)
        assert _gap_ok(keys[u], keep[u], table[u], base, by_sensor), u
        out.append((peak, eligible, slot))
    return out


def _close(got, want):
    if not np.isfinite(want):
        return got == want
    return abs(got - want) <= 1e-12 * abs(want)


def _run(dev, keys, keep, table, ticks, by_sensor, margin, min_eligible, select=None, with_clear=True):
    """ONE call of the entry point over sentinels; everything back on the host as numpy."""
    from gdn_amd import ops
    U, n, R = keys.shape
    state = ops.fleet_state(torch.zeros((U, n, W), device=dev), W)
    ops.fleet_state_views(state, U, n, W)[0][:, 0] = torch.from_numpy(ticks).to(dev)
    before = state.clone()
    d_keys, d_keep, d_table = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (keys, keep, table))
    thr = torch.arange(U, dtype=torch.float64, device=dev) + 123.456
    clear = torch.full((U,), -7.0, dtype=torch.float64, device=dev)
    frac = (torch.arange(U, dtype=torch.float64, device=dev) % 7 + 2.0) / 9.0
    peak = torch.full((U,), 55.5, dtype=torch.float64, device=dev)
    eligible = torch.full((U,), -9, dtype=torch.int32, device=dev)
    slot = torch.full((U,), -9, dtype=torch.int32, device=dev)
    ws = ops.fleet_ring_threshold_workspace(U, R, dev)
    sel = None if select is None else torch.tensor(select, dtype=torch.uint8, device=dev)
    ops.fleet_ring_threshold(state, d_keys, d_keep, d_table, W, margin, min_eligible, ws, thr, peak, eligible, slot,
                             select=sel, clear_frac=frac if with_clear else None, clear=clear if with_clear else None,
                             by_sensor=by_sensor)
    assert torch.equal(state, before)                                # the launch reads the states
    assert same(d_keys, torch.from_numpy(np.ascontiguousarray(keys)).to(dev))
    return tuple(t.cpu().numpy() for t in (thr, clear, frac, peak, eligible, slot))


def _check(got, want, margin, min_eligible, select=None, with_clear=True, what=()):
    thr, clear, frac, peak, eligible, slot = got
    rewritten = 0
    for u, (w_peak, w_elig, w_slot) in enumerate(want):
        at = (u,) + tuple(what)
        assert int(eligible[u]) == w_elig and int(slot[u]) == w_slot, (at, eligible[u], slot[u], w_elig, w_slot)
        assert _close(float(peak[u]), w_peak), (at, peak[u], w_peak)
        selected = select is None or bool(select[u])
        w_thr = ref.ring_threshold(123.456 + u, w_peak, w_elig, margin, min_eligible, selected)
        if w_thr == 123.456 + u:                                     # left out, starved or no eligible slot: its bits
            assert thr[u] == np.float64(u) + 123.456 and clear[u] == -7.0, (at, thr[u], clear[u])
            continue
        rewritten += 1
        assert _close(float(thr[u]), w_thr) and thr[u] == peak[u] * np.float64(margin), (at, thr[u], w_thr)
        assert clear[u] == (thr[u] * frac[u] if with_clear else -7.0), (at, clear[u])
    return rewritten


# n = 1 | 64 | 65 | 129: one lane of a sensor group, a full group, a second group of one, a third.  R = 64: the smallest
# ring, two tiles of 61 slots; 130: three tiles and an odd pitch.
@pytest.mark.parametrize("by_sensor", [False, True], ids=["tick", "sensor"])
@pytest.mark.parametrize("R", [64, 130])
@pytest.mark.parametrize("n", [1, 64, 65, 129])
def test_the_entry_point_equals_the_yardstick_over_sentinels(n, R, by_sensor, gpu_device):
    dev = gpu_device
    table = tables(torch.device("cpu"), gen(n, R), units=6 * len(PATTERNS) * len(PLANTS), n=n).numpy()
    combos, keys, keep, ticks, planted = _scenarios(n, R, by_sensor, 1000 * n + R + by_sensor, table)
    want = _expect(keys, keep, table, ticks, by_sensor)
    margin, min_eligible = 1.0625, 5
    rewritten = 0
    for u0 in range(0, len(combos), 3):                              # U = 3; every fourth call leaves its middle unit out
        select = [1, 0, 1] if (u0 // 3) % 4 == 1 else None
        cut = slice(u0, u0 + 3)
        got = _run(dev, keys[cut], keep[cut], table[cut], ticks[cut], by_sensor, margin, min_eligible, select)
        rewritten += _check(got, want[cut], margin, min_eligible, select, what=combos[u0])
    assert 0 < rewritten < len(combos)
    for u, (base, pattern, plant) in enumerate(combos):              # what the plants are there to show
        peak, eligible, slot = want[u]
        if pattern == "all":
            assert eligible == R - 3
            if plant == "base+3":
                assert slot == planted[u]                            # the first slot past the seam is counted
            if plant == "base+1":
                assert slot != planted[u] and slot in ((planted[u] + 1) % R, (planted[u] + 2) % R, (planted[u] - 1) % R)
        if pattern == "none":
            assert (peak, eligible, slot) == (-np.inf, 0, -1)
        if pattern == "runs":
            assert eligible <= 2                                     # below min_eligible: the sentinel stays
    # U = 1 (a single stream's call), without the clear pair
    for u in (0, 7, len(combos) - 1):
        cut = slice(u, u + 1)
        got = _run(dev, keys[cut], keep[cut], table[cut], ticks[cut], by_sensor, 1.0, 1, with_clear=False)
        _check(got, want[cut], 1.0, 1, with_clear=False, what=combos[u])


# 61 * 256 + 5 slots: 257 tiles per unit, so the finisher's threads take more than one partial each
@pytest.mark.parametrize("by_sensor", [False, True], ids=["tick", "sensor"])
def test_a_long_ring_folds_many_partials(by_sensor, gpu_device):
    dev, n, R = gpu_device, 3, 61 * 256 + 5
    rng = np.random.default_rng(R + by_sensor)
    keys = rng.random((3, n, R))
    keep = (rng.random((3, R)) < 0.9).astype(np.uint8)
    keep[2] = 1
    ticks = np.array([5 * R + R // 2, R - 1, 3 * R], dtype=np.int64)
    planted = [R - 1, 61 * 200 + 60, 0]                 # unit 2: base 0, slots 0 .. 2 straddle the seam; R - 1 holds three
    for u, q in enumerate(planted):
        for j, big in enumerate(BIG):
            keys[u, 1, (q - 3 + j) % R] = big
        keep[u, [(q - 3 + j) % R for j in range(4)]] = 1
    if by_sensor:
        keys.view(np.uint64)[:, 2, ::11] = ref.FILLER
    else:
        keys.view(np.uint64)[np.broadcast_to((keep == 0)[:, None, :], keys.shape)] = ref.FILLER
    table = tables(torch.device("cpu"), gen(R), units=3, n=n).numpy()
    want = _expect(keys, keep, table, ticks, by_sensor)
    assert [w[2] for w in want] == planted[:2] + [R - 1] and want[2][1] == R - 3
    got = _run(dev, keys, keep, table, ticks, by_sensor, 1.05, 64)
    assert _check(got, want, 1.05, 64) == 3


@pytest.mark.parametrize("n", [5, 129])
def test_the_peak_is_the_scorers_maximum_bit_for_bit(n, gpu_device):
    from gdn_amd import ops
    dev, R = gpu_device, 130
    g = gen(n, R)
    pred, gt = torch.rand((R, n), generator=g).to(dev), torch.rand((R, n), generator=g).to(dev)
    table = tables(dev, g, units=1, n=n)
    keys = ops.score_keys(pred, gt, R).view(1, n, R).contiguous()
    keep = torch.ones((1, R), dtype=torch.uint8, device=dev)
    _scores, anomaly = ops.score_smooth_max(pred, gt, table[0], want_scores=False)
    assert not bool(anomaly[:3].any()) and float(anomaly[3:].max()) > 0
    state = ops.fleet_state(torch.zeros((1, n, W), device=dev), W)              # ticks = 0: base 0
    thr = torch.zeros((1,), dtype=torch.float64, device=dev)
    peak, eligible, slot = thr.clone(), torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    ops.fleet_ring_threshold(state, keys, keep, table, W, 1.0, 1, ops.fleet_ring_threshold_workspace(1, R, dev), thr, peak,
                             eligible, slot)
    assert same(peak, anomaly[3:].max().view(1)) and same(thr, peak)
    assert int(eligible) == R - 3 and int(slot) == 3 + int(anomaly[3:].argmax())


# ------------------------------------------------------------------------------------------------ StreamDetector
def _period(n, t, g, missing, w):
    series = torch.rand((n, t), generator=g)
    if missing:
        hit = torch.rand(series.shape, generator=g) < 0.01
        hit[:, :w] = False                                           # the period begins on real readings
        series[hit] = float("nan")
    return series


@pytest.mark.parametrize("gaps", [False, True], ids=["plain", "sensor_gaps"])
def test_recalibrating_a_freshly_seeded_detector_gives_back_its_calibration(gaps, gpu_device):
    from gdn_amd import harness
    dev = gpu_device
    n, w = MSL[:2]
    model = model_on(dev, MSL)
    R = 130
    series = _period(n, w + R, gen(R, gaps), gaps, w).to(dev)
    kw = dict(gaps=True, calib_gaps=True, calib="sensor", min_kept=8) if gaps else {}
    # the precondition, on the evaluator's own output: the period's maximum sits at a tick >= 3
    if gaps:
        ev = harness.SeriesEvaluator(model, None, None, batch=8192, use_graph=False, series=series, gaps=True, min_kept=8,
                                     calib="sensor")
    else:
        ev = harness.SeriesEvaluator(model, None, series[:, w:].t().contiguous(), batch=8192, use_graph=False,
                                     series=series)
    anomaly = ev.step().clone()
    assert int(anomaly.argmax()) >= 3 and float(anomaly.max()) > 0 and not bool(anomaly[:3].any())
    assert int((anomaly == anomaly.max()).sum()) == 1
    det = harness.StreamDetector.from_calibration(model, series, 4, recal=R, recal_min=64, wide=False, use_graph=False,
                                                  **kw)
    assert det.ring_peak is None and det.recal_threshold is None     # off: nothing allocated
    table, threshold = det.med_iqr.clone(), det.threshold.clone()
    assert same(threshold, anomaly.max().view(1))
    if gaps:
        assert int((det.ring_keys.view(torch.int64) == -1).sum()) > 0
    det.threshold.fill_(-77.0)
    pointer = det.threshold.data_ptr()
    done = det.recalibrate(threshold=1.0)
    assert done == (n if gaps else R)
    assert same(det.med_iqr, table) and same(det.threshold, threshold) and det.threshold.data_ptr() == pointer
    assert same(det.ring_peak, threshold) and int(det.ring_eligible) == R - 3
    assert int(det.ring_peak_slot) == int(anomaly.argmax())          # R = T - w: slot = tick
    det.threshold.fill_(-77.0)
    det.recalibrate(threshold=False)                                 # the table only
    assert float(det.threshold) == -77.0
    det.recalibrate()                                                # the constructor's setting: off
    assert float(det.threshold) == -77.0


def _shifted(r, n, g, shift):
    return torch.rand((r, n), generator=g) + shift


def test_a_live_detector_follows_its_ring_through_the_same_graph(gpu_device):
    from gdn_amd import harness
    dev = gpu_device
    n, w = MSL[:2]
    model = model_on(dev, MSL)
    g = gen(77)
    R, chunk = 64, 8
    det = harness.StreamDetector(model, tables(dev, g, units=1, n=n)[0], 5.0, torch.rand((n, w), generator=g).to(dev),
                                 chunk, top_m=2, wide=False, recal=R, recal_min=8, exclude_alarms=False,
                                 recal_threshold=1.125, events=dict(on=1, off=1, lo=2.5, cap=32))
    assert same(det.clear_frac, torch.tensor([0.5], dtype=torch.float64, device=dev))
    for step in range(25):                                           # 200 ticks, the level moves half-way
        det.push(_shifted(chunk, n, g, 0.0 if step < 12 else 0.4).to(dev))
    graph = det.graph
    assert graph is not None
    thr_ptr, clear_ptr = det.threshold.data_ptr(), det.clear.data_ptr()
    kept = det.recalibrate()
    assert kept == R and det.recals == 1
    ticks = det.status()[0]
    want = ref.ring_peak(det.ring_keys.cpu().numpy(), det.ring_keep.cpu().numpy(), det.med_iqr.cpu().numpy(), ticks % R)
    assert ticks == 200 and want[1] == R - 3 == int(det.ring_eligible) and want[2] == int(det.ring_peak_slot)
    thr = float(det.threshold)
    assert _close(float(det.ring_peak), want[0]) and _close(thr, want[0] * 1.125) and thr != 5.0
    assert thr == float(det.ring_peak) * 1.125 and float(det.clear) == thr * 0.5
    assert det.threshold.data_ptr() == thr_ptr and det.clear.data_ptr() == clear_ptr
    # later pushes alarm against the new threshold through the same graph object
    flags = []
    for shift in (0.4, 0.4, 3.0, 0.4):
        scores, _sensors, alarm = det.push(_shifted(chunk, n, g, shift).to(dev))
        assert det.graph is graph
        assert torch.equal(alarm, (scores[:, 0] > thr).to(torch.int32))
        flags += alarm.tolist()
    assert 0 < sum(flags) < len(flags)
    table = det.episodes().numpy()
    assert table["count"] >= 1                                       # the episodes ran against the new levels


# ------------------------------------------------------------------------------------------------ StreamFleet
@pytest.mark.parametrize("options", ["plain", "sensor", "events"])
def test_the_fleet_writes_the_thresholds_of_one_detector_per_unit(options, gpu_device):
    from test_gpu_fleet_recal import OPTIONS, RECAL_MIN, UNITS, _assert_units_equal, _pair, _push_both, _ticks
    dev = gpu_device
    g = gen(len(options), 3)
    fleet, dets, n, _w = _pair(dev, OPTIONS[options], 8, g, recal_threshold=1.05)
    missing = fleet.with_gaps
    # unit 0 alarms on every tick (threshold 0): too few kept ticks; unit 2 is silent throughout
    script = [(8, [8, 8, 0, 8, 8]), (3, [3, 3, 0, 3, 3]), (8, [8, 5, 0, 8, 1]), (8, [8, 8, 0, 8, 8]), (8, [8, 8, 0, 8, 8])]
    for step, (r, counts) in enumerate(script):
        _push_both(fleet, dets, _ticks(UNITS, r, n, g, missing).to(dev), counts, 8, step)
    graph, before = fleet.graph, fleet.threshold.clone()
    fleet.recalibrate()
    done = [det.recalibrate() for det in dets]
    assert fleet.graph is graph
    _assert_units_equal(fleet, dets, "recalibrated")
    for u, det in enumerate(dets):
        assert same(fleet.threshold[u:u + 1], det.threshold), u
        if fleet.events is not None:
            assert same(fleet.clear[u:u + 1], det.clear), u
        if done[u]:
            assert same(fleet.ring_peak[u:u + 1], det.ring_peak), u
            assert int(fleet.ring_eligible[u]) == int(det.ring_eligible), u
            assert int(fleet.ring_peak_slot[u]) == int(det.ring_peak_slot), u
    assert same(fleet.threshold[2:3], before[2:3]) and int(fleet.ring_eligible[2]) == 0      # silent
    if fleet.calib == "tick":
        assert done[0] == 0 and same(fleet.threshold[0:1], before[0:1])                      # starved
        assert int(fleet.ring_eligible[0]) < RECAL_MIN
    assert done[3] and not same(fleet.threshold[3:4], before[3:4])                           # never alarmed: re-derived
    assert same(fleet.threshold[3:4], fleet.ring_peak[3:4] * 1.05)
    # a unit left out through units= keeps its threshold, the others are written again
    fleet.threshold.fill_(9.0)
    fleet.recalibrate(units=[0, 2, 3, 4])
    assert float(fleet.threshold[1]) == 9.0 and same(fleet.threshold[3:4], dets[3].threshold)
    fleet.recalibrate(threshold=False)                               # the tables only
    assert float(fleet.threshold[1]) == 9.0
    fleet.threshold.copy_(torch.cat([det.threshold for det in dets]))
    if fleet.events is not None:
        fleet.clear.copy_(torch.cat([det.clear for det in dets]))
    for step, (r, counts) in enumerate([(8, [8, 8, 0, 8, 8]), (2, [2, 1, 0, 2, 2])]):
        _push_both(fleet, dets, _ticks(UNITS, r, n, g, missing).to(dev), counts, 8, 100 + step)
        assert fleet.graph is graph
    _assert_units_equal(fleet, dets, "after")


# ------------------------------------------------------------------------------------------------ save / load
def test_saved_in_one_process_and_resumed_in_another_across_recalibrations(gpu_device, tmp_path):
    from _ring_threshold_worker import build, final, run
    want = {}
    for kind in ("detector", "fleet"):
        obj = build(kind, gpu_device)
        run(kind, obj, 0, gpu_device)
        run(kind, obj, 1, gpu_device)
        want[kind] = final(obj)
        assert obj.recals >= 2
    paths = [str(tmp_path / "det.npz"), str(tmp_path / "fleet.npz"), str(tmp_path / "out.npz")]
    for args in (["save"] + paths[:2], ["resume"] + paths):          # one fresh process per side of the cut
        done = subprocess.run([sys.executable, os.path.join(HERE, "_ring_threshold_worker.py")] + args, timeout=150,
                              capture_output=True, text=True)
        assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    from gdn_amd import harness
    assert harness.checkpoint_recal_threshold(harness.read_stream_checkpoint(paths[0])) == 1.05
    assert "clear_frac" in harness.read_stream_checkpoint(paths[1])
    with np.load(paths[2]) as got:
        for kind in want:
            for k, v in want[kind].items():
                a = got[f"{kind}/{k}"]
                assert a.dtype == v.dtype and a.shape == v.shape and a.tobytes() == v.tobytes(), (kind, k)
    # a file written with recal_threshold is refused, by field name, by a detector built without it
    det = build("detector", gpu_device, recal_threshold=None)
    with pytest.raises(ValueError, match="recal_threshold"):
        det.load_state_dict(harness.read_stream_checkpoint(paths[0]))
    fleet = build("fleet", gpu_device, recal_threshold=None)
    with pytest.raises(ValueError, match="recal_threshold"):
        fleet.load_state_dict(harness.read_stream_checkpoint(paths[1]))
    # ... and a file written without it loads as it always did
    sd = det.state_dict()
    assert "recal_threshold" not in sd and "clear_frac" not in sd
    det.load_state_dict(sd)


# ------------------------------------------------------------------------------------------------ off by default
@pytest.mark.parametrize("kind", ["detector", "fleet"])
def test_off_by_default_nothing_is_launched_and_the_threshold_stays(kind, gpu_device, monkeypatch):
    from _ring_threshold_worker import build, final, run
    from gdn_amd import _lib as binding
    names = []
    real_call = binding.call

    def spy(name, *args):
        names.append(name)
        return real_call(name, *args)
    monkeypatch.setattr(binding, "call", spy)
    off = build(kind, gpu_device, recal_threshold=None)
    threshold = off.threshold.clone()
    run(kind, off, 0, gpu_device)
    run(kind, off, 1, gpu_device)
    assert off.recals >= 2 and same(off.threshold, threshold)
    assert off.ring_peak is None and off.clear_frac is None and "gdn_fleet_ring_threshold" not in names
    old = build(kind, gpu_device, recal_threshold=None, old_api=True)   # the keyword never passed, recalibrate() bare
    run(kind, old, 0, gpu_device)
    run(kind, old, 1, gpu_device)
    a, b = final(off), final(old)
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    on = build(kind, gpu_device)
    run(kind, on, 0, gpu_device)
    assert "gdn_fleet_ring_threshold" in names and not same(on.threshold, threshold)
