"""What tests/test_gpu_fleet_prep_units.py and tests/test_gpu_fleet_handover.py share: per-unit prep tables
for the fleet of tests/_fleet_case.py, a driver that pushes a fleet and one detector per unit the same rows in the same
cuts, and the comparison of one unit's memory with a detector's."""
import torch

from _fleet_case import CHUNK, DOWN, LOG, N, TOP_M, UNITS, same, setup

ALL = dict(gaps=True, events=dict(on=2, off=2, cap=8), recal=64, recal_min=8, recal_every=8, calib="sensor",
           recal_threshold=1.5)


def make_prep_units(dev, down=DOWN, n=N, units=UNITS):
    """A min-max table per unit: unit u's duty point lies 5 u higher and its range is 100 + 10 u wide, so no two units
    share a scale or an offset and _fleet_case.raw_ticks stays within about [0, 1] under each."""
    from gdn_amd.prep import Prep, PrepUnits
    preps = []
    for u in range(units):
        lo = 50.0 + 10.0 * torch.arange(n, dtype=torch.float64) - 5.0 * u
        scale = torch.full((n,), 1.0 / (100.0 + 10.0 * u), dtype=torch.float64)
        stats = torch.stack([lo, lo + 100.0 + 10.0 * u, lo + 50.0, torch.full((n,), 1000.0, dtype=torch.float64)], dim=1)
        preps.append(Prep(torch.stack([scale, 0.0 - lo * scale], dim=1).to(dev), stats.to(dev), down))
    return PrepUnits.from_preps(preps)


def build(dev, kw, prep=None, use_graph=True, seed=1):
    """(model, fleet, (med_iqr, threshold, history)) of _fleet_case.setup under the options `kw`."""
    from gdn_amd import harness
    model, med_iqr, threshold, history = setup(dev, seed)
    fleet = harness.StreamFleet(model, med_iqr, threshold, history, CHUNK, top_m=TOP_M, log=LOG, wide=False,
                                use_graph=use_graph, prep=prep, **kw)
    return model, fleet, (med_iqr, threshold, history)


def detector(model, med_iqr, threshold, history, kw, prep=None):
    from gdn_amd import harness
    return harness.StreamDetector(model, med_iqr, float(threshold), history.contiguous(), CHUNK, top_m=TOP_M, log=LOG,
                                  wide=False, use_graph=False, prep=prep, **kw)


def detectors(model, fleet, seeds, kw):
    med_iqr, threshold, history = seeds
    return {u: detector(model, med_iqr[u], threshold[u], history[u], kw, fleet.unit_prep(u)) for u in range(fleet.units)}


def each_count(counts, r, units=UNITS):
    return [r] * units if counts is None else [int(v) for v in (counts.tolist() if torch.is_tensor(counts) else counts)]


def push_both(fleet, dets, ticks, counts=None):
    """fleet.push(ticks, counts), and every detector of `dets` (unit -> detector) its unit's real rows of every cut the
    fleet makes.  Returns the fleet's views and, per unit, the views of the detector's last push."""
    got = fleet.push(ticks, counts)
    span = CHUNK * (fleet.prep.down if fleet.prep is not None else 1)
    r = ticks.shape[1]
    each = each_count(counts, r, fleet.units)
    last = {}
    for s in range(0, r, span):
        rows = min(span, r - s)
        for u, det in dets.items():
            k = min(max(each[u] - s, 0), rows)
            if k:
                last[u] = det.push(ticks[u, s:s + k].contiguous())
    return got, last


def assert_unit_is(fleet, u, det, what=""):
    """Unit u's block of everything the fleet remembers equals the detector's memory, bit for bit."""
    from gdn_amd import ops
    assert torch.equal(fleet.unit_state(u), det.state), (what, u, "state")
    assert same(fleet.med_iqr[u], det.med_iqr), (what, u, "med_iqr")
    assert same(fleet.threshold[u:u + 1], det.threshold.view(1)), (what, u, "threshold")
    assert torch.equal(fleet.log_ticks[u], det.log_ticks) and torch.equal(fleet.log_sensors[u], det.log_sensors), (what, u)
    if fleet.with_gaps:
        assert torch.equal(fleet.gaps[u], det.gaps), (what, u, "gaps")
    if fleet.recal:
        assert same(fleet.ring_keys[u], det.ring_keys) and torch.equal(fleet.ring_keep[u], det.ring_keep), (what, u, "ring")
    if fleet.events is not None:
        assert torch.equal(fleet.events[u], det.events) and same(fleet.clear[u:u + 1], det.clear), (what, u, "events")
        if fleet.clear_frac is not None and det.clear_frac is not None:
            assert same(fleet.clear_frac[u:u + 1], det.clear_frac.view(1)), (what, u, "clear_frac")
    if fleet.prep is not None:
        ticks, words = ops.fleet_prep_views(fleet.pend, fleet.units, fleet.n, fleet.prep.down)
        p = det.raw_pending
        assert words[u].tolist() == [p] * words.shape[1], (what, u, "pending")
        assert same(ticks[u, :p], det._pend[det._pend_at][:p]), (what, u, "open group")


def unit_memory(mem, u):
    """Unit u's part of _fleet_case.memory(fleet)."""
    out = {}
    for k, v in mem.items():
        if k.startswith("pending_ticks"):
            if k == f"pending_ticks{u}":
                out["pending_ticks"] = v
        else:
            out[k] = v[u]
    return out
