"""GPU suite of the fleet archive evaluator: gdn_fleet_series_keys / _smooth_max / _smooth_topm and their
_gaps forms against the single-series launches per unit, and harness.FleetEvaluator against one SeriesEvaluator per
unit.  The arithmetic and its order per unit are the same, so every comparison is exact bits (`same`): no tolerance.

The evaluator cases run the MSL shape of tests/_fleet_case.py (n = 27, w = 15: the shape forward_series has a kernel
for) with U = 3 and T_raw = w + 45.  The rings are recal = 64, the smallest ring a fleet takes (64 <= R), so the 45
scored ticks seed a ring that is not full; gaps cases pass min_kept = 8, since 45 ticks cannot hold the default 64."""
import numpy as np
import pytest
import torch

from _fleet_case import MSL, assert_same_memory, gen, memory, model_on, same

pytestmark = pytest.mark.gpu

GDN_ERR_ARG, GDN_ERR_UNSUPPORTED = -1, -3
FAKE = 4096          # a non-null address that is never dereferenced: every refusal precedes the launch
UNITS, TICKS, RING, MIN_KEPT = 3, 45, 64, 8


def _planes(units, t, n, dev, *seed):
    g = gen(units, t, n, *seed)
    return torch.rand((units, t, n), generator=g).to(dev), torch.rand((units, t, n), generator=g).to(dev), g


# ------------------------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("units,t,n,m", [(3, 21, 5, 3), (2, 2, 5, 0), (3, 37, 130, 8), (2, 2100, 7, 0)])
def test_plain_launches_write_every_units_single_series_bits(units, t, n, m, gpu_device):
    from gdn_amd import ops
    dev = gpu_device
    pred, gt, _ = _planes(units, t, n, dev)
    for pitch in (t, t + 5):                                         # the filler in slots t .. pitch-1 too
        keys = ops.fleet_series_keys(pred, gt, pitch)
        assert keys.shape == (units, n, pitch)
        for u in range(units):
            assert same(keys[u], ops.score_keys(pred[u], gt[u], pitch)), (u, pitch)
    keys = ops.fleet_series_keys(pred, gt, t)
    counts = torch.full((units, n), t, dtype=torch.int32, device=dev)
    med_iqr = torch.full((units, n, 2), float("nan"), dtype=torch.float64, device=dev)
    ops.fleet_select_counts(keys, counts, 1, ops.fleet_select_workspace(units, n, t, dev), med_iqr)
    scores, anomaly = ops.fleet_series_smooth_max(pred, gt, med_iqr)
    only = ops.fleet_series_smooth_max(pred, gt, med_iqr, want_scores=False)
    assert only[0] is None and same(only[1], anomaly)
    assert scores.shape == (units, n, t) and anomaly.shape == (units, t)
    for u in range(units):
        table = ops.score_select(ops.score_keys(pred[u], gt[u], t), 1, n, t, t)
        assert same(med_iqr[u], table), u
        want_scores, want = ops.score_smooth_max(pred[u], gt[u], table)
        assert same(scores[u], want_scores) and same(anomaly[u], want), u
        assert bool((anomaly[u, :3] == 0.0).all()) and bool((scores[u, :, :3] == 0.0).all()), u     # every unit's own
    if t < 4:
        assert bool((anomaly == 0.0).all()) and bool((scores == 0.0).all())
    if m:
        top_scores, top_sensors = ops.fleet_series_smooth_topm(pred, gt, med_iqr, m)
        assert top_scores.shape == (units, t, m) and top_sensors.dtype == torch.int32
        assert same(top_scores[:, :, 0], anomaly)
        for u in range(units):
            ws, wi = ops.score_smooth_topm(pred[u], gt[u], med_iqr[u], m)
            assert same(top_scores[u], ws) and same(top_sensors[u], wi), u


def _gap_case(dev):
    units, t, n = 3, 21, 5
    pred, gt, g = _planes(units, t, n, dev, 7)
    valid = (torch.rand((units, t, n), generator=g) >= 0.1).to(torch.uint8)
    valid[0, -3:] = 0                                                # the LAST three rows of a unit ...
    valid[1, :3] = 0                                                 # ... and the FIRST three of its neighbour
    return pred, gt, valid.to(dev), units, t, n


def test_gaps_launches_write_every_units_bits_and_nothing_crosses_a_seam(gpu_device):
    from gdn_amd import ops
    dev = gpu_device
    pred, gt, valid, units, t, n = _gap_case(dev)
    m = 3
    keep = valid.all(dim=2).to(torch.uint8)
    by_tick = ops.fleet_series_keys(pred, gt, t, keep=keep)
    by_sensor = ops.fleet_series_keys(pred, gt, t, valid=valid)
    counts = valid.sum(dim=1).to(torch.int32)
    assert int(counts.min()) >= 1
    med_iqr = torch.full((units, n, 2), float("nan"), dtype=torch.float64, device=dev)
    ops.fleet_select_counts(by_sensor, counts, 1, ops.fleet_select_workspace(units, n, t, dev), med_iqr)
    scores, anomaly = ops.fleet_series_smooth_max(pred, gt, med_iqr, valid=valid)
    top_scores, top_sensors = ops.fleet_series_smooth_topm(pred, gt, med_iqr, m, valid=valid)
    for u in range(units):
        assert same(by_tick[u], ops.score_keys(pred[u], gt[u], t, keep=keep[u])), u
        solo_keys = ops.score_keys(pred[u], gt[u], t, valid=valid[u])
        assert same(by_sensor[u], solo_keys), u
        assert same(med_iqr[u], ops.score_select_counts(solo_keys, 1, n, t, counts[u], 1)), u
        want_scores, want = ops.score_smooth_max(pred[u], gt[u], med_iqr[u], valid=valid[u])
        assert same(scores[u], want_scores) and same(anomaly[u], want), u
        ws, wi = ops.score_smooth_topm(pred[u], gt[u], med_iqr[u], m, valid=valid[u])
        assert same(top_scores[u], ws) and same(top_sensors[u], wi), u
    # the seam in both directions: whatever the middle unit holds, its neighbours' bits stay
    pred2, gt2, valid2 = pred.clone(), gt.clone(), valid.clone()
    pred2[1], gt2[1], valid2[1] = pred[1] + 3.0, gt[1] * 0.5, 1 - valid[1]
    scores2, anomaly2 = ops.fleet_series_smooth_max(pred2, gt2, med_iqr, valid=valid2)
    top2, _ = ops.fleet_series_smooth_topm(pred2, gt2, med_iqr, m, valid=valid2)
    for u in (0, 2):
        assert same(scores2[u], scores[u]) and same(anomaly2[u], anomaly[u]) and same(top2[u], top_scores[u]), u
    assert not same(anomaly2[1], anomaly[1])
    # unit 1's first three rows are missing: its ticks 0 - 2 are zeros of its own, and its tick 3 sees only row 3
    assert bool((scores[1, :, :3] == 0.0).all())


def test_gaps_launches_with_every_byte_valid_write_the_plain_bits(gpu_device):
    from gdn_amd import ops
    dev = gpu_device
    pred, gt, _valid, units, t, n = _gap_case(dev)
    valid = torch.ones((units, t, n), dtype=torch.uint8, device=dev)
    keep = torch.ones((units, t), dtype=torch.uint8, device=dev)
    plain = ops.fleet_series_keys(pred, gt, t + 2)
    assert same(ops.fleet_series_keys(pred, gt, t + 2, keep=keep), plain)
    assert same(ops.fleet_series_keys(pred, gt, t + 2, valid=valid), plain)
    med_iqr = torch.rand((units, n, 2), generator=gen(3), dtype=torch.float64).to(dev)
    scores, anomaly = ops.fleet_series_smooth_max(pred, gt, med_iqr)
    gap_scores, gap_anomaly = ops.fleet_series_smooth_max(pred, gt, med_iqr, valid=valid)
    assert same(gap_scores, scores) and same(gap_anomaly, anomaly)
    top = ops.fleet_series_smooth_topm(pred, gt, med_iqr, 3)
    gap_top = ops.fleet_series_smooth_topm(pred, gt, med_iqr, 3, valid=valid)
    assert same(gap_top[0], top[0]) and same(gap_top[1], top[1])


def test_argument_refusals(gpu_device):
    from gdn_amd import _lib, ops
    dev = gpu_device
    lib = _lib.load()
    pred, gt, valid, units, t, n = _gap_case(dev)
    med_iqr = torch.ones((units, n, 2), dtype=torch.float64, device=dev)
    with pytest.raises(_lib.GdnHipError, match="gdn_fleet_series_smooth_topm"):
        ops.fleet_series_smooth_topm(pred, gt, med_iqr, 9)
    with pytest.raises(_lib.GdnHipError, match="gdn_fleet_series_smooth_topm"):
        ops.fleet_series_smooth_topm(pred, gt, med_iqr, 6)                                   # m > n = 5
    with pytest.raises(ValueError, match="exclude each other"):
        ops.fleet_series_keys(pred, gt, t, keep=valid.all(dim=2).to(torch.uint8), valid=valid)

    def keys(units=3, t=21, n=5, pitch=21, keep=None, valid=None):
        return lib.gdn_fleet_series_keys(FAKE, FAKE, keep, valid, units, t, n, pitch, FAKE, None)
    assert keys(keep=FAKE, valid=FAKE) == GDN_ERR_ARG
    assert keys(units=0) == GDN_ERR_UNSUPPORTED and keys(units=4097) == GDN_ERR_UNSUPPORTED
    assert keys(n=0) == GDN_ERR_UNSUPPORTED and keys(n=4097) == GDN_ERR_UNSUPPORTED
    assert keys(t=0) == GDN_ERR_ARG and keys(pitch=20) == GDN_ERR_ARG
    assert keys(units=64, t=2048, n=4096, pitch=2048) == GDN_ERR_UNSUPPORTED                 # a 4 GiB key block
    assert keys(units=32, t=2048, n=4096, pitch=2049) == GDN_ERR_UNSUPPORTED                 # just over 2 GiB
    assert lib.gdn_fleet_series_smooth_max(FAKE, FAKE, FAKE, 0, 21, 5, None, FAKE, None) == GDN_ERR_UNSUPPORTED
    assert lib.gdn_fleet_series_smooth_max(FAKE, FAKE, FAKE, 64, 2048, 4096, None, FAKE, None) == GDN_ERR_UNSUPPORTED
    assert lib.gdn_fleet_series_smooth_max_gaps(FAKE, FAKE, FAKE, 3, 21, 5, None, FAKE, None, None) == GDN_ERR_ARG
    assert lib.gdn_fleet_series_smooth_topm(FAKE, FAKE, FAKE, 3, 21, 5, 9, FAKE, FAKE, None) == GDN_ERR_UNSUPPORTED
    assert lib.gdn_fleet_series_smooth_topm(FAKE, FAKE, FAKE, 0, 21, 5, 3, FAKE, FAKE, None) == GDN_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ evaluator level
FORMS = {"plain": {}, "top_m": dict(top_m=3), "scores": dict(want_scores=True),
         "gaps": dict(gaps=True, min_kept=MIN_KEPT), "sensor": dict(gaps=True, min_kept=MIN_KEPT, calib="sensor")}


def _series(dev, gaps: bool, *seed):
    n, w = MSL[:2]
    g = gen(UNITS, TICKS, *seed)
    series = torch.rand((UNITS, n, w + TICKS), generator=g)
    if gaps:
        hit = torch.rand(series.shape, generator=g) < 0.02
        hit[:, :, :w] = False                                        # every unit begins on real readings
        series[hit] = float("nan")
        series[0, 2, -3:] = float("nan")                             # a unit that ends inside a run ...
        series[1, 2, w:w + 3] = float("inf")                         # ... and a neighbour whose scored ticks begin in one
    return series.to(dev), g


def _solo(model, series, u, batch, **form):
    from gdn_amd import harness
    w = MSL[1]
    if form.get("gaps"):
        return harness.SeriesEvaluator(model, None, None, batch, use_graph=False, series=series[u].contiguous(), **form)
    return harness.SeriesEvaluator(model, None, series[u][:, w:].t().contiguous(), batch, use_graph=False,
                                   series=series[u].contiguous(), **form)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_fleet_evaluator_step_is_every_units_series_evaluator_step(form, gpu_device):
    from gdn_amd import harness
    dev = gpu_device
    kw = FORMS[form]
    model = model_on(dev, MSL)
    series, _ = _series(dev, bool(kw.get("gaps")), len(form))
    fe = harness.FleetEvaluator(model, series, batch=16, **kw)       # three forward spans per unit
    anomaly = fe.step()
    assert anomaly.shape == (UNITS, TICKS) and fe.pred.shape == (UNITS, TICKS, MSL[0])
    first = {k: getattr(fe, k).clone() for k in ("pred", "med_iqr", "anomaly")}
    assert same(fe.step(), first["anomaly"]) and fe.graph is not None            # a replay: the same bits
    assert same(fe.pred, first["pred"]) and same(fe.med_iqr, first["med_iqr"])
    assert same(fe.thresholds(), fe.anomaly.amax(dim=1))
    if kw.get("gaps"):
        total, run = fe.status_gaps()
        assert total.shape == run.shape == (UNITS, MSL[0]) and fe.kept.shape == (UNITS,)
        assert same(fe.raw_series, series) and bool(torch.isfinite(fe.series).all())
    else:
        with pytest.raises(ValueError, match="gaps=False"):
            fe.status_gaps()
    for u in range(UNITS):
        ev = _solo(model, series, u, 16, **kw)
        want = ev.step()
        assert same(fe.pred[u], ev.pred) and same(fe.y[u], ev.y), u
        assert same(fe.med_iqr[u], ev.med_iqr) and same(fe.anomaly[u], want), u
        if form == "top_m":
            assert same(fe.top_scores[u], ev.top_scores) and same(fe.top_sensors[u], ev.top_sensors), u
        if form == "scores":
            assert same(fe.scores[u], ev.scores), u
        if kw.get("gaps"):
            assert int(fe.kept[u]) == ev.kept, u
            assert same(fe.series[u], ev.series) and same(fe.valid[u], ev.valid) and same(fe.keep[u], ev.keep), u
            solo_total, solo_run = ev.status_gaps()
            assert torch.equal(total[u], solo_total) and torch.equal(run[u], solo_run), u
        if form == "sensor":
            assert same(fe.counts[u], ev.counts), u
        else:
            assert fe.counts is None


def test_a_unit_is_what_localise_and_episodes_take(gpu_device):
    from gdn_amd import harness
    dev = gpu_device
    model = model_on(dev, MSL)
    series, _ = _series(dev, False, 11)
    fe = harness.FleetEvaluator(model, series, batch=64, top_m=3)
    fe.step()
    ev = _solo(model, series, 1, 64, top_m=3)
    ev.step()
    ticks = [0, 3, 17, TICKS - 1]
    got, want = harness.localise(fe.unit(1), ticks), harness.localise(ev, ticks)
    for name in want._fields:
        assert same(getattr(got, name), getattr(want, name)), name
    hi = float(ev.anomaly.median())
    got, want = harness.episodes(fe.unit(1), hi).numpy(), harness.episodes(ev, hi).numpy()
    assert want["count"] >= 1 and sorted(got) == sorted(want)
    for name in want:
        assert np.array_equal(got[name], want[name]), name
    with pytest.raises(ValueError, match="top_m"):
        harness.localise(harness.FleetEvaluator(model, series, batch=64, use_graph=False).unit(0), ticks)
    with pytest.raises(ValueError, match="outside"):
        fe.unit(UNITS)


@pytest.mark.parametrize("form", ["plain", "gaps", "sensor"])
def test_fleet_deploys_what_from_calibration_builds(form, gpu_device):
    from gdn_amd import harness
    dev = gpu_device
    kw = FORMS[form]
    model = model_on(dev, MSL)
    series, g = _series(dev, bool(kw.get("gaps")), 5, len(form))
    fe = harness.FleetEvaluator(model, series, batch=16, **kw)
    fe.step()
    got = fe.fleet(chunk=2, recal=RING)
    calib = dict(kw, calib_gaps=True) if kw else {}
    want = harness.StreamFleet.from_calibration(model, series, 2, recal=RING, **calib)
    assert_same_memory(memory(got), memory(want))
    assert (got.calib, got.recal, got.with_gaps, got.wide) == (want.calib, want.recal, want.with_gaps, want.wide)
    assert int(got.ring_keep.sum()) > 0 and bool((got.ring_keep[:, :RING - TICKS] == 0).all())    # a ring not yet full
    if kw:
        assert torch.equal(got.calib_kept, want.calib_kept)
    else:
        assert got.calib_kept is None and want.calib_kept is None
    ticks = torch.rand((UNITS, 2, MSL[0]), generator=g)
    if kw:
        ticks[1, 0, 3] = float("nan")
    ticks = ticks.to(dev)
    a, b = got.push(ticks), want.push(ticks)
    for x, y in zip(a, b):
        assert same(x, y)
    assert_same_memory(memory(got), memory(want))
