"""GPU suite of the streaming detector's rolling calibration: gdn_score_select on a key plane with the
filler scattered over its slots, gdn_stream_calib_write[_gaps] and harness.StreamDetector(recal=R) against
tests/_stream_recal_ref.py.  The ring is exact (torch.equal, bit patterns), the ring writer only reads the stream (a
recal=R detector that never recalibrates writes the bits of a recal=0 one), a recalibration is ONE select straight from
the ring, equal to gdn_score_quantiles over the kept rows, and the pushes after it equal a table switch between two
pushes.  Model shapes n = 5 and n = 70 (across the 64-sensor tile), 250 ticks, fixed seeds."""
import functools

import numpy as np
import pytest
import torch

import _stream_recal_ref as rref
from test_gpu_stream import PLANNED, _detector, _model

pytestmark = pytest.mark.gpu

T = 250
SHAPES = {"n5": (5, 4, 3, 16), "n70": (70, 6, 8, 16)}
SIZES = (1, 3, 37, 64, 65)               # pushes of a detector of chunk 64: 65 is split into 64 + 1


def _bits(t):
    return t.contiguous().view(torch.int64)


def _stream_of(shape, seed=0):
    n, w = SHAPES[shape][:2]
    g = torch.Generator().manual_seed(1000 + seed + 7 * n + w)
    return torch.rand((n, w), generator=g), torch.rand((T, n), generator=g)


@functools.lru_cache(maxsize=None)
def _threshold(shape):
    """The stream's top scores under _table, from ONE quiet detector (the scores do not depend on the push size):
    the threshold halfway between the two sorted scores at nine tenths, so that about one tick in ten alarms."""
    dev = torch.device("cuda:0")
    n, w = SHAPES[shape][:2]
    history, stream = _stream_of(shape)
    det = _detector(_model(dev, *SHAPES[shape]), history, w, 64, dev, top_m=min(3, n), use_graph=False)
    top = torch.cat([det.push(stream[t0:t0 + 64].to(dev))[0][:, 0].clone() for t0 in range(0, T, 64)])
    srt = top.sort().values
    k = int(0.9 * T)
    return float((srt[k - 1] + srt[k]) / 2)


def _build(shape, dev, chunk, **kw):
    n, w = SHAPES[shape][:2]
    history, stream = _stream_of(shape)
    kw.setdefault("threshold", _threshold(shape))
    det = _detector(_model(dev, *SHAPES[shape]), history, w, chunk, dev, top_m=min(3, n), **kw)
    return det, stream.to(dev)


def _drive(det, stream, sizes, start=0, stop=None, after=None):
    """Pushes of `sizes` (cycled) over stream[start:stop]; one record per SUB-push, taken as it returns: (pred, chunk,
    alarm, valid or None, top_scores, top_sensors, state).  `after(det)` runs after every sub-push."""
    rec = []
    inner = type(det)._push

    def spy(ticks):
        out = inner(det, ticks)
        r = det._last
        rec.append((det.pred[:r].clone(), det.chunk_buf[:r].clone(), det.alarm[:r].clone(),
                    det.valid[:r].clone() if det.valid is not None else None, det.top_scores[:r].clone(),
                    det.top_sensors[:r].clone(), det.state.clone()))
        if after is not None:
            after(det)
        return out
    det._push = spy
    stop = stream.shape[0] if stop is None else stop
    t0, i = start, 0
    while t0 < stop:
        r = min(sizes[i % len(sizes)], stop - t0)
        det.push(stream[t0:t0 + r])
        t0, i = t0 + r, i + 1
    del det._push
    return rec


def _cat(rec, j):
    return torch.cat([r[j] for r in rec])


def _ref_ring(rec, n, R, exclude=True, gaps=False, min_ticks=None):
    ring = rref.CalibRing(n, R, exclude_alarms=exclude, min_ticks=min_ticks)
    for r in rec:
        ring.push(r[0].cpu().numpy(), r[1].cpu().numpy(), r[2].cpu().numpy(),
                  r[3].cpu().numpy().astype(bool) if gaps else None)
    return ring


def _assert_ring(det, ring, what):
    assert torch.equal(det.ring_keep.cpu(), torch.from_numpy(ring.keep)), what
    assert torch.equal(_bits(det.ring_keys).cpu(), torch.from_numpy(rref.bits(ring.keys).view(np.int64))), what


# ------------------------------------------------------------------------------------------------ the select alone
@pytest.mark.parametrize("n,t,pitch", [(5, 50, 100), (5, 1500, 4096), (5, 20000, 34816), (70, 1500, 4096)],
                         ids=["finisher_only", "one_workgroup", "multi_launch", "one_workgroup_n70"])
def test_select_with_the_filler_scattered_over_the_slots(n, t, pitch, gpu_device):
    """No project code of the rolling calibration: the single-block select with total < pitch and the filler in
    arbitrary slots (so far: behind the keys, or in the middle through the multi-GPU exchange's blocks)."""
    from gdn_amd import ops
    dev = gpu_device
    g = torch.Generator().manual_seed(n + t)
    pred, gt = torch.rand((t, n), generator=g).to(dev), torch.rand((t, n), generator=g).to(dev)
    keys = ops.score_keys(pred, gt, t)
    slots = torch.randperm(pitch - 1, generator=g)[:t] + 1           # slot 0 holds the filler: the routes' "first key"
    plane = torch.full((n, pitch), -1, dtype=torch.int64, device=dev).view(torch.float64)
    plane[:, slots.to(dev)] = keys
    assert int((_bits(plane) == -1).sum()) == n * (pitch - t)
    before = plane.clone()
    got = ops.score_select(plane, 1, n, pitch, t)
    want = ops.score_quantiles(pred, gt)
    assert torch.equal(got, want), (n, t, pitch)
    assert torch.equal(_bits(plane), _bits(before))                  # the input is never written


# ------------------------------------------------------------------------------------------------ the ring
@pytest.mark.parametrize("exclude", [True, False], ids=["exclude_alarms", "keep_alarms"])
@pytest.mark.parametrize("R", [64, 100])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_ring_equals_the_reference_fed_the_detectors_own_records(shape, R, exclude, gpu_device):
    """Pushes of 1, 3, 37, 64 and 65 ticks: the ring wraps (R = 64 four times) and wraps inside a 64-row tile (the
    push of 64 from tick 41 crosses slot 63 | 0 and slot 99 | 0)."""
    dev = gpu_device
    n = SHAPES[shape][0]
    det, stream = _build(shape, dev, 64, recal=R, exclude_alarms=exclude)
    assert not det.ring_keep.any() and bool((_bits(det.ring_keys) == -1).all())          # empty at first
    rec = _drive(det, stream, SIZES)
    assert [len(r[2]) for r in rec] == [1, 3, 37, 64, 64, 1, 1, 3, 37, 39] and det.graph is not None
    alarm = _cat(rec, 2)
    assert 1 <= int((alarm != 0).sum()) < T // 2
    ring = _ref_ring(rec, n, R, exclude)
    assert ring.ticks == T == det.status()[0]
    _assert_ring(det, ring, (shape, R, exclude))
    last = alarm[T - R:] != 0
    assert int(det.ring_keep.sum()) == (R - int(last.sum()) if exclude else R)
    assert bool(last.any())                                          # an alarmed tick is among the last R


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_ring_writer_only_reads_the_stream(shape, use_graph, gpu_device):
    dev = gpu_device
    plain, stream = _build(shape, dev, 37, use_graph=use_graph)
    rolling, _ = _build(shape, dev, 37, use_graph=use_graph, recal=64)
    a, b = _drive(plain, stream, SIZES), _drive(rolling, stream, SIZES)
    assert len(a) == len(b) > 10
    for pa, pb in zip(a, b):                                         # after every (sub-)push
        for j in (0, 1, 2, 4, 5, 6):
            assert torch.equal(pa[j], pb[j]), (j, use_graph)
    assert torch.equal(plain.log_ticks, rolling.log_ticks) and torch.equal(plain.log_sensors, rolling.log_sensors)
    assert plain.status()[:2] == rolling.status()[:2] and plain.status()[1] > 0
    assert (rolling.graph is not None) == use_graph == (plain.graph is not None)
    assert plain.ring_keys is None and int(rolling.ring_keep.sum()) > 0
    with pytest.raises(ValueError, match="recal=0"):
        plain.recalibrate()


# ------------------------------------------------------------------------------------------------ the ring write alone
@pytest.mark.parametrize("n", rref.STAGE_N)
@pytest.mark.parametrize("mode", ["plain", "gaps", "sensor"])
def test_one_ring_write_launch_equals_numpy_from_a_staged_tick_counter(mode, n, gpu_device):
    """ops.stream_calib_write alone, against numpy (tests/_stream_recal_ref.py, tests/_sensor_calib_ref.py's ring) and
    no device code: the one body a stream and a fleet's units share has no other anchor outside itself.  One launch
    per (count = c, R, staged tick counter, exclude_alarms) onto a ring full of a sentinel: keys as bit patterns, keep
    flags, exactly `count` keep bytes changed, the state as it was.  (tests/test_cpu_stream_recal.py shows on the
    reference alone that every (mode, n) here meets a kept tick and a filler.)"""
    from gdn_amd import ops
    dev = gpu_device
    met_kept = met_filler = False
    for count, R in rref.STAGE_COUNT_R:
        pred, chunk, alarm, valid = rref.stage_inputs(n, count)
        assert alarm[0] != 0 or count == 1
        assert alarm[-1] == 0 and valid[-1].all() and (count == 1 or not valid[0].all())
        on_dev = [torch.from_numpy(a).to(dev) for a in (pred, chunk, alarm, valid)]
        for ticks in rref.stage_ticks(count, R):
            for exclude in (True, False):
                what = (mode, n, count, R, ticks, exclude)
                want_keys, want_keep = rref.stage_ring(mode, n, R, ticks, exclude, pred, chunk, alarm, valid)
                state = ops.stream_state_empty(n, 1, dev)
                state[0] = ticks
                before = state.clone()
                ring_keys, ring_keep = ops.stream_calib_ring(n, R, dev)
                ring_keys.fill_(rref.SENTINEL_KEY)
                ring_keep.fill_(rref.SENTINEL_KEEP)
                ops.stream_calib_write(state, on_dev[0], on_dev[1], on_dev[2], ring_keys, ring_keep, exclude,
                                       count=count, valid=None if mode == "plain" else on_dev[3],
                                       by_sensor=mode == "sensor")
                got_keys, got_keep = _bits(ring_keys).cpu().numpy(), ring_keep.cpu().numpy()
                np.testing.assert_array_equal(got_keys, want_keys.view(np.int64), err_msg=str(what))
                np.testing.assert_array_equal(got_keep, want_keep, err_msg=str(what))
                assert int((got_keep != rref.SENTINEL_KEEP).sum()) == count, what
                assert torch.equal(state, before), what
                met_kept |= bool((want_keep == 1).any())
                met_filler |= bool((want_keys == rref.FILLER_BITS).any())
    assert met_kept and met_filler, (mode, n)


# ------------------------------------------------------------------------------------------------ recalibrate
def _device_order_switch(delta, tables, sizes, m, threshold):
    """_stream_recal_ref.run_switched with the normalised error as the kernels round it, (delta - med) * (1 / den)
    (one reciprocal per sensor, then a product: DESIGN §3.8), so that the float64 results can be compared bit for
    bit.  `sizes`: the ticks of every push, in order; a switch falls between two of them."""
    state = rref.SwitchedStreamRef(tables[0][1], m, threshold)
    switch = dict(tables)
    outs, t0 = [], 0
    for r in sizes:
        if t0 in switch:
            state.switch(switch[t0])
        outs.append(_push_normalised(state, (delta[t0:t0 + r] - state.med) * (1.0 / state.den)))
        t0 += r
    return tuple(np.concatenate([o[j] for o in outs]) for j in range(4))


def _push_normalised(state, a):
    """StreamRef.push from the normalised errors on (the same lines, without the division)."""
    ext = np.vstack([state.carry, a])
    sm = (((ext[:-3] + ext[1:-2]) + ext[2:-1]) + ext[3:]) / 4.0
    sm[np.arange(len(a)) + state.ticks < 3] = 0.0
    idx = np.argsort(-sm, axis=1, kind="stable")[:, :state.m]
    vals = np.take_along_axis(sm, idx, axis=1)
    with np.errstate(invalid="ignore"):
        flags = vals[:, 0] > state.threshold
    state.carry = ext[-3:].copy()
    state.ticks += len(a)
    return sm, vals, idx, flags


@pytest.mark.parametrize("shape", list(SHAPES))
def test_recalibrate_is_one_select_from_the_ring_and_a_table_switch_for_the_next_pushes(shape, gpu_device):
    from gdn_amd import ops
    dev = gpu_device
    n = SHAPES[shape][0]
    R, cut, m = 100, 150, min(3, n)
    thr = _threshold(shape)
    det, stream = _build(shape, dev, 64, recal=R)
    by_hand, _ = _build(shape, dev, 64)                              # recal=0: its table is switched by hand below
    rec = _drive(det, stream, SIZES, stop=cut)
    hand = _drive(by_hand, stream, SIZES, stop=cut)
    graph, table0 = det.graph, det.med_iqr.clone()
    assert graph is not None and det.calibration()[1] == 0
    total = det.recalibrate()
    assert total == int(det.ring_keep.sum()) >= det.recal_min == 64 and det.graph is graph
    assert (det.recals, det.recal_kept) == (1, total) and det.calibration()[1] == total
    pred, gt, alarm = _cat(rec, 0), _cat(rec, 1), _cat(rec, 2)
    kept = torch.nonzero(alarm[cut - R:] == 0).view(-1) + (cut - R)
    assert len(kept) == total < R
    assert torch.equal(det.med_iqr, ops.score_quantiles(pred[kept].contiguous(), gt[kept].contiguous()))
    assert torch.equal(det.calibration()[0], det.med_iqr) and not torch.equal(det.med_iqr, table0)
    np.testing.assert_array_equal(det.med_iqr.cpu().numpy(), _ref_ring(rec, n, R).table())
    assert float(det.threshold) == thr                               # the threshold is the caller's
    # the next pushes: a recal=0 detector whose table is overwritten at the same tick, bit for bit ...
    by_hand.med_iqr.copy_(det.med_iqr)
    rec2 = _drive(det, stream, SIZES, start=cut)
    hand2 = _drive(by_hand, stream, SIZES, start=cut)
    assert det.graph is graph
    for pa, pb in zip(rec + rec2, hand + hand2):
        for j in (0, 2, 4, 5, 6):
            assert torch.equal(pa[j], pb[j]), j
    # ... and the float64 table-switch reference on the recorded predictions, in the kernels' operation order
    both = rec + rec2
    delta = rref.keys_of(_cat(both, 0).cpu().numpy(), _cat(both, 1).cpu().numpy())
    tables = [(0, table0.cpu().numpy()), (cut, det.med_iqr.cpu().numpy())]
    _sm, vals, idx, flags = _device_order_switch(delta, tables, [len(r[2]) for r in both], m, thr)
    got = _cat(both, 4).cpu().numpy()
    print(f"{shape}: worst |top score - float64 table-switch reference| {np.abs(got - vals).max():.3e}")
    assert torch.equal(_cat(both, 4).cpu(), torch.from_numpy(vals))
    assert torch.equal(_cat(both, 5).cpu(), torch.from_numpy(idx.astype(np.int32)))
    assert _cat(both, 2).cpu().numpy().astype(bool).tolist() == flags.tolist() and flags[:cut].any()
    # the division form of tests/_stream_ref.py (run_switched) agrees at the scoring suite's float64 bar
    _sm, vals_div, _idx, _flags, _state = rref.run_switched(delta, tables, 5, m=m, threshold=thr)
    np.testing.assert_allclose(got, vals_div, rtol=1e-12, atol=1e-13)


def test_with_too_few_kept_ticks_recalibrate_writes_nothing(gpu_device):
    dev = gpu_device
    det, stream = _build("n5", dev, 16, recal=64, recal_min=60)
    _drive(det, stream, (16,), stop=59)
    before = det.med_iqr.clone()
    assert det.recalibrate() == 0 and torch.equal(_bits(det.med_iqr), _bits(before)) and det.recals == 0
    det, stream = _build("n5", dev, 16, recal=64, recal_min=60, exclude_alarms=False)
    _drive(det, stream, (16,), stop=60)
    assert det.recalibrate() == 60 and not torch.equal(det.med_iqr, before)


# ------------------------------------------------------------------------------------------------ seeding
def test_from_calibration_seeds_the_ring_with_the_last_calibration_ticks(gpu_device):
    """At the SWaT shape (two sensor tiles, the second ragged): from_calibration's SeriesEvaluator runs the fused
    series forward, which has no kernel at the d = 16 shapes of the other tests."""
    from gdn_amd import harness, ops
    dev = gpu_device
    n, w = PLANNED[:2]
    model = _model(dev, *PLANNED)
    t = 200
    normal = torch.rand((n, w + t), generator=torch.Generator().manual_seed(31 + n)).to(dev)
    gt = normal[:, w:].t().contiguous()
    ev = harness.SeriesEvaluator(model, None, gt, batch=8192, use_graph=False, series=normal)
    ev.step()
    det = harness.StreamDetector.from_calibration(model, normal, 16, top_m=min(3, n), recal=256)      # R >= T - w
    assert torch.equal(det.med_iqr, ev.med_iqr)
    assert det.ring_keep.cpu().tolist() == [0] * 56 + [1] * 200
    assert torch.equal(det.ring_keys[:, 56:], ops.score_keys(ev.pred, gt, t))            # oldest first
    assert bool((_bits(det.ring_keys[:, :56]) == -1).all())
    det.med_iqr.zero_()
    assert det.recalibrate() == t and torch.equal(det.med_iqr, ev.med_iqr)               # bit for bit
    det = harness.StreamDetector.from_calibration(model, normal, 16, top_m=min(3, n), recal=100)      # R < T - w
    assert det.ring_keep.cpu().tolist() == [1] * 100
    assert torch.equal(det.ring_keys, ops.score_keys(ev.pred[-100:], gt[-100:], 100))
    assert det.recalibrate() == 100
    assert torch.equal(det.med_iqr, ops.score_quantiles(ev.pred[-100:], gt[-100:]))
    # the stream starts at slot 0: three ticks replace the three oldest seeded ticks
    det.exclude_alarms = False
    more = torch.rand((3, n), generator=torch.Generator().manual_seed(32)).to(dev)
    det.push(more)
    assert torch.equal(det.ring_keys[:, :3], ops.score_keys(det.pred[:3], more, 3))
    assert torch.equal(det.ring_keys[:, 3:], ops.score_keys(ev.pred[-97:], gt[-97:], 97)) and bool(det.ring_keep.all())


# ------------------------------------------------------------------------------------------------ missing readings
def test_with_gaps_an_incomplete_tick_is_not_kept_and_clean_ticks_give_the_plain_ring(gpu_device):
    from gdn_amd import ops
    dev = gpu_device
    shape, R = "n5", 100
    n = SHAPES[shape][0]
    det, stream = _build(shape, dev, 64, recal=R, gaps=True)
    holes = torch.rand(stream.shape, generator=torch.Generator().manual_seed(5)) < 0.03   # about 3 % of the readings
    raw = stream.clone()
    raw[holes.to(dev)] = float("nan")
    rec = _drive(det, raw, SIZES)
    valid, alarm = _cat(rec, 3).bool(), _cat(rec, 2)
    complete = valid.all(dim=1)
    assert torch.equal(complete.cpu(), ~holes.any(dim=1)) and 5 <= int((~complete[T - R:]).sum())
    assert 1 <= int((alarm != 0).sum()) < T // 2
    kept = complete & (alarm == 0)
    assert int(kept[T - R:].sum()) >= det.recal_min == 64            # enough complete, quiet ticks to recalibrate
    ring = _ref_ring(rec, n, R, gaps=True)
    _assert_ring(det, ring, "gaps")
    for tick in torch.nonzero(~complete[T - R:]).view(-1).tolist():  # an incomplete tick's slot: all filler, keep 0
        slot = (T - R + tick) % R
        assert int(det.ring_keep[slot]) == 0 and bool((_bits(det.ring_keys[:, slot]) == -1).all())
    assert det.recalibrate() == int(kept[T - R:].sum())
    rows = torch.nonzero(kept[T - R:]).view(-1) + (T - R)
    assert torch.equal(det.med_iqr, ops.score_quantiles(_cat(rec, 0)[rows].contiguous(), _cat(rec, 1)[rows].contiguous()))
    # without a missing reading: the ring and the table of a gaps=False detector
    gappy, _ = _build(shape, dev, 64, recal=R, gaps=True)
    plain, _ = _build(shape, dev, 64, recal=R)
    _drive(gappy, stream, SIZES)
    _drive(plain, stream, SIZES)
    assert torch.equal(gappy.ring_keep, plain.ring_keep) and torch.equal(_bits(gappy.ring_keys), _bits(plain.ring_keys))
    assert gappy.recalibrate() == plain.recalibrate() > 0 and torch.equal(gappy.med_iqr, plain.med_iqr)


# ------------------------------------------------------------------------------------------------ recal_every
def test_recal_every_recalibrates_after_the_sub_pushes_that_cross_a_multiple(gpu_device):
    dev = gpu_device
    shape, E = "n5", 50
    kw = dict(recal=64, recal_min=16)
    det, stream = _build(shape, dev, 16, recal_every=E, **kw)
    by_hand, _ = _build(shape, dev, 16, **kw)
    calls = []
    inner = type(det).recalibrate
    det.recalibrate = lambda: calls.append((det._handed, inner(det)))
    _drive(det, stream, (37,))                                       # pushes of 37 = sub-pushes of 16, 16 and 5
    del det.recalibrate
    want, handed = [], 0
    for t0 in range(0, T, 37):
        for s in range(t0, min(T, t0 + 37), 16):
            r = min(16, min(T, t0 + 37) - s)
            if (handed + r) // E > handed // E:
                want.append(handed + r)
            handed += r
    assert want == [53, 106, 164, 201, 250] and [c[0] for c in calls] == want
    assert all(c[1] >= 16 for c in calls) and det.recals == 5 and det.recal_kept == calls[-1][1]

    def at_the_same_ticks(d):
        if d.status()[0] in want:
            d.recalibrate()
    _drive(by_hand, stream, (37,), after=at_the_same_ticks)
    assert by_hand.recals == 5 and torch.equal(by_hand.med_iqr, det.med_iqr)
    assert torch.equal(by_hand.state, det.state) and torch.equal(_bits(by_hand.ring_keys), _bits(det.ring_keys))
