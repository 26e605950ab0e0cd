"""GPU suite of the fleet's missing readings and alarm episodes: gdn_fleet_fill / _score_gaps / _advance_gaps / _events and
harness.StreamFleet(gaps=, events=).  The yardstick is never the code under test: every fleet launch is compared with the
single-stream ops.stream_* launch on each unit's slice (the episodes with tests/_episodes_ref.py's sequential definition
too), and StreamFleet with U StreamDetectors pushed each unit's real rows in the same cuts.  The arithmetic and its order
per unit are the same, so every comparison is exact: torch.equal, float64 on its bit patterns.  No tolerance."""
import numpy as np
import pytest
import torch

import _episodes_ref as ref
from test_gpu_fleet import (CHUNK, LOG, SHAPES, TICKS, TOP_M, UNITS, _gen, _i32, _model, _outputs,
                            _real_rows_of_last_cut, _same, _staged_fleet, _tables)

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


def _with_missing(values, g, share=0.3):
    """`values` with about `share` of its entries replaced by NaN, +inf and -inf in turn (host tensor in, host out)."""
    hit = torch.rand(values.shape, generator=g) < share
    kind = torch.randint(0, 3, values.shape, generator=g)
    out = values.clone()
    for k, bad in enumerate((NAN, INF, -INF)):
        out[hit & (kind == k)] = bad
    return out


def _clamped(counts, c):
    return [min(max(int(v), 0), c) for v in counts]


# ------------------------------------------------------------------------------------------------ fill
# c = 8 | 9 and 32 | 33: the borders between the workgroups of 1, 4 and 16 waves (8 is also DEPTH); 17 and 129: ragged
# row segments; n = 64 | 65: one sensor group | a second one of one lane
@pytest.mark.parametrize("c", [1, 8, 9, 17, 32, 33, 129])
@pytest.mark.parametrize("n", [1, 64, 65, 130])
def test_fill_equals_the_single_stream_launch_per_unit_and_other_rows_are_untouched(n, c, gpu_device):
    from gdn_amd import ops
    dev, w, units = gpu_device, 4, 5
    g = _gen(n, c, 7)
    state = ops.fleet_state(torch.rand((units, n, w + 1), generator=g).to(dev), w)
    hist = ops.fleet_state_views(state, units, n, w)[2]
    before = state.clone()
    for counts in ([c, c - 1, (c + 1) // 2, 1, 0], [c + 5, -3, c, 0, 1]):
        real = _clamped(counts, c)
        raw = _with_missing(torch.rand((units, c, n), generator=g), g)
        raw[0, :, n - 1] = NAN                                       # a sensor missing in every row of unit 0
        raw[2, 0, 0] = 0.25                                          # ... and one that starts on a real reading
        for u, cnt in enumerate(real):
            raw[u, cnt:] = torch.tensor([NAN, INF, -INF])[u % 3]     # not readings at all: rows at or beyond the count
        raw = raw.to(dev)
        got = (torch.full((units, c, n), -7.0, device=dev), torch.full((units, c, n), 9, dtype=torch.uint8, device=dev),
               torch.full((units, 2, n), -7, dtype=torch.int32, device=dev))
        want = tuple(t.clone() for t in got)
        ops.fleet_fill(state, raw, _i32(counts, dev), w, *got)
        for u, cnt in enumerate(real):
            if cnt:
                ops.stream_fill(state[u], raw[u], w, want[0][u], want[1][u], want[2][u], count=cnt)
        for a, b, what in zip(got, want, ("filled", "valid", "gap_chunk")):
            assert _same(a, b), (what, counts)
        for u, cnt in enumerate(real):                               # rows at or beyond the count: the sentinel
            assert (got[0][u, cnt:] == -7).all() and (got[1][u, cnt:] == 9).all(), (u, counts)
            assert bool(torch.isfinite(got[0][u, :cnt]).all()) and bool((got[1][u, :cnt] <= 1).all())
            if cnt == 0:
                assert (got[2][u] == -7).all(), (u, counts)          # a silent unit: gap_chunk too
        cnt = real[0]                                                # the dead sensor holds hist[i, w - 1]
        assert (got[0][0, :cnt, n - 1] == hist[0, n - 1, w - 1]).all() and not got[1][0, :cnt, n - 1].any()
        assert got[2][0, :, n - 1].tolist() == [cnt, cnt]
        if real[2]:
            assert got[0][2, 0, 0] == 0.25 and got[1][2, 0, 0] == 1
    assert torch.equal(state, before)                                # the launch reads the states


# ------------------------------------------------------------------------------------------------ score / advance
@pytest.mark.parametrize("c", [1, 9, 17])
@pytest.mark.parametrize("n", [1, 65, 129])
def test_score_and_advance_with_gaps_equal_the_single_stream_launches_per_unit(n, c, gpu_device):
    from gdn_amd import ops
    dev, w, log_len = gpu_device, 4, 8
    g = _gen(n, c, 11)
    units = len(TICKS)
    state, med_iqr, thr, chunk, pred = _staged_fleet(n, w, c, dev, g)
    for m in sorted({1, min(3, n)}):
        state_m, ref_state = state.clone(), state.clone()
        gaps = torch.zeros((units, 2, n), dtype=torch.int64, device=dev)
        logs = (torch.full((units, log_len), -1, dtype=torch.int64, device=dev),
                torch.full((units, log_len, m), -1, dtype=torch.int32, device=dev))
        ref_gaps, ref_logs = gaps.clone(), tuple(t.clone() for t in logs)
        for counts in ([c, c, c, (c + 1) // 2, 1, 0], [0, 1, c - 1, c, c, c]):
            raw = _with_missing(chunk.cpu(), g)
            raw[3, 0, 0] = NAN                                       # (real in both rounds, whatever the draw)
            raw = raw.to(dev)
            filled, valid = torch.zeros_like(raw), torch.zeros(raw.shape, dtype=torch.uint8, device=dev)
            gap_chunk = torch.zeros((units, 2, n), dtype=torch.int32, device=dev)
            ops.fleet_fill(state_m, raw, _i32(counts, dev), w, filled, valid, gap_chunk)      # (checked above)
            got, want = _outputs(units, c, m, dev), _outputs(units, c, m, dev)
            ops.fleet_score(state_m, pred, filled, med_iqr, thr, _i32(counts, dev), w, m, *got, valid=valid)
            for u, cnt in enumerate(counts):
                if cnt:
                    ops.stream_score(ref_state[u], pred[u], filled[u], med_iqr[u], thr[u:u + 1], m, want[0][u],
                                     want[1][u], want[2][u], count=cnt, valid=valid[u])
            for a, b, what in zip(got, want, ("top_scores", "top_sensors", "alarm")):
                assert _same(a, b), (what, m, counts)                # rows at or beyond counts[u]: the sentinel in both
            assert torch.equal(state_m, ref_state)                   # the score launch reads the states
            held = (state_m.clone(), gaps.clone(), logs[0].clone(), logs[1].clone())
            ops.fleet_advance(state_m, filled, pred, med_iqr, got[2], got[1], _i32(counts, dev), w, m, *logs,
                              valid=valid, gap_chunk=gap_chunk, gaps=gaps)
            for u, cnt in enumerate(counts):
                if cnt:
                    ops.stream_advance(ref_state[u], filled[u], pred[u], med_iqr[u], got[2][u], got[1][u], w, m,
                                       ref_logs[0][u], ref_logs[1][u], count=cnt, valid=valid[u],
                                       gap_chunk=gap_chunk[u], gaps=ref_gaps[u])
            assert torch.equal(state_m, ref_state), (m, counts)      # counters, carry and hist of every unit
            assert torch.equal(gaps, ref_gaps), (m, counts)
            assert torch.equal(logs[0], ref_logs[0]) and torch.equal(logs[1], ref_logs[1]), (m, counts)
            for u, cnt in enumerate(counts):
                if cnt == 0:                                         # a silent unit: every byte as it was
                    for now, then in zip((state_m, gaps, logs[0], logs[1]), held):
                        assert torch.equal(now[u], then[u]), (u, counts)
        assert int(gaps[:, 0].sum()) > 0                             # readings were missing: the counters moved


# ------------------------------------------------------------------------------------------------ events
EV_UNITS, EV_FIRST = 3, [0, 5, 1000]
EV_HI, EV_LO = [1.0, 1.0, 2.0], [0.5, 1.0, -1.0]                     # unit 1: no hysteresis; unit 2: a negative level


def _event_scores(total, on, off, hi, rng):
    """`total` scores as runs of above / below / between / NaN ticks of 1 .. max(on, off) + 2 ticks; the above values
    repeat, so that equal peaks meet the first-peak-tick rule."""
    out = np.empty((0,), dtype=np.float64)
    above = np.array([2.5, 3.0, 3.0, 2.5, 2.0]) * hi
    while len(out) < total:
        kind, length = rng.integers(0, 5), rng.integers(1, max(on, off) + 3)
        if kind <= 1:
            run = above[rng.integers(0, len(above), size=length)]
        elif kind == 2:
            run = np.full(length, -3.0)                              # at or below every clear level
        elif kind == 3:
            run = np.full(length, 0.75 * hi)                         # between lo and hi for units 0 and 2
        else:
            run = np.array([NAN, -0.0, NAN][:min(length, 3)])
        out = np.concatenate([out, run])
    return out[:total]


# c = 1, 9 | 257 | 1100: the tiles of 256, 1024 and 4096 ticks
@pytest.mark.parametrize("E", [0, 2, 64])
@pytest.mark.parametrize("on,off", [(1, 1), (3, 12)])
@pytest.mark.parametrize("c", [1, 9, 257, 1100])
@pytest.mark.parametrize("m", [1, 3])
def test_events_equal_the_single_stream_launch_per_unit_and_the_sequential_definition(m, c, on, off, E, gpu_device):
    from gdn_amd import ops
    dev, units = gpu_device, EV_UNITS
    rng = np.random.default_rng(1000 * c + 10 * on + m)
    sched = [[c, c, (c + 1) // 2], [c, c, 1], [c - 1, c, c], [c, c, 0], [c, 0, c], [1, c, c], [c, c, c]]
    totals = [sum(row[u] for row in sched) for u in range(units)]
    series = [_event_scores(totals[u], on, off, EV_HI[u], rng) for u in range(units)]
    before_silence = sum(row[1] for row in sched[:4])                # unit 1 goes silent in the middle of an episode
    series[1][before_silence - (on + 1):before_silence] = 3.0
    others = [rng.random((totals[u], m)) for u in range(units)]      # columns 1 .. m - 1: not looked at
    sensors = [rng.integers(0, 4000, size=(totals[u], m), dtype=np.int32) for u in range(units)]
    state = ops.fleet_state(torch.zeros((units, 1, 1), device=dev), 1)
    counters = ops.fleet_state_views(state, units, 1, 1)[0]
    counters[:, 0] = torch.tensor(EV_FIRST, device=dev)
    hi = torch.tensor(EV_HI, dtype=torch.float64, device=dev)
    lo = torch.tensor(EV_LO, dtype=torch.float64, device=dev)
    events = ops.fleet_events_alloc(units, m, E, dev)
    assert events.shape == (units, ops._lib.load().gdn_stream_events_bytes(m, E) // 8)
    ref_events = events.clone()
    at, open_seen = [0] * units, False
    for step, counts in enumerate(sched):
        scores = torch.full((units, c, m), 9e9, dtype=torch.float64)             # beyond the count: far above hi
        who = torch.full((units, c, m), -1, dtype=torch.int32)
        for u, cnt in enumerate(counts):
            rows = np.concatenate([series[u][at[u]:at[u] + cnt, None], others[u][at[u]:at[u] + cnt, 1:]], axis=1)
            scores[u, :cnt] = torch.from_numpy(rows)
            who[u, :cnt] = torch.from_numpy(sensors[u][at[u]:at[u] + cnt])
        scores, who = scores.to(dev), who.to(dev)
        held = events.clone()
        ops.fleet_events(state, scores, who, hi, lo, _i32(counts, dev), 1, 1, on, off, E, events)
        for u, cnt in enumerate(counts):
            if cnt:
                ops.stream_events(state[u], scores[u], who[u], hi[u:u + 1], lo[u:u + 1], on, off, E, ref_events[u],
                                  count=cnt)
            else:
                assert torch.equal(events[u], held[u]), (step, u)    # a silent unit's block: byte for byte
                open_seen = open_seen or (u == 1 and bool(held[u, 1] != 0))
            at[u] += cnt
        assert torch.equal(events, ref_events), step                 # the whole block of every unit
        counters[:, 0] += _i32(counts, dev)                          # what the advance launch does to the tick counters
    assert open_seen                                                 # unit 1 was silent with an episode open
    most = 0
    for u in range(units):
        want = ref.episodes(series[u], sensors[u], EV_HI[u], EV_LO[u], on, off, E, first_tick=EV_FIRST[u])
        carry, start, end, peak_tick, peak, sens = ops.stream_events_views(events[u], m, E)
        rows = min(int(carry[0]), E)
        got = {"start": start[:rows].cpu().numpy(), "end": end[:rows].cpu().numpy(), "peak": peak[:rows].cpu().numpy(),
               "peak_tick": peak_tick[:rows].cpu().numpy(), "sensors": sens[:rows].cpu().numpy(), "count": int(carry[0])}
        assert ref.same(got, want), (u, got["count"], want["count"])
        most = max(most, got["count"])
    assert most > (2 if c >= 257 else 0)                             # episodes were raised; E = 2 overflows its table


# ------------------------------------------------------------------------------------------------ StreamFleet
EVENTS = dict(on=2, off=3, cap=16)


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_fleet_with_gaps_and_events_writes_the_bits_of_one_detector_per_unit(shape, wide, use_graph, gpu_device):
    from gdn_amd import harness, ops
    dev = gpu_device
    n, w = SHAPES[shape][:2]
    model = _model(dev, SHAPES[shape])
    g = _gen(n, w, wide, 3)
    history = torch.rand((UNITS, n, w + 2), generator=g).to(dev)
    med_iqr = _tables(UNITS, n, dev, g)
    # levels that the scores cross: every unit's raise level is the median score of a pilot detector (the yardstick's
    # side) over 8 ticks of the same distribution, so that episodes open AND close during the script
    levels = []
    for u in range(UNITS):
        pilot = harness.StreamDetector(model, med_iqr[u], INF, history[u].contiguous(), CHUNK, use_graph=False, wide=wide)
        gp = _gen(n, u, 17)
        seen = [pilot.push(torch.rand((CHUNK, n), generator=gp).to(dev))[0][:, 0].clone() for _ in range(2)]
        levels.append(float(torch.cat(seen).median()))
    threshold = torch.tensor(levels, dtype=torch.float64)
    assert min(levels) > 0
    lo = [0.9 * levels[0], levels[1], 0.5 * levels[2]]
    fleet = harness.StreamFleet(model, med_iqr, threshold, history, CHUNK, top_m=TOP_M, log=LOG, use_graph=use_graph,
                                wide=wide, gaps=True, events=dict(lo=lo, **EVENTS))
    dets = [harness.StreamDetector(model, med_iqr[u], float(threshold[u]), history[u].contiguous(), CHUNK, top_m=TOP_M,
                                   log=LOG, use_graph=False, wide=wide, gaps=True, events=dict(lo=lo[u], **EVENTS))
            for u in range(UNITS)]
    assert fleet.graph is None and _same(fleet.clear, torch.tensor(lo, dtype=torch.float64, device=dev))
    script = [(4, None), (1, None), (4, (4, 0, 2)), (4, _i32([1, 0, 4], dev)), (9, None), (9, [9, 5, 0]),
              (2, torch.tensor([0, 2, 1]))]
    total, first_graph = [0] * UNITS, None
    for step, (r, counts) in enumerate(script):
        ticks = _with_missing(torch.rand((UNITS, r, n), generator=g), g, share=0.15)
        ticks[:, 0, step % n] = NAN                                  # a reading missing in every unit's first row
        ticks[step % UNITS, r // 2] = NAN                            # a whole dropped tick
        if step == 4:
            ticks[:, 3:] = NAN               # six of them in a row: every score falls to 0.0 and open episodes close
        each = [r] * UNITS if counts is None else [int(v) for v in (counts.tolist() if torch.is_tensor(counts) else counts)]
        for u, cnt in enumerate(each):
            ticks[u, cnt:] = INF                                     # rows that are not real: not missing readings
        ticks = ticks.to(dev)
        got = fleet.push(ticks, counts)
        for u, cnt in enumerate(each):
            total[u] += cnt
            if cnt == 0:
                continue                                             # a silent unit: its detector is not pushed
            want = dets[u].push(ticks[u, :cnt])
            real = _real_rows_of_last_cut(cnt, r, CHUNK)
            if real:                                                 # (then the detector's last cut is the same cut)
                for a, b, what in zip(got, want, ("top_scores", "top_sensors", "alarm")):
                    assert _same(a[u, :real], b), (step, u, what)
                assert torch.equal(fleet.valid[u, :real], dets[u].valid[:real]), (step, u)
                assert torch.equal(fleet.chunk_buf[u, :real], dets[u].chunk_buf[:real]), (step, u)
        assert fleet.status()[0].tolist() == total, step
        if use_graph:
            first_graph = fleet.graph if first_graph is None else first_graph
            assert fleet.graph is not None and fleet.graph is first_graph      # one graph for the whole script
        else:
            assert fleet.graph is None
    ticks_u, alarms_u, logged_u = fleet.status()
    missing_total, missing_run = fleet.status_gaps()
    assert missing_total.shape == (UNITS, n) and missing_total.dtype == torch.int64 and int(missing_total.sum()) > 0
    raised = closed = 0
    for u, det in enumerate(dets):
        assert torch.equal(fleet.unit_state(u), det.state), u        # counters, carry, hist: the whole block
        t, a, log_ticks, log_sensors, episodes, is_open = det.status()
        assert (int(ticks_u[u]), int(alarms_u[u]), int(logged_u[u])) == (t, a, len(log_ticks)), u
        assert torch.equal(fleet.log_ticks[u], det.log_ticks) and torch.equal(fleet.log_sensors[u], det.log_sensors), u
        for mine, single in zip((missing_total[u], missing_run[u]), det.status_gaps()):
            assert torch.equal(mine, single), u
        assert torch.equal(fleet.events[u], det.events), u           # the carry and the whole table
        mine, single = fleet.episodes(u), det.episodes()
        for field in mine._fields:
            assert _same(getattr(mine, field), getattr(single, field)), (u, field)
        raised += episodes
        closed += int((mine.end[:episodes] >= 0).sum())
    print(f"[fleet gaps+events {shape}] alarms {alarms_u.tolist()} of {total} ticks, episodes raised {raised} closed "
          f"{closed}, missing {int(missing_total.sum())}")
    assert int(alarms_u.sum()) > 0 and raised > 0 and closed > 0     # the script raises alarms, opens and closes episodes
    with pytest.raises(ValueError, match="units 0"):
        fleet.episodes(UNITS)


def test_the_default_fleet_issues_the_launches_it_always_did(gpu_device, monkeypatch):
    from gdn_amd import _lib as binding, harness
    dev = gpu_device
    n, w = SHAPES["msl"][:2]
    model = _model(dev, SHAPES["msl"])
    g = _gen(n, w, 5)
    fleet = harness.StreamFleet(model, _tables(UNITS, n, dev, g), 1.0, torch.rand((UNITS, n, w), generator=g).to(dev),
                                CHUNK, top_m=TOP_M, log=LOG, use_graph=False, wide=False)
    assert fleet.with_gaps is False and fleet.events is None and fleet.raw_buf is None and fleet.valid is None
    fleet.push(torch.rand((UNITS, CHUNK, n), generator=g).to(dev))          # (the model folds its constants once)
    calls, real_call = [], binding.call

    def recording(name, *args):
        calls.append((name, args))
        return real_call(name, *args)
    monkeypatch.setattr(binding, "call", recording)
    fleet.push(torch.rand((UNITS, CHUNK, n), generator=g).to(dev), [4, 0, 2])
    monkeypatch.undo()
    names = [name for name, _ in calls]
    assert names[0] == "gdn_fleet_windows" and names[-2:] == ["gdn_fleet_score", "gdn_fleet_advance"]
    assert len(names) > 3 and not any("fleet" in nm or "stream" in nm for nm in names[1:-2])     # the forward's launches
    u, c, m, s = UNITS, CHUNK, TOP_M, torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()                                       # noqa: E731
    assert calls[0][1] == (p(fleet.state), p(fleet.chunk_buf), p(fleet.counts), u, c, n, w, p(fleet.x), s)
    assert calls[-2][1] == (p(fleet.state), p(fleet.pred), p(fleet.chunk_buf), p(fleet.med_iqr), p(fleet.threshold),
                            p(fleet.counts), u, c, n, w, m, p(fleet.top_scores), p(fleet.top_sensors), p(fleet.alarm), s)
    assert calls[-1][1] == (p(fleet.state), p(fleet.chunk_buf), p(fleet.pred), p(fleet.med_iqr), p(fleet.alarm),
                            p(fleet.top_sensors), p(fleet.counts), u, c, n, w, m, p(fleet.log_ticks),
                            p(fleet.log_sensors), LOG, s)
    with pytest.raises(ValueError, match="gaps=False"):
        fleet.status_gaps()
    with pytest.raises(ValueError, match="events=None"):
        fleet.episodes(0)
