"""GPU suite of the streaming fleet: gdn_fleet_init / _windows / _score / _advance and harness.StreamFleet.  The yardstick
is never the code under test: every fleet launch is compared with the single-stream ops.stream_* launch on each unit's
slice, and StreamFleet with U StreamDetectors pushed each unit's real rows in the same cuts.  The arithmetic and its
order per unit are the same, so every comparison is exact: torch.equal, float64 on its bit patterns.  No tolerance."""
import copy
import functools

import pytest
import torch

from test_gpu_forward_parity import random_params

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _gen(*seed):
    return torch.Generator().manual_seed(sum((j + 1) * 1009 * int(s) for j, s in enumerate(seed)) + 5)


def _tables(units, n, dev, g):
    med = torch.rand((units, n), generator=g, dtype=torch.float64) * 0.1
    iqr = torch.rand((units, n), generator=g, dtype=torch.float64) * 0.2 + 0.05
    return torch.stack([med, iqr], dim=2).contiguous().to(dev)


def _i32(values, dev):
    return torch.tensor(values, dtype=torch.int32, device=dev)


# ------------------------------------------------------------------------------------------------ init, windows
@pytest.mark.parametrize("c", [1, 9])
@pytest.mark.parametrize("n,w", [(1, 1), (5, 5), (130, 15), (5, 257), (2, 1024)])
@pytest.mark.parametrize("units", [1, 3])
def test_windows_equal_the_single_stream_launch_per_unit_and_other_rows_are_zero(units, n, w, c, gpu_device):
    from gdn_amd import ops
    dev = gpu_device
    g = _gen(units, n, w, c)
    history = torch.rand((units, n, w + 3), generator=g).to(dev)
    state = ops.fleet_state(history, w)
    words = ops._lib.load().gdn_stream_state_bytes(n, w) // 8
    assert state.shape == (units, words) and state.dtype == torch.int64
    for u in range(units):                                           # gdn_fleet_init = gdn_stream_init per unit
        assert torch.equal(state[u], ops.stream_state(history[u].contiguous(), w))
    counters, carry, hist = ops.fleet_state_views(state, units, n, w)
    assert torch.equal(hist, history[:, :, -w:]) and not counters.any() and not carry.any()
    for u in range(units):
        for mine, single in zip((counters[u], carry[u], hist[u]), ops.stream_state_views(state[u], n, w)):
            assert mine.data_ptr() == single.data_ptr() and mine.shape == single.shape
    chunk = torch.rand((units, c, n), generator=g).to(dev)
    before = state.clone()
    launches = [[0, 1, c], [c, 0, 1], [1, c, 0]] if units == 3 else [[0], [1], [c]]
    for counts in launches:
        x = torch.full((units, c, n, w), float("nan"), device=dev)
        ops.fleet_windows(state, chunk, _i32(counts, dev), w, x)
        want = torch.zeros((units, c, n, w), device=dev)
        for u, cnt in enumerate(counts):
            if cnt:
                ops.stream_windows(state[u], chunk[u], w, want[u], count=cnt)
        assert torch.equal(x, want), counts                          # (a NaN left in x compares unequal)
        for u, cnt in enumerate(counts):
            assert not x[u, cnt:].any()
    assert torch.equal(state, before)                                # the launch reads the states
    # a count outside 0 .. c is clamped on the device
    x = torch.full((units, c, n, w), float("nan"), device=dev)
    ops.fleet_windows(state, chunk, _i32([c + 5, -3, c][:units], dev), w, x)
    ops.fleet_windows(state, chunk, _i32([c, 0, c][:units], dev), w, want)
    assert torch.equal(x, want)


# ------------------------------------------------------------------------------------------------ score
TICKS = [0, 1, 2, 3, 1000, 5]          # the units' stream positions: the first-three-ticks rule and the carry both act


def _staged_fleet(n, w, c, dev, g, ticks=TICKS):
    """U = len(ticks) states at those positions with a random carry, tables and thresholds of their own, a chunk and a
    prediction in [0, 1]; sensors 0 and 1 of unit 0 tie (same table row, same readings, same carry)."""
    from gdn_amd import ops
    units = len(ticks)
    state = ops.fleet_state(torch.rand((units, n, w), generator=g).to(dev), w)
    counters, carry, _ = ops.fleet_state_views(state, units, n, w)
    counters[:, 0] = torch.tensor(ticks, device=dev)
    carry.copy_(torch.rand((units, 3, n), generator=g, dtype=torch.float64) * 2 - 0.5)
    med_iqr = _tables(units, n, dev, g)
    chunk = torch.rand((units, c, n), generator=g).to(dev)
    pred = torch.rand((units, c, n), generator=g).to(dev)
    if n >= 2:
        med_iqr[0, 1] = med_iqr[0, 0]
        chunk[0, :, 1] = chunk[0, :, 0]
        pred[0, :, 1] = pred[0, :, 0]
        carry[0, :, 1] = carry[0, :, 0]
    pred[1, c - 1, n // 2] = float("nan")                            # a NaN prediction: a NaN score, never an alarm
    threshold = (torch.rand((units,), generator=g, dtype=torch.float64) * 2).to(dev)
    return state, med_iqr, threshold, chunk, pred


def _outputs(units, c, m, dev, fill=-7):
    return (torch.full((units, c, m), float(fill), dtype=torch.float64, device=dev),
            torch.full((units, c, m), fill, dtype=torch.int32, device=dev),
            torch.full((units, c), fill, dtype=torch.int32, device=dev))


def _single_scores(state, pred, chunk, med_iqr, threshold, counts, m, outs):
    from gdn_amd import ops
    for u, cnt in enumerate(counts):
        if cnt:
            ops.stream_score(state[u], pred[u], chunk[u], med_iqr[u], threshold[u:u + 1], m, outs[0][u], outs[1][u],
                             outs[2][u], count=cnt)


@pytest.mark.parametrize("c", [1, 8, 9, 17])
@pytest.mark.parametrize("n", [1, 64, 65, 128, 129, 200])
def test_scores_equal_the_single_stream_launch_per_unit_and_other_rows_are_untouched(n, c, gpu_device):
    from gdn_amd import ops
    dev = gpu_device
    w = 4
    state, med_iqr, threshold, chunk, pred = _staged_fleet(n, w, c, dev, _gen(n, c))
    units = len(TICKS)
    before = state.clone()
    for m in sorted({1, min(8, n)}):
        for counts in ([c, c, c, (c + 1) // 2, 1, 0], [0, 1, c - 1, c, c, c]):
            got, want = _outputs(units, c, m, dev), _outputs(units, c, m, dev)
            ops.fleet_score(state, pred, chunk, med_iqr, threshold, _i32(counts, dev), w, m, *got)
            _single_scores(state, pred, chunk, med_iqr, threshold, counts, m, want)
            for a, b, what in zip(got, want, ("top_scores", "top_sensors", "alarm")):
                assert _same(a, b), (what, m, counts)
            for u, cnt in enumerate(counts):                         # rows at or beyond counts[u]: the sentinel
                assert (got[0][u, cnt:] == -7).all() and (got[1][u, cnt:] == -7).all() and (got[2][u, cnt:] == -7).all()
            if m >= 2:                                               # the tie of unit 0: the lower sensor first
                top, who = got[0][0, :counts[0]], got[1][0, :counts[0]]
                tied = _bits(top[:, 0]) == _bits(top[:, 1])
                assert bool((who[:, 0][tied] < who[:, 1][tied]).all())
    assert torch.equal(state, before)


# ------------------------------------------------------------------------------------------------ advance
def _check_advance(n, w, c, m, log_len, rounds, dev, g, ticks, alarm_of=None, threshold=None):
    from gdn_amd import ops
    units = len(ticks)
    state, med_iqr, thr, chunk, pred = _staged_fleet(n, w, c, dev, g, ticks)
    if threshold is not None:
        thr.fill_(threshold)
    ref_state = state.clone()                                        # the single-stream launches run on a copy
    logs = ref_logs = (None, None)
    if log_len:
        logs = (torch.full((units, log_len), -1, dtype=torch.int64, device=dev),
                torch.full((units, log_len, m), -1, dtype=torch.int32, device=dev))
        ref_logs = tuple(t.clone() for t in logs)
    for counts in rounds:
        scores, sensors, alarm = _outputs(units, c, m, dev, fill=0)
        ops.fleet_score(state, pred, chunk, med_iqr, thr, _i32(counts, dev), w, m, scores, sensors, alarm)
        if alarm_of is not None:
            alarm.copy_(alarm_of(units, c).to(dev))
        idle = [u for u, cnt in enumerate(counts) if cnt == 0]
        state_before = state.clone()
        logs_before = tuple(None if t is None else t.clone() for t in logs)
        ops.fleet_advance(state, chunk, pred, med_iqr, alarm, sensors, _i32(counts, dev), w, m, *logs)
        for u, cnt in enumerate(counts):
            if cnt:
                ops.stream_advance(ref_state[u], chunk[u], pred[u], med_iqr[u], alarm[u], sensors[u], w, m,
                                   None if not log_len else ref_logs[0][u], None if not log_len else ref_logs[1][u],
                                   count=cnt)
        assert torch.equal(state, ref_state), counts                 # counters, carry and hist of every unit
        for u in idle:                                               # a silent unit: every byte as it was
            assert torch.equal(state[u], state_before[u])
            if log_len:
                assert torch.equal(logs[0][u], logs_before[0][u]) and torch.equal(logs[1][u], logs_before[1][u])
        if log_len:
            assert torch.equal(logs[0], ref_logs[0]) and torch.equal(logs[1], ref_logs[1]), counts
    return ops.fleet_state_views(state, units, n, w)[0].cpu(), logs


def _random_flags(seed):
    return lambda units, c: (torch.rand((units, c), generator=_gen(seed, units, c)) < 0.5).to(torch.int32)


def test_advance_rolls_every_unit_by_its_own_count_and_leaves_a_silent_unit_untouched(gpu_device):
    rounds = [[0, 1, 4, 5, 9], [9, 0, 5, 4, 1], [5, 4, 0, 0, 9]]
    counters, _ = _check_advance(5, 5, 9, 2, 16, rounds, gpu_device, _gen(1), [0, 1, 2, 3, 1000],
                                 alarm_of=_random_flags(3))
    assert counters[:, 0].tolist() == [14, 6, 11, 12, 1019]


def test_advance_of_the_longest_window_by_one_tick(gpu_device):
    counters, _ = _check_advance(2, 1024, 1, 1, 4, [[1, 1], [0, 1]], gpu_device, _gen(2), [0, 7], alarm_of=_random_flags(4))
    assert counters[:, 0].tolist() == [1, 9]


def test_a_full_log_drops_entries_and_alarms_keeps_counting(gpu_device):
    def five(units, c):
        flags = torch.zeros((units, c), dtype=torch.int32)
        flags[0, [0, 2, 3, 5, 8]] = 1
        flags[1, 4] = 1
        return flags
    counters, logs = _check_advance(5, 5, 9, 2, 2, [[9, 9, 9], [9, 0, 9]], gpu_device, _gen(3), [0, 2, 50], alarm_of=five)
    assert counters[:, 1].tolist() == [10, 1, 0] and counters[:, 2].tolist() == [2, 1, 0]
    assert logs[0][0].tolist() == [0, 2] and logs[0][1].tolist() == [2 + 4, -1]


def test_advance_without_a_log(gpu_device):
    counters, logs = _check_advance(7, 3, 4, 3, 0, [[4, 2, 0], [1, 4, 4]], gpu_device, _gen(4), [0, 1, 9],
                                    alarm_of=_random_flags(5))
    assert logs == (None, None) and counters[:, 2].tolist() == [0, 0, 0]


def test_more_than_256_alarms_in_one_push_take_a_second_compaction_round(gpu_device):
    counters, logs = _check_advance(3, 2, 300, 1, 512, [[300, 299]], gpu_device, _gen(5), [0, 40],
                                    threshold=float("-inf"))
    # every score of a real row is > -inf except the NaN one (unit 1, row 299: beyond its count here)
    assert counters[:, 1].tolist() == [300, 299] and counters[:, 2].tolist() == [300, 299]
    assert logs[0][0, :300].tolist() == list(range(300)) and logs[0][1, :299].tolist() == list(range(40, 339))


# ------------------------------------------------------------------------------------------------ StreamFleet
SHAPES = {"msl": (27, 15, 20, 64, 1, 32), "mlp2_n20_w8_k6": (20, 8, 6, 32, 2, 48)}
UNITS, CHUNK, TOP_M, LOG = 3, 4, 3, 6


@functools.lru_cache(maxsize=None)
def _cpu_model(n, w, k, d, layers, inter):
    return random_params(n, w, k, d, seed=n + w, out_layer_num=layers, inter=inter)


def _model(dev, shape):
    return copy.deepcopy(_cpu_model(*shape)).to(dev).eval()


def _real_rows_of_last_cut(cnt, r, chunk):
    start = ((r - 1) // chunk) * chunk                               # the last of the pushes r ticks are split into
    return max(0, min(cnt - start, r - start))


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_fleet_writes_the_bits_of_one_detector_per_unit(shape, wide, use_graph, gpu_device):
    from gdn_amd import harness, ops
    dev = gpu_device
    n, w = SHAPES[shape][:2]
    model = _model(dev, SHAPES[shape])
    g = _gen(n, w, wide)
    history = torch.rand((UNITS, n, w + 2), generator=g).to(dev)
    med_iqr = _tables(UNITS, n, dev, g)
    threshold = torch.tensor([0.5, 1.0, 1.5], dtype=torch.float64)
    fleet = harness.StreamFleet(model, med_iqr, threshold, history, CHUNK, top_m=TOP_M, log=LOG, use_graph=use_graph,
                                wide=wide)
    dets = [harness.StreamDetector(model, med_iqr[u], float(threshold[u]), history[u].contiguous(), CHUNK, top_m=TOP_M,
                                   log=LOG, use_graph=False, wide=wide) for u in range(UNITS)]
    assert fleet.graph is None and fleet.wide is wide
    script = [(4, None), (1, None), (4, (4, 0, 2)), (4, _i32([1, 0, 4], dev)), (9, None), (9, [9, 5, 0]),
              (2, torch.tensor([0, 2, 1]))]
    total, first_graph = [0] * UNITS, None
    for step, (r, counts) in enumerate(script):
        ticks = torch.rand((UNITS, r, n), generator=g).to(dev)
        each = [r] * UNITS if counts is None else [int(v) for v in (counts.tolist() if torch.is_tensor(counts) else counts)]
        got = fleet.push(ticks, counts)
        assert got[0].shape == (UNITS, r - ((r - 1) // CHUNK) * CHUNK, TOP_M)      # the last cut of the push
        for u, cnt in enumerate(each):
            total[u] += cnt
            if cnt == 0:
                continue                                             # a silent unit: its detector is not pushed
            want = dets[u].push(ticks[u, :cnt])
            real = _real_rows_of_last_cut(cnt, r, CHUNK)
            if real:                                                 # (then the detector's last cut is the same cut)
                for a, b, what in zip(got, want, ("top_scores", "top_sensors", "alarm")):
                    assert _same(a[u, :real], b), (step, u, what)
        # the counts are data: the same graph, other counts, the counters of every unit follow them
        assert fleet.status()[0].tolist() == total, step
        if use_graph:
            first_graph = fleet.graph if first_graph is None else first_graph
            assert fleet.graph is not None and fleet.graph is first_graph
        else:
            assert fleet.graph is None
    ticks_u, alarms_u, logged_u = fleet.status()
    assert int(alarms_u.sum()) > 0                                   # the script raises alarms: the log is exercised
    for u, det in enumerate(dets):
        assert torch.equal(fleet.unit_state(u), det.state), u        # counters, carry, hist: the whole block
        for a, b in zip(ops.stream_state_views(fleet.unit_state(u), n, w), ops.stream_state_views(det.state, n, w)):
            assert _same(a, b)
        t, a, log_ticks, log_sensors = det.status()
        assert (int(ticks_u[u]), int(alarms_u[u]), int(logged_u[u])) == (t, a, len(log_ticks)), u
        assert torch.equal(fleet.log_ticks[u], det.log_ticks) and torch.equal(fleet.log_sensors[u], det.log_sensors), u
    with pytest.raises(ValueError, match="counts"):
        fleet.push(torch.rand((UNITS, 2, n)).to(dev), [3, 0, 0])
    assert fleet.status()[0].tolist() == total                       # a refused push moved nothing


def test_from_calibration_gives_every_unit_the_detectors_table_threshold_and_history(gpu_device):
    from gdn_amd import harness, ops
    dev = gpu_device
    shape = SHAPES["msl"]
    n, w = shape[:2]
    model = _model(dev, shape)
    series = torch.rand((UNITS, n, 200), generator=_gen(11)).to(dev)
    fleet = harness.StreamFleet.from_calibration(model, series, CHUNK, top_m=2, wide=False)
    assert fleet.units == UNITS and fleet.med_iqr.shape == (UNITS, n, 2) and fleet.threshold.shape == (UNITS,)
    for u in range(UNITS):
        det = harness.StreamDetector.from_calibration(model, series[u].contiguous(), CHUNK, top_m=2, wide=False,
                                                      use_graph=False)
        assert _same(fleet.med_iqr[u], det.med_iqr), u
        assert _same(fleet.threshold[u:u + 1], det.threshold), u
        assert torch.equal(fleet.unit_state(u), det.state), u
        assert torch.equal(ops.stream_state_views(fleet.unit_state(u), n, w)[2], series[u, :, -w:])
