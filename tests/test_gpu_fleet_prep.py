"""GPU suite of a fleet's raw-readings front end: gdn_fleet_prep_ticks against the float64 restatement
(tests/_prep_ref.py) and against gdn_prep_ticks on each unit's slice, and harness.StreamFleet(prep=) against a plain
fleet fed the completed medians and against one StreamDetector(prep=) per unit.  Every comparison is on bit patterns:
the arithmetic per reading is one, so there is no tolerance."""
import numpy as np
import pytest
import torch

import _prep_ref as ref
from _fleet_case import (CHUNK, DOWN, LOG, MSL, N, TOP_M, UNITS, assert_same_memory, bits, gen, make_prep, memory,
                         model_on, raw_ticks, same, setup)

pytestmark = pytest.mark.gpu

QNAN32 = 0x7fc00000
SENTINEL = -7.0
KINDS = ("zero", "one", "nogroup", "full")          # unit u runs them rotated by u: every launch is ragged


def _i32(values, dev):
    return torch.tensor(values, dtype=torch.int32, device=dev)


def _table(n, g, dev):
    scale = torch.rand((n,), generator=g, dtype=torch.float64) * 0.02 + 0.001
    offset = torch.rand((n,), generator=g, dtype=torch.float64) - 0.5
    return torch.stack([scale, offset], dim=1).contiguous().to(dev)


def _count(kind, p, down, rows):
    if kind == "zero":
        return 0
    if kind == "one":
        return down - p                              # closes exactly the open group
    if kind == "nogroup":
        return max(0, (down - 1 - p + 1) // 2)       # p + k < down; 0 when the group has no room (down = 1)
    return rows                                      # c * down, whatever is pending


def _check_launch(raw, counts, state, tab_np, down, c, pend, table, dev):
    """One launch with `counts` raw rows per unit, checked against the restatement over each unit's real rows.  `state`
    holds per unit the float64 raw ticks of its open group (host)."""
    from gdn_amd import ops
    units, rows, n = raw.shape
    tiles = (n + 63) // 64
    out = torch.full((units, c, n), SENTINEL, device=dev)
    got_counts = _i32([-9] * units, dev)
    ticks, words = ops.fleet_prep_views(pend, units, n, down)
    before_ticks, before_words = ticks.clone(), words.clone()
    ops.fleet_prep_ticks(raw, _i32(counts, dev), pend, down, table, out, got_counts)
    raw_np = raw.cpu().numpy().astype(np.float64)
    want_counts = []
    for u in range(units):
        k = min(max(counts[u], 0), rows)
        have = np.concatenate([state[u], raw_np[u, :k]], axis=0)
        groups = have.shape[0] // down
        want_counts.append(groups)
        if groups:
            want = ref.series(have[:groups * down], tab_np, down)[0].T              # [groups, n] fp32
            assert np.array_equal(ref.bits32(out[u, :groups].cpu().numpy()), ref.bits32(want)), (u, counts)
        assert bool((out[u, groups:] == SENTINEL).all()), (u, counts)               # rows >= counts[u]: not written
        state[u] = have[groups * down:]
        p = state[u].shape[0]
        if k == 0:                                                                   # silent: every byte stays
            assert torch.equal(bits(ticks[u]), bits(before_ticks[u])) and torch.equal(words[u], before_words[u]), u
        assert words[u].tolist() == [p] * tiles, (u, counts)                        # every tile's own word
        got_open = ticks[u, :p].cpu().numpy()
        assert np.array_equal(got_open.view(np.int64), np.ascontiguousarray(state[u]).view(np.int64)), (u, counts)
    assert got_counts.tolist() == want_counts, counts
    return out, want_counts


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("down", [1, 3, 10, 17, 33, 64])
def test_kernel_equals_the_restatement_over_each_units_real_rows(down, dtype, gpu_device):
    from gdn_amd import ops
    dev = gpu_device
    for units in (1, 3):
        for n in (1, 65, 130):
            for c in (1, 5):
                g = gen(down, units, n, c)
                rows = c * down
                table = _table(n, g, dev)
                tab_np = table.cpu().numpy()
                pend = ops.fleet_prep_state(units, n, down, dev)
                assert pend.numel() * 8 == ops._lib.load().gdn_fleet_prep_bytes(units, n, down) and not pend.any()
                state = [np.zeros((0, n)) for _ in range(units)]
                for step in range(len(KINDS)):
                    raw = raw_ticks(g, rows, dtype, dev, units, n)
                    gone = torch.rand((units, rows, n), generator=g) < 0.15         # a NaN inside a group: left out
                    raw[gone.to(dev)] = float("nan")
                    raw[0, :, 0] = float("inf")                                      # groups with no finite reading
                    raw[0, ::2, 0] = float("-inf")
                    raw[0, rows // 2, 0] = float("nan")
                    if dtype == torch.float64:                                       # a payload: the bits are kept
                        raw.view(torch.int64)[-1, -1, -1] = 0x7ff8000000000123
                    counts = [_count(KINDS[(step + u) % len(KINDS)], state[u].shape[0], down, rows) for u in range(units)]
                    out, done = _check_launch(raw, counts, state, tab_np, down, c, pend, table, dev)
                    if done[0]:
                        assert bool((out[0, :done[0], 0].view(torch.int32) == QNAN32).all())
                    if step == len(KINDS) - 1 and down > 1:
                        assert counts[0] == rows and done[0] == c                    # c * down on a non-zero pending
                # a count above rows or below 0 on the device is clamped
                raw = raw_ticks(g, rows, dtype, dev, units, n)
                twin, twin_state = pend.clone(), [s.copy() for s in state]
                _check_launch(raw, [rows + 5, -3, rows][:units], state, tab_np, down, c, pend, table, dev)
                _check_launch(raw, [rows, 0, rows][:units], twin_state, tab_np, down, c, twin, table, dev)
                a, b = ops.fleet_prep_views(pend, units, n, down), ops.fleet_prep_views(twin, units, n, down)
                assert torch.equal(a[1], b[1])
                for u in range(units):
                    p = int(a[1][u, 0])
                    assert torch.equal(bits(a[0][u, :p]), bits(b[0][u, :p]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_kernel_equals_gdn_prep_ticks_on_each_units_slice(dtype, gpu_device):
    from gdn_amd import ops
    dev = gpu_device
    units, n, c, down = 3, 130, 5, 10
    g = gen(units, n, c, down)
    table = _table(n, g, dev)
    raw = raw_ticks(g, c * down, dtype, dev, units, n)
    raw[(torch.rand((units, c * down, n), generator=g) < 0.1).to(dev)] = float("nan")
    pend = ops.fleet_prep_state(units, n, down, dev)
    out = torch.full((units, c, n), SENTINEL, device=dev)
    counts = _i32([0] * units, dev)
    ops.fleet_prep_ticks(raw, _i32([c * down] * units, dev), pend, down, table, out, counts)
    assert counts.tolist() == [c] * units and not ops.fleet_prep_views(pend, units, n, down)[1].any()
    planes = [torch.zeros((down - 1, n), dtype=torch.float64, device=dev) for _ in range(2)]
    for u in range(units):
        single = torch.full((c, n), SENTINEL, device=dev)
        assert ops.prep_ticks(raw[u], planes[0], 0, planes[1], down, table, single) == c
        assert torch.equal(out[u].view(torch.int32), single.view(torch.int32)), u


# ------------------------------------------------------------------------------------------------ StreamFleet(prep=)
SCRIPT = [(5, None), (7, [7, 3, 0]), (16, "device"), (3, [0, 3, 1]), (37, None), (37, [37, 20, 5]),
          (2, torch.tensor([1, 2, 0]))]
DEVICE_COUNTS = [16, 9, 2]
OPTIONS = {"plain": dict(), "gaps": dict(gaps=True),
           "recal_events": dict(recal=64, recal_min=8, events=dict(on=2, off=2, cap=8))}


def _drive(fleet, plain, dets, dtype, dev, g, script, open_ticks):
    """Push `script` into the prep= fleet; feed `plain` the restatement's medians of every cut with counts = groups and
    every detector its unit's real raw rows of the cut.  `open_ticks`: per unit the raw ticks of its open group (host
    float64), moved along."""
    tab_np = fleet.prep.table.cpu().numpy()
    span = CHUNK * DOWN
    for step, (r, counts) in enumerate(script):
        raw = raw_ticks(g, r, dtype, dev)
        if plain.with_gaps:
            raw[0, :, 3] = float("nan")                              # a sensor of unit 0 out for the whole stream
            raw[1, 0, 5] = float("inf")                              # one reading: left out of its median
        each = [r] * UNITS if counts is None else DEVICE_COUNTS if isinstance(counts, str) else \
            [int(v) for v in (counts.tolist() if torch.is_tensor(counts) else counts)]
        got = fleet.push(raw, _i32(DEVICE_COUNTS, dev) if isinstance(counts, str) else counts)
        raw_np = raw.cpu().numpy().astype(np.float64)
        want = None
        for s in range(0, r, span):                                  # a sub-push: at most chunk * down raw rows
            rows = min(span, r - s)
            medians = torch.zeros((UNITS, CHUNK, N))
            groups = []
            for u in range(UNITS):
                k = min(max(each[u] - s, 0), rows)
                have = np.concatenate([open_ticks[u], raw_np[u, s:s + k]], axis=0)
                gu = have.shape[0] // DOWN
                groups.append(gu)
                if gu:
                    medians[u, :gu] = torch.from_numpy(ref.series(have[:gu * DOWN], tab_np, DOWN)[0].T.copy())
                open_ticks[u] = have[gu * DOWN:]
                if k:
                    dets[u].push(raw[u, s:s + k].contiguous())
            want = plain.push(medians[:, :max(groups)].contiguous().to(dev), groups) if any(groups) else None
        # the last cut: `counts` holds the model ticks each unit completed, the views cover what a unit can have
        # completed, and the real rows equal the plain fleet's
        assert fleet.counts.tolist() == groups, step
        assert got[0].shape == (UNITS, min(CHUNK, (DOWN - 1 + rows) // DOWN), TOP_M), step
        for u, gu in enumerate(groups):
            for a, b, what in zip(got, want or (), ("top_scores", "top_sensors", "alarm")):
                assert same(a[u, :gu], b[u, :gu]), (step, u, what)


def _assert_contract(fleet, plain, dets, open_ticks):
    from gdn_amd import ops
    mine = memory(fleet)
    assert_same_memory({k: v for k, v in mine.items() if not k.startswith("pending")}, memory(plain))
    ticks, words = ops.fleet_prep_views(fleet.pend, UNITS, N, DOWN)
    for u, det in enumerate(dets):
        assert torch.equal(fleet.unit_state(u), det.state), u
        assert same(fleet.med_iqr[u], det.med_iqr), u
        assert torch.equal(fleet.log_ticks[u], det.log_ticks) and torch.equal(fleet.log_sensors[u], det.log_sensors), u
        if fleet.with_gaps:
            assert torch.equal(fleet.gaps[u], det.gaps), u
        if fleet.recal:
            assert same(fleet.ring_keys[u], det.ring_keys) and torch.equal(fleet.ring_keep[u], det.ring_keep), u
        if fleet.events is not None:
            assert torch.equal(fleet.events[u], det.events), u
        p = open_ticks[u].shape[0]
        assert words[u].tolist() == [p] * words.shape[1] and det.raw_pending == p, u
        want = torch.from_numpy(np.ascontiguousarray(open_ticks[u])).to(ticks.device)
        assert same(ticks[u, :p], want) and same(det._pend[det._pend_at][:p], want), u


def _three(dev, use_graph, kw):
    from gdn_amd import harness
    model, med_iqr, threshold, history = setup(dev)
    prep = make_prep(dev)
    common = dict(top_m=TOP_M, log=LOG, wide=False, **kw)
    fleet = harness.StreamFleet(model, med_iqr, threshold, history, CHUNK, use_graph=use_graph, prep=prep, **common)
    plain = harness.StreamFleet(model, med_iqr, threshold, history, CHUNK, use_graph=False, **common)
    dets = [harness.StreamDetector(model, med_iqr[u], float(threshold[u]), history[u].contiguous(), CHUNK,
                                   use_graph=False, prep=prep, **common) for u in range(UNITS)]
    return model, fleet, plain, dets


@pytest.mark.parametrize("case", ["plain-graph-f32", "plain-graph-f64", "plain-eager-f32", "gaps-graph-f64",
                                  "recal_events-graph-f32"])
def test_prep_fleet_writes_the_bits_of_a_plain_fleet_fed_the_medians_and_of_one_prep_detector_per_unit(case, gpu_device):
    dev = gpu_device
    options, how, raw_dtype = case.split("-")
    use_graph = how == "graph"
    dtype = torch.float32 if raw_dtype == "f32" else torch.float64
    _, fleet, plain, dets = _three(dev, use_graph, OPTIONS[options])
    assert fleet.prep is not None and fleet._prep_graphs == {} and fleet.graph is None
    g = gen(7)
    open_ticks = [np.zeros((0, N)) for _ in range(UNITS)]
    _drive(fleet, plain, dets, dtype, dev, g, SCRIPT[:1], open_ticks)
    first = dict(fleet._prep_graphs)
    _drive(fleet, plain, dets, dtype, dev, g, SCRIPT[1:], open_ticks)
    if use_graph:                                                    # one graph for every mix of pending and counts
        assert list(first) == [dtype] and list(fleet._prep_graphs) == [dtype]
        assert fleet._prep_graphs[dtype] is first[dtype] and fleet.graph is None
    else:
        assert first == {} and fleet._prep_graphs == {} and fleet.graph is None
    assert int(fleet.status()[1].sum()) > 0                          # the script raises alarms: the logs are exercised
    if fleet.with_gaps:                                              # an all-missing raw group is a missing reading
        total, run = fleet.status_gaps()
        assert int(total[0, 3]) == int(fleet.status()[0][0]) > 0
        for mine, want in zip((total, run), plain.status_gaps()):
            assert torch.equal(mine, want)
    if fleet.recal:
        fleet.recalibrate()
        plain.recalibrate()
        for det in dets:
            det.recalibrate()
    _assert_contract(fleet, plain, dets, open_ticks)
    with pytest.raises(ValueError, match="counts"):
        fleet.push(raw_ticks(g, 2, dtype, dev), [3, 0, 0])
    with pytest.raises(TypeError, match="float32 or torch.float64"):
        fleet.push(raw_ticks(g, 2, torch.float16, dev))
    _assert_contract(fleet, plain, dets, open_ticks)                 # a refused push moved nothing


def test_a_second_raw_dtype_gets_a_staging_buffer_and_a_graph_of_its_own(gpu_device):
    dev = gpu_device
    _, fleet, plain, dets = _three(dev, True, {})
    g = gen(8)
    open_ticks = [np.zeros((0, N)) for _ in range(UNITS)]
    _drive(fleet, plain, dets, torch.float32, dev, g, SCRIPT[:2], open_ticks)
    _drive(fleet, plain, dets, torch.float64, dev, g, SCRIPT[1:4], open_ticks)     # the open groups carry over
    f32 = fleet._prep_graphs[torch.float32]
    _drive(fleet, plain, dets, torch.float32, dev, g, SCRIPT[4:5], open_ticks)
    assert sorted(fleet._prep_graphs, key=str) == [torch.float32, torch.float64]
    assert fleet._prep_graphs[torch.float32] is f32
    _assert_contract(fleet, plain, dets, open_ticks)


def test_from_calibration_passes_prep_through_and_the_series_is_a_prepared_one(gpu_device):
    from gdn_amd import harness
    dev = gpu_device
    model, n = model_on(dev, MSL), MSL[0]
    prep = make_prep(dev, n=n)
    series = torch.rand((UNITS, n, 120), generator=gen(12)).to(dev)
    fleet = harness.StreamFleet.from_calibration(model, series, CHUNK, top_m=2, wide=False, prep=prep)
    plain = harness.StreamFleet.from_calibration(model, series, CHUNK, top_m=2, wide=False)
    assert fleet.prep is prep and same(fleet.med_iqr, plain.med_iqr) and torch.equal(fleet.state, plain.state)
    with pytest.raises(ValueError, match="prep: fitted on"):
        harness.StreamFleet.from_calibration(model, series, CHUNK, prep=make_prep(dev, n=n + 1))
    with pytest.raises(ValueError, match="prep: its table is on"):
        harness.StreamFleet.from_calibration(model, series, CHUNK, prep=make_prep(torch.device("cpu"), n=n))


def test_a_parameter_change_drops_the_graph_of_the_raw_push(gpu_device):
    """tests/test_gpu_prep.py's test of the same name on a prep= fleet: the graph held under the raw dtype is captured
    again, and the fleet goes on bit for bit like a fresh one put at the same point of the streams."""
    from gdn_amd import harness
    dev = gpu_device
    model, med_iqr, threshold, history = setup(dev)
    prep = make_prep(dev)
    g = gen(13)

    def build():
        return harness.StreamFleet(model, med_iqr, threshold, history, CHUNK, top_m=TOP_M, log=LOG, wide=False, prep=prep)
    fleet = build()
    fleet.push(raw_ticks(g, 16, torch.float64, dev))
    fleet.push(raw_ticks(g, 7, torch.float64, dev), [7, 2, 0])
    before = fleet._prep_graphs[torch.float64]
    with torch.no_grad():
        model.out_layer.mlp[0].bias.data.add_(0.5)
        model.embedding.weight.data[3].mul_(1.5)
    model.invalidate_constants()
    fresh = build()
    fresh.state.copy_(fleet.state)                                   # the same point of the same streams
    fresh.pend.copy_(fleet.pend)
    fresh.log_ticks.copy_(fleet.log_ticks)
    fresh.log_sensors.copy_(fleet.log_sensors)
    for r, counts in ((16, None), (9, [9, 0, 4])):                   # the re-capturing push, then a replay
        raw = raw_ticks(g, r, torch.float64, dev)
        a, b = fleet.push(raw, counts), fresh.push(raw, counts)
        assert fleet.counts.tolist() == fresh.counts.tolist()
        for u, gu in enumerate(fleet.counts.tolist()):
            assert all(same(x[u, :gu], y[u, :gu]) for x, y in zip(a, b)), u
    assert list(fleet._prep_graphs) == [torch.float64] and fleet._prep_graphs[torch.float64] is not before
    assert_same_memory(memory(fleet), memory(fresh))
