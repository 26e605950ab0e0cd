"""GPU suite of per-unit prep tables: gdn_fleet_prep_ticks_units against the float64 restatement
(tests/_prep_ref.py) with tables[u] per unit, against gdn_prep_ticks on each unit's slice and against the shared entry
point, and harness.StreamFleet(prep=PrepUnits) against one StreamDetector(prep=prep.unit(u)) per unit.  Every comparison
is on bit patterns: the arithmetic per reading is one, so there is no tolerance."""
import numpy as np
import pytest
import torch

import _prep_ref as ref
from _fleet_case import CHUNK, UNITS, assert_same_memory, bits, gen, make_prep, memory, raw_ticks, same
from _fleet_units_case import ALL, assert_unit_is, build, detectors, make_prep_units, push_both
from test_gpu_fleet_prep import KINDS, QNAN32, SENTINEL, _count, _i32, _table

pytestmark = pytest.mark.gpu


def _tables(units, n, g, dev):
    return torch.stack([_table(n, g, dev) for _ in range(units)]).contiguous()


def _check_launch(raw, counts, state, tabs_np, down, c, pend, tables, dev):
    """tests/test_gpu_fleet_prep.py's check of one launch with the restatement reading tabs_np[u] for unit u."""
    from gdn_amd import ops
    units, rows, n = raw.shape
    tiles = (n + 63) // 64
    out = torch.full((units, c, n), SENTINEL, device=dev)
    got_counts = _i32([-9] * units, dev)
    ticks, words = ops.fleet_prep_views(pend, units, n, down)
    before_ticks, before_words = ticks.clone(), words.clone()
    ops.fleet_prep_ticks(raw, _i32(counts, dev), pend, down, tables, out, got_counts)
    raw_np = raw.cpu().numpy().astype(np.float64)
    want_counts = []
    for u in range(units):
        k = min(max(counts[u], 0), rows)
        have = np.concatenate([state[u], raw_np[u, :k]], axis=0)
        groups = have.shape[0] // down
        want_counts.append(groups)
        if groups:
            want = ref.series(have[:groups * down], tabs_np[u], down)[0].T              # [groups, n] fp32
            assert np.array_equal(ref.bits32(out[u, :groups].cpu().numpy()), ref.bits32(want)), (u, counts)
        assert bool((out[u, groups:] == SENTINEL).all()), (u, counts)                   # rows >= counts[u]: not written
        state[u] = have[groups * down:]
        p = state[u].shape[0]
        if k == 0:                                                                       # silent: every byte stays
            assert torch.equal(bits(ticks[u]), bits(before_ticks[u])) and torch.equal(words[u], before_words[u]), u
        assert words[u].tolist() == [p] * tiles, (u, counts)
        got_open = ticks[u, :p].cpu().numpy()
        assert np.array_equal(got_open.view(np.int64), np.ascontiguousarray(state[u]).view(np.int64)), (u, counts)
    assert got_counts.tolist() == want_counts, counts
    return out, want_counts


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("down", [1, 3, 10, 64])
def test_kernel_equals_the_restatement_with_each_units_own_table(down, dtype, gpu_device):
    from gdn_amd import ops
    dev = gpu_device
    for units in (1, 3):
        for n in (1, 65, 130):
            for c in (1, 5):
                g = gen(down, units, n, c, 3)
                rows = c * down
                tables = _tables(units, n, g, dev)
                tabs_np = tables.cpu().numpy()
                assert units == 1 or not np.array_equal(tabs_np[0], tabs_np[1])         # the tables really differ
                pend = ops.fleet_prep_state(units, n, down, dev)
                state = [np.zeros((0, n)) for _ in range(units)]
                for step in range(len(KINDS)):
                    raw = raw_ticks(g, rows, dtype, dev, units, n)
                    gone = torch.rand((units, rows, n), generator=g) < 0.15             # a NaN inside a group: left out
                    raw[gone.to(dev)] = float("nan")
                    raw[0, :, 0] = float("inf")                                          # groups with no finite reading
                    raw[0, ::2, 0] = float("-inf")
                    raw[0, rows // 2, 0] = float("nan")
                    counts = [_count(KINDS[(step + u) % len(KINDS)], state[u].shape[0], down, rows) for u in range(units)]
                    out, done = _check_launch(raw, counts, state, tabs_np, down, c, pend, tables, dev)
                    if done[0]:
                        assert bool((out[0, :done[0], 0].view(torch.int32) == QNAN32).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_kernel_equals_gdn_prep_ticks_with_the_units_table_and_the_same_rows_differ_between_units(dtype, gpu_device):
    from gdn_amd import ops
    dev = gpu_device
    units, n, c, down = 3, 130, 5, 10
    g = gen(units, n, c, down, 4)
    tables = _tables(units, n, g, dev)
    raw = raw_ticks(g, c * down, dtype, dev, 1, n).expand(units, -1, -1).contiguous()  # every unit reads the SAME rows
    raw[(torch.rand((units, c * down, n), generator=g) < 0.1).to(dev)] = float("nan")
    pend = ops.fleet_prep_state(units, n, down, dev)
    out = torch.full((units, c, n), SENTINEL, device=dev)
    counts = _i32([0] * units, dev)
    ops.fleet_prep_ticks(raw, _i32([c * down] * units, dev), pend, down, tables, out, counts)
    assert counts.tolist() == [c] * units and not ops.fleet_prep_views(pend, units, n, down)[1].any()
    planes = [torch.zeros((down - 1, n), dtype=torch.float64, device=dev) for _ in range(2)]
    for u in range(units):
        single = torch.full((c, n), SENTINEL, device=dev)
        assert ops.prep_ticks(raw[u], planes[0], 0, planes[1], down, tables[u], single) == c
        assert torch.equal(out[u].view(torch.int32), single.view(torch.int32)), u
    # a kernel that read tables[0] for every unit would make unit 0's table the others' too
    clean = raw_ticks(g, c * down, dtype, dev, 1, n).expand(units, -1, -1).contiguous()
    ops.fleet_prep_ticks(clean, _i32([c * down] * units, dev), pend, down, tables, out, counts)
    assert not torch.equal(out[1], out[0]) and not torch.equal(out[2], out[0]) and not torch.equal(out[2], out[1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_the_shared_entry_point_equals_the_per_unit_one_given_u_copies_of_its_table(dtype, gpu_device):
    from gdn_amd import ops
    dev = gpu_device
    units, n, c, down = 3, 65, 5, 3
    g = gen(units, n, c, down, 5)
    table = _table(n, g, dev)
    copies = table.unsqueeze(0).expand(units, -1, -1).contiguous()
    pends = [ops.fleet_prep_state(units, n, down, dev) for _ in range(2)]
    for counts in ([7, 0, 15], [15, 4, 1], [0, 0, 2]):
        raw = raw_ticks(g, c * down, dtype, dev, units, n)
        raw[(torch.rand((units, c * down, n), generator=g) < 0.1).to(dev)] = float("nan")
        outs = [torch.full((units, c, n), SENTINEL, device=dev) for _ in range(2)]
        done = [_i32([-9] * units, dev) for _ in range(2)]
        ops.fleet_prep_ticks(raw, _i32(counts, dev), pends[0], down, table, outs[0], done[0])
        ops.fleet_prep_ticks(raw, _i32(counts, dev), pends[1], down, copies, outs[1], done[1])
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)) and torch.equal(done[0], done[1])
        assert torch.equal(pends[0], pends[1])
    with pytest.raises(ValueError, match=r"tables of shape \[3, 65, 2\]"):
        ops.fleet_prep_ticks(raw, _i32(counts, dev), pends[1], down, copies[:2].contiguous(), outs[1], done[1])


# ------------------------------------------------------------------------------------ StreamFleet(prep=PrepUnits)
SCRIPT = [(5, None), (7, [7, 3, 0]), (16, None), (3, [0, 3, 1]), (37, None), (37, [37, 20, 5]), (2, [1, 2, 0])]
OPTIONS = {"plain": dict(), "gaps_events_recal": {k: v for k, v in ALL.items() if k in ("gaps", "events", "recal", "recal_min")}}


def _raw(g, r, dtype, dev, gaps):
    raw = raw_ticks(g, r, dtype, dev)
    if gaps:
        raw[0, :, 3] = float("nan")                              # a sensor of unit 0 out for the whole stream
        raw[1, 0, 5] = float("inf")                              # one reading: left out of its median
    return raw


def _drive(fleet, dets, script, g, dtype, dev):
    """Push `script`; where a detector's last push completed what its unit completed in the fleet's last cut, the
    returned rows (top scores, top sensors, alarm) are compared too.  Returns how many such comparisons were made."""
    compared = 0
    for r, counts in script:
        got, last = push_both(fleet, dets, _raw(g, r, dtype, dev, fleet.with_gaps), counts)
        for u, gu in enumerate(fleet.counts.tolist()):
            if u in last and gu and last[u][0].shape[0] == gu:
                for a, b, what in zip(got, last[u], ("top_scores", "top_sensors", "alarm")):
                    assert same(a[u, :gu], b), (r, counts, u, what)
                compared += 1
    return compared


@pytest.mark.parametrize("case", ["plain-graph-f32", "plain-eager-f64", "gaps_events_recal-graph-f64"])
def test_a_per_unit_prep_fleet_writes_the_bits_of_one_detector_per_unit_with_that_units_table(case, gpu_device, tmp_path):
    from gdn_amd import harness
    from gdn_amd.prep import PrepUnits
    dev = gpu_device
    options, how, raw_dtype = case.split("-")
    dtype = torch.float32 if raw_dtype == "f32" else torch.float64
    kw = OPTIONS[options]
    prep = make_prep_units(dev)
    model, fleet, seeds = build(dev, kw, prep, use_graph=how == "graph")
    dets = detectors(model, fleet, seeds, kw)
    assert all(same(dets[u].prep.table, prep.tables[u]) for u in range(UNITS))
    g = gen(21)
    compared = _drive(fleet, dets, SCRIPT[:4], g, dtype, dev)
    first = dict(fleet._prep_graphs)
    # save and load mid-stream: the loaded fleet goes on as the uninterrupted one
    path = str(tmp_path / "fleet.npz")
    fleet.save(path)
    back = harness.StreamFleet.load(path, model, prep=prep, device=dev, use_graph=how == "graph")
    assert_same_memory(memory(fleet), memory(back))
    g2 = gen(22)
    compared += _drive(fleet, dets, SCRIPT[4:], g2, dtype, dev)
    g2 = gen(22)
    for r, counts in SCRIPT[4:]:
        back.push(_raw(g2, r, dtype, dev, back.with_gaps), counts)
    assert compared >= 4 and int(fleet.status()[1].sum()) > 0
    if how == "graph":
        assert list(fleet._prep_graphs) == [dtype] and fleet._prep_graphs[dtype] is first[dtype] and fleet.graph is None
    if fleet.recal:
        fleet.recalibrate()
        back.recalibrate()
        for det in dets.values():
            det.recalibrate()
    for u in range(UNITS):
        assert_unit_is(fleet, u, dets[u], case)
        if fleet.events is not None:
            for a, b in zip(fleet.episodes(u), dets[u].episodes()):
                assert same(a, b), u
    assert_same_memory(memory(fleet), memory(back))
    # the file knows which tables it was saved under
    with pytest.raises(ValueError, match="fleet checkpoint: prep_units_sha256.*one shared Prep"):
        harness.StreamFleet.load(path, model, prep=make_prep(dev), device=dev)
    with pytest.raises(ValueError, match="fleet checkpoint: prep_units_sha256 differs"):
        harness.StreamFleet.load(path, model, prep=PrepUnits.from_preps([prep.unit(2), prep.unit(1), prep.unit(0)]),
                                 device=dev)
    with pytest.raises(ValueError, match="per-unit tables of 4 units"):
        harness.StreamFleet.load(path, model, prep=make_prep_units(dev, units=UNITS + 1), device=dev)


def test_a_shared_prep_file_refuses_per_unit_tables_and_from_calibration_takes_them(gpu_device, tmp_path):
    from gdn_amd import harness
    from _fleet_case import MSL, model_on
    dev = gpu_device
    model, fleet, _ = build(dev, {}, make_prep(dev))
    fleet.push(raw_ticks(gen(23), 6, torch.float32, dev))
    path = str(tmp_path / "shared.npz")
    fleet.save(path)
    assert "prep_units_sha256" not in harness.read_stream_checkpoint(path)             # the file is what it always was
    with pytest.raises(ValueError, match="fleet checkpoint: prep_units_sha256.*resumed with per-unit tables"):
        harness.StreamFleet.load(path, model, prep=make_prep_units(dev), device=dev)
    harness.StreamFleet.load(path, model, prep=make_prep(dev), device=dev)
    msl, n = model_on(dev, MSL), MSL[0]
    prep = make_prep_units(dev, n=n)
    series = torch.rand((UNITS, n, 120), generator=gen(12)).to(dev)
    cal = harness.StreamFleet.from_calibration(msl, series, CHUNK, top_m=2, wide=False, prep=prep)
    assert cal.prep is prep
    with pytest.raises(ValueError, match="per-unit tables of 2 units, the fleet has units = 3"):
        harness.StreamFleet.from_calibration(msl, series, CHUNK, prep=make_prep_units(dev, n=n, units=2))
