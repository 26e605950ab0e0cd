"""GPU suite of the alarm episodes: gdn_episodes_scan and gdn_stream_events against the sequential
definition in tests/_episodes_ref.py.  Nothing here is floating-point arithmetic, so every comparison is exact
(torch.equal / the 64-bit patterns of the peaks).

The archive kernels' borders: a thread owns 8 ticks, a wave 512, a workgroup one tile of 2048; the scan of the tile
aggregates gives a thread one tile up to 256 tiles and two beyond.  T = 1, 2: one thread; 255, 256, 257: a partial
wave, thread 31's last tick, thread 32's first; 2047, 2048, 2049: the tile border; 4097: three tiles, the last of one
tick; 70001: 35 tiles, a ragged tail; 600001: 293 tiles, two per thread of the aggregate scan."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _episodes_ref as ref

pytestmark = pytest.mark.gpu

TILE = 2048
HI, LO = 1.0, 0.5
A, B, MID, NAN = 2.0, 0.0, 0.7, float("nan")
SIZES = (1, 2, 255, 256, 257, 2047, 2048, 2049, 4097, 70001)
DELAYS = ((1, 1), (3, 5), (64, 2), (4096, 4096))


def _pattern(on, off):
    """(scores, offsets): every feature of the issue's list once, and the offset of the tick each one turns on (its
    last tick for a run that must or must not raise / clear, its first for the others)."""
    parts, marks, at = [], [], 0

    def add(values, mark=None):
        nonlocal at
        values = list(values)
        if mark is not None and values:
            marks.append(at + (len(values) - 1 if mark == "last" else 0))
        parts.extend(values)
        at += len(values)
    add([A] * on + [3.0], "first")                      # an episode raised at tick on - 1 (shift 0)
    add([B] * off)
    add([A] * (on - 1), "last")                         # on - 1 above ticks: must not raise
    add([B] * off)
    add([A] * on, "last")                               # exactly on: raises on its last tick
    add([MID] * 3, "first")                             # strictly between lo and hi: neither
    add([B] * (off - 1), "last")                        # off - 1 below ticks inside an episode: must not clear
    add([2.5, 3.0, 3.0, 2.5], "first")                  # equal peaks: the first one wins
    add([NAN] * max(1, off - 1), "first")               # NaN scores are below (and never the peak)
    add([A, -0.0, A])
    add([B] * off, "last")                              # clears on its last tick
    add([MID, NAN, MID])
    add([A] * (on + TILE + 7), "first")                 # a run over two tiles (three once shifted)
    add([B] * (off + 1))
    add([A] * (on + 2 * TILE + 3), "first")             # ... over three
    add([MID] * 2 + [B] * off)
    add([A] * on + [B] * off, "first")                  # short episodes back to back
    add([A] * on + [B] * off)
    return np.array(parts, dtype=np.float64), marks


def _crafted(T, on, off, shift=0):
    p, _ = _pattern(on, off)
    s = np.concatenate([np.full(shift, B), np.tile(p, (T - shift) // len(p) + 1)])[:T]
    return np.ascontiguousarray(s)


def _sensors(T, m, seed=0):
    return np.random.default_rng(seed + T).integers(0, 4000, size=(T, m), dtype=np.int32)


def _scan(dev, s, sens, hi, lo, on, off, cap, first_tick=0, **kw):
    from gdn_amd import ops
    t = ops.episodes_scan(torch.from_numpy(s).to(dev), torch.from_numpy(sens).to(dev), hi, lo, on, off, cap, first_tick,
                          **kw)
    return t


def _host(table, cap):
    start, end, peak_tick, peak, sensors, count = table
    count = int(count.item())
    rows = min(count, cap)
    return {"start": start[:rows].cpu().numpy(), "end": end[:rows].cpu().numpy(), "peak": peak[:rows].cpu().numpy(),
            "peak_tick": peak_tick[:rows].cpu().numpy(), "sensors": sensors[:rows].cpu().numpy(), "count": count}


def _cut(want, cap):
    out = {k: (v if k == "count" else v[:cap]) for k, v in want.items()}
    return out


def _check(dev, s, sens, hi, lo, on, off, first_tick=0, grids=(0, 1, 7)):
    """The scan at cap 4096 against the reference, twice and through forced grids; then cap = 3 and cap = 0."""
    want = ref.episodes(s, sens, hi, lo, on, off, 4096, first_tick)
    got = None
    for g in grids + (0,):
        again = _host(_scan(dev, s, sens, hi, lo, on, off, 4096, first_tick, grid=g), 4096)
        assert ref.same(again, want), (len(s), on, off, g, again["count"], want["count"])
        got = again
    for cap in (3, 0):
        small = _host(_scan(dev, s, sens, hi, lo, on, off, cap, first_tick), cap)
        assert ref.same(small, _cut(want, cap)), (len(s), on, off, cap)
    return got


@pytest.mark.parametrize("T", SIZES)
@pytest.mark.parametrize("on,off", DELAYS)
def test_scan_equals_the_definition_at_every_border_size(T, on, off, gpu_device):
    m = (1, 3, 8)[(T + on) % 3]
    s, sens = _crafted(T, on, off), _sensors(T, m)
    got = _check(gpu_device, s, sens, HI, LO, on, off, first_tick=5)
    if T >= 2 * (on + off) + 8:
        assert got["count"] >= 2
    if T > on:
        assert got["start"][0] == 5                     # raised at tick on - 1


@pytest.mark.parametrize("on,off", DELAYS)
def test_every_feature_on_the_tile_border_and_away_from_it(on, off, gpu_device):
    p, marks = _pattern(on, off)
    shifts = sorted({(TILE - k) % TILE for k in marks} | {(TILE - 1 - k) % TILE for k in marks[:4]} | {700})
    for shift in shifts:
        T = shift + len(p) + 5                          # ends inside the next copy's first run: open at the last tick
        s = _crafted(T, on, off, shift)
        got = _check(gpu_device, s, _sensors(T, 3, shift), HI, LO, on, off, grids=(0,) if shift % 3 else (0, 2))
        assert got["count"] >= 3, shift
    s = _crafted(len(p) + on + 1, on, off)              # the last episode is open at the last tick
    got = _check(gpu_device, s, _sensors(len(s), 1), HI, LO, on, off, grids=(0,))
    assert got["end"][-1] == -1 or got["count"] > 4096


def test_more_tiles_than_threads_in_the_aggregate_scan(gpu_device):
    T = 600001
    s = _crafted(T, 3, 5)
    got = _check(gpu_device, s, _sensors(T, 2), HI, LO, 3, 5, grids=(0, 3))
    assert got["count"] > 256                           # (cap = 3 inside _check: more episodes than the table keeps)


def test_no_episode_negative_levels_and_a_random_series(gpu_device):
    dev = gpu_device
    g = np.random.default_rng(11)
    s = g.standard_normal(9000).cumsum() * 0.2 + g.standard_normal(9000)
    sens = _sensors(9000, 3)
    assert _check(dev, s, sens, 1e9, 1e9, 1, 1)["count"] == 0
    hi = float(np.quantile(s, 0.9))
    for on, off, gap in ((1, 1, 0.0), (3, 5, 0.3), (64, 2, 0.1)):
        got = _check(dev, s, sens, hi, hi - gap, on, off, first_tick=123456789012)
        assert got["count"] >= 1
    neg = -np.abs(s) - 1.0
    got = _check(dev, neg, sens, float(np.quantile(neg, 0.8)), float(np.quantile(neg, 0.6)), 2, 3)
    assert got["count"] >= 1 and (got["peak"] < 0).all()


@pytest.mark.parametrize("on,off", DELAYS)
def test_pieces_chained_through_the_carry_equal_one_scan(on, off, gpu_device):
    from gdn_amd import ops
    dev = gpu_device
    p, marks = _pattern(on, off)
    T = len(p) + 3 * TILE
    s, sens = _crafted(T, on, off, 17), _sensors(T, 3)
    want = ref.episodes(s, sens, HI, LO, on, off, 64, first_tick=9)
    assert want["count"] >= 4
    inside = 17 + marks[-3] + on + 5                    # inside the run over three tiles
    for cuts in ([1], [TILE], [inside], sorted({1, 2, TILE, inside, inside + 1, T - 1})):
        table = ops.episodes_table(64, 3, dev)
        carry = torch.zeros((ops.EPISODES_CARRY_WORDS,), dtype=torch.int64, device=dev)
        at = 0
        for c in cuts + [T]:
            _scan(dev, s[at:c], sens[at:c], HI, LO, on, off, 64, first_tick=9 + at, carry_in=carry if at else None,
                  carry_out=carry, table=table)
            at = c
        assert ref.same(_host(table, 64), want), cuts
        assert int(carry[0]) == want["count"]


def test_argument_errors_arrive_before_any_launch(gpu_device):
    from gdn_amd import _lib, ops
    dev = gpu_device
    lib = _lib.load()
    T, m, cap = 100, 2, 8
    s = torch.from_numpy(_crafted(T, 1, 1)).to(dev)
    sens = torch.from_numpy(_sensors(T, m)).to(dev)
    table = [t.fill_(-7) for t in ops.episodes_table(cap, m, dev)]
    before = [t.clone() for t in table]
    ws = torch.zeros((lib.gdn_episodes_workspace_bytes(T, cap) // 8,), dtype=torch.int64, device=dev)
    start, end, peak_tick, peak, sensors, count = table

    def call(T=T, m=m, hi=HI, lo=LO, on=1, off=1, first=0, E=cap, scores=s, ws=ws, count=count):
        ptr = lambda t: None if t is None else t.data_ptr()
        return lib.gdn_episodes_scan(ptr(scores), ptr(sens), T, m, hi, lo, on, off, first, E, None, None, ptr(start),
                                     ptr(end), ptr(peak_tick), ptr(peak), ptr(sensors), ptr(count), ptr(ws), None)
    ARG, UNSUPPORTED = -1, -3
    assert call(lo=2.0) == ARG and call(hi=float("nan")) == ARG and call(lo=float("nan")) == ARG
    assert call(scores=None) == ARG and call(ws=None) == ARG and call(count=None) == ARG and call(first=-1) == ARG
    assert call(T=0) == UNSUPPORTED and call(T=(1 << 26) + 1) == UNSUPPORTED and call(m=0) == UNSUPPORTED
    assert call(m=9) == UNSUPPORTED and call(on=0) == UNSUPPORTED and call(on=4097) == UNSUPPORTED
    assert call(off=0) == UNSUPPORTED and call(off=4097) == UNSUPPORTED and call(E=-1) == UNSUPPORTED
    assert call(E=(1 << 20) + 1) == UNSUPPORTED
    assert lib.gdn_episodes_workspace_bytes(0, 8) == 0 and lib.gdn_episodes_workspace_bytes(8, -1) == 0
    # the stream form
    ev = ops.stream_events_alloc(m, cap, dev).fill_(-7)
    ev0 = ev.clone()
    state = torch.zeros((64,), dtype=torch.int64, device=dev)
    ts = torch.zeros((16, m), dtype=torch.float64, device=dev)
    ti = torch.zeros((16, m), dtype=torch.int32, device=dev)
    thr = torch.ones((1,), dtype=torch.float64, device=dev)

    def push(c=16, count=16, m=m, on=1, off=1, E=cap, state=state, events=ev):
        ptr = lambda t: None if t is None else t.data_ptr()
        return lib.gdn_stream_events(ptr(state), ts.data_ptr(), ti.data_ptr(), thr.data_ptr(), thr.data_ptr(), c, count,
                                     m, on, off, E, ptr(events), None)
    assert push(state=None) == ARG and push(events=None) == ARG and push(count=0) == ARG and push(count=17) == ARG
    assert push(c=4097, count=4097) == UNSUPPORTED and push(m=9) == UNSUPPORTED and push(on=0) == UNSUPPORTED
    assert push(off=4097) == UNSUPPORTED and push(E=-1) == UNSUPPORTED
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(table, before)) and torch.equal(ev, ev0)
    ev.zero_()
    assert call() == 0 and push() == 0                   # and the same calls with sound arguments run
    torch.cuda.synchronize()
    assert int(count.item()) == ref.episodes(s.cpu().numpy(), sens.cpu().numpy(), HI, LO, 1, 1, cap)["count"]


# ------------------------------------------------------------------------------------------------ stream = archive
STREAM_T = 420
MODELS = {"small": (12, 4, 3, 16), "planned": (40, 10, 8, 64)}
EVENTS = dict(on=3, off=4, cap=32)


@functools.lru_cache(maxsize=None)
def _stream_case(name, dev, gaps=False):
    """(model, series [n, w + T] on the device, the evaluator after its step, hi, lo, the reference's table): a random
    series with planted excursions, hi chosen among fixed quantiles of the evaluator's scores so that the reference
    finds 3 to 20 episodes."""
    from gdn_amd import harness
    from test_gpu_stream import _model
    n, w, k, d = MODELS[name]
    model = _model(dev, n, w, k, d)
    g = torch.Generator().manual_seed(99 + n)
    s = torch.rand((n, w + STREAM_T), generator=g)
    for j, t0 in enumerate(range(w + 30, w + STREAM_T - 30, 45)):      # excursions of 6 .. 22 ticks on two sensors
        s[(3 * j) % n, t0:t0 + 6 + 2 * j] += 3.0 + 0.5 * j
        s[(5 * j + 1) % n, t0 + 2:t0 + 5 + j] += 2.0
    if gaps:
        s[:, w:][torch.rand((n, STREAM_T), generator=g) < 0.02] = float("nan")
        s[2, w + 100:w + 130] = float("inf")
    s = s.to(dev)
    if gaps:
        ev = harness.SeriesEvaluator(model, None, None, batch=128, use_graph=False, series=s, top_m=3, gaps=True,
                                     min_kept=32)
    elif d < 32:                                        # (no series kernel below d = 32: the evaluator reads windows)
        windows = s.unfold(1, w, 1).permute(1, 0, 2)[:STREAM_T].contiguous()
        ev = harness.SeriesEvaluator(model, windows, s[:, w:].t().contiguous(), batch=128, use_graph=False, top_m=3)
    else:
        ev = harness.SeriesEvaluator(model, None, s[:, w:].t().contiguous(), batch=128, use_graph=False, series=s, top_m=3)
    ev.step()
    scores, sens = ev.top_scores[:, 0].cpu().numpy(), ev.top_sensors.cpu().numpy()
    for q in (0.9, 0.85, 0.8, 0.7, 0.95):
        hi = float(np.quantile(scores, q))
        lo = hi - 0.25 * abs(hi)
        want = ref.episodes(scores, sens, hi, lo, EVENTS["on"], EVENTS["off"], EVENTS["cap"])
        if 3 <= want["count"] <= 20:
            break
    assert 3 <= want["count"] <= 20, want["count"]      # the precondition: an empty table cannot pass
    raw = ev.raw_series if gaps else s
    return model, raw, ev, hi, lo, want


def _pushes(kind, chunk):
    if kind == "mixed":
        sizes, at, out = (1, 3, chunk, 2, chunk + 2, chunk, 5), 0, []
        while at < STREAM_T:
            for r in sizes:
                if at < STREAM_T:
                    out.append((at, min(STREAM_T, at + r)))
                    at += r
        return out
    r = {"one": 1, "three": 3, "chunk": chunk, "chunk_plus_two": chunk + 2}[kind]
    return [(t0, min(STREAM_T, t0 + r)) for t0 in range(0, STREAM_T, r)]


def _detector(model, s, w, ev, hi, lo, chunk, events=True, **kw):
    from gdn_amd import harness
    return harness.StreamDetector(model, ev.med_iqr, hi, s[:, :w].contiguous(), chunk, top_m=3,
                                  events=dict(EVENTS, lo=lo) if events else None, **kw)


@pytest.mark.parametrize("name", list(MODELS))
@pytest.mark.parametrize("kind", ["one", "three", "chunk", "chunk_plus_two", "mixed"])
@pytest.mark.parametrize("use_graph", [True, False])
def test_stream_table_equals_the_archive_scan_and_the_definition(name, kind, use_graph, gpu_device):
    from gdn_amd import harness
    model, s, ev, hi, lo, want = _stream_case(name, gpu_device)
    w, chunk = MODELS[name][1], 16
    archive = harness.episodes(ev, hi, lo, on=EVENTS["on"], off=EVENTS["off"], cap=EVENTS["cap"])
    assert ref.same(archive.numpy(), want)
    det = _detector(model, s, w, ev, hi, lo, chunk, use_graph=use_graph)
    stream = s[:, w:].t().contiguous()
    for a, b in _pushes(kind, chunk):
        det.push(stream[a:b])
    got = det.episodes()
    assert ref.same(got.numpy(), want)
    rows = min(want["count"], EVENTS["cap"])
    for name_ in ("start", "end", "peak_tick", "sensors"):
        assert torch.equal(getattr(got, name_)[:rows], getattr(archive, name_)[:rows])
    assert torch.equal(got.peak[:rows].view(torch.int64), archive.peak[:rows].view(torch.int64))
    status = det.status()
    assert status[0] == STREAM_T and status[-2:] == (want["count"], bool(want["end"][-1] == -1))
    loc = harness.localise(ev, archive.peak_tick[:rows])               # one localisation per incident
    assert loc.ticks.shape[0] == rows and torch.equal(loc.sensors[:, 0].int(), archive.sensors[:rows, 0])


@pytest.mark.parametrize("kind", ["chunk", "mixed"])
def test_stream_with_missing_readings_and_with_a_ring(kind, gpu_device):
    from gdn_amd import harness
    dev = gpu_device
    model, s, ev, hi, lo, want = _stream_case("small", dev, True)
    w, chunk = MODELS["small"][1], 16
    stream = s[:, w:].t().contiguous()
    det = _detector(model, s, w, ev, hi, lo, chunk, gaps=True)
    for a, b in _pushes(kind, chunk):
        det.push(stream[a:b])
    assert ref.same(det.episodes().numpy(), want)
    assert ref.same(harness.episodes(ev, hi, lo, on=EVENTS["on"], off=EVENTS["off"], cap=EVENTS["cap"]).numpy(), want)
    model, s, ev, hi, lo, want = _stream_case("small", dev)
    stream = s[:, w:].t().contiguous()
    with_events = _detector(model, s, w, ev, hi, lo, chunk, recal=64)
    without = _detector(model, s, w, ev, hi, lo, chunk, events=False, recal=64)
    for a, b in _pushes(kind, chunk):
        with_events.push(stream[a:b])
        without.push(stream[a:b])
    assert ref.same(with_events.episodes().numpy(), want)
    assert torch.equal(with_events.ring_keys.view(torch.int64), without.ring_keys.view(torch.int64))
    assert torch.equal(with_events.ring_keep, without.ring_keep)


def test_save_mid_episode_load_and_continue(tmp_path, gpu_device):
    from gdn_amd import harness
    dev = gpu_device
    model, s, ev, hi, lo, want = _stream_case("small", dev)
    w, chunk = MODELS["small"][1], 16
    stream = s[:, w:].t().contiguous()
    ends = np.where(want["end"] < 0, STREAM_T, want["end"])
    j = int(np.argmax(ends - want["start"]))            # the longest episode
    cut = int(want["start"][j]) + 2                     # two ticks into it: above, not raised yet (on = 3)
    cut2 = int(want["peak_tick"][j]) + 1                # ... and raised, just after its peak
    assert 0 < cut < cut2 <= STREAM_T
    path = str(tmp_path / "det.npz")
    for at in (cut, cut2):
        first = _detector(model, s, w, ev, hi, lo, chunk)
        for a in range(0, at, 7):
            first.push(stream[a:min(at, a + 7)])
        first.save(path)
        second = harness.StreamDetector.load(path, model, device=dev)
        assert second.events_cfg == first.events_cfg and torch.equal(second.clear, first.clear)
        for a in range(at, STREAM_T, chunk):
            second.push(stream[a:a + chunk])
        assert ref.same(second.episodes().numpy(), want), at
    keys = set(np.load(path).files)
    plain = _detector(model, s, w, ev, hi, lo, chunk, events=False)
    plain.push(stream[:chunk])
    plain_path = str(tmp_path / "plain.npz")
    plain.save(plain_path)
    assert keys - set(np.load(plain_path).files) == {"events", "events_cfg", "events_lo"}
    # mismatched configurations are refused by the field's name, on real files
    with pytest.raises(ValueError, match="events: the detector was saved with"):
        plain.load_state_dict(harness.read_stream_checkpoint(path))
    with pytest.raises(ValueError, match="events: the detector was saved without"):
        first.load_state_dict(harness.read_stream_checkpoint(plain_path))
    for field, value in (("on", 2), ("off", 9), ("cap", 8)):
        other = harness.StreamDetector(model, ev.med_iqr, hi, s[:, :w].contiguous(), chunk, top_m=3,
                                       events=dict(dict(EVENTS, lo=lo), **{field: value}))
        with pytest.raises(ValueError, match=rf"events\.{field} = "):
            other.load_state_dict(harness.read_stream_checkpoint(path))
    other = harness.StreamDetector(model, ev.med_iqr, hi, s[:, :w].contiguous(), chunk, top_m=2, events=dict(EVENTS, lo=lo))
    with pytest.raises(ValueError, match=r"events\.m = |top_m"):
        other.load_state_dict(harness.read_stream_checkpoint(path))


@pytest.mark.parametrize("use_graph", [True, False])
def test_off_means_off(use_graph, gpu_device):
    dev = gpu_device
    model, s, ev, hi, lo, want = _stream_case("small", dev)
    w, chunk = MODELS["small"][1], 16
    stream = s[:, w:].t().contiguous()
    on = _detector(model, s, w, ev, hi, lo, chunk, use_graph=use_graph, log=64)
    off = _detector(model, s, w, ev, hi, lo, chunk, events=False, use_graph=use_graph, log=64)
    assert off.events is None and off.clear is None and len(off.status()) == 4
    for a, b in _pushes("mixed", chunk):
        outs = [d.push(stream[a:b]) for d in (on, off)]
        for x, y in zip(*outs):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
        assert torch.equal(on.pred[:b - a], off.pred[:b - a])
    assert torch.equal(on.state, off.state) and torch.equal(on.log_ticks, off.log_ticks)
    assert torch.equal(on.log_sensors, off.log_sensors)
    assert set(on.state_dict()) - set(off.state_dict()) == {"events", "events_cfg", "events_lo"}
    with pytest.raises(ValueError, match="events=None"):
        off.episodes()
