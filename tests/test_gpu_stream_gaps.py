"""GPU suite of the streaming detector's missing readings: gdn_stream_fill / _score_gaps /
_advance_gaps and harness.StreamDetector(gaps=True) against tests/_stream_gaps_ref.py.  The fill is exact
(torch.equal), a stream without a missing reading gives the bits of a gaps=False detector, a stream with missing
readings gives the windows and predictions of a gaps=False detector pushed the filled ticks, the scores meet the
scoring suite's float64 bar (rtol 1e-12, atol 1e-13), and nothing depends on how the stream is cut into pushes."""

import numpy as np
import pytest
import torch

import _stream_gaps_ref as gref
from conftest import load_golden
from test_gpu_stream import PLANNED, _detector, _model, _table

pytestmark = pytest.mark.gpu

T = 37
NS, WS = (1, 5, 63, 65, 130), (3, 15)
COUNTS = (1, 2, 3, 7, 8, 9, 37)
NAN, INF = float("nan"), float("inf")
RTOL, ATOL = 1e-12, 1e-13                # test_top_scores_agree_with_the_float64_helper's bar


def _missing_pattern(raw, w, chunk):
    """The missing readings of every test, written into raw [T', n] (a clone is returned) for pushes of `chunk`:
    row 0 of the first push (it reaches into hist) and of the second; a run across a push boundary; a run across a
    segment boundary of the fill (rows 6 .. 9: the fill cuts a push of 17 .. 64 rows into segments of 2, 3 or 4 rows,
    a shorter one into single rows); a sensor missing for a whole push and for more than w ticks in all; every
    sensor missing at one tick; +inf and -inf."""
    raw = raw.clone()
    t, n = raw.shape
    s = lambda j: j % n
    raw[0, s(0)] = NAN
    if chunk < t:
        raw[chunk, s(4)] = NAN
        raw[max(0, chunk - 2):chunk + 2, s(1)] = NAN
    raw[6:10, s(2)] = NAN
    start = chunk if 2 * chunk <= t else 0
    raw[start:min(t, start + max(chunk, w + 1)), s(3)] = NAN
    if t > 12:
        raw[12, :] = NAN
    if t > 15:
        raw[14, s(0)] = INF
        raw[15, s(n - 1)] = -INF
        raw[15, s(5)] = INF
    return raw


def _stream_of(n, w, t=T, seed=0):
    g = torch.Generator().manual_seed(seed + 7 * n + w)
    return torch.rand((n, w), generator=g), torch.rand((t, n), generator=g)


# ------------------------------------------------------------------------------------------------ 1. the fill alone
@pytest.mark.parametrize("w", WS)
@pytest.mark.parametrize("n", NS)
def test_fill_equals_ffill_and_leaves_rows_beyond_count_alone(n, w, gpu_device):
    from gdn_amd import ops
    dev = gpu_device
    c = 64
    history, clean = _stream_of(n, w, t=c)
    state = ops.stream_state(history.to(dev), w)
    before = state.clone()
    for count in COUNTS + (c,):
        raw = _missing_pattern(clean[:count], w, count)
        if count >= 3:
            raw[:, (n - 1) % n] = NAN                                # a sensor with no real reading in the push
            raw[count - 1, 0] = NAN                                  # a trailing run that ends the push
        buf = torch.full((c, n), -7.0)
        buf[:count] = raw
        filled = torch.full((c, n), -7.0, device=dev)
        valid = torch.full((c, n), 9, dtype=torch.uint8, device=dev)
        gap_chunk = torch.full((2, n), -9, dtype=torch.int32, device=dev)
        ops.stream_fill(state, buf.to(dev), w, filled, valid, gap_chunk, count=count)
        want_f, want_v, want_missing, want_trail = gref.ffill(raw.numpy(), history[:, -1].numpy())
        assert torch.equal(filled[:count].cpu(), torch.from_numpy(want_f)), (n, w, count)
        assert torch.equal(valid[:count].cpu(), torch.from_numpy(want_v.astype(np.uint8))), (n, w, count)
        assert gap_chunk.cpu().tolist() == [want_missing.tolist(), want_trail.tolist()], (n, w, count)
        assert (filled[count:] == -7.0).all() and (valid[count:] == 9).all()      # rows >= count keep the sentinel
        assert torch.isfinite(filled[:count]).all()
    assert torch.equal(state, before)                                # the fill writes none of the state


# ------------------------------------------------------------------------------------------------ the launches, no model
def _push_ops(history, raw, pred, med_iqr, chunk, m, thr, dev):
    """The gap launches of a push with `pred` [T, n] standing in for the forward: concatenated outputs and the end."""
    from gdn_amd import ops
    n, w = history.shape
    t = raw.shape[0]
    state = ops.stream_state(history.to(dev), w)
    c = chunk
    raw_buf, chunk_buf, pbuf = (torch.zeros((c, n), device=dev) for _ in range(3))
    valid = torch.zeros((c, n), dtype=torch.uint8, device=dev)
    gap_chunk = torch.zeros((2, n), dtype=torch.int32, device=dev)
    gaps = torch.zeros((2, n), dtype=torch.int64, device=dev)
    ts = torch.zeros((c, m), dtype=torch.float64, device=dev)
    ti = torch.zeros((c, m), dtype=torch.int32, device=dev)
    al = torch.zeros((c,), dtype=torch.int32, device=dev)
    log_t = torch.zeros((64,), dtype=torch.int64, device=dev)
    log_s = torch.zeros((64, m), dtype=torch.int32, device=dev)
    threshold = torch.tensor([thr], dtype=torch.float64, device=dev)
    outs = []
    for t0 in range(0, t, c):
        r = min(c, t - t0)
        raw_buf[:r].copy_(raw[t0:t0 + r])
        pbuf[:r].copy_(pred[t0:t0 + r])
        ops.stream_fill(state, raw_buf, w, chunk_buf, valid, gap_chunk, count=r)
        ops.stream_score(state, pbuf, chunk_buf, med_iqr, threshold, m, ts, ti, al, count=r, valid=valid)
        ops.stream_advance(state, chunk_buf, pbuf, med_iqr, al, ti, w, m, log_t, log_s, count=r, valid=valid,
                           gap_chunk=gap_chunk, gaps=gaps)
        outs.append((chunk_buf[:r].clone(), valid[:r].clone(), ts[:r].clone(), ti[:r].clone(), al[:r].clone()))
    cat = tuple(torch.cat([o[j] for o in outs]) for j in range(5))
    return cat, state, gaps, log_t, log_s


def _assert_scores(ts, ti, vals, idx, what):
    got = ts.cpu().numpy()
    assert not np.isnan(got).any(), what
    worst = np.abs(got - vals).max()
    print(f"{what}: worst absolute top-score error against float64 {worst:.2e}")
    np.testing.assert_allclose(got, vals, rtol=RTOL, atol=ATOL, err_msg=str(what))
    bar = ATOL + RTOL * np.abs(vals)
    apart = np.ones(vals.shape, dtype=bool)                          # rank r is apart from its neighbours in rank
    apart[:, :-1] &= (vals[:, :-1] - vals[:, 1:]) > 2 * bar[:, :-1]
    apart[:, 1:] &= (vals[:, :-1] - vals[:, 1:]) > 2 * bar[:, 1:]
    apart[:, -1] = False                                             # (its lower neighbour is not in the list)
    np.testing.assert_array_equal(ti.cpu().numpy()[apart], idx[apart], err_msg=str(what))


@pytest.mark.parametrize("w", WS)
@pytest.mark.parametrize("n", NS)
def test_launches_equal_the_ref_and_do_not_depend_on_the_push_size(n, w, gpu_device):
    dev = gpu_device
    m = min(3, n)
    history, clean = _stream_of(n, w, seed=1)
    pred = torch.rand((T, n), generator=torch.Generator().manual_seed(n + w))
    med_iqr = _table(n, dev)
    raw = _missing_pattern(clean, w, 8)                              # one pattern for every push size
    filled, valid, total, run = gref.ffill_chunked(raw.numpy(), history[:, -1].numpy(), T)
    delta = np.abs(pred.numpy().astype(np.float64) - filled.astype(np.float64))
    _sm, top, _idx, _fl, _st = gref.run_chunked(delta, valid, med_iqr.cpu().numpy(), T, m=m)
    srt = np.sort(top[:, 0])
    cut = int(np.argmax(np.diff(srt)))
    thr = float((srt[cut] + srt[cut + 1]) / 2)                       # in the widest gap of the top scores: no tick near it
    _sm, vals, idx, flags, want = gref.run_chunked(delta, valid, med_iqr.cpu().numpy(), T, m=m, threshold=thr)
    first = None
    for chunk in COUNTS:
        (f, v, ts, ti, al), state, gaps, log_t, log_s = _push_ops(history, raw, pred, med_iqr, chunk, m, thr, dev)
        assert torch.equal(f.cpu(), torch.from_numpy(filled)), chunk
        assert torch.equal(v.cpu(), torch.from_numpy(valid.astype(np.uint8))), chunk
        _assert_scores(ts, ti, vals, idx, (n, w, chunk))
        assert al.cpu().numpy().astype(bool).tolist() == flags.tolist(), chunk
        assert gaps.cpu().tolist() == [total.tolist(), run.tolist()], chunk
        assert gaps.cpu().tolist() == [want.missing_total.tolist(), want.missing_run.tolist()]
        from gdn_amd import ops
        counters, carry, hist = ops.stream_state_views(state, n, w)
        assert counters.tolist() == [T, int(flags.sum()), int(flags.sum())]
        assert log_t[:int(flags.sum())].cpu().tolist() == [tick for tick, _ in want.log]
        whole = np.concatenate([history.numpy(), filled.T], axis=1)
        assert torch.equal(hist.cpu(), torch.from_numpy(whole[:, -w:].copy())), chunk
        np.testing.assert_allclose(carry.cpu().numpy(), want.carry, rtol=1e-12, atol=1e-13)
        assert (carry.cpu().numpy()[~valid[-3:]] == 0.0).all()       # a missing reading's carry entry: exactly 0.0
        end = (ts, ti, al, state, gaps, log_t, log_s)
        if first is None:
            first = end
        for a, b in zip(end, first):                                 # chunk invariance, bit for bit
            assert torch.equal(a, b), chunk


# ------------------------------------------------------------------------------------------------ the detector
DETECTORS = {"n5": (5, 3, 3, 16), "n63": (63, 15, 10, 64), "n65": (65, 3, 10, 64), "n130": (130, 15, 10, 64),
             "planned": (20, 5, 4, 64), "staged": (20, 5, 4, 24)}


def _run(det, stream, chunk):
    """The stream in pushes of `chunk`: per push (x, pred, top_scores, top_sensors, alarm, valid or None, state)."""
    outs = []
    for t0 in range(0, stream.shape[0], chunk):
        ts, ti, al = det.push(stream[t0:t0 + chunk])
        r = len(al)
        outs.append((det.x[:r].clone(), det.pred[:r].clone(), ts.clone(), ti.clone(), al.clone(),
                     det.valid[:r].clone() if det.valid is not None else None, det.state.clone()))
    return outs


def _cat(outs, j):
    return torch.cat([o[j] for o in outs])


def _setup(shape, dev, seed=2):
    n, w = shape[:2]
    model = _model(dev, *shape)
    history, clean = _stream_of(n, w, seed=seed)
    s = torch.cat([history, clean.t()], dim=1)                       # test_gpu_stream's [n, w + T]: _detector cuts it
    return model, s, history, clean


@pytest.mark.parametrize("chunk", [5, 37])
@pytest.mark.parametrize("shape", ["n5", "n130"])
def test_without_a_missing_reading_the_detector_writes_the_bits_of_a_plain_one(shape, chunk, gpu_device):
    dev = gpu_device
    shape = DETECTORS[shape]
    n, w = shape[:2]
    model, s, _history, clean = _setup(shape, dev)
    med_iqr = _table(n, dev)
    stream = clean.to(dev)
    m = min(3, n)
    for use_graph in (True, False):                                  # replayed (chunk 5: six replays, a ragged push) and eager
        plain = _detector(model, s, w, chunk, dev, med_iqr=med_iqr, threshold=0.5, top_m=m, use_graph=use_graph)
        gappy = _detector(model, s, w, chunk, dev, med_iqr=med_iqr, threshold=0.5, top_m=m, use_graph=use_graph,
                          gaps=True)
        a, b = _run(plain, stream, chunk), _run(gappy, stream, chunk)
        for pa, pb in zip(a, b):                                     # after every push
            for j in (0, 1, 2, 3, 4, 6):
                assert torch.equal(pa[j], pb[j]), (j, use_graph)
            assert bool(pb[5].all())
        assert torch.equal(plain.log_ticks, gappy.log_ticks) and torch.equal(plain.log_sensors, gappy.log_sensors)
        assert plain.status()[:2] == gappy.status()[:2] and plain.status()[1] > 0
        total, run = gappy.status_gaps()
        assert not total.any() and not run.any()
        assert (gappy.graph is not None) == use_graph
    with pytest.raises(ValueError, match="gaps=False"):
        plain.status_gaps()


@pytest.mark.parametrize("shape", list(DETECTORS))
def test_with_missing_readings_windows_pred_scores_and_counters(shape, gpu_device):
    """Tests 3, 4 and 7 of the issue at every detector shape, the planned matrix-core route (n = 20, d = 64) and a
    staged route (d = 24) among them."""
    from gdn_amd import ops
    dev = gpu_device
    shape = DETECTORS[shape]
    n, w = shape[:2]
    chunk, m = 8, min(3, n)
    model, s, history, clean = _setup(shape, dev)
    med_iqr = _table(n, dev)
    raw = _missing_pattern(clean, w, chunk)
    filled, valid, total, run = gref.ffill_chunked(raw.numpy(), history[:, -1].numpy(), T)
    filled_t = torch.from_numpy(filled).to(dev)
    plain = _detector(model, s, w, chunk, dev, med_iqr=med_iqr, top_m=m)
    want = _run(plain, filled_t, chunk)
    pred = _cat(want, 1)
    delta = np.abs(pred.cpu().numpy().astype(np.float64) - filled.astype(np.float64))
    _sm, top, _i, _f, _s = gref.run_chunked(delta, valid, med_iqr.cpu().numpy(), chunk, m=m)
    srt = np.sort(top[:, 0])
    cut = int(np.argmax(np.diff(srt)))
    thr = float((srt[cut] + srt[cut + 1]) / 2)
    _sm, vals, idx, flags, ref_state = gref.run_chunked(delta, valid, med_iqr.cpu().numpy(), chunk, m=m, threshold=thr)
    det = _detector(model, s, w, chunk, dev, med_iqr=med_iqr, threshold=thr, top_m=m, gaps=True)
    got = _run(det, raw.to(dev), chunk)
    whole = torch.cat([history.to(dev), filled_t.t()], dim=1)
    t0 = 0
    for pg, pw in zip(got, want):                                    # after every push
        r = pg[0].shape[0]
        assert torch.equal(pg[0], pw[0]) and torch.equal(pg[1], pw[1]), t0
        assert torch.equal(pg[5].cpu(), torch.from_numpy(valid[t0:t0 + r].astype(np.uint8)))
        t0 += r
        hist = ops.stream_state_views(pg[6], n, w)[2]
        assert torch.equal(hist, whole[:, t0:t0 + w]), t0            # hist ends on the last w FILLED ticks
    assert torch.equal(det.chunk_buf[:T % chunk], filled_t[-(T % chunk):])
    _assert_scores(_cat(got, 2), _cat(got, 3), vals, idx, shape)
    al = _cat(got, 4).cpu().numpy().astype(bool)
    assert al.tolist() == flags.tolist() and flags.any() and not flags.all()
    missing_total, missing_run = det.status_gaps()
    assert missing_total.dtype == torch.int64 and missing_total.tolist() == total.tolist()
    assert missing_run.tolist() == run.tolist() == ref_state.missing_run.tolist()
    ticks, alarms, log_ticks, log_sensors = det.status()
    assert (ticks, alarms) == (T, int(flags.sum()))
    assert log_ticks.cpu().tolist() == np.nonzero(flags)[0].tolist()
    assert torch.equal(log_sensors, _cat(got, 3)[torch.from_numpy(np.nonzero(flags)[0]).to(dev)])
    # localise() reads the filled chunk
    loc = det.localise(rows=[0])
    assert torch.equal(loc.observed[0], det.chunk_buf[0, loc.sensors[0]]) and torch.isfinite(loc.observed).all()


def test_the_ticks_after_a_missing_reading_can_alarm(gpu_device):
    dev = gpu_device
    n, w = PLANNED[:2]
    model, s, history, clean = _setup(PLANNED, dev, seed=5)
    raw = clean.clone()
    raw[19, 2] = NAN                                                 # a dropped reading ...
    raw[20, 2] += 50.0                                               # ... and a spike one tick later
    s_raw = torch.cat([history, raw.t()], dim=1)
    quiet = _detector(model, s_raw, w, 5, dev, top_m=3, gaps=True)
    top = _cat(_run(quiet, raw.to(dev), 5), 2)[:, 0]
    assert not torch.isnan(top).any()
    srt = top.sort().values
    cut = int(torch.argmax(srt[1:] - srt[:-1]))
    thr = float((srt[cut] + srt[cut + 1]) / 2)                       # in the widest gap between sorted top scores
    det = _detector(model, s_raw, w, 5, dev, threshold=thr, top_m=3, gaps=True)
    got = _run(det, raw.to(dev), 5)
    al, ti = _cat(got, 4).bool(), _cat(got, 3)
    assert torch.equal(al, top > thr)
    assert bool(al[20]) and int(ti[20, 0]) == 2                      # the spike's tick is flagged, by the spiked sensor
    assert not bool(al[19])                                          # the dropped reading itself raised nothing
    # the plain detector is blind there: the NaN error sits in the means of ticks 19 .. 22
    blind = _detector(model, s_raw, w, 5, dev, threshold=thr, top_m=3)
    assert not _cat(_run(blind, raw.to(dev), 5), 4)[19:23].any()


@pytest.mark.parametrize("shape", ["n5", "n65"])
def test_detector_results_do_not_depend_on_the_push_size(shape, gpu_device):
    dev = gpu_device
    shape = DETECTORS[shape]
    n, w = shape[:2]
    m = min(3, n)
    model, s, _history, clean = _setup(shape, dev, seed=3)
    med_iqr = _table(n, dev)
    raw = _missing_pattern(clean, w, 8).to(dev)
    first = None
    for chunk in (1, 2, 3, 5, 8, 9, 37):
        det = _detector(model, s, w, chunk, dev, med_iqr=med_iqr, threshold=0.5, top_m=m, gaps=True)
        got = _run(det, raw, chunk)
        total, run = det.status_gaps()
        end = (_cat(got, 2), _cat(got, 3), _cat(got, 4), det.state, det.log_ticks, det.log_sensors, total, run)
        assert int(end[2].sum()) > 0
        if first is None:
            first = end
        for a, b in zip(end, first):
            assert torch.equal(a, b), chunk


def test_graph_replay_equals_eager_launches_with_missing_readings(gpu_device):
    dev = gpu_device
    shape = DETECTORS["n130"]
    n, w = shape[:2]
    model, s, _history, clean = _setup(shape, dev, seed=4)
    raw = _missing_pattern(clean, w, 5).to(dev)
    med_iqr = _table(n, dev)
    graphed = _detector(model, s, w, 5, dev, med_iqr=med_iqr, threshold=0.5, top_m=3, use_graph=True, gaps=True)
    eager = _detector(model, s, w, 5, dev, med_iqr=med_iqr, threshold=0.5, top_m=3, use_graph=False, gaps=True)
    a, b = _run(graphed, raw, 5), _run(eager, raw, 5)                # seven full pushes and one of two ticks
    assert graphed.graph is not None and eager.graph is None
    for pa, pb in zip(a, b):
        assert all(torch.equal(u, v) for u, v in zip(pa, pb))
    assert torch.equal(graphed.gaps, eager.gaps) and bool(graphed.gaps.any())
    assert torch.equal(graphed.log_ticks, eager.log_ticks) and torch.equal(graphed.log_sensors, eager.log_sensors)
    # one push of all 37 ticks through a detector of chunk 5 is the same eight pushes
    split = _detector(model, s, w, 5, dev, med_iqr=med_iqr, threshold=0.5, top_m=3, gaps=True)
    split.push(raw)
    assert torch.equal(split.state, eager.state) and torch.equal(split.gaps, eager.gaps)
    # one full replay of chunk = 64
    history, clean64 = _stream_of(n, w, t=128, seed=6)
    raw64 = _missing_pattern(clean64, w, 64).to(dev)
    s64 = torch.cat([history, clean64.t()], dim=1)
    g64 = _detector(model, s64, w, 64, dev, med_iqr=med_iqr, threshold=0.5, top_m=3, use_graph=True, gaps=True)
    e64 = _detector(model, s64, w, 64, dev, med_iqr=med_iqr, threshold=0.5, top_m=3, use_graph=False, gaps=True)
    a, b = _run(g64, raw64, 64), _run(e64, raw64, 64)                # the capturing push, then one replay
    for pa, pb in zip(a, b):
        assert all(torch.equal(u, v) for u, v in zip(pa, pb))
    assert g64.graph is not None and torch.equal(g64.gaps, e64.gaps)
    filled, _valid, total, run = gref.ffill_chunked(raw64.cpu().numpy(), history[:, -1].numpy(), 64)
    assert [t.tolist() for t in g64.status_gaps()] == [total.tolist(), run.tolist()]
    assert torch.equal(g64.chunk_buf.cpu(), torch.from_numpy(filled[64:]))


def test_refusals_name_history_and_series(gpu_device):
    from gdn_amd import harness
    dev = gpu_device
    shape = DETECTORS["n5"]
    n, w = shape[:2]
    model, s, _history, _clean = _setup(shape, dev)
    bad = s.clone()
    bad[2, w - 1] = NAN
    with pytest.raises(ValueError, match=r"(?s)history.*gaps"):
        _detector(model, bad, w, 4, dev, gaps=True)
    longer = torch.cat([torch.full((n, 2), NAN), s[:, :w]], dim=1)   # not finite before the last w ticks: fine
    harness.StreamDetector(model, _table(n, dev), 1.0, longer.to(dev), 4, gaps=True)
    n, w = PLANNED[:2]                                               # (the calibration's series route: its shape)
    model = _model(dev, *PLANNED)
    normal = torch.rand((n, w + 200), generator=torch.Generator().manual_seed(21))
    det = harness.StreamDetector.from_calibration(model, normal.to(dev), 16, top_m=3, gaps=True)
    assert det.with_gaps and det.valid is not None and tuple(det.gaps.shape) == (2, n)
    normal[1, 30] = NAN
    with pytest.raises(ValueError, match=r"(?s)series.*gaps"):
        harness.StreamDetector.from_calibration(model, normal.to(dev), 16, top_m=3, gaps=True)


# ------------------------------------------------------------------------------------------------ command line
def test_command_line_stream_gaps_counts_equal_a_detector_run_by_hand(gpu_device, tmp_path, capsys):
    from gdn_amd import harness, main as cli
    from test_gpu_localise import _write_cli_dataset
    data, p = load_golden("cli_msl_slice")
    batch, w, dim, stride, topk, seed, inter = (int(v) for v in data["meta_cfg"])
    data = dict(data)
    test_raw = np.array(data["test_raw"], dtype=np.float64)
    columns, sensors = [str(c) for c in data["columns_test"]], [str(f) for f in data["features"]]
    holes = [(w + 5, sensors[0]), (w + 6, sensors[0]), (w + 16, sensors[1]), (w + 40, sensors[0])]
    for row, name in holes:                                          # (test row, sensor): dropped readings of the csv
        test_raw[row, columns.index(name)] = np.nan
    data["test_raw"] = test_raw
    root = str(tmp_path / "data")
    _write_cli_dataset(data, root)
    ckpt = str(tmp_path / "ckpt.pt")
    torch.save(p, ckpt)
    argv = ["-dataset", "msl", "-data_root", root, "-device", "cuda", "-batch", str(batch), "-slide_win", str(w),
            "-dim", str(dim), "-slide_stride", str(stride), "-topk", str(topk), "-random_seed", str(seed),
            "-out_layer_inter_dim", str(inter), "-val_ratio", str(float(data["val_ratio"])), "-report", "best",
            "-load_model_path", ckpt]
    cli.main(argv + ["-stream", "16"])
    plain = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("stream:")]
    assert len(plain) == 1 and "missing" not in plain[0]             # without the flag: the line it printed before
    assert plain[0].startswith("stream: ") and " alarm ticks" in plain[0] and "ticks in pushes of 16" in plain[0]
    cli.main(argv + ["-stream", "16", "-stream_gaps"])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("stream:")]
    assert len(line) == 1

    import random
    random.seed(seed)
    torch.manual_seed(seed)
    m = cli.Main({"batch": batch, "epoch": 1, "slide_win": w, "dim": dim, "slide_stride": stride, "comment": "",
                  "seed": seed, "out_layer_num": 1, "out_layer_inter_dim": inter, "decay": 0,
                  "val_ratio": float(data["val_ratio"]), "topk": topk},
                 {"save_path": "msl", "dataset": "msl", "report": "best", "device": "cuda", "load_model_path": ckpt,
                  "data_root": root, "stream": 16, "stream_gaps": True})
    m.run()
    capsys.readouterr()
    res = m.stream_result
    n_test = m.test_series.shape[1] - w
    want_missing = int((~torch.isfinite(m.test_series[:, w:])).sum())
    assert want_missing >= len(holes)
    # by hand: calibrate on the validation block, replay the test series
    val_ticks = m.train_dataset.starts[m.val_dataloader.loader.dataset.tensors[0].to(gpu_device)]
    normal = m.train_series[:, int(val_ticks.min()) - w:int(val_ticks.max()) + 1].contiguous()
    det = harness.StreamDetector.from_calibration(m.model, normal, 16, history=m.test_series[:, :w], top_m=3, gaps=True)
    ticks = m.test_series[:, w:].t().contiguous()
    for t0 in range(0, n_test, 16):
        det.push(ticks[t0:t0 + 16])
    scored, alarms, log_ticks, _log_sensors = det.status()
    total, _run_ = det.status_gaps()
    assert (res["ticks"], res["alarms"]) == (scored, alarms) and scored == n_test
    assert res["missing"] == int(total.sum()) == want_missing
    assert res["gap_sensors"] == int((total > 0).sum()) >= 1
    np.testing.assert_array_equal(res["log_ticks"], log_ticks.cpu().numpy())
    assert f"{alarms} alarm ticks" in line[0]
    assert f"{res['missing']} missing readings held on {res['gap_sensors']} sensors" in line[0]
