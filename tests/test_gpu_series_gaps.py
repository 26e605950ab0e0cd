"""GPU suite of the resident series with missing readings: gdn_series_fill, gdn_score_keys_keep, the
`_gaps` smooth launches, harness.SeriesEvaluator(gaps=True) and StreamDetector.from_calibration(calib_gaps=True)
against tests/_series_gaps_ref.py.  The fill is exact (torch.equal), a finite series gives the bits of gaps=False, a
series with missing readings gives the predictions of a gaps=False evaluator on the filled series and the table of
gdn_score_quantiles on the complete rows, the scores meet the float64 bar of tests/test_gpu_stream_gaps.py (rtol 1e-12,
atol 1e-13), and a gaps=True detector pushed the raw ticks writes the evaluator's results bit for bit."""
import numpy as np
import pytest
import torch

import _series_gaps_ref as sref
from conftest import load_golden
from test_gpu_stream import _model
from test_gpu_stream_gaps import ATOL, RTOL, _assert_scores

pytestmark = pytest.mark.gpu

NAN = float("nan")
SHAPES = {"n5": (5, 3, 3, 16), "n65": (65, 3, 10, 64), "n130": (130, 15, 10, 64), "planned": (20, 5, 4, 64),
          "staged": (20, 5, 4, 24)}
LENGTH_OF = {"b": 37, "c": 64, "d": 300, "e": 65, "f": 129}          # one scored length per pattern: every length once
MIN_KEPT = sref.MIN_KEPT


def _bits(x):
    return x.contiguous().view(torch.int32)


def _raw(shape, pattern, t, dev, seed=0):
    n, w = shape[:2]
    raw = sref.with_pattern(sref.clean_series(n, w, t, seed), w, pattern)
    return raw, torch.from_numpy(raw).to(dev)


def _evaluator(model, raw_d, **kw):
    from gdn_amd import harness
    kw.setdefault("use_graph", False)
    return harness.SeriesEvaluator(model, None, None, 64, series=raw_d, gaps=True, min_kept=MIN_KEPT, **kw)


def _plain(model, series_d, w, **kw):
    """A gaps=False evaluator on a finite series; on its windows where the model has no series kernel (d = 16)."""
    from gdn_amd import harness
    kw.setdefault("use_graph", False)
    y = series_d[:, w:].t().contiguous()
    if model.embedding.weight.shape[1] >= 24:
        return harness.SeriesEvaluator(model, None, y, 64, series=series_d, **kw)
    return harness.SeriesEvaluator(model, series_d.unfold(1, w, 1).permute(1, 0, 2).contiguous()[:-1], y, 64, **kw)


# ------------------------------------------------------------------------------------------------ 1. the fill
def _assert_fill(raw, w, dev, what):
    from gdn_amd import ops
    raw_d = torch.from_numpy(raw).to(dev)
    before = _bits(raw_d).clone()
    filled, gt, valid, keep, counters = ops.series_fill(raw_d, w)
    want = sref.fill(raw, w)
    assert torch.equal(filled.cpu(), torch.from_numpy(want[0])), what
    assert torch.equal(gt.cpu(), torch.from_numpy(want[1])), what
    assert torch.equal(valid.cpu(), torch.from_numpy(want[2].astype(np.uint8))), what
    assert torch.equal(keep.cpu(), torch.from_numpy(want[3].astype(np.uint8))), what
    assert counters.dtype == torch.int64 and counters.cpu().tolist() == [want[4].tolist(), want[5].tolist()], what
    assert torch.equal(_bits(raw_d), before), what                   # raw is untouched, NaN payloads included
    assert torch.isfinite(filled).all()


@pytest.mark.parametrize("n,w", [(5, 3), (65, 3), (130, 15), (20, 5)])
def test_fill_equals_the_ref_on_every_pattern_and_length(n, w, gpu_device):
    for t in sref.LENGTHS:
        for pattern in sref.PATTERNS:
            if pattern == "d" and t < 300:
                continue
            raw = sref.with_pattern(sref.clean_series(n, w, t), w, pattern)
            _assert_fill(raw, w, gpu_device, (n, w, t, pattern))


def test_fill_looks_back_over_more_than_sixty_four_blocks_and_takes_one_sensor(gpu_device):
    n, w, t = 3, 3, 9000
    raw = sref.clean_series(n, w, t)
    raw[1, w + 100:w + 5100] = NAN                                   # 5000 ticks: 78 blocks without a real reading
    raw[2, t - 500:] = np.inf                                        # a trailing run of 503 ticks
    _assert_fill(raw, w, gpu_device, "long runs")
    one = sref.with_pattern(sref.clean_series(1, 2, 70), 2, "c")
    _assert_fill(one, 2, gpu_device, "n = 1")


def test_refusals_are_raised_before_any_forward(gpu_device):
    from gdn_amd import harness
    dev = gpu_device
    shape = SHAPES["n5"]
    n, w = shape[:2]
    model = _model(dev, *shape)

    def no_forward(*_a, **_k):
        raise AssertionError("a forward was launched")
    model.forward_series = model.forward_into = no_forward
    raw, raw_d = _raw(shape, "c", 64, dev)
    bad = raw_d.clone()
    bad[2, w - 1] = NAN
    with pytest.raises(ValueError, match=r"(?s)series.*gaps"):
        _evaluator(model, bad)
    sparse = raw_d.clone()
    sparse[0, w + 5:] = NAN                                          # five complete ticks are left
    with pytest.raises(ValueError, match=r"(?s)min_kept = 8.*kept = 5"):
        _evaluator(model, sparse)
    del model.forward_series, model.forward_into                     # an accepted series: the evaluator is built
    ev = harness.SeriesEvaluator(model, None, None, 64, series=sparse, gaps=True, min_kept=5, use_graph=False)
    assert ev.kept == 5
    model.forward_series = model.forward_into = no_forward
    gt = raw_d[:, w:].t().contiguous()
    with pytest.raises(ValueError, match="y_all"):
        harness.SeriesEvaluator(model, None, gt, 64, series=raw_d, gaps=True)
    windows = raw_d.unfold(1, w, 1).permute(1, 0, 2).contiguous()[:-1]
    with pytest.raises(ValueError, match="window tensor"):
        harness.SeriesEvaluator(model, windows, None, 64, gaps=True)
    with pytest.raises(ValueError, match="bf16"):
        harness.SeriesEvaluator(model, None, None, 64, series=raw_d.bfloat16(), gaps=True)
    with pytest.raises(ValueError, match=r"(?s)calib_gaps.*gaps=True"):
        harness.StreamDetector.from_calibration(model, raw_d, 16, calib_gaps=True)
    with pytest.raises(ValueError, match=r"(?s)series.*gaps"):       # the old refusal, without calib_gaps
        harness.StreamDetector.from_calibration(model, raw_d, 16, gaps=True)
    with pytest.raises(ValueError, match=r"(?s)min_kept.*kept"):
        harness.StreamDetector.from_calibration(model, sparse, 16, gaps=True, calib_gaps=True, min_kept=MIN_KEPT)
    with pytest.raises(ValueError, match="gaps=False"):
        _plain(_model(dev, *shape), torch.from_numpy(sref.clean_series(n, w, 37)).to(dev), w).status_gaps()


# ------------------------------------------------------------------------------------------------ 2. no gap
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("shape", ["planned", "staged", "n130"])
def test_on_a_finite_series_gaps_writes_the_bits_of_a_plain_evaluator(shape, use_graph, gpu_device):
    dev = gpu_device
    shape = SHAPES[shape]
    w = shape[1]
    model = _model(dev, *shape)
    _raw_np, raw_d = _raw(shape, "a", 129, dev)
    for kw in (dict(top_m=0), dict(top_m=3), dict(want_scores=True)):
        a = _plain(model, raw_d, w, use_graph=use_graph, **kw)
        b = _evaluator(model, raw_d, use_graph=use_graph, **kw)
        for _ in range(2):                                           # captured: the capture's replay, then one more
            a.step()
            b.step()
        assert (b.graph is not None) == use_graph
        assert b.kept == b.t == 129 and bool(b.valid.all()) and bool(b.keep.all())
        assert torch.equal(b.series, raw_d) and torch.equal(b.y, a.y)
        for name in ("pred", "med_iqr", "anomaly", "scores", "top_scores", "top_sensors"):
            x, y = getattr(a, name), getattr(b, name)
            assert (x is None) == (y is None), name
            if x is not None:
                assert torch.equal(x, y), (name, kw)
        total, run = b.status_gaps()
        assert not total.any() and not run.any()


# ------------------------------------------------------------------------------------------------ 3. with gaps
@pytest.mark.parametrize("pattern", list(LENGTH_OF))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_with_gaps_pred_table_scores_and_counters(shape, pattern, gpu_device):
    from gdn_amd import harness, ops
    dev = gpu_device
    shape = SHAPES[shape]
    n, w = shape[:2]
    t, m = LENGTH_OF[pattern], min(3, n)
    model = _model(dev, *shape)
    raw, raw_d = _raw(shape, pattern, t, dev)
    filled, gt, valid, keep, total, run = sref.fill(raw, w)
    ev = _evaluator(model, raw_d, top_m=m)
    anomaly = ev.step()
    assert torch.equal(ev.series.cpu(), torch.from_numpy(filled)) and torch.equal(_bits(ev.raw_series), _bits(raw_d))
    assert torch.equal(ev.y.cpu(), torch.from_numpy(gt)) and ev.kept == int(keep.sum())
    assert torch.equal(ev.valid.cpu(), torch.from_numpy(valid.astype(np.uint8)))
    assert torch.equal(ev.keep.cpu(), torch.from_numpy(keep.astype(np.uint8)))
    assert [c.tolist() for c in ev.status_gaps()] == [total.tolist(), run.tolist()]
    plain = _plain(model, torch.from_numpy(filled).to(dev), w)
    plain.step()
    assert torch.equal(ev.pred, plain.pred)
    rows = torch.from_numpy(np.nonzero(keep)[0]).to(dev)
    assert torch.equal(ev.med_iqr, ops.score_quantiles(ev.pred[rows].contiguous(), ev.y[rows].contiguous()))
    pred = ev.pred.cpu().numpy()
    np.testing.assert_allclose(ev.med_iqr.cpu().numpy(), sref.table(pred, gt, keep), rtol=RTOL, atol=ATOL)
    sm, vals, idx = sref.scores(pred, gt, valid, ev.med_iqr.cpu().numpy(), m)
    _assert_scores(ev.top_scores, ev.top_sensors, vals, idx, (shape, pattern))
    assert torch.equal(anomaly, ev.top_scores[:, 0]) and not torch.isnan(anomaly).any()
    full = _evaluator(model, raw_d, want_scores=True)
    assert torch.equal(full.step(), anomaly) and torch.equal(full.med_iqr, ev.med_iqr)
    got = full.scores.cpu().numpy()
    print(f"{shape} {pattern}: worst absolute score error against float64 {np.abs(got - sm).max():.2e}")
    np.testing.assert_allclose(got, sm, rtol=RTOL, atol=ATOL)
    gone = ~(valid[3:] | valid[2:-1] | valid[1:-2] | valid[:-3])     # all four taps missing: exactly 0.0
    assert (got.T[3:][gone] == 0.0).all() and (got[:, :3] == 0.0).all()
    # localise reads the filled series: the observed value of a missing reading is the held one
    loc = harness.localise(ev, [0, t - 1])
    assert torch.equal(loc.observed, ev.y[loc.ticks.view(-1, 1), loc.sensors]) and torch.isfinite(loc.observed).all()
    assert torch.isfinite(loc.attention).all()


# ------------------------------------------------------------------------------------------------ 4. the stream
@pytest.mark.parametrize("chunk", [5, 37])
@pytest.mark.parametrize("pattern", ["b", "c", "e", "f"])
@pytest.mark.parametrize("shape", ["n5", "n130"])
def test_a_gaps_detector_pushed_the_raw_ticks_writes_the_evaluators_bits(shape, pattern, chunk, gpu_device):
    from gdn_amd import harness
    dev = gpu_device
    shape = SHAPES[shape]
    n, w = shape[:2]
    t, m = LENGTH_OF[pattern], min(3, n)
    model = _model(dev, *shape)
    _raw_np, raw_d = _raw(shape, pattern, t, dev)
    ev = _evaluator(model, raw_d, top_m=m)
    ev.step()
    det = harness.StreamDetector(model, ev.med_iqr, float("inf"), raw_d[:, :w].contiguous(), chunk, gaps=True, top_m=m)
    stream = raw_d[:, w:].t().contiguous()
    outs = []
    for t0 in range(0, t, chunk):
        ts, ti, _al = det.push(stream[t0:t0 + chunk])
        r = ts.shape[0]
        outs.append((det.pred[:r].clone(), ts.clone(), ti.clone(), det.valid[:r].clone()))
    pred, ts, ti, valid = (torch.cat([o[j] for o in outs]) for j in range(4))
    assert torch.equal(pred, ev.pred) and torch.equal(valid, ev.valid)
    assert torch.equal(ts, ev.top_scores) and torch.equal(ti, ev.top_sensors)
    assert all(torch.equal(a, b) for a, b in zip(det.status_gaps(), ev.status_gaps()))
    assert int(ev.status_gaps()[0].sum()) > 0


# ------------------------------------------------------------------------------------------------ 5. the select route
def test_the_one_workgroup_select_takes_the_filler_of_incomplete_ticks(gpu_device):
    from gdn_amd import ops
    dev = gpu_device
    shape = SHAPES["n5"]
    n, w = shape[:2]
    t = 4100
    raw = sref.bursts(sref.clean_series(n, w, t), w)
    _f, _gt, _valid, keep, _total, _run = sref.fill(raw, w)
    assert 0.6 * t < keep.sum() < 0.8 * t
    ev = _evaluator(_model(dev, *shape), torch.from_numpy(raw).to(dev))
    anomaly = ev.step()
    assert ev.kept == int(keep.sum()) and not torch.isnan(anomaly).any()
    rows = torch.from_numpy(np.nonzero(keep)[0]).to(dev)
    assert torch.equal(ev.med_iqr, ops.score_quantiles(ev.pred[rows].contiguous(), ev.y[rows].contiguous()))
    keys = ops.score_keys(ev.pred, ev.y, t, keep=ev.keep)
    _table, path = ops.score_select_paths(keys, 1, n, t, ev.kept)
    assert torch.equal(_table, ev.med_iqr) and set(path.tolist()) <= {0, 1}      # (the one-workgroup route reports 0 / 1)
    assert bool((keys[:, torch.from_numpy(~keep).to(dev)].view(torch.int64) == -1).all())


# ------------------------------------------------------------------------------------------------ 6. from_calibration
def test_from_calibration_with_gaps_in_the_period(gpu_device):
    from gdn_amd import harness, ops
    dev = gpu_device
    shape = SHAPES["planned"]
    n, w = shape[:2]
    t, R = 300, 512
    model = _model(dev, *shape)
    raw = sref.bursts(sref.clean_series(n, w, t, seed=3), w, every=9, length=2, seed=3)
    raw[4, -2:] = NAN                                                # the period ends inside a run
    raw_d = torch.from_numpy(raw).to(dev)
    ev = _evaluator(model, raw_d, top_m=3)
    anomaly = ev.step()
    det = harness.StreamDetector.from_calibration(model, raw_d, 16, top_m=3, gaps=True, calib_gaps=True,
                                                  min_kept=MIN_KEPT, recal=R, recal_min=MIN_KEPT)
    assert torch.equal(det.med_iqr, ev.med_iqr) and torch.equal(det.threshold, anomaly.max().reshape(1))
    hist = ops.stream_state_views(det.state, n, w)[2]
    assert torch.equal(hist, ev.series[:, -w:]) and torch.isfinite(hist).all()
    assert det.calib_kept == ev.kept and 0 < ev.kept < t
    assert not det.gaps.any()                                        # the stream's own counters start at zero
    # the ring: the period's t ticks in the last t slots, with their own keep flags; the filler where one is 0
    assert torch.equal(det.ring_keep[R - t:], ev.keep) and not det.ring_keep[:R - t].any()
    want = ops.score_keys(ev.pred, ev.y, t, keep=ev.keep)
    assert torch.equal(_bits(det.ring_keys[:, R - t:]), _bits(want))
    dropped = det.ring_keys[:, R - t:][:, ev.keep == 0].view(torch.int64)
    assert dropped.numel() > 0 and bool((dropped == -1).all())
    assert bool((det.ring_keys[:, :R - t].view(torch.int64) == -1).all())
    before = det.med_iqr.clone()
    assert det.recalibrate() == ev.kept and torch.equal(det.med_iqr, before)      # the table, bit for bit
    # a ring shorter than the period: its last R ticks
    short = harness.StreamDetector.from_calibration(model, raw_d, 16, top_m=3, gaps=True, calib_gaps=True,
                                                    min_kept=MIN_KEPT, recal=64, recal_min=MIN_KEPT)
    assert torch.equal(short.ring_keep, ev.keep[-64:]) and torch.equal(_bits(short.ring_keys), _bits(want[:, -64:]))
    with pytest.raises(ValueError, match=r"(?s)series.*gaps"):       # the old refusal stays without calib_gaps
        harness.StreamDetector.from_calibration(model, raw_d, 16, top_m=3, gaps=True)
    # a finite period: calib_gaps changes nothing
    clean = torch.from_numpy(sref.clean_series(n, w, t, seed=3)).to(dev)
    a = harness.StreamDetector.from_calibration(model, clean, 16, top_m=3, gaps=True, recal=R)
    b = harness.StreamDetector.from_calibration(model, clean, 16, top_m=3, gaps=True, calib_gaps=True, recal=R)
    assert torch.equal(a.med_iqr, b.med_iqr) and torch.equal(a.threshold, b.threshold)
    assert torch.equal(a.state, b.state) and torch.equal(a.ring_keep, b.ring_keep)
    assert torch.equal(_bits(a.ring_keys), _bits(b.ring_keys)) and a.calib_kept is None and b.calib_kept == t


# ------------------------------------------------------------------------------------------------ 7. capture, command line
@pytest.mark.parametrize("kw", [dict(top_m=3), dict(want_scores=True)], ids=["top3", "scores"])
def test_a_captured_step_replayed_twice_equals_the_eager_launches(kw, gpu_device):
    dev = gpu_device
    shape = SHAPES["n130"]
    model = _model(dev, *shape)
    _raw_np, raw_d = _raw(shape, "f", 129, dev)
    eager = _evaluator(model, raw_d, **kw)
    eager.step()
    graphed = _evaluator(model, raw_d, use_graph=True, **kw)
    for _ in range(3):                                               # the capture's replay and two more
        graphed.step()
        assert graphed.graph is not None and eager.graph is None
        for name in ("pred", "med_iqr", "anomaly", "scores", "top_scores", "top_sensors"):
            x, y = getattr(eager, name), getattr(graphed, name)
            if x is not None:
                assert torch.equal(x, y), name
        graphed.pred.fill_(NAN)                                      # the next replay rewrites everything
        graphed.med_iqr.zero_()


def test_command_line_stream_calib_gaps_equals_a_detector_run_by_hand(gpu_device, tmp_path, capsys):
    import random

    from gdn_amd import harness, main as cli
    from test_gpu_localise import _write_cli_dataset
    data, p = load_golden("cli_msl_slice")
    batch, w, dim, stride, topk, seed, inter = (int(v) for v in data["meta_cfg"])
    data = dict(data)
    columns, sensors = [str(c) for c in data["columns_train"]], [str(f) for f in data["features"]]
    train_raw = np.array(data["train_raw"], dtype=np.float64)
    # the validation block of this seed (main.py's draw): windows val_start .. of range(w, T, stride)
    windows = len(range(w, train_raw.shape[0], stride))
    val_len = int(windows * float(data["val_ratio"]))
    random.seed(seed)
    lo = w + random.randrange(int(windows * (1 - float(data["val_ratio"])))) * stride
    holes = [(lo + 3, sensors[0]), (lo + 4, sensors[0]), (lo + 20, sensors[1]), (lo + 40, sensors[0])]
    for row, name in holes:                                          # (train row, sensor): dropped readings of the csv
        train_raw[row, columns.index(name)] = np.nan
    data["train_raw"] = train_raw
    root = str(tmp_path / "data")
    _write_cli_dataset(data, root)
    ckpt = str(tmp_path / "ckpt.pt")
    torch.save(p, ckpt)
    argv = ["-dataset", "msl", "-data_root", root, "-device", "cuda", "-batch", str(batch), "-slide_win", str(w),
            "-dim", str(dim), "-slide_stride", str(stride), "-topk", str(topk), "-random_seed", str(seed),
            "-out_layer_inter_dim", str(inter), "-val_ratio", str(float(data["val_ratio"])), "-report", "best",
            "-load_model_path", ckpt]
    cli.main(argv + ["-stream", "16", "-stream_gaps", "-stream_calib_gaps"])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("stream:")]
    assert len(line) == 1
    with pytest.raises(ValueError, match=r"(?s)series.*gaps"):       # without the flag: the refusal it always gave
        cli.main(argv + ["-stream", "16", "-stream_gaps"])
    capsys.readouterr()

    random.seed(seed)
    torch.manual_seed(seed)
    m = cli.Main({"batch": batch, "epoch": 1, "slide_win": w, "dim": dim, "slide_stride": stride, "comment": "",
                  "seed": seed, "out_layer_num": 1, "out_layer_inter_dim": inter, "decay": 0,
                  "val_ratio": float(data["val_ratio"]), "topk": topk},
                 {"save_path": "msl", "dataset": "msl", "report": "best", "device": "cuda", "load_model_path": ckpt,
                  "data_root": root, "stream": 16, "stream_gaps": True, "stream_calib_gaps": True})
    m.run()
    capsys.readouterr()
    res = m.stream_result
    # by hand: calibrate on the validation block with its holes, replay the test series
    val_ticks = m.train_dataset.starts[m.val_dataloader.loader.dataset.tensors[0].to(gpu_device)]
    assert int(val_ticks.min()) == lo and len(val_ticks) == val_len
    normal = m.train_series[:, lo - w:int(val_ticks.max()) + 1].contiguous()
    assert int((~torch.isfinite(normal)).sum()) == len(holes)
    det = harness.StreamDetector.from_calibration(m.model, normal, 16, history=m.test_series[:, :w], top_m=3, gaps=True,
                                                  calib_gaps=True)
    ticks = m.test_series[:, w:].t().contiguous()
    for t0 in range(0, ticks.shape[0], 16):
        det.push(ticks[t0:t0 + 16])
    scored, alarms, log_ticks, _log_sensors = det.status()
    assert (res["ticks"], res["alarms"]) == (scored, alarms) and scored == ticks.shape[0]
    assert res["calib_kept"] == det.calib_kept == val_len - len(holes)           # four ticks lost a reading
    assert res["threshold"] == float(det.threshold.item()) and np.isfinite(res["threshold"])
    np.testing.assert_array_equal(res["log_ticks"], log_ticks.cpu().numpy())
    assert f"{alarms} alarm ticks" in line[0]
    assert f"calibrated on {res['calib_kept']} complete validation ticks" in line[0]
