"""GPU suite of the streaming detector: gdn_stream_windows / _score / _advance and harness.StreamDetector.  The stream
must equal the batch path on [history | stream]: the same windows (torch.equal with unfold), the same forward
(torch.equal with forward_into on materialised windows), the same float64 scoring (torch.equal with ONE
gdn_score_smooth_topm over the whole series; 1e-12 against tests/_stream_ref.py, the scoring suite's bar), graph
replay equal to eager launches, and state that survives pushes of every size.  T = 37 ticks everywhere."""
import functools

import numpy as np
import pytest
import torch

import _stream_ref as ref
from conftest import load_golden
from test_gpu_forward_parity import _assert_fp32_grade, random_params

pytestmark = pytest.mark.gpu

T = 37
PLANNED = (127, 15, 30, 64)


@functools.lru_cache(maxsize=None)
def _cpu_model(n, w, k, d, layers=1, inter=32):
    model = random_params(n, w, k, d, seed=n + w, out_layer_num=layers, inter=inter)
    return model, {key: v.detach().clone() for key, v in model.state_dict().items()}


def _model(dev, n, w, k, d, layers=1, inter=32):
    import copy
    return copy.deepcopy(_cpu_model(n, w, k, d, layers, inter)[0]).to(dev).eval()


def _series(n, w, seed=0):
    """S [n, w + T]: the history S[:, :w], the stream S[:, w:].t(), and every window U[t] = S[:, t : t + w]."""
    s = torch.rand((n, w + T), generator=torch.Generator().manual_seed(seed + 7 * n + w))
    return s


def _windows_of(s, w):
    return s.unfold(1, w, 1).permute(1, 0, 2).contiguous()          # [T + 1, n, w]


def _table(n, dev, seed=1):
    g = torch.Generator().manual_seed(seed + n)
    med = torch.rand((n,), generator=g, dtype=torch.float64) * 0.1
    iqr = torch.rand((n,), generator=g, dtype=torch.float64) * 0.2 + 0.05
    return torch.stack([med, iqr], dim=1).contiguous().to(dev)


def _detector(model, s, w, chunk, dev, med_iqr=None, threshold=float("inf"), **kw):
    from gdn_amd import harness
    med_iqr = _table(s.shape[0], dev) if med_iqr is None else med_iqr
    return harness.StreamDetector(model, med_iqr, threshold, s[:, :w].contiguous().to(dev), chunk, **kw)


def _run(det, stream, chunk):
    """The stream in pushes of `chunk` (the last one ragged): concatenated (pred, top_scores, top_sensors, alarm)."""
    outs = []
    for t0 in range(0, stream.shape[0], chunk):
        ts, ti, al = det.push(stream[t0:t0 + chunk])
        outs.append((det.pred[:len(al)].clone(), ts.clone(), ti.clone(), al.clone()))
    return tuple(torch.cat([o[j] for o in outs]) for j in range(4))


# ------------------------------------------------------------------------------------------------ windows
@pytest.mark.parametrize("n,w,chunk", [(5, 4, 1), (5, 4, 2), (127, 15, 5), (127, 15, 37), (130, 65, 16), (700, 15, 3)])
def test_windows_equal_unfold_after_every_push_and_hist_ends_on_the_last_w_ticks(n, w, chunk, gpu_device):
    from gdn_amd import ops
    dev = gpu_device
    s = _series(n, w)
    sd = s.to(dev)
    want = _windows_of(sd, w)
    stream = sd[:, w:].t().contiguous()
    state = ops.stream_state(sd[:, :w].contiguous(), w)
    counters, carry, hist = ops.stream_state_views(state, n, w)
    assert torch.equal(hist, sd[:, :w]) and counters.tolist() == [0, 0, 0] and not carry.any()
    m = min(3, n)
    buf = torch.zeros((chunk, n), device=dev)
    x = torch.full((chunk, n, w), -7.0, device=dev)
    pred = torch.zeros((chunk, n), device=dev)
    alarm = torch.zeros((chunk,), dtype=torch.int32, device=dev)
    sensors = torch.zeros((chunk, m), dtype=torch.int32, device=dev)
    med_iqr = _table(n, dev)
    for t0 in range(0, T, chunk):
        r = min(chunk, T - t0)
        buf[:r].copy_(stream[t0:t0 + r])
        x.fill_(-7.0)
        ops.stream_windows(state, buf, w, x, count=r)
        assert torch.equal(x[:r], want[t0:t0 + r]), t0
        assert (x[r:] == -7.0).all()                                 # rows beyond count are not written
        ops.stream_advance(state, buf, pred, med_iqr, alarm, sensors, w, m, count=r)
        assert torch.equal(hist, sd[:, t0 + r:t0 + r + w]), t0
    assert torch.equal(hist, sd[:, -w:]) and counters.tolist() == [T, 0, 0]
    # a history longer than the window: its last w columns
    assert torch.equal(ops.stream_state_views(ops.stream_state(sd, w), n, w)[2], sd[:, -w:])


# ------------------------------------------------------------------------------------------------ forward
ROUTES = {"planned": PLANNED, "large": (700, 15, 30, 64), "long_window": (130, 65, 10, 64),
          "any_width": (127, 15, 30, 48), "mlp_head": PLANNED + (2, 32)}


@pytest.mark.parametrize("route", list(ROUTES))
def test_pred_equals_forward_into_on_the_materialised_windows(route, gpu_device):
    dev = gpu_device
    shape = ROUTES[route]
    n, w = shape[:2]
    model = _model(dev, *shape)
    s = _series(n, w)
    want_x = _windows_of(s, w).to(dev)
    stream = s[:, w:].t().contiguous().to(dev)
    chunk = 8                                                        # 4 replays of one graph, then a ragged push of 5
    det = _detector(model, s, w, chunk, dev, top_m=3)
    out = torch.empty((chunk, n), device=dev)
    for t0 in range(0, T, chunk):
        r = min(chunk, T - t0)
        det.push(stream[t0:t0 + r])
        assert torch.equal(det.x[:r], want_x[t0:t0 + r])
        model.forward_into(want_x[t0:t0 + r].contiguous(), out[:r], wide=det.wide)
        assert torch.equal(det.pred[:r], out[:r]), (route, t0)
    assert det.graph is not None and det.status()[0] == T


# ------------------------------------------------------------------------------------------------ score
SCORE_MODELS = {5: (5, 4, 3, 16), 127: PLANNED, 130: (130, 15, 10, 64)}


@pytest.mark.parametrize("chunk", [1, 2, 3, 5, 8, 9, 37])
@pytest.mark.parametrize("m", [1, 3, 8])
@pytest.mark.parametrize("n", [5, 127, 130])
def test_chunked_scores_equal_one_topm_launch_over_the_whole_series(n, m, chunk, gpu_device):
    from gdn_amd import ops
    dev = gpu_device
    shape = SCORE_MODELS[n]
    w = shape[1]
    model = _model(dev, *shape)
    s = _series(n, w, seed=chunk)
    if m > n:
        with pytest.raises(ValueError, match="top_m"):
            _detector(model, s, w, chunk, dev, top_m=m)
        return
    stream = s[:, w:].t().contiguous().to(dev)
    det = _detector(model, s, w, chunk, dev, top_m=m)
    pred, ts, ti, al = _run(det, stream, chunk)
    want_s, want_i = ops.score_smooth_topm(pred, stream, det.med_iqr, m)
    assert torch.equal(ts, want_s) and torch.equal(ti, want_i)
    assert (ts[:3] == 0).all() and not al.any()
    ticks, alarms, log_ticks, log_sensors = det.status()
    assert (ticks, alarms, log_ticks.numel(), tuple(log_sensors.shape)) == (T, 0, 0, (0, m))
    # the carry the state ends on: the normalised errors of the last three ticks
    carry = ops.stream_state_views(det.state, n, w)[1]
    a = ((pred[-3:].double() - stream[-3:].double()).abs() - det.med_iqr[:, 0]) * (1.0 / (det.med_iqr[:, 1].abs() + 1e-2))
    torch.testing.assert_close(carry, a, rtol=1e-13, atol=1e-15)        # a few ulp of float64


def test_top_scores_agree_with_the_float64_helper(gpu_device):
    dev = gpu_device
    n, w = PLANNED[:2]
    model = _model(dev, *PLANNED)
    s = _series(n, w, seed=3)
    stream = s[:, w:].t().contiguous().to(dev)
    det = _detector(model, s, w, 5, dev, top_m=3)
    pred, ts, ti, _al = _run(det, stream, 5)
    delta = np.abs(pred.cpu().numpy().astype(np.float64) - stream.cpu().numpy().astype(np.float64))
    _sm, vals, idx, _flags, _state = ref.run_chunked(delta, det.med_iqr.cpu().numpy(), 5, m=3)
    got = ts.cpu().numpy()
    err = np.abs(got - vals) / np.maximum(np.abs(vals), 1e-300)
    print(f"stream top-3 T={T} N={n}: worst relative score error against float64 {err[vals != 0].max():.2e}")
    np.testing.assert_allclose(got[:, 0], vals[:, 0], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(got, vals, rtol=1e-12, atol=1e-13)


def _spiked(n, w):
    s = _series(n, w, seed=5)
    s[2, w + 20] += 50.0                                             # a spike: its tick alarms at any sane threshold
    return s


@pytest.mark.parametrize("chunk", [1, 5, 37])
def test_alarm_flags_counters_and_the_log(chunk, gpu_device):
    dev = gpu_device
    n, w = PLANNED[:2]
    model = _model(dev, *PLANNED)
    s = _spiked(n, w)
    stream = s[:, w:].t().contiguous().to(dev)
    _p, scores, _i, none = _run(_detector(model, s, w, chunk, dev), stream, chunk)
    assert not none.any()                                            # threshold inf
    top = scores[:, 0]
    thr = float(top.sort().values[T - 6])                            # the five largest scores lie above it
    det = _detector(model, s, w, chunk, dev, threshold=thr, top_m=3)
    short = _detector(model, s, w, chunk, dev, threshold=thr, top_m=3, log=2)
    mute = _detector(model, s, w, chunk, dev, threshold=thr, top_m=3, log=0)
    _p, ts, ti, al = _run(det, stream, chunk)
    assert torch.equal(ts[:, 0], top)
    want = ts[:, 0] > thr
    assert torch.equal(al.bool(), want) and bool(want[20]) and 2 < int(want.sum()) <= 5
    ticks, alarms, log_ticks, log_sensors = det.status()
    at = torch.nonzero(want).view(-1)
    assert (ticks, alarms) == (T, int(want.sum()))
    assert torch.equal(log_ticks, at) and torch.equal(log_sensors, ti[at])
    _run(short, stream, chunk)
    ticks, alarms, log_ticks, log_sensors = short.status()
    assert (ticks, alarms) == (T, int(want.sum()))                   # a full log drops entries, the count goes on
    assert torch.equal(log_ticks, at[:2]) and torch.equal(log_sensors, ti[at[:2]])
    _run(mute, stream, chunk)
    assert mute.status()[:2] == (T, int(want.sum())) and mute.status()[2].numel() == 0
    # strict comparison: a threshold equal to the largest score silences that tick
    exact = _detector(model, s, w, chunk, dev, threshold=float(top.max()))
    assert not _run(exact, stream, chunk)[3].any()


def test_a_nan_tick_does_not_alarm(gpu_device):
    dev = gpu_device
    shape = SCORE_MODELS[5]
    n, w = shape[:2]
    model = _model(dev, *shape)
    s = _series(n, w, seed=9)
    s[:, w + 10] = float("nan")
    stream = s[:, w:].t().contiguous().to(dev)
    det = _detector(model, s, w, 5, dev, threshold=-1e300, top_m=2)
    _p, ts, _ti, al = _run(det, stream, 5)
    top = ts[:, 0]
    assert torch.isnan(top[10:14]).all() and not al[10:14].any()     # the NaN error sits in four 4-tap means
    assert torch.equal(al.bool(), top > -1e300) and bool(al[:10].all())      # every other tick does alarm
    assert det.status()[1] == int(al.sum())


# ------------------------------------------------------------------------------------------------ graph against eager
def test_graph_replay_equals_eager_launches_and_a_ragged_last_push(gpu_device):
    dev = gpu_device
    n, w = PLANNED[:2]
    model = _model(dev, *PLANNED)
    s = _spiked(n, w)
    stream = s[:, w:].t().contiguous().to(dev)
    thr = 3.0
    graphed = _detector(model, s, w, 5, dev, threshold=thr, top_m=3, use_graph=True)
    eager = _detector(model, s, w, 5, dev, threshold=thr, top_m=3, use_graph=False)
    got, want = _run(graphed, stream, 5), _run(eager, stream, 5)     # seven full pushes and one of two ticks
    assert graphed.graph is not None and eager.graph is None
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert torch.equal(graphed.state, eager.state)
    assert torch.equal(graphed.log_ticks, eager.log_ticks) and torch.equal(graphed.log_sensors, eager.log_sensors)
    # one push of all 37 ticks through a detector of chunk 5 is the same eight pushes
    split = _detector(model, s, w, 5, dev, threshold=thr, top_m=3)
    ts, ti, al = split.push(stream)
    assert len(al) == 2 and torch.equal(ts, got[1][-2:]) and torch.equal(split.state, eager.state)
    # host ticks are taken too
    host = _detector(model, s, w, 5, dev, threshold=thr, top_m=3)
    host.push(stream.cpu())
    assert torch.equal(host.state, eager.state)


def test_a_parameter_change_drops_the_graph(gpu_device):
    dev = gpu_device
    n, w = PLANNED[:2]
    model = _model(dev, *PLANNED)
    s = _series(n, w, seed=11)
    stream = s[:, w:].t().contiguous().to(dev)
    det = _detector(model, s, w, 5, dev, top_m=3)
    det.push(stream[:5])
    det.push(stream[5:10])
    before = det.graph
    with torch.no_grad():
        model.out_layer.mlp[0].bias.data.add_(0.5)
        model.embedding.weight.data[3].mul_(1.5)
    model.invalidate_constants()
    fresh = _detector(model, s, w, 5, dev, top_m=3)
    fresh.state.copy_(det.state)                                     # the same point of the same stream
    for t0 in (10, 15):                                              # the re-capturing push, then a replay
        a, b = det.push(stream[t0:t0 + 5]), fresh.push(stream[t0:t0 + 5])
        assert all(torch.equal(u, v) for u, v in zip(a, b)) and torch.equal(det.pred, fresh.pred)
        assert torch.equal(det.state, fresh.state)
    assert det.graph is not before
    out = torch.empty((5, n), device=dev)
    model.forward_into(det.x, out, wide=det.wide)
    assert torch.equal(det.pred, out)


# ------------------------------------------------------------------------------------------------ calibration, localisation
def test_from_calibration_takes_the_evaluators_table_and_its_maximum(gpu_device):
    from gdn_amd import harness, ops
    dev = gpu_device
    n, w = PLANNED[:2]
    model = _model(dev, *PLANNED)
    normal = torch.rand((n, w + 200), generator=torch.Generator().manual_seed(21)).to(dev)
    det = harness.StreamDetector.from_calibration(model, normal, 16, top_m=3)
    ev = harness.SeriesEvaluator(model, None, normal[:, w:].t().contiguous(), batch=8192, use_graph=False, series=normal)
    anomaly = ev.step()
    assert torch.equal(det.med_iqr, ev.med_iqr) and det.med_iqr.data_ptr() != ev.med_iqr.data_ptr()
    assert float(det.threshold) == float(anomaly.max())
    assert torch.equal(ops.stream_state_views(det.state, n, w)[2], normal[:, -w:])
    # the stream that follows the calibration period continues its series: with the evaluator's own table the
    # detector on [normal[:, -w:] | more] reproduces an evaluator step over that series with the table frozen
    more = torch.rand((T, n), generator=torch.Generator().manual_seed(22)).to(dev)
    pred, ts, ti, al = _run(det, more, 16)
    want_s, want_i = ops.score_smooth_topm(pred, more, ev.med_iqr, 3)
    assert torch.equal(ts, want_s) and torch.equal(ti, want_i) and torch.equal(al.bool(), want_s[:, 0] > det.threshold)
    whole = torch.cat([normal[:, -w:], more.t()], dim=1).contiguous()
    assert torch.equal(det.x[:5], _windows_of(whole, w)[32:37])     # the last push: ticks 32 .. 36
    other = harness.StreamDetector.from_calibration(model, normal, 16, history=normal[:, :w + 3])
    assert torch.equal(ops.stream_state_views(other.state, n, w)[2], normal[:, 3:w + 3])


def test_localise_equals_attention_at_on_the_same_windows_and_sensors(gpu_device):
    dev = gpu_device
    n, w = PLANNED[:2]
    model = _model(dev, *PLANNED)
    s = _spiked(n, w)
    stream = s[:, w:].t().contiguous().to(dev)
    det = _detector(model, s, w, 8, dev, threshold=3.0, top_m=3)
    det.push(stream[:16])
    ts, ti, al = det.push(stream[16:24])                             # ticks 16 .. 23: the spike is at 20
    rows = torch.nonzero(al).view(-1)
    assert rows.numel() > 0 and 4 in rows.tolist()
    loc = det.localise()
    sensors = ti[rows].long()
    at = rows.view(-1, 1).expand(-1, 3)
    want = model.attention_at(det.x, at.reshape(-1), sensors.reshape(-1))
    assert torch.equal(loc.attention, want.reshape(rows.numel(), 3, -1))
    assert torch.equal(loc.ticks, rows + 16) and torch.equal(loc.sensors, sensors) and torch.equal(loc.scores, ts[rows])
    assert torch.equal(loc.neighbours, model.attention_neighbours()[sensors])
    assert torch.equal(loc.predicted, det.pred[at, sensors]) and torch.equal(loc.observed, stream[16:24][at, sensors])
    assert int(loc.sensors[rows.tolist().index(4), 0]) == 2          # the spiked sensor leads its tick
    one = det.localise(rows=[4])
    assert torch.equal(one.attention, loc.attention[rows.tolist().index(4)][None])
    with pytest.raises(ValueError):
        det.localise(rows=[8])


# ------------------------------------------------------------------------------------------------ guarded push
def test_a_tick_beyond_the_operand_range_is_recomputed_on_the_device(gpu_device):
    """operand_range == "auto" on the planned route: the push is the guarded launch.  One tick of the stream in raw
    units (x 1e5, beyond the 65504 of the 16-bit operands) must leave predictions as good as the fp32 kernels': the bar
    of test_raw_unit_inputs_equal_the_float64_oracle_without_any_switch (_assert_fp32_grade), for the detector's pred
    and for forward_into(x, wide=True) on the same windows alike."""
    dev = gpu_device
    n, w, k, d = PLANNED
    model = _model(dev, *PLANNED)
    p = _cpu_model(*PLANNED)[1]
    assert model.operand_range == "auto"
    s = _series(n, w, seed=13)
    s[:, w + 9] *= 1.0e5
    stream = s[:, w:].t().contiguous().to(dev)
    windows = _windows_of(s, w)
    det = _detector(model, s, w, 8, dev)
    assert det.wide is False and det._guarded()
    graph = None
    for t0 in (0, 8, 16):                   # in range (the capture), six of eight windows out of range (a replay), all
        det.push(stream[t0:t0 + 8])
        graph = model.learned_graph.cpu()
        x = windows[t0:t0 + 8].contiguous()
        assert torch.equal(det.x, x.to(dev))
        _assert_fp32_grade(det.pred, p, x, k, graph, what=f"stream push at {t0}")
        wide = model.forward_into(x.to(dev), torch.empty((8, n), device=dev), wide=True)
        _assert_fp32_grade(wide, p, x, k, graph, what=f"wide forward at {t0}")
    assert float(windows[8:16].abs().max()) > 65504.0 and float(windows[:8].abs().max()) < 1.0
    guards = list(model._constants().guards.values())
    assert guards and all(g.tolist() == [0, 0] for g in guards)      # whatever was raised has been consumed


# ------------------------------------------------------------------------------------------------ command line
def test_command_line_stream_counts_equal_a_detector_run_by_hand(gpu_device, tmp_path, capsys):
    from gdn_amd import harness, main as cli
    from test_gpu_localise import _write_cli_dataset
    import random
    data, p = load_golden("cli_msl_slice")
    batch, w, dim, stride, topk, seed, inter = (int(v) for v in data["meta_cfg"])
    root = str(tmp_path / "data")
    _write_cli_dataset(data, root)
    ckpt = str(tmp_path / "ckpt.pt")
    torch.save(p, ckpt)
    argv = ["-dataset", "msl", "-data_root", root, "-device", "cuda", "-batch", str(batch), "-slide_win", str(w),
            "-dim", str(dim), "-slide_stride", str(stride), "-topk", str(topk), "-random_seed", str(seed),
            "-out_layer_inter_dim", str(inter), "-val_ratio", str(float(data["val_ratio"])), "-report", "best",
            "-load_model_path", ckpt]
    info_plain = cli.main(argv)
    printed_plain = capsys.readouterr().out
    assert "stream:" not in printed_plain
    info = cli.main(argv + ["-stream", "16"])
    printed = capsys.readouterr().out
    report = lambda text: [ln for ln in text.splitlines() if ln.startswith(("F1 score:", "precision:", "recall:"))]
    assert report(printed) == report(printed_plain) and tuple(info) == tuple(info_plain)
    line = [ln for ln in printed.splitlines() if ln.startswith("stream:")]
    assert len(line) == 1

    def drive(stream):
        random.seed(seed)
        torch.manual_seed(seed)
        m = cli.Main({"batch": batch, "epoch": 1, "slide_win": w, "dim": dim, "slide_stride": stride, "comment": "",
                      "seed": seed, "out_layer_num": 1, "out_layer_inter_dim": inter, "decay": 0,
                      "val_ratio": float(data["val_ratio"]), "topk": topk},
                     {"save_path": "msl", "dataset": "msl", "report": "best", "device": "cuda", "load_model_path": ckpt,
                      "data_root": root, "stream": stream})
        m.run()
        return m
    m = drive(16)
    res = m.stream_result
    n_test = m.test_series.shape[1] - w
    assert res["chunk"] == 16 and res["ticks"] == n_test
    assert f"{res['alarms']} alarm ticks" in line[0] and f"{n_test} ticks in pushes of 16" in line[0]
    # by hand: calibrate on the validation block, replay the test series
    val_ticks = m.train_dataset.starts[m.val_dataloader.loader.dataset.tensors[0].to(gpu_device)]
    normal = m.train_series[:, int(val_ticks.min()) - w:int(val_ticks.max()) + 1].contiguous()
    det = harness.StreamDetector.from_calibration(m.model, normal, 16, history=m.test_series[:, :w], top_m=3)
    ticks = m.test_series[:, w:].t().contiguous()
    flags = torch.cat([det.push(ticks[t0:t0 + 16])[2].clone() for t0 in range(0, n_test, 16)])
    scored, alarms, log_ticks, log_sensors = det.status()
    assert (scored, alarms) == (res["ticks"], res["alarms"]) and alarms == int(flags.sum())
    assert res["threshold"] == float(det.threshold)
    np.testing.assert_array_equal(res["log_ticks"], log_ticks.cpu().numpy())
    np.testing.assert_array_equal(res["log_sensors"], log_sensors.cpu().numpy())
    np.testing.assert_array_equal(res["log_ticks"], torch.nonzero(flags).view(-1).cpu().numpy()[:4096])
