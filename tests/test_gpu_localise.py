"""GPU suite of anomaly localisation: gdn_score_smooth_topm (which sensors deviate), gdn_attention_mean /
gdn_attention_at (which neighbours they were reading, from raw data), SeriesEvaluator(top_m=...), harness.localise
and the command line's -localise.  The yardstick is the float64 helper of tests/_localise_ref.py, pinned to the
oracle by tests/test_cpu_localise.py.  Bars: scores 1e-12 relative (the scoring suite's), attention 2e-6 absolute +
1e-5 relative (the project's bar for alpha against the float64 oracle)."""
import os

import numpy as np
import pytest
import torch

import _localise_ref as ref
from conftest import SCORE_CASES, load_golden

pytestmark = pytest.mark.gpu

ATT_ATOL, ATT_RTOL = 2e-6, 1e-5


# ------------------------------------------------------------------------------------------------ top m
def _check_topm(pred, gt, m, dev, scores=None):
    from gdn_amd import ops
    pred_d, gt_d = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    med_iqr = ops.score_quantiles(pred_d, gt_d)
    ts, ti = ops.score_smooth_topm(pred_d, gt_d, med_iqr, m)
    table, anomaly = ops.score_smooth_max(pred_d, gt_d, med_iqr, want_scores=True)
    torch.cuda.synchronize()
    assert ts.shape == (pred.shape[0], m) and ts.dtype == torch.float64 and ti.dtype == torch.int32
    got_v, got_i = ts.cpu().numpy(), ti.cpu().numpy().astype(np.int64)
    want = ref.scores_f64(pred, gt) if scores is None else scores
    want_v, want_i = ref.topm(want, m)
    err = np.abs(got_v - want_v) / np.maximum(np.abs(want_v), 1e-300)
    lo, hi = got_v[:, 1:], got_v[:, :-1]
    close = (lo != hi) & (np.abs(hi - lo) <= ref.TIE_REL * np.maximum(np.abs(hi), np.abs(lo)))
    skip = ref.skippable_ticks(want, m) | close.any(axis=1)
    skip[:3] = False
    print(f"top-{m} T={pred.shape[0]} N={pred.shape[1]}: worst relative score error {err[want_v != 0].max():.2e}, "
          f"ticks skipped {int(skip.sum())} ({ref.skipped_share(skip):.4%})")
    np.testing.assert_allclose(got_v, want_v, rtol=1e-12, atol=1e-13)
    assert ref.skipped_share(skip) <= ref.SKIP_CAP
    np.testing.assert_array_equal(got_i[~skip], want_i[~skip])
    np.testing.assert_array_equal(got_i[:3], np.tile(np.arange(m), (3, 1)))
    assert (got_v[:3] == 0).all()
    # the same bits as gdn_score_smooth_max: column 0 is its anomaly, and the whole answer is the top m of its table
    assert torch.equal(ts[:, 0], anomaly)
    bit_v, bit_i = ref.topm(table.cpu().numpy(), m)
    np.testing.assert_array_equal(got_v, bit_v)
    np.testing.assert_array_equal(got_i, bit_i)
    return got_v, got_i


@pytest.mark.parametrize("m", [1, 3, 8])
@pytest.mark.parametrize("case", SCORE_CASES)
def test_topm_on_the_score_fixtures(case, m, gpu_device):
    from gdn_amd import _lib, ops
    data, _ = load_golden(case)
    if m > data["pred"].shape[1]:          # fewer sensors than m: refused before any launch
        pred, gt = (torch.from_numpy(data[key]).to(gpu_device) for key in ("pred", "gt"))
        with pytest.raises(_lib.GdnHipError, match="GDN_ERR_UNSUPPORTED"):
            ops.score_smooth_topm(pred, gt, ops.score_quantiles(pred, gt), m)
        return
    _check_topm(data["pred"], data["gt"], m, gpu_device, scores=data["scores"])


@pytest.mark.parametrize("m", [1, 3, 8])
@pytest.mark.parametrize("t,n", [(32768, 127), (1000, 27), (2048, 4096)])
def test_topm_on_seeded_data(t, n, m, gpu_device):
    pred, gt = ref.seeded_scores(t, n, seed=t + n)
    _check_topm(pred, gt, m, gpu_device)


def test_topm_exact_ties_resolve_to_the_lower_sensor(gpu_device):
    """The fixture's exact ties between sensors are its first three ticks (every score 0; its other ties are between
    ticks): wherever two reported scores are equal, the lower sensor comes first."""
    data, _ = load_golden("perf_T777_N5_ties")
    got_v, got_i = _check_topm(data["pred"], data["gt"], 3, gpu_device, scores=data["scores"])
    tie = got_v[:, :-1] == got_v[:, 1:]
    assert tie.any(), "the fixture holds exact ties among the reported scores"
    assert (np.diff(got_i, axis=1)[tie] > 0).all()


@pytest.mark.parametrize("m", [3, 8])
def test_topm_duplicated_sensors_tie_at_every_tick(m, gpu_device):
    """Sensors with identical data have identical scores bit for bit: ties at every tick, also across the 128-sensor
    sweeps of the kernel (copies 130 sensors apart) — the lower sensor is always named first."""
    pred, gt = ref.seeded_scores(1500, 300, seed=21)
    for src, dst in ((5, 6), (5, 135), (40, 299), (200, 201)):
        pred[:, dst], gt[:, dst] = pred[:, src], gt[:, src]
    got_v, got_i = _check_topm(pred, gt, m, gpu_device)
    tie = got_v[3:, :-1] == got_v[3:, 1:]
    assert tie.sum() > 20
    assert (np.diff(got_i[3:], axis=1)[tie] > 0).all()


@pytest.mark.parametrize("t,n,cut", [(1000, 27, 498), (4099, 200, 2)])
def test_topm_two_halves_with_a_halo_equal_one_run(t, n, cut, gpu_device):
    from gdn_amd import ops
    pred, gt = (torch.from_numpy(a).to(gpu_device) for a in ref.seeded_scores(t, n, seed=7))
    med_iqr = ops.score_quantiles(pred, gt)
    whole_v, whole_i = ops.score_smooth_topm(pred, gt, med_iqr, 3)
    parts = []
    for s0, s1 in ((0, cut), (cut, t)):
        hp = hg = None
        if s0 > 0:
            hp = torch.zeros((3, n), device=gpu_device)
            hg = torch.zeros((3, n), device=gpu_device)
            have = min(3, s0)
            hp[3 - have:] = pred[s0 - have:s0]
            hg[3 - have:] = gt[s0 - have:s0]
        parts.append(ops.score_smooth_topm(pred[s0:s1].contiguous(), gt[s0:s1].contiguous(), med_iqr, 3,
                                           first_tick=s0, halo_pred=hp, halo_gt=hg))
    assert torch.equal(torch.cat([p[0] for p in parts]), whole_v)
    assert torch.equal(torch.cat([p[1] for p in parts]), whole_i)


# ------------------------------------------------------------------------------------------------ attention
def _model(n, w, k, d, dev, layers=1, seed=11):
    from gdn_amd import GDN
    torch.manual_seed(seed)
    model = GDN([torch.zeros((2, 1), dtype=torch.long)], n, dim=d, input_dim=w, topk=k, out_layer_num=layers,
                out_layer_inter_dim=32)
    with torch.no_grad():
        gnn = model.gnn_layers[0].gnn
        gnn.att_em_i.uniform_(-0.3, 0.3)
        gnn.att_em_j.uniform_(-0.3, 0.3)
        gnn.att_i.uniform_(-0.5, 0.5)
        gnn.att_j.uniform_(-0.5, 0.5)
    params = {key: v.detach().clone() for key, v in model.state_dict().items()}
    return model.to(dev).eval(), params


def _series(n, t, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((n, t), generator=g) * 2.0 - 0.5


def _ref_mean(params, series, first, batch, w, graph, weights=None, chunk=32):
    """The float64 weighted mean, a chunk of windows at a time (4096 sensors x hundreds of windows)."""
    wt = np.ones(batch) if weights is None else np.asarray(weights, dtype=np.float64)
    total, nb = None, None
    for s in range(0, batch, chunk):
        e = min(batch, s + chunk)
        alpha, nb = ref.attention_rows(params, ref.windows_of(series, first + s, e - s, w), graph)
        part = np.tensordot(wt[s:e], alpha, axes=(0, 0))
        total = part if total is None else total + part
    return (total / wt.sum() if wt.sum() > 0 else np.zeros_like(total)), nb


SHAPES = [(127, 15, 30, 64), (512, 30, 64, 128), (700, 15, 30, 64), (127, 100, 30, 64), (127, 15, 30, 48),
          (4096, 15, 30, 64)]


def _check_at(model, params, series, n, w, k, dev, q=48):
    g = np.random.default_rng(3)
    t_raw = series.shape[1]
    windows = np.sort(g.integers(0, t_raw - w + 1, size=q))
    windows[0], windows[-1] = 0, t_raw - w                        # both ends of the series
    sensors = g.integers(0, n, size=q)
    sensors[:2] = (0, n - 1)
    sd = series.to(dev)
    got = model.attention_at(sd, torch.from_numpy(windows).to(dev), torch.from_numpy(sensors).to(dev))
    graph = model.learned_graph.cpu()
    nbg = model.attention_neighbours().cpu().numpy()
    assert got.shape == (q, k + 1) and got.dtype == torch.float32
    x = torch.stack([series[:, b:b + w] for b in windows])        # [q, n, w]
    alpha, nb = ref.attention_rows(params, x, graph)
    want = alpha[np.arange(q), sensors]
    np.testing.assert_array_equal(nbg, nb)                        # the reference edge order, -1 padding
    got_np = got.cpu().numpy()
    print(f"attention_at n={n} w={w} k={k}: max |hip - float64| = {np.abs(got_np - want).max():.2e}")
    np.testing.assert_allclose(got_np, want, atol=ATT_ATOL, rtol=ATT_RTOL)
    np.testing.assert_allclose(got_np.sum(axis=1), 1.0, atol=1e-5)
    assert (got_np[nb[sensors] < 0] == 0).all()                   # padding slots are exactly 0
    # the windows addressing gives the same bits
    got_w = model.attention_at(x.to(dev), torch.arange(q, device=dev), torch.from_numpy(sensors).to(dev))
    assert torch.equal(got_w, got)
    return got


def _check_mean(model, params, series, n, w, k, dev, first, batch):
    sd = series.to(dev)
    mean, nbg = model.attention_series(sd, first, batch)
    graph = model.learned_graph.cpu()
    mask = (torch.arange(batch) % 3 != 1).float()
    mask[: batch // 5] = 0.0
    masked, _ = model.attention_series(sd, first, batch, weights=mask.to(dev))
    want, nb = _ref_mean(params, series, first, batch, w, graph)
    want_m, _ = _ref_mean(params, series, first, batch, w, graph, weights=mask.numpy())
    np.testing.assert_array_equal(nbg.cpu().numpy(), nb)
    for name, got, exp in (("plain", mean, want), ("masked", masked, want_m)):
        got_np = got.cpu().numpy()
        print(f"attention_series {name} n={n} w={w} k={k} windows={batch}: max |hip - float64| = "
              f"{np.abs(got_np - exp).max():.2e}")
        assert got.shape == (n, k + 1)
        np.testing.assert_allclose(got_np, exp, atol=ATT_ATOL, rtol=ATT_RTOL)
        np.testing.assert_allclose(got_np.sum(axis=1), 1.0, atol=1e-5)
        assert (got_np[nb < 0] == 0).all()
    # same bits: a second run, and the windows addressing
    again, _ = model.attention_series(sd, first, batch, weights=mask.to(dev))
    assert torch.equal(again, masked)
    xw = ref.windows_of(series, first, batch, w).to(dev)
    assert torch.equal(model.attention_windows(xw)[0], mean)
    assert torch.equal(model.attention_windows(xw, weights=mask.to(dev))[0], masked)
    zero, _ = model.attention_series(sd, first, batch, weights=torch.zeros(batch, device=dev))
    assert not zero.any()


@pytest.mark.parametrize("n,w,k,d", SHAPES, ids=["-".join(str(v) for v in s) for s in SHAPES])
def test_attention_at_from_raw_data(n, w, k, d, gpu_device):
    model, params = _model(n, w, k, d, gpu_device)
    _check_at(model, params, _series(n, 600 + w), n, w, k, gpu_device)


@pytest.mark.parametrize("n,w,k,d", SHAPES, ids=["-".join(str(v) for v in s) for s in SHAPES])
def test_attention_series_mean_from_raw_data(n, w, k, d, gpu_device):
    batch = 4096 if (n, w, k, d) == SHAPES[0] else 300
    model, params = _model(n, w, k, d, gpu_device)
    _check_mean(model, params, _series(n, batch + w + 9), n, w, k, gpu_device, first=7, batch=batch)


def test_attention_of_an_mlp_head_model(gpu_device):
    n, w, k, d = 40, 8, 6, 16
    model, params = _model(n, w, k, d, gpu_device, layers=2)
    series = _series(n, 400 + w)
    _check_at(model, params, series, n, w, k, gpu_device)
    _check_mean(model, params, series, n, w, k, gpu_device, first=0, batch=400)


def test_attention_mean_keeps_the_bar_over_32768_windows(gpu_device):
    n, w, k, d = 127, 15, 30, 64
    model, params = _model(n, w, k, d, gpu_device)
    series = _series(n, 32768 + w)
    mean, _ = model.attention_series(series.to(gpu_device), 0, 32768)
    want, _ = _ref_mean(params, series, 0, 32768, w, model.learned_graph.cpu(), chunk=2048)
    print(f"attention_series over 32768 windows: max |hip - float64| = {np.abs(mean.cpu().numpy() - want).max():.2e}")
    np.testing.assert_allclose(mean.cpu().numpy(), want, atol=ATT_ATOL, rtol=ATT_RTOL)


def test_attention_refuses_bf16_and_cpu_inputs_by_name(gpu_device):
    from gdn_amd import _lib
    model, _ = _model(27, 5, 5, 16, gpu_device)
    series = _series(27, 100).to(gpu_device)
    with pytest.raises(_lib.GdnHipError, match="bfloat16"):
        model.attention_series(series.bfloat16(), 0, 8)
    with pytest.raises(_lib.GdnHipError, match="bfloat16"):
        model.attention_at(series.bfloat16(), [0], [0])
    with pytest.raises(_lib.GdnHipError, match="bfloat16"):
        model.attention_windows(torch.zeros((4, 27, 5), dtype=torch.bfloat16, device=gpu_device))
    with pytest.raises(_lib.GdnHipError, match="HIP device"):
        model.attention_series(series.cpu(), 0, 8)
    with pytest.raises(_lib.GdnHipError, match="HIP device"):
        model.attention_at(series.cpu(), [0], [0])
    with pytest.raises(ValueError):
        model.attention_at(series, [96], [0])                 # the window runs past the series
    with pytest.raises(ValueError):
        model.attention_at(series, [0], [27])


# ------------------------------------------------------------------------------------------------ evaluator
def _evaluator_case(dev, n=27, w=5, k=5, d=64, t=3000):
    model, params = _model(n, w, k, d, dev)
    series = _series(n, t + w, seed=9)
    series[3, 1000:1040] += 1.5                                # a stuck sensor: clearly separated scores
    y = series[:, w:].t().contiguous()
    return model, params, series, y


def test_evaluator_top_m_graph_replay_equals_eager_and_keeps_the_anomaly(gpu_device):
    from gdn_amd import harness
    model, _params, series, y = _evaluator_case(gpu_device)
    sd, yd = series.to(gpu_device), y.to(gpu_device)
    eager = harness.SeriesEvaluator(model, None, yd, batch=512, use_graph=False, series=sd, top_m=3)
    graphed = harness.SeriesEvaluator(model, None, yd, batch=512, use_graph=True, series=sd, top_m=3)
    plain = harness.SeriesEvaluator(model, None, yd, batch=512, use_graph=True, series=sd)
    a_e = eager.step().clone()
    graphed.step()
    a_g = graphed.step().clone()                                # a replay
    a_0 = plain.step().clone()
    torch.cuda.synchronize()
    assert torch.equal(graphed.top_scores, eager.top_scores) and torch.equal(graphed.top_sensors, eager.top_sensors)
    assert torch.equal(a_g, a_e) and torch.equal(a_g, a_0)
    assert torch.equal(graphed.anomaly, graphed.top_scores[:, 0])
    assert plain.top_scores is None and plain.top_m == 0
    with pytest.raises(ValueError):
        harness.SeriesEvaluator(model, None, yd, batch=512, series=sd, top_m=9)


def test_localise_agrees_with_the_float64_helper(gpu_device):
    from gdn_amd import harness
    model, params, series, y = _evaluator_case(gpu_device)
    ev = harness.SeriesEvaluator(model, None, y.to(gpu_device), batch=512, use_graph=True, series=series.to(gpu_device),
                                 top_m=3)
    anomaly = ev.step()
    ticks = torch.topk(anomaly, 20).indices.sort().values
    loc = harness.localise(ev, ticks)
    tk = ticks.cpu().numpy()
    pred = ev.pred.cpu().numpy()
    scores = ref.scores_f64(pred, y.numpy())
    want_v, want_i = ref.topm(scores, 3)
    skip_all = ref.skippable_ticks(scores, 3)
    assert ref.skipped_share(skip_all) <= ref.SKIP_CAP
    skip = skip_all[tk]
    sens = loc.sensors.cpu().numpy()
    assert sens.shape == (20, 3) and loc.attention.shape == (20, 3, 6) and loc.neighbours.shape == (20, 3, 6)
    np.testing.assert_allclose(loc.scores.cpu().numpy(), want_v[tk], rtol=1e-12, atol=1e-13)
    np.testing.assert_array_equal(sens[~skip], want_i[tk][~skip])
    np.testing.assert_array_equal(loc.predicted.cpu().numpy(), pred[tk[:, None], sens])
    np.testing.assert_array_equal(loc.observed.cpu().numpy(), y.numpy()[tk[:, None], sens])
    x = torch.stack([series[:, b:b + 5] for b in tk])
    alpha, nb = ref.attention_rows(params, x, model.learned_graph.cpu())
    np.testing.assert_array_equal(loc.neighbours.cpu().numpy(), nb[sens])
    np.testing.assert_allclose(loc.attention.cpu().numpy(), alpha[np.arange(20)[:, None], sens], atol=ATT_ATOL,
                               rtol=ATT_RTOL)
    one = harness.localise(ev, ticks[:4], m=1)
    assert torch.equal(one.sensors, loc.sensors[:4, :1]) and torch.equal(one.attention, loc.attention[:4, :1])
    with pytest.raises(ValueError):
        harness.localise(harness.SeriesEvaluator(model, None, y.to(gpu_device), batch=512,
                                                 series=series.to(gpu_device)), ticks)


def _write_cli_dataset(data, root):
    import pandas as pd
    os.makedirs(os.path.join(root, "msl"), exist_ok=True)
    pd.DataFrame(data["train_raw"], columns=[str(c) for c in data["columns_train"]]).to_csv(os.path.join(root, "msl", "train.csv"))
    pd.DataFrame(data["test_raw"], columns=[str(c) for c in data["columns_test"]]).to_csv(os.path.join(root, "msl", "test.csv"))
    with open(os.path.join(root, "msl", "list.txt"), "w") as f:
        f.write("\n".join(str(c) for c in data["features"]) + "\n")


def test_command_line_localise_writes_what_localise_returns(gpu_device, tmp_path, capsys):
    from gdn_amd import harness, main as cli
    data, p = load_golden("cli_msl_slice")
    batch, w, dim, stride, topk, seed, inter = (int(v) for v in data["meta_cfg"])
    root = str(tmp_path / "data")
    _write_cli_dataset(data, root)
    ckpt = str(tmp_path / "ckpt.pt")
    torch.save(p, ckpt)
    out = str(tmp_path / "where.npz")
    argv = ["-dataset", "msl", "-data_root", root, "-device", "cuda", "-batch", str(batch), "-slide_win", str(w),
            "-dim", str(dim), "-slide_stride", str(stride), "-topk", str(topk), "-random_seed", str(seed),
            "-out_layer_inter_dim", str(inter), "-val_ratio", str(float(data["val_ratio"])), "-report", "best",
            "-load_model_path", ckpt]
    info_plain = cli.main(argv)
    printed_plain = capsys.readouterr().out
    assert not os.path.exists(out)
    info = cli.main(argv + ["-localise", out])
    report = lambda text: [ln for ln in text.splitlines() if ln.startswith(("F1 score:", "precision:", "recall:"))]
    assert report(capsys.readouterr().out) == report(printed_plain) and tuple(info) == tuple(info_plain)
    saved = np.load(out)
    assert float(saved["threshold"]) == float(info[4])
    # the same structure from an evaluator of our own on the same data
    args = cli.build_parser().parse_args(argv)
    import random
    random.seed(args.random_seed)
    torch.manual_seed(args.random_seed)
    m = cli.Main({"batch": batch, "epoch": 1, "slide_win": w, "dim": dim, "slide_stride": stride, "comment": "",
                  "seed": seed, "out_layer_num": 1, "out_layer_inter_dim": inter, "decay": 0,
                  "val_ratio": float(data["val_ratio"]), "topk": topk},
                 {"save_path": "msl", "dataset": "msl", "report": "best", "device": "cuda", "load_model_path": ckpt,
                  "data_root": root})
    m.run()
    gt = m.test_series[:, w:].t().contiguous()
    ev = harness.SeriesEvaluator(m.model, None, gt, batch=8192, use_graph=False, series=m.test_series, top_m=3)
    anomaly = ev.step()
    ticks = torch.nonzero(anomaly > float(info[4])).view(-1)
    assert ticks.numel() > 0 and np.array_equal(saved["ticks"], ticks.cpu().numpy())
    want = harness.localise(ev, ticks).numpy()
    for name, arr in want.items():
        np.testing.assert_array_equal(saved[name], arr, err_msg=name)
