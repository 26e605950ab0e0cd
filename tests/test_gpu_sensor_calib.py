"""GPU suite of the calibration on each sensor's own readings: gdn_score_keys_valid,
gdn_score_key_counts, gdn_score_select_counts on every route of the select, gdn_stream_calib_write_sensor,
harness.SeriesEvaluator(calib="sensor") and StreamDetector(calib="sensor") against tests/_sensor_calib_ref.py.
Tables, counts, keys, rings and sensors are compared bit for bit with the numpy reference.  The smoothed scores come
from the `_gaps` sweep, which this feature does not touch: they are compared bit for bit with that sweep run on the
REFERENCE's table, and with numpy at the sweep's own float64 bar (tests/test_gpu_stream_gaps.py: the kernel multiplies
by one reciprocal per sensor where numpy divides)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _sensor_calib_ref as cref
import _series_gaps_ref as sref
from test_gpu_stream import _model
from test_gpu_stream_gaps import _assert_scores
from test_gpu_stream_recal import _drive

pytestmark = pytest.mark.gpu

N_SELECT = 70                                                # the keys kernel crosses a 64-sensor tile
# name -> (blocks, pitch): the single-slice finisher, the one-workgroup select (flat, then blocked), the digit passes
SELECT_SHAPES = {"slice": (1, 300), "onewg": (1, 5000), "multi": (1, 40000), "blocked": (2, 2048)}
MOTIVATING = (40, 8, 6, 64)                                  # n, w, k, d; t = 1500


def _f64_bits(t):
    return t.contiguous().view(torch.int64)


def _same_table(got, want, what):
    got = got.cpu().numpy()
    assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(want).view(np.uint64)), (what, got, want)


def _select_inputs(name):
    """(gt [blocks, pitch, n] fp32 with pred = 0, valid [blocks, pitch, n] bool, counts [n]) of one shape: i.i.d.
    errors (every seventh sensor in steps of 1/8: ties), the real slots of a sensor a seeded random subset of its
    blocks * pitch slots whose size runs through 1, 2, 3, all, all but one, 4096, 4095, an even and an odd count."""
    blocks, pitch = SELECT_SHAPES[name]
    slots = blocks * pitch
    g = np.random.default_rng(100 + pitch)
    gt = g.random((slots, N_SELECT)).astype(np.float32)
    gt[:, ::7] = np.round(gt[:, ::7] * 8) / 8
    special = [c for c in (1, 2, 3, slots, slots - 1, 4096, 4095, 150, 151) if c <= slots]
    counts = np.array(special + [int(c) for c in g.integers(4, slots + 1, N_SELECT - len(special))])
    valid = np.zeros((slots, N_SELECT), dtype=bool)
    for s, c in enumerate(counts):
        valid[g.permutation(slots)[:c], s] = True
    return gt.reshape(blocks, pitch, N_SELECT), valid.reshape(blocks, pitch, N_SELECT), counts


def _keys_of(gt, valid, dev):
    """keys [blocks, n, pitch] through score_keys(valid=), one launch per block."""
    from gdn_amd import ops
    blocks, pitch, n = gt.shape
    keys = torch.empty((blocks, n, pitch), dtype=torch.float64, device=dev)
    zero = torch.zeros((pitch, n), dtype=torch.float32, device=dev)
    for b in range(blocks):
        ops.score_keys(zero, torch.from_numpy(gt[b]).to(dev), pitch, out=keys[b],
                       valid=torch.from_numpy(valid[b].astype(np.uint8)).to(dev))
    return keys


def _select_tables(dev="cuda:0"):
    """name -> (med_iqr [n, 2], counts [n] as score_key_counts gives them), on whatever route the environment picks."""
    from gdn_amd import ops
    out = {}
    for name, (blocks, pitch) in SELECT_SHAPES.items():
        gt, valid, _counts = _select_inputs(name)
        keys = _keys_of(gt, valid, dev)
        counts = ops.score_key_counts(keys, blocks, N_SELECT, pitch)
        out[name] = (ops.score_select_counts(keys, blocks, N_SELECT, pitch, counts).cpu(), counts.cpu())
    return out


_WANT = {}


def _want_table(name):
    if name not in _WANT:                                    # computed once, shared, never changed
        gt, valid, counts = _select_inputs(name)
        slots = gt.shape[0] * gt.shape[1]
        table, got = cref.table(np.zeros((slots, N_SELECT), dtype=np.float32), gt.reshape(slots, N_SELECT),
                                valid.reshape(slots, N_SELECT))
        assert np.array_equal(got, counts)
        _WANT[name] = (table, counts)
    return _WANT[name]


def _assert_select_tables(tables, what):
    for name in SELECT_SHAPES:
        want, counts = _want_table(name)
        assert tables[name][1].tolist() == counts.tolist(), (what, name)
        _same_table(tables[name][0], want, (what, name))


# ------------------------------------------------------------------------------------------------ 1. the library
def test_every_route_of_the_select_equals_numpy_on_each_sensors_own_keys(gpu_device):
    _assert_select_tables(_select_tables(gpu_device), "default")


@pytest.mark.parametrize("env", [{"GDN_SELECT_MULTI": "1"}, {"GDN_SELECT_BRACKET": "0"}], ids=["multi", "no-bracket"])
def test_the_select_knobs_act_on_the_counts_entry_too(env, gpu_device, tmp_path):
    """Both knobs are read once per process: a fresh child runs the four shapes under each."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, torch; sys.path.insert(0, %r); sys.path.insert(0, %r + '/tests');"
            "import test_gpu_sensor_calib as m; torch.save(m._select_tables(), sys.argv[1])")
    f = str(tmp_path / "tables.pt")
    subprocess.run([sys.executable, "-c", code % (root, root), f], check=True, timeout=300, env=dict(os.environ, **env))
    _assert_select_tables(torch.load(f, weights_only=True), env)


@pytest.mark.parametrize("name", list(SELECT_SHAPES))
def test_equal_counts_give_the_bits_of_the_plain_select(name, gpu_device):
    from gdn_amd import ops
    dev = gpu_device
    blocks, pitch = SELECT_SHAPES[name]
    gt, _valid, _counts = _select_inputs(name)
    T = blocks * pitch - 37                                  # 37 filler slots behind the keys of the last block
    valid = np.ones(gt.shape, dtype=bool)
    valid[-1, pitch - 37:] = False
    keys = _keys_of(gt, valid, dev)
    counts = torch.full((N_SELECT,), T, dtype=torch.int32, device=dev)
    assert torch.equal(ops.score_key_counts(keys, blocks, N_SELECT, pitch), counts)
    a = ops.score_select(keys, blocks, N_SELECT, pitch, T)
    b = ops.score_select_counts(keys, blocks, N_SELECT, pitch, counts)
    assert torch.equal(_f64_bits(a), _f64_bits(b))


def test_the_bracket_settles_a_sensor_from_4096_real_keys_on(gpu_device):
    """pitch 32768, n = 8, i.i.d. keys.  The one-workgroup select tries its sample brackets when a sensor has at least
    4096 real keys — per sensor now — and, as before, when at least half of its 1024 sampled slots (every 32nd) hold a
    real key; the validity planes keep the sampled slots real so that the count alone decides.  The brackets miss with
    probability < 1e-6 per sensor, so path 0 is asserted."""
    from gdn_amd import ops
    dev = gpu_device
    pitch, n = 32768, 8
    counts = [32768, 20000, 4096, 4095, 4097, 1500, 3, 8192]
    g = np.random.default_rng(77)
    gt = g.random((pitch, n)).astype(np.float32)
    valid = np.zeros((pitch, n), dtype=bool)
    sampled = np.arange(0, pitch, 32)
    others = np.setdiff1d(np.arange(pitch), sampled)
    for s, c in enumerate(counts):
        take = min(c, sampled.size)
        valid[sampled[:take], s] = True
        valid[g.permutation(others)[:c - take], s] = True
    keys = _keys_of(gt[None], valid[None], dev)
    got = ops.score_key_counts(keys, 1, n, pitch)
    assert got.cpu().tolist() == counts
    path = torch.full((n,), -1, dtype=torch.int32, device=dev)
    table = ops.score_select_counts(keys, 1, n, pitch, got, path=path)
    assert path.cpu().tolist() == [0 if c >= 4096 else 1 for c in counts]
    want, _ = cref.table(np.zeros((pitch, n), dtype=np.float32), gt, valid)
    _same_table(table, want, "pitch 32768")


@pytest.mark.parametrize("name", ["slice", "onewg", "multi"])
def test_rows_below_min_count_keep_what_they_held(name, gpu_device):
    from gdn_amd import ops
    dev = gpu_device
    blocks, pitch = SELECT_SHAPES[name]
    gt, valid, counts = _select_inputs(name)
    keys = _keys_of(gt, valid, dev)
    min_count = 152
    assert (counts < min_count).sum() >= 5 and (counts >= min_count).sum() >= 5
    sentinel = torch.arange(2 * N_SELECT, dtype=torch.float64, device=dev).view(N_SELECT, 2) - 1000.0
    out = sentinel.clone()
    dcounts = torch.from_numpy(counts.astype(np.int32)).to(dev)
    ops.score_select_counts(keys, blocks, N_SELECT, pitch, dcounts, min_count=min_count, out=out)
    want, _ = _want_table(name)
    want = np.where((counts >= min_count)[:, None], want, sentinel.cpu().numpy())
    _same_table(out, want, name)
    zero = torch.zeros_like(dcounts)                         # counts below 1 never write, whatever min_count says
    out = sentinel.clone()
    ops.score_select_counts(keys, blocks, N_SELECT, pitch, zero, min_count=0, out=out)
    assert torch.equal(out, sentinel)


def test_keys_with_an_all_ones_plane_are_the_plain_keys_and_missing_readings_the_filler(gpu_device):
    from gdn_amd import ops
    dev = gpu_device
    t, n, pitch = 131, N_SELECT, 140
    g = torch.Generator().manual_seed(3)
    pred, gt = torch.rand((t, n), generator=g).to(dev), torch.rand((t, n), generator=g).to(dev)
    ones = torch.ones((t, n), dtype=torch.uint8, device=dev)
    assert torch.equal(_f64_bits(ops.score_keys(pred, gt, pitch, valid=ones)), _f64_bits(ops.score_keys(pred, gt, pitch)))
    valid = torch.rand((t, n), generator=g) < 0.7
    got = ops.score_keys(pred, gt, pitch, valid=valid.to(torch.uint8).to(dev))
    want = cref.keys_valid(pred.cpu().numpy(), gt.cpu().numpy(), valid.numpy(), pitch)
    assert np.array_equal(got.cpu().numpy().view(np.uint64), want)
    counts = ops.score_key_counts(got, 1, n, pitch)
    assert counts.dtype == torch.int32 and counts.cpu().tolist() == (want != cref.FILLER).sum(axis=1).tolist()
    with pytest.raises(ValueError, match="exclude each other"):
        ops.score_keys(pred, gt, pitch, valid=ones, keep=ones[:, 0].contiguous())


# ------------------------------------------------------------------------------------------------ 2. the evaluator
def _motivating(dev, d):
    n, w, k, _ = MOTIVATING
    raw = cref.motivating_series(n, w, 1500)
    return _model(dev, n, w, k, d), raw, torch.from_numpy(raw).to(dev)


@pytest.mark.parametrize("d", [64, 16], ids=["series-route", "window-route-fp32"])
def test_the_evaluator_calibrates_forty_sensors_that_share_hardly_a_complete_tick(d, gpu_device):
    from gdn_amd import harness, ops
    dev = gpu_device
    n, w = MOTIVATING[:2]
    m = 3
    model, raw, raw_d = _motivating(dev, d)
    with pytest.raises(ValueError, match=r"(?s)min_kept = 64.*kept = "):           # today's rule: too few complete ticks
        harness.SeriesEvaluator(model, None, None, 256, series=raw_d, gaps=True, use_graph=False)
    ev = harness.SeriesEvaluator(model, None, None, 256, series=raw_d, gaps=True, calib="sensor", use_graph=False,
                                 top_m=m)
    _filled, gt, valid, _keep, total, _run = sref.fill(raw, w)
    assert ev.counts.dtype == torch.int32 and ev.counts.cpu().tolist() == (1500 - total).tolist()
    assert ev.kept == int((1500 - total).min()) >= 64
    assert (ev._windows is not None) == (d == 16)
    anomaly = ev.step()
    pred = ev.pred.cpu().numpy()
    want, counts = cref.table(pred, gt, valid)
    _same_table(ev.med_iqr, want, "evaluator")
    # the sweep is the unchanged `_gaps` launch: bit for bit on the reference's table, numpy at the sweep's own bar
    ts, ti = ops.score_smooth_topm(ev.pred, ev.y, torch.from_numpy(want).to(dev), m, valid=ev.valid)
    assert torch.equal(ev.top_scores, ts) and torch.equal(ev.top_sensors, ti) and torch.equal(anomaly, ts[:, 0])
    sm, vals, idx = sref.scores(pred, gt, valid, want, m)
    _assert_scores(ev.top_scores, ev.top_sensors, vals, idx, ("sensor", d))
    full = harness.SeriesEvaluator(model, None, None, 256, series=raw_d, gaps=True, calib="sensor", use_graph=False,
                                   want_scores=True)
    assert torch.equal(full.step(), anomaly) and torch.equal(full.med_iqr, ev.med_iqr)
    np.testing.assert_allclose(full.scores.cpu().numpy(), sm, rtol=1e-12, atol=1e-13)
    loc = harness.localise(ev, [0, 1499])
    assert torch.equal(loc.observed, ev.y[loc.ticks.view(-1, 1), loc.sensors])
    # the captured step replays what the eager one launched
    cap = harness.SeriesEvaluator(model, None, None, 256, series=raw_d, gaps=True, calib="sensor", use_graph=True,
                                  top_m=m)
    for _ in range(2):
        cap.step()
    assert cap.graph is not None
    for name in ("pred", "med_iqr", "top_scores", "top_sensors"):
        assert torch.equal(getattr(cap, name), getattr(ev, name)), name
    short = raw_d.clone()
    short[7, w + 30:] = float("nan")
    with pytest.raises(ValueError, match=r"(?s)min_kept = 64.*sensors \[7\].*\[\d+\] real readings"):
        harness.SeriesEvaluator(model, None, None, 256, series=short, gaps=True, calib="sensor", use_graph=False)


def test_on_a_finite_series_calib_sensor_writes_the_bits_of_a_plain_evaluator(gpu_device):
    from gdn_amd import harness
    dev = gpu_device
    n, w, k, d = MOTIVATING
    model = _model(dev, n, w, k, d)
    series = torch.from_numpy(sref.clean_series(n, w, 300)).to(dev)
    plain = harness.SeriesEvaluator(model, None, series[:, w:].t().contiguous(), 64, series=series, use_graph=False,
                                    top_m=3)
    ev = harness.SeriesEvaluator(model, None, None, 64, series=series, gaps=True, calib="sensor", use_graph=False, top_m=3)
    plain.step()
    ev.step()
    assert ev.kept == 300 and ev.counts.cpu().tolist() == [300] * n
    for name in ("pred", "med_iqr", "top_scores", "top_sensors"):
        assert torch.equal(getattr(plain, name), getattr(ev, name)), name


# ------------------------------------------------------------------------------------------------ 3. the detector
def test_an_immediate_recalibration_returns_the_evaluators_table(gpu_device):
    from gdn_amd import harness
    dev = gpu_device
    n, w = MOTIVATING[:2]
    model, raw, raw_d = _motivating(dev, 64)
    ev = harness.SeriesEvaluator(model, None, None, 8192, series=raw_d, gaps=True, calib="sensor", use_graph=False)
    ev.step()
    det = harness.StreamDetector.from_calibration(model, raw_d, 64, gaps=True, calib_gaps=True, calib="sensor",
                                                  recal=2048, top_m=3)
    assert det.calib == "sensor" and det.calib_kept == ev.kept and torch.equal(det.calib_counts, ev.counts)
    assert torch.equal(det.med_iqr, ev.med_iqr)
    ring = cref.SensorRing(n, 2048)
    ring.seed(ev.pred.cpu().numpy(), ev.y.cpu().numpy(), ev.valid.cpu().numpy().astype(bool))
    assert np.array_equal(det.ring_keys.cpu().numpy().view(np.uint64), ring.keys)
    assert det.ring_keep.cpu().tolist() == ring.keep.tolist()
    det.med_iqr.fill_(-1.0)
    assert det.recalibrate() == n
    assert torch.equal(_f64_bits(det.med_iqr), _f64_bits(ev.med_iqr))
    assert det.recal_counts.dtype == torch.int64 and torch.equal(det.recal_counts, ev.counts.cpu().long())
    assert det.recal_kept == ev.kept


def test_a_dead_sensor_keeps_its_row_and_no_longer_stops_the_others(gpu_device):
    from gdn_amd import harness
    dev = gpu_device
    n, w = MOTIVATING[:2]
    model, raw, raw_d = _motivating(dev, 64)
    dead, R = 5, 256
    g = torch.Generator().manual_seed(9)
    stream = torch.rand((300, n), generator=g)
    stream[torch.rand((300, n), generator=g) < 0.05] = float("nan")
    stream[:, dead] = float("nan")
    stream = stream.to(dev)
    for calib in ("sensor", "tick"):
        det = harness.StreamDetector.from_calibration(model, raw_d, 64, gaps=True, calib_gaps=True, min_kept=8,
                                                      calib=calib, recal=R, recal_min=64, top_m=3)
        before = det.med_iqr.clone()
        rec = _drive(det, stream, (1, 7, 64))
        if calib == "tick":
            assert det.recalibrate() == 0 and torch.equal(det.med_iqr, before)     # not one complete tick: nothing, ever
            continue
        ring = cref.SensorRing(n, R)                        # (300 pushed ticks: nothing of the seed is left)
        for r in rec:
            ring.push(r[0].cpu().numpy(), r[1].cpu().numpy(), r[2].cpu().numpy(), r[3].cpu().numpy().astype(bool))
        assert np.array_equal(det.ring_keys.cpu().numpy().view(np.uint64), ring.keys)
        assert det.ring_keep.cpu().tolist() == ring.keep.tolist()
        want, counts = ring.table(64, before.cpu().numpy())
        assert counts[dead] == 0 and (np.delete(counts, dead) >= 64).all()
        assert det.recalibrate() == n - 1
        _same_table(det.med_iqr, want, "ring")
        assert torch.equal(det.med_iqr[dead], before[dead]) and not torch.equal(det.med_iqr, before)
        assert det.recal_counts.tolist() == counts.tolist() and det.recal_kept == int(np.delete(counts, dead).min())
        assert det.recals == 1


# ------------------------------------------------------------------------------------------------ 4. command line
def test_command_line_calib_by_sensor_prints_the_range_of_the_per_sensor_counts(gpu_device, tmp_path, capsys):
    import random

    from conftest import load_golden
    from gdn_amd import main as cli
    from test_gpu_localise import _write_cli_dataset
    data, p = load_golden("cli_msl_slice")
    batch, w, dim, stride, topk, seed, inter = (int(v) for v in data["meta_cfg"])
    data = dict(data)
    columns, sensors = [str(c) for c in data["columns_train"]], [str(f) for f in data["features"]]
    train_raw = np.array(data["train_raw"], dtype=np.float64)
    windows = len(range(w, train_raw.shape[0], stride))              # the validation block of this seed (main.py's draw)
    val_len = int(windows * float(data["val_ratio"]))
    random.seed(seed)
    lo = w + random.randrange(int(windows * (1 - float(data["val_ratio"])))) * stride
    for row, name in [(lo + 3, sensors[0]), (lo + 4, sensors[0]), (lo + 20, sensors[1]), (lo + 40, sensors[0])]:
        train_raw[row, columns.index(name)] = np.nan
    data["train_raw"] = train_raw
    root = str(tmp_path / "data")
    _write_cli_dataset(data, root)
    ckpt = str(tmp_path / "ckpt.pt")
    torch.save(p, ckpt)
    argv = ["-dataset", "msl", "-data_root", root, "-device", "cuda", "-batch", str(batch), "-slide_win", str(w),
            "-dim", str(dim), "-slide_stride", str(stride), "-topk", str(topk), "-random_seed", str(seed),
            "-out_layer_inter_dim", str(inter), "-val_ratio", str(float(data["val_ratio"])), "-report", "best",
            "-load_model_path", ckpt, "-stream", "16", "-stream_gaps"]
    with pytest.raises(ValueError, match="-calib_by_sensor needs -stream C -stream_gaps -stream_calib_gaps"):
        cli.main(argv + ["-calib_by_sensor"])
    capsys.readouterr()
    cli.main(argv + ["-stream_calib_gaps", "-calib_by_sensor", "-stream_recal", "64", "-stream_recal_every", "32"])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("stream:")]
    assert len(line) == 1, line
    print(line[0])
    # sensor 0 lost three readings of the block, sensor 1 one, the others none
    assert f"calibrated per sensor on {val_len - 3} to {val_len} real validation readings" in line[0]
    assert "recalibrations from a ring of 64 ticks" in line[0]
