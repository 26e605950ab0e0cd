"""GPU suite of the raw-readings front end: gdn_prep_stats / gdn_prep_series / gdn_prep_ticks against the
float64 restatement (tests/_prep_ref.py) and against what the reference's own scripts produced
(tests/golden/prep_ref.npz), bit for bit; harness.StreamDetector(prep=) pushed raw ticks against a plain detector
pushed the prepared series, bit for bit; and the two command lines in child processes."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _prep_ref as ref
from conftest import GOLDEN, ROOT
from test_gpu_stream import _detector, _model, _table

pytestmark = pytest.mark.gpu

TINY = (7, 5, 3, 16)                 # n, w, k, d: the stream tests' helper at the fixture's seven sensors
SERIES = (7, 5, 3, 32)               # ... at d = 32: the narrowest width forward_series (calibration, the command line) takes
DTYPES = {"fp32": torch.float32, "float64": torch.float64}


@functools.lru_cache(maxsize=None)
def _gold():
    with np.load(os.path.join(GOLDEN, "prep_ref.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _raw_case(t_raw, n, dtype):
    """Seeded raw readings [t_raw, n] on per-sensor scales with ~4 % NaN and a few infinities, as `dtype` would hold
    them (float64 array of the values the device sees)."""
    g = np.random.default_rng(1000 * t_raw + n)
    x = g.standard_normal((t_raw, n)) * (10.0 ** g.integers(-3, 5, size=n))[None, :] + g.standard_normal(n)[None, :] * 50
    x[g.random((t_raw, n)) < 0.04] = np.nan
    x[g.random((t_raw, n)) < 0.005] = np.inf
    x[g.random((t_raw, n)) < 0.005] = -np.inf
    if dtype == "fp32":
        x = x.astype(np.float32).astype(np.float64)
    x.setflags(write=False)
    return x


def _dev(x, dtype, dev):
    return torch.from_numpy(np.array(x)).to(DTYPES[dtype]).to(dev)


def _bits64(t):
    return t.detach().cpu().contiguous().view(torch.int64)


# ------------------------------------------------------------------------------------------------ stats
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("t_raw,n", [(403, 7), (1000, 65), (37, 1)])
def test_stats_equal_the_restatement_and_are_reproducible(t_raw, n, dtype, gpu_device):
    from gdn_amd import ops
    x = _raw_case(t_raw, n, dtype)
    want = ref.stats(x)
    raw = _dev(x, dtype, gpu_device)
    got = ops.prep_stats(raw)
    again = ops.prep_stats(raw)
    assert torch.equal(_bits64(got), _bits64(again))                  # a fixed summation order
    got = got.cpu().numpy()
    for col in (0, 1, 3):                                             # min, max, count: exact
        assert np.array_equal(got[:, col].view(np.int64), want[:, col].view(np.int64)), col
    finite = np.where(np.isfinite(x), np.abs(x), 0.0).max(axis=0)
    bound = t_raw * 2.0 ** -53 * finite                              # what any summation order meets
    err = np.abs(got[:, 2] - want[:, 2])
    print(f"stats {t_raw}x{n} {dtype}: max |mean - fsum mean| / bound = {np.max(err / np.maximum(bound, 1e-300)):.3g}")
    assert (err <= bound).all()


def test_stats_of_a_sensor_without_readings_and_of_one_with_infinities(gpu_device):
    from gdn_amd import ops
    x = np.array(_raw_case(37, 1, "float64")).repeat(3, axis=1)
    x[:, 0] = np.nan
    x[::2, 0] = np.inf
    x[:, 1] = np.arange(37.0)
    x[5, 1], x[9, 1], x[20, 1] = np.inf, -np.inf, np.nan
    want = ref.stats(x)
    assert (want[0] == 0.0).all() and tuple(want[1, [0, 1, 3]]) == (0.0, 36.0, 34.0)
    for dtype in DTYPES:
        got = ops.prep_stats(_dev(x, dtype, gpu_device)).cpu().numpy()
        assert np.array_equal(got[:2].view(np.int64), want[:2].view(np.int64)), dtype   # (integers: the sum is exact)


# ------------------------------------------------------------------------------------------------ series
def _groups(down):
    return 70 if down <= 10 else 3           # 70 groups cross the 64-group tile of a workgroup


@pytest.mark.parametrize("tail", [0, 1, -1])
@pytest.mark.parametrize("down", [1, 2, 9, 10, 64])
@pytest.mark.parametrize("n", [7, 65])
def test_series_equal_the_restatement_bit_for_bit(n, down, tail, gpu_device):
    from gdn_amd import ops
    t_raw = _groups(down) * down + tail
    g = np.random.default_rng(n + down)
    tab = np.stack([1.0 / (g.random(n) * 100 + 0.5), g.standard_normal(n)], axis=1)
    labels = (g.random(t_raw) < 0.1).astype(np.float64)
    for dtype in DTYPES:
        x = _raw_case(t_raw, n, dtype)
        want, want_lab, _ = ref.series(x, tab, down, labels=labels)
        got, lab = ops.prep_series(_dev(x, dtype, gpu_device), torch.from_numpy(tab).to(gpu_device), down,
                                   labels=torch.from_numpy(labels).to(gpu_device))
        assert got.shape == (n, t_raw // down) and got.dtype == torch.float32 and got.is_contiguous()
        assert np.array_equal(ref.bits32(got.cpu().numpy()), ref.bits32(want)), dtype
        assert np.array_equal(lab.cpu().numpy(), want_lab)
        fill = g.standard_normal(n)
        want_f, _, _ = ref.series(x, tab, down, fill=fill)
        got_f, none = ops.prep_series(_dev(x, dtype, gpu_device), torch.from_numpy(tab).to(gpu_device), down,
                                      fill=torch.from_numpy(fill).to(gpu_device))
        assert none is None and np.array_equal(ref.bits32(got_f.cpu().numpy()), ref.bits32(want_f)), dtype
        assert not np.isnan(want_f).any()


def test_series_equal_the_references_own_output(gpu_device):
    from gdn_amd import Prep
    gold = _gold()
    dev = gpu_device
    dtype = "float64"                         # the reference's files are float64
    prep = Prep.fit(_dev(gold["train"], dtype, dev), down=int(gold["down"]))
    assert np.array_equal(prep.table.cpu().numpy().view(np.int64), gold["ref_table"].view(np.int64))
    for name in ("train", "test"):
        got, lab = prep.series(_dev(gold[name], dtype, dev), labels=torch.from_numpy(gold[name + "_labels"]).to(dev))
        assert np.array_equal(ref.bits32(got.cpu().numpy()), ref.bits32(gold["ref_" + name].T.astype(np.float32)))
        assert np.array_equal(lab.cpu().numpy(), gold["ref_" + name + "_labels"])
        skipped, lab_s = prep.series(_dev(gold[name], dtype, dev), skip=3,
                                     labels=torch.from_numpy(gold[name + "_labels"]).to(dev))
        assert torch.equal(skipped, got[:, 3:]) and torch.equal(lab_s, lab[3:]) and skipped.is_contiguous()
    assert (prep.series(_dev(gold["train"], dtype, dev))[0][3] == 0.0).all()           # the constant sensor: exactly 0
    # fp32 raw readings: the restatement on the values fp32 holds
    x32 = gold["test"].astype(np.float32)
    got, _ = prep.series(torch.from_numpy(x32).to(dev))
    want, _, _ = ref.series(x32.astype(np.float64), gold["ref_table"], int(gold["down"]))
    assert np.array_equal(ref.bits32(got.cpu().numpy()), ref.bits32(want))
    with pytest.raises(ValueError, match=r"t_raw = 9 .* down = 10"):
        prep.series(torch.zeros((9, 7), dtype=torch.float64, device=dev))


def test_series_without_a_fill_leaves_missing_readings_out_of_the_median(gpu_device):
    from gdn_amd import ops
    g = np.random.default_rng(5)
    x = g.standard_normal((40, 7)) * 30
    x[1:10, 0] = np.nan                       # group 0 of sensor 0: 1 finite reading
    x[12:20, 0] = np.inf                      # group 1: 2
    x[25, 0] = -np.inf                        # group 2: 9
    x[30:40, 0] = np.nan                      # group 3: none
    x[:, 4] = np.nan                          # a sensor with none at all
    tab = ref.table(ref.stats(x))
    want, _, _ = ref.series(x, tab, 10)
    assert np.isnan(want[0, 3]) and np.isnan(want[4]).all() and np.isnan(want).sum() == 5
    assert want[0, 0] == np.float32(x[0, 0] * tab[0, 0] + tab[0, 1])
    for dtype in DTYPES:
        xs = x.astype(np.float32).astype(np.float64) if dtype == "fp32" else x
        want, _, _ = ref.series(xs, tab, 10)
        got, _ = ops.prep_series(_dev(xs, dtype, gpu_device), torch.from_numpy(tab).to(gpu_device), 10)
        got = got.cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(ref.bits32(got)[~np.isnan(want)], ref.bits32(want)[~np.isnan(want)])


def test_series_with_the_mean_fill_follow_the_reference_on_the_nan_pair(gpu_device):
    from gdn_amd import Prep
    gold = _gold()
    dev = gpu_device
    prep = Prep.fit(torch.from_numpy(gold["train_nan"]).to(dev), down=int(gold["down"]))
    assert np.array_equal(prep.table.cpu().numpy().view(np.int64), gold["ref_table_nan"].view(np.int64))
    for name in ("train", "test"):
        raw = gold[name + "_nan"]
        got, lab = prep.series(torch.from_numpy(raw).to(dev), fill="mean",
                               labels=torch.from_numpy(gold[name + "_labels"]).to(dev))
        filled = ref.series(raw, gold["ref_table_nan"], int(gold["down"]), fill=np.zeros(7))[2]
        ref.assert_filled_rule(got.cpu().numpy(), gold["ref_" + name + "_nan"].T, filled)
        assert np.array_equal(lab.cpu().numpy(), gold["ref_" + name + "_labels_nan"])


# ------------------------------------------------------------------------------------------------ raw ticks
PUSHES = [1, 3, 10, 7, 25, 40, 40, 1, 9]


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("down,c", [(10, 4), (1, 40)])
def test_ticks_in_uneven_pushes_equal_the_series_and_keep_the_tail(down, c, dtype, gpu_device):
    from gdn_amd import ops
    gold = _gold()
    dev = gpu_device
    x = gold["test_nan"][:sum(PUSHES)]
    if dtype == "fp32":
        x = x.astype(np.float32).astype(np.float64)
    raw = _dev(x, dtype, dev)
    tab = torch.from_numpy(gold["ref_table_nan"]).to(dev)
    want, _ = ops.prep_series(raw, tab, down)
    planes = [torch.full((max(1, down - 1), 7), -7.0, dtype=torch.float64, device=dev) for _ in range(2)]
    out = torch.full((c, 7), -7.0, device=dev)
    rows, pending, at, cur = [], 0, 0, 0
    for r in PUSHES:
        out.fill_(-7.0)
        groups = ops.prep_ticks(raw[at:at + r], planes[cur], pending, planes[cur ^ 1], down, tab, out)
        at += r
        assert groups == (pending + r) // down
        rows.append(out[:groups].clone())
        assert (out[groups:] == -7.0).all()                            # rows beyond the completed groups are not written
        pending = (pending + r) % down
        cur ^= 1
        tail = torch.from_numpy(x[at - pending:at]).to(dev)
        assert torch.equal(_bits64(planes[cur][:pending]), _bits64(tail)), at        # NaN readings included
        if down == 1:
            assert pending == 0
    got = torch.cat(rows)
    assert got.shape[0] == sum(PUSHES) // down
    assert np.array_equal(ref.bits32(got.cpu().numpy()), ref.bits32(want.t().cpu().numpy()))
    with pytest.raises(ValueError, match="more than the"):
        ops.prep_ticks(raw[:c * down + down], planes[0], 0, planes[1], down, tab, out)
    with pytest.raises(ValueError, match="alias"):
        ops.prep_ticks(raw[:1], planes[0], 0, planes[0], down, tab, out)


# ------------------------------------------------------------------------------------------------ detector
def _stream_case(dev, with_nan=False):
    """(prep, history [7, w], raw stream [207, 7] float64 on the device, prepared stream [20, 7] fp32)."""
    from gdn_amd import Prep
    gold = _gold()
    w = TINY[1]
    prep = Prep.fit(torch.from_numpy(gold["train"]).to(dev), down=10)
    x = gold["test"].copy()
    if with_nan:
        x[70:80, 2] = np.nan                  # whole raw groups of single sensors: missing model ticks
        x[120:140, 4] = np.inf
        x[101, 0] = x[155, 6] = np.nan        # single raw readings: left out of their medians
    raw = torch.from_numpy(x).to(dev)
    series, _ = prep.series(raw)
    return prep, series[:, :w].contiguous(), raw[w * 10:].contiguous(), series[:, w:].t().contiguous()


def _assert_same_detector(a, b, n, w):
    from gdn_amd import ops
    assert torch.equal(a.state, b.state)
    for va, vb in zip(ops.stream_state_views(a.state, n, w), ops.stream_state_views(b.state, n, w)):
        assert torch.equal(va, vb)
    sa, sb = a.status(), b.status()
    assert sa[:2] == sb[:2] and torch.equal(sa[2], sb[2]) and torch.equal(sa[3], sb[3])
    assert torch.equal(_bits64(a.med_iqr), _bits64(b.med_iqr))


def _drive_both(det, plain, raw, prepared, pieces):
    """Hand `raw` to det in `pieces`, one sub-push at a time (harness.raw_push_plan), and the model ticks each
    completes to `plain`; every returned view and the prediction must be equal bit for bit."""
    from gdn_amd.harness import raw_push_plan
    at = done = 0
    for piece in pieces:
        for rows, groups, left, _ in raw_push_plan(det.raw_pending, piece, det.prep.down, det.chunk):
            got = det.push(raw[at:at + rows])
            at += rows
            assert det.raw_pending == left and all(v.shape[0] == groups for v in got)
            if groups:
                want = plain.push(prepared[done:done + groups])
                done += groups
                for g, wv in zip(got, want):
                    assert torch.equal(g, wv), (at, done)
                assert torch.equal(det.pred[:groups], plain.pred[:groups])
                assert torch.equal(_bits64(det.chunk_buf[:groups].double()), _bits64(plain.chunk_buf[:groups].double()))
    assert at == raw.shape[0]
    return done


def test_detector_on_raw_ticks_equals_a_plain_detector_on_the_prepared_series(gpu_device):
    dev = gpu_device
    n, w = TINY[:2]
    model = _model(dev, *TINY)
    prep, hist, raw, prepared = _stream_case(dev)
    s = torch.cat([hist, prepared.t()], dim=1).cpu()
    kw = dict(threshold=0.5, top_m=3, use_graph=False)
    det = _detector(model, s, w, 4, dev, prep=prep, **kw)
    plain = _detector(model, s, w, 4, dev, **kw)
    done = _drive_both(det, plain, raw, prepared, [1, 13, 40, 6, 40, 40, 27, 40])
    assert done == 20 and det.raw_pending == 7 and det.status()[4] == 7 and len(plain.status()) == 4
    _assert_same_detector(det, plain, n, w)
    # fp32 raw ticks from the host, one push split by the detector itself: the restatement's series, the same state
    det32 = _detector(model, s, w, 4, dev, prep=prep, **kw)
    x32 = raw.cpu().float()
    ts, ti, al = det32.push(x32)
    want32, _ = prep.series(torch.cat([torch.zeros((w * 10, n)), x32]).to(dev))
    plain32 = _detector(model, s, w, 4, dev, **kw)
    plain32.push(want32[:, w:].t().contiguous())
    assert det32.raw_pending == 7 and ts.shape[0] == det32._last
    _assert_same_detector(det32, plain32, n, w)
    with pytest.raises(TypeError, match="raw"):
        det32.push(raw.half())


def test_detector_graph_replay_of_aligned_raw_pushes_equals_eager(gpu_device):
    dev = gpu_device
    n, w = TINY[:2]
    model = _model(dev, *TINY)
    prep, hist, raw, prepared = _stream_case(dev)
    s = torch.cat([hist, prepared.t()], dim=1).cpu()
    det = _detector(model, s, w, 4, dev, prep=prep, threshold=0.5, top_m=3, use_graph=True)
    plain = _detector(model, s, w, 4, dev, threshold=0.5, top_m=3, use_graph=False)
    done = _drive_both(det, plain, raw, prepared, [40, 40, 40, 40, 40, 7])       # eager + capture, 4 replays, a tail
    assert done == 20 and list(det._prep_graphs) == [torch.float64] and det.raw_pending == 7
    _assert_same_detector(det, plain, n, w)
    # one long push from an open group: the first sub-push closes it (eager), the aligned ones after it replay
    det.push(raw[:3 + 40 + 40])
    plain.push(prep.series(torch.cat([raw[200:], raw[:83]]))[0].t().contiguous())
    assert det.raw_pending == 0
    _assert_same_detector(det, plain, n, w)


def test_a_parameter_change_drops_the_graph_of_the_raw_push(gpu_device):
    """tests/test_gpu_stream.py's test of the same name on a prep= detector pushed whole groups of float64 raw ticks:
    the graph held under that dtype is captured again, and the detector goes on bit for bit like a fresh one that was
    put at the same point of the stream."""
    dev = gpu_device
    n, w = TINY[:2]
    model = _model(dev, *TINY)
    prep, hist, raw, prepared = _stream_case(dev)
    s = torch.cat([hist, prepared.t()], dim=1).cpu()
    det = _detector(model, s, w, 4, dev, prep=prep, top_m=3)
    det.push(raw[:40])
    det.push(raw[40:80])
    before = det._prep_graphs[torch.float64]
    assert list(det._prep_graphs) == [torch.float64] and det.graph is None and det.raw_pending == 0
    with torch.no_grad():
        model.out_layer.mlp[0].bias.data.add_(0.5)
        model.embedding.weight.data[3].mul_(1.5)
    model.invalidate_constants()
    fresh = _detector(model, s, w, 4, dev, prep=prep, top_m=3)
    fresh.state.copy_(det.state)                                     # the same point of the same stream
    for t0 in (80, 120):                                             # the re-capturing push, then a replay
        a, b = det.push(raw[t0:t0 + 40]), fresh.push(raw[t0:t0 + 40])
        assert all(torch.equal(u, v) for u, v in zip(a, b)) and torch.equal(det.pred, fresh.pred)
        assert torch.equal(det.state, fresh.state)
    assert list(det._prep_graphs) == [torch.float64] and det._prep_graphs[torch.float64] is not before
    _assert_same_detector(det, fresh, n, w)
    out = torch.empty((4, n), device=dev)
    model.forward_into(det.x, out, wide=det.wide)
    assert torch.equal(det.pred, out)


def test_detector_with_gaps_takes_a_missing_raw_group_as_a_missing_reading(gpu_device):
    dev = gpu_device
    n, w = TINY[:2]
    model = _model(dev, *TINY)
    prep, hist, raw, prepared = _stream_case(dev, with_nan=True)
    assert torch.isnan(prepared).sum() == 3 and torch.isfinite(hist).all()
    s = torch.cat([hist, torch.nan_to_num(prepared.t())], dim=1).cpu()
    kw = dict(threshold=0.5, top_m=3, use_graph=False, gaps=True)
    det = _detector(model, s, w, 4, dev, prep=prep, **kw)
    plain = _detector(model, s, w, 4, dev, **kw)
    from gdn_amd.harness import raw_push_plan
    at = done = 0
    for piece in [1, 13, 40, 6, 40, 40, 27, 40]:
        for rows, groups, left, _ in raw_push_plan(det.raw_pending, piece, 10, 4):
            got = det.push(raw[at:at + rows])
            at += rows
            if groups:
                want = plain.push(prepared[done:done + groups])
                done += groups
                assert all(torch.equal(g, wv) for g, wv in zip(got, want))
                assert torch.equal(det.valid[:groups], plain.valid[:groups])
                assert torch.equal(det.chunk_buf[:groups], plain.chunk_buf[:groups])
    _assert_same_detector(det, plain, n, w)
    (ta, ra), (tb, rb) = det.status_gaps(), plain.status_gaps()
    assert torch.equal(ta, tb) and torch.equal(ra, rb) and int(ta.sum()) == 3


def test_detector_recalibrates_on_model_ticks(gpu_device):
    from gdn_amd import harness
    dev = gpu_device
    n, w = SERIES[:2]
    model = _model(dev, *SERIES)
    prep, hist, raw, prepared = _stream_case(dev)
    normal, _ = prep.series(torch.from_numpy(_gold()["train"]).to(dev))
    kw = dict(history=hist, top_m=3, use_graph=False, recal=64, recal_every=16, recal_min=16)
    det = harness.StreamDetector.from_calibration(model, normal, 4, prep=prep, **kw)
    plain = harness.StreamDetector.from_calibration(model, normal, 4, **kw)
    assert det.prep is prep and plain.prep is None
    _drive_both(det, plain, raw, prepared, [1, 13, 40, 6, 40, 40, 27, 40])
    assert det.recals == plain.recals == 1 and det.recal_kept == plain.recal_kept      # 20 model ticks cross 16 once
    assert torch.equal(det.ring_keys.view(torch.int64), plain.ring_keys.view(torch.int64))
    assert torch.equal(det.ring_keep, plain.ring_keep)
    _assert_same_detector(det, plain, n, w)


def test_a_detector_without_prep_writes_what_the_batch_path_writes(gpu_device):
    from gdn_amd import ops
    dev = gpu_device
    n, w = TINY[:2]
    model = _model(dev, *TINY)
    _prep, hist, _raw, prepared = _stream_case(dev)
    s = torch.cat([hist, prepared.t()], dim=1).cpu()
    det = _detector(model, s, w, 4, dev, threshold=0.5, top_m=3)
    assert det.prep is None and not hasattr(det, "_pend")
    outs = []
    for t0 in range(0, 20, 4):
        ts, ti, al = det.push(prepared[t0:t0 + 4])
        outs.append((det.pred[:4].clone(), ts.clone(), ti.clone(), al.clone()))
    pred, ts, ti, al = (torch.cat([o[j] for o in outs]) for j in range(4))
    x = s.to(dev).unfold(1, w, 1).permute(1, 0, 2).contiguous()[:20]
    want_pred = torch.empty((20, n), device=dev)
    model.forward_into(x, want_pred, wide=det.wide)
    want_s, want_i = ops.score_smooth_topm(pred, prepared, _table(n, dev), 3)
    assert torch.equal(pred, want_pred) and torch.equal(ts, want_s) and torch.equal(ti, want_i)
    assert torch.equal(al.bool(), want_s[:, 0] > 0.5) and det.graph is not None and len(det.status()) == 4


# ------------------------------------------------------------------------------------------------ command lines
def test_command_lines_prepare_the_files_and_replay_the_raw_one(gpu_device, tmp_path):
    import pandas as pd
    from test_gpu_forward_parity import random_params
    gold = _gold()
    n, w, k, d = SERIES
    names = [f"S{i:02d}" for i in range(n)]
    for name in ("train", "test"):
        df = pd.DataFrame(gold[name], columns=[" " + c for c in names])          # names to be stripped
        df.insert(0, "Timestamp", np.arange(len(df)))                            # a column to be dropped
        df["attack"] = gold[name + "_labels"]
        df.to_csv(tmp_path / f"raw_{name}.csv")
    ckpt = str(tmp_path / "ckpt.pt")
    torch.save(random_params(n, w, k, d, seed=n + w).state_dict(), ckpt)
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = tmp_path / "data" / "fix"
    subprocess.run([sys.executable, "-m", "gdn_amd.prep", "-train", str(tmp_path / "raw_train.csv"), "-test",
                    str(tmp_path / "raw_test.csv"), "-out", str(out), "-skip", "2", "-drop_cols", "1"],
                   check=True, timeout=300, env=env, cwd=str(tmp_path))
    assert open(out / "list.txt").read().split() == names
    train, test = pd.read_csv(out / "train.csv", index_col=0), pd.read_csv(out / "test.csv", index_col=0)
    assert list(train.columns) == names + ["attack"] and train.index[0] == 2
    assert np.array_equal(ref.bits32(train[names].to_numpy()), ref.bits32(gold["ref_train"][2:]))
    assert np.array_equal(ref.bits32(test[names].to_numpy()), ref.bits32(gold["ref_test"]))
    assert np.array_equal(test["attack"].to_numpy(), gold["ref_test_labels"])
    argv = ["-dataset", "fix", "-data_root", str(tmp_path / "data"), "-device", "cuda", "-batch", "8", "-slide_win", str(w),
            "-dim", str(d), "-slide_stride", "1", "-topk", str(k), "-val_ratio", "0.3", "-load_model_path", ckpt,
            "-stream", "4"]
    res = str(tmp_path / "res.npz")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_prep_cli_worker.py"), res] + argv + ["--"] + argv
                   + ["-stream_raw", str(tmp_path / "raw_test.csv"), "-prep", str(out / "prep.npz")],
                   check=True, timeout=300, env=env, cwd=str(tmp_path))
    with np.load(res) as z:
        plain = {key[2:]: z[key] for key in z.files if key.startswith("0/")}
        raw = {key[2:]: z[key] for key in z.files if key.startswith("1/")}
    assert set(raw) - set(plain) == {"raw_ticks", "raw_pending"} and set(plain) <= set(raw)
    assert int(raw["raw_ticks"]) == 257 - 10 * w and int(raw["raw_pending"]) == 7 and int(plain["ticks"]) == 25 - w
    for key in plain:
        assert np.array_equal(plain[key], raw[key]), key
