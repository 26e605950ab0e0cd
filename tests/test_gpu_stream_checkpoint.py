"""GPU suite of the streaming detector's checkpoint: a stream cut by StreamDetector.save and .load
writes the bits of the uninterrupted stream.  Detector A takes every push, B the pushes up to tick 59 and is saved, C is
StreamDetector.load of B's file and takes the rest; every push's top_scores / top_sensors / alarm / pred and, at the
end, the state's bytes, the table, the threshold, the log, the counters, the gap counters and the ring are torch.equal.
n = 70 (two 64-sensor tiles, the second partial), w = 5, d = 16, k = 5; 160 ticks; chunk 8, top_m 3, a log of 8."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_gpu_stream import _model, _table

pytestmark = pytest.mark.gpu

N, W, K, D = 70, 5, 5, 16
T, CUT, CHUNK, TOP_M, LOG, DOWN = 160, 59, 8, 3, 8, 4
SIZES = (1, 2, 3, 5, 8, 9, 37)                      # then "the rest": tests/test_gpu_stream.py's cuts
RAW_SIZES = (1, 2, 3, 5, 8, 9, 37, 64, 32)          # raw ticks: 28 = 7 groups, so the 37 opens on a group boundary
ROLLING = dict(recal=64, recal_every=48, recal_min=16)
CASES = {
    "plain": {},
    "gaps": dict(gaps=True),
    "recal": dict(ROLLING),
    "gaps_recal_sensor": dict(gaps=True, calib="sensor", **ROLLING),
    "prep": dict(prep=True),
    "mlp_head": dict(layers=2),
    "eager_resume": dict(resume_graph=False),
}
HERE = os.path.dirname(os.path.abspath(__file__))


def _bits(t):
    return t.contiguous().view(torch.int64)


def _cuts(lo, hi, sizes):
    """[lo, hi) in pushes of `sizes`, the last one "the rest" (cut short where the sizes overrun)."""
    out, at = [], lo
    for s in sizes:
        if at + s >= hi:
            break
        out.append((at, at + s))
        at += s
    return out + [(at, hi)]


class Case:
    """One configuration: the model, the ticks (model ticks [160, n] fp32, or raw ticks [643, n] float64 under
    prep=), the pushes before and after the cut, and `build(threshold, use_graph)`."""

    def __init__(self, name, dev):
        from gdn_amd import Prep
        cfg = dict(CASES[name])
        self.name, self.dev = name, dev
        self.resume_graph = cfg.pop("resume_graph", True)
        layers = cfg.pop("layers", 1)
        self.model = _model(dev, N, W, K, D, layers, 32)
        g = torch.Generator().manual_seed(4242)
        self.history = torch.rand((N, W), generator=g).to(dev)
        ticks = torch.rand((T, N), generator=g)
        self.prep = None
        self.unit = 1
        if cfg.pop("prep", False):
            # raw = 5 + 10 * (the model tick + a wobble inside its group); the table maps [5, 15] back onto [0, 1]
            raw = 5.0 + 10.0 * ticks.double().repeat_interleave(DOWN, dim=0)
            raw = torch.cat([raw, raw[:3]]) + 0.05 * torch.rand((T * DOWN + 3, N), generator=g, dtype=torch.float64)
            table = torch.tensor([0.1, -0.5], dtype=torch.float64).repeat(N, 1).to(dev)
            stats = torch.tensor([5.0, 15.0, 10.0, 1000.0], dtype=torch.float64).repeat(N, 1).to(dev)
            self.prep = Prep(table, stats, DOWN)
            cfg["prep"] = self.prep
            ticks, self.unit = raw, DOWN
            cut = CUT * DOWN + 3                        # leaves raw_pending = 3
            self.before, self.after = _cuts(0, cut, RAW_SIZES), _cuts(cut, raw.shape[0], RAW_SIZES)
        else:
            self.before, self.after = _cuts(0, CUT, SIZES), _cuts(CUT, T, SIZES)
        if cfg.get("gaps"):
            ticks[torch.rand((T, N), generator=g) < 0.03] = float("nan")         # before and after the cut
            ticks[50:70, 7] = float("inf")                                          # one sensor missing ACROSS it
            if cfg.get("calib") == "sensor":
                ticks[:, 66] = float("nan")                                         # one sensor with no reading at all
        self.ticks = ticks.to(dev)
        self.cfg = cfg
        self.med_iqr = None

    def table(self):
        """The median / IQR of this stream's own errors (gdn_score_quantiles over the predictions and the held ticks
        of ONE run without a ring): a table the recalibrations resemble, so that the scores before and after one are
        of a kind and one threshold raises alarms on both sides of the cut."""
        from gdn_amd import harness, ops
        if self.med_iqr is None:
            cfg = {k: v for k, v in self.cfg.items() if k in ("gaps", "prep")}
            det = harness.StreamDetector(self.model, _table(N, self.dev), float("inf"), self.history, CHUNK,
                                         top_m=TOP_M, use_graph=False, **cfg)
            step, pred, gt = CHUNK * self.unit, [], []
            for s in range(0, self.ticks.shape[0], step):
                r = det.push(self.ticks[s:s + step])[2].shape[0]
                pred.append(det.pred[:r].clone())
                gt.append(det.chunk_buf[:r].clone())
            self.med_iqr = ops.score_quantiles(torch.cat(pred), torch.cat(gt))
            assert self.med_iqr.shape == (N, 2) and bool(torch.isfinite(self.med_iqr).all())
        return self.med_iqr

    def build(self, threshold, use_graph=True, med_iqr=None):
        from gdn_amd import harness
        det = harness.StreamDetector(self.model, self.table() if med_iqr is None else med_iqr, threshold, self.history,
                                     CHUNK, top_m=TOP_M, log=LOG, use_graph=use_graph, **self.cfg)
        if self.cfg.get("calib") == "sensor":           # what from_calibration(calib_gaps=True) leaves: carried over too
            det.calib_kept = 123
            det.calib_counts = torch.arange(N, dtype=torch.int32, device=self.dev) + 123
        return det

    def threshold(self):
        """Twelve or more of the 160 top scores above it, two to six of them before the cut: from ONE quiet run
        (threshold inf) of this configuration handed the pushes of the test, so that it recalibrates where they do."""
        quiet = self.build(float("inf"), use_graph=False)
        inner, tops = quiet._launch, []

        def spy(count, guard):                          # (eager: every sub-push is one _launch)
            inner(count, guard)
            tops.append(quiet.top_scores[:count, 0].clone())
        quiet._launch = spy
        for lo, hi in self.before + self.after:
            quiet.push(self.ticks[lo:hi])
        top = torch.cat(tops)
        assert top.shape[0] == T and bool(torch.isfinite(top).all())
        srt = top.sort(descending=True).values
        for k in range(12, 80):
            thr = float((srt[k - 1] + srt[k]) / 2)
            if 2 <= int((top[:CUT] > thr).sum()) <= 6:
                return thr
        raise AssertionError("no threshold leaves two to six alarms before the cut")


def _take(det, ticks, pushes):
    """One record per push, cloned as it returns: (top_scores, top_sensors, alarm, pred[:r])."""
    rec = []
    for lo, hi in pushes:
        ts, ti, al = det.push(ticks[lo:hi])
        rec.append((ts.clone(), ti.clone(), al.clone(), det.pred[:al.shape[0]].clone()))
    return rec


def _assert_records(got, want, what):
    assert len(got) == len(want)
    for i, (g, wv) in enumerate(zip(got, want)):
        for j, name in enumerate(("top_scores", "top_sensors", "alarm", "pred")):
            assert g[j].shape == wv[j].shape and torch.equal(g[j], wv[j]), (what, "push", i, name)


def _final(det):
    """Everything a continuation left behind, on the host, bit patterns where a NaN may sit."""
    ticks, alarms, log_ticks, log_sensors = det.status()[:4]
    out = {"state": det.state.cpu(), "med_iqr": _bits(det.med_iqr).cpu(), "threshold": _bits(det.threshold).cpu(),
           "ticks": torch.tensor(ticks), "alarms": torch.tensor(alarms), "status_log_ticks": log_ticks.cpu(),
           "status_log_sensors": log_sensors.cpu(), "log_ticks": det.log_ticks.cpu(), "log_sensors": det.log_sensors.cpu(),
           "handed": torch.tensor(det._handed), "raw_pending": torch.tensor(det.raw_pending),
           "recals": torch.tensor(det.recals), "recal_kept": torch.tensor(det.recal_kept),
           "calib_kept": torch.tensor(-1 if det.calib_kept is None else det.calib_kept)}
    if det.with_gaps:
        out["missing_total"], out["missing_run"] = det.status_gaps()
    if det.recal:
        out["ring_keys"], out["ring_keep"] = _bits(det.ring_keys).cpu(), det.ring_keep.cpu()
    if det.recal_counts is not None:
        out["recal_counts"] = det.recal_counts
    if det.calib_counts is not None:
        out["calib_counts"] = det.calib_counts.cpu()
    if det.prep is not None:
        out["pending"] = _bits(det._pend[det._pend_at][:det.raw_pending]).cpu()
    return out


def _assert_final(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), (what, k)


def _shapes_of_an_empty_localisation(det):
    return [tuple(f.shape) for f in det.localise()]


@functools.lru_cache(maxsize=None)
def _uninterrupted(name):
    """(the case, its threshold, A's records of every push, A's final state): computed once per configuration."""
    case = Case(name, torch.device("cuda:0"))
    thr = case.threshold()
    a = case.build(thr)
    rec = _take(a, case.ticks, case.before + case.after)
    return case, thr, rec, _final(a)


@pytest.mark.parametrize("name", list(CASES))
def test_a_stream_cut_by_save_and_load_writes_the_bits_of_the_uninterrupted_one(name, gpu_device, tmp_path):
    from gdn_amd import harness
    case, thr, rec_a, final_a = _uninterrupted(name)
    assert int(final_a["ticks"]) == T and int(final_a["alarms"]) > LOG       # a log that is not restored cannot pass
    assert final_a["status_log_ticks"].shape[0] == LOG
    fresh = case.build(thr)
    b = case.build(thr)
    rec_b = _take(b, case.ticks, case.before)
    at_cut = _final(b)
    assert int(at_cut["ticks"]) == CUT and 1 <= int(at_cut["alarms"])
    assert int(at_cut["status_log_ticks"][0]) < CUT <= int(final_a["status_log_ticks"][-1])   # entries of both sides
    if case.prep is not None:
        assert b.raw_pending == 3 and at_cut["pending"].shape == (3, N)
    if b.with_gaps:
        assert int(at_cut["missing_run"][7]) == CUT - 50 and int(final_a["missing_total"][7]) >= 20
    if b.recal:
        assert b.recals == 1 and int(final_a["recals"]) == 3                   # handed ticks 48 | 96, 144
        assert not torch.equal(_bits(b.med_iqr), _bits(fresh.med_iqr))        # the saved table is not the constructor's
        if b.calib == "sensor":
            assert int(at_cut["recal_counts"][66]) == 0 and torch.equal(b.med_iqr[66], fresh.med_iqr[66])
    path = str(tmp_path / "det.npz")
    b.save(path)
    assert sorted(os.listdir(tmp_path)) == ["det.npz"]
    sd = harness.read_stream_checkpoint(path)               # allow_pickle=False: no Python objects
    assert all(isinstance(v, np.ndarray) and v.dtype != object for v in sd.values())
    assert sd["state"].dtype == np.uint8 and sd["state"].tobytes() == b.state.cpu().numpy().tobytes()
    assert not any(k in sd for k in ("chunk_buf", "raw_buf", "x", "pred", "top_scores", "alarm", "valid", "gap_chunk"))
    c = harness.StreamDetector.load(path, case.model, prep=case.prep, device="cuda", use_graph=case.resume_graph)
    # the loaded detector: B's memory in allocations of its own, nothing pushed yet, no graph
    _assert_final(_final(c), at_cut, (name, "loaded"))
    assert c.state.data_ptr() != b.state.data_ptr() and c._last == 0 and c.graph is None
    assert c._config() == b._config() and c.use_graph == case.resume_graph
    if c.with_gaps:
        assert c.valid[:c._last].shape == (0, N)
    assert _shapes_of_an_empty_localisation(c) == _shapes_of_an_empty_localisation(fresh)
    ptrs = (c.state.data_ptr(), c.med_iqr.data_ptr(), c.threshold.data_ptr())
    rec_c = _take(c, case.ticks, case.after)
    assert ptrs == (c.state.data_ptr(), c.med_iqr.data_ptr(), c.threshold.data_ptr())
    assert (c.graph is not None or bool(c.prep is not None and c._prep_graphs)) == case.resume_graph
    _assert_records(rec_b + rec_c, rec_a, name)
    _assert_final(_final(c), final_a, (name, "final"))


def test_state_dict_is_read_only_and_load_state_dict_rewinds_in_place(gpu_device):
    """state_dict() in the middle of a stream leaves the pushes after it as they were; loading that dict into the SAME
    detector later takes it back to that tick, and the pushes repeat bit for bit (graph dropped and captured again)."""
    from gdn_amd import harness
    case, thr, rec_a, final_a = _uninterrupted("gaps_recal_sensor")
    d = case.build(thr)
    rec_before = _take(d, case.ticks, case.before)
    sd = d.state_dict()
    assert all(isinstance(v, np.ndarray) for v in sd.values())
    harness.stream_checkpoint_check(sd, d._expect())
    kept = {k: v.copy() for k, v in sd.items()}
    rec_after = _take(d, case.ticks, case.after)
    _assert_records(rec_before + rec_after, rec_a, "saved in passing")
    _assert_final(_final(d), final_a, "saved in passing")
    assert all(sd[k].tobytes() == kept[k].tobytes() for k in kept)          # the dict does not alias live memory
    assert d.graph is not None
    d.load_state_dict(sd)
    assert d.graph is None and d._last == 0 and d.status()[0] == CUT
    _assert_records(_take(d, case.ticks, case.after), rec_after, "rewound")
    _assert_final(_final(d), final_a, "rewound")


def test_load_refuses_other_weights_another_prep_and_a_damaged_file_by_name(gpu_device, tmp_path):
    from gdn_amd import Prep, harness
    case, thr, _rec, _final_a = _uninterrupted("prep")
    b = case.build(thr)
    _take(b, case.ticks, case.before)
    path = str(tmp_path / "det.npz")
    b.save(path)
    with pytest.raises(ValueError, match="prep"):
        harness.StreamDetector.load(path, case.model)
    other = Prep(case.prep.table, case.prep.stats, DOWN + 1)
    with pytest.raises(ValueError, match="prep_down"):
        harness.StreamDetector.load(path, case.model, prep=other)
    with pytest.raises(ValueError, match="w = "):
        harness.StreamDetector.load(path, _model(gpu_device, N, W + 1, K, D), prep=case.prep)
    moved = _model(gpu_device, N, W, K, D)
    with torch.no_grad():
        moved.gnn_layers[0].bn.running_mean[0] += 0.5
    with pytest.raises(ValueError, match="check_model"):
        harness.StreamDetector.load(path, moved, prep=case.prep)
    assert harness.StreamDetector.load(path, moved, prep=case.prep, check_model=False).status()[0] == CUT
    sd = harness.read_stream_checkpoint(path)
    del sd["pending"]
    damaged = str(tmp_path / "damaged.npz")
    harness.write_stream_checkpoint(damaged, sd)
    with pytest.raises(ValueError, match="pending"):
        harness.StreamDetector.load(damaged, case.model, prep=case.prep)
    plain = Case("plain", gpu_device).build(thr)
    with pytest.raises(ValueError, match="prep"):
        plain.load_state_dict(harness.read_stream_checkpoint(path), check_model=False)


def _child(args, limit=120):
    """One fresh process per GPU step, under its own time limit; a non-zero exit ends the test."""
    done = subprocess.run([sys.executable, os.path.join(HERE, "_stream_checkpoint_worker.py")] + args, timeout=limit,
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]


def test_saved_in_one_process_and_resumed_in_another(gpu_device, tmp_path):
    name = "gaps_recal_sensor"
    case, thr, rec_a, final_a = _uninterrupted(name)
    ckpt, out, setup = str(tmp_path / "det.npz"), str(tmp_path / "resumed.npz"), str(tmp_path / "setup.npz")
    np.savez(setup, threshold=np.float64(thr), med_iqr=case.table().cpu().numpy())
    _child(["save", name, setup, ckpt])
    assert os.path.exists(ckpt)
    _child(["resume", name, ckpt, out])
    with np.load(out, allow_pickle=False) as z:
        got = {k: torch.from_numpy(z[k]) for k in z.files}
    first = len(case.before)
    for i in range(len(case.after)):
        for j, field in enumerate(("top_scores", "top_sensors", "alarm", "pred")):
            assert torch.equal(got[f"push{i}/{field}"], rec_a[first + i][j].cpu()), (i, field)
    for k, want in final_a.items():
        assert got["final/" + k].dtype == want.dtype and torch.equal(got["final/" + k], want), k


def test_command_line_saves_the_detector_and_a_resumed_run_goes_on_where_it_stopped(gpu_device, tmp_path, capsys):
    """-stream_save after a full replay, then -stream_resume of that file: the test series is used up, so the resumed
    run pushes nothing and reports the saved detector's counters and log, and the tick it resumed from."""
    from conftest import load_golden
    from gdn_amd import harness, main as cli
    from test_gpu_localise import _write_cli_dataset
    data, p = load_golden("cli_msl_slice")
    batch, w, dim, stride, topk, seed, inter = (int(v) for v in data["meta_cfg"])
    root = str(tmp_path / "data")
    _write_cli_dataset(data, root)
    weights, ckpt = str(tmp_path / "ckpt.pt"), str(tmp_path / "det.npz")
    torch.save(p, weights)
    argv = ["-dataset", "msl", "-data_root", root, "-device", "cuda", "-batch", str(batch), "-slide_win", str(w),
            "-dim", str(dim), "-slide_stride", str(stride), "-topk", str(topk), "-random_seed", str(seed),
            "-out_layer_inter_dim", str(inter), "-val_ratio", str(float(data["val_ratio"])), "-report", "best",
            "-load_model_path", weights, "-stream", "16"]
    first = cli.from_args(argv + ["-stream_save", ckpt])
    first.run()
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("stream:")]
    assert len(line) == 1 and "resumed" not in line[0] and "resumed_from" not in first.stream_result
    n_test = first.test_series.shape[1] - w
    sd = harness.read_stream_checkpoint(ckpt)
    assert int(sd["handed"]) == n_test == first.stream_result["ticks"] and int(sd["chunk"]) == 16
    again = cli.from_args(argv + ["-stream_resume", ckpt])
    again.run()
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("stream:")]
    assert len(line) == 1 and f"resumed at tick {n_test}" in line[0]
    res = again.stream_result
    assert res["resumed_from"] == n_test and res["ticks"] == n_test
    for k in ("alarms", "threshold"):
        assert res[k] == first.stream_result[k], k
    for k in ("log_ticks", "log_sensors"):
        np.testing.assert_array_equal(res[k], first.stream_result[k])
