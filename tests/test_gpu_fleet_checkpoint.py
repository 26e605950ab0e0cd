"""GPU suite of a fleet's save / resume (harness.StreamFleet.state_dict / load_state_dict / save / load): a
fleet stream cut by a save and a load — in this process or across two others — writes the bits of the uninterrupted
one.  Every comparison is torch.equal on bit patterns: every push's outputs on the real rows, and everything the fleet
remembers at the end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _fleet_case import (CHUNK, DOWN, LOG, MSL, N, SHAPE, TOP_M, UNITS, assert_same_memory, gen, make_prep, memory, model_on,
                         raw_ticks, same, setup, tables)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# model ticks per push and unit (None: all); about 120 in all, cut after the seventh push
PUSHES = [(4, None), (3, [3, 1, 0]), (9, None), (4, [4, 0, 2]), (17, None), (4, None), (30, None),
          (2, [2, 2, 1]), (4, None), (25, None), (9, [9, 5, 0]), (12, None)]
# raw ticks per push under prep= (down = 4): at the cut the units hold 0, 1 and 2 raw ticks of an open group
RAW_PUSHES = [(16, None), (13, [13, 5, 0]), (37, None), (15, [15, 0, 6]), (70, None), (16, None), (121, None),
              (7, [7, 6, 3]), (16, None), (99, None), (38, [38, 21, 0]), (48, None)]
CUT = 7
CASES = {"plain": dict(), "gaps": dict(gaps=True), "recal": dict(recal=64, recal_every=48, recal_min=8),
         "gaps_recal_sensor": dict(gaps=True, recal=64, recal_every=48, recal_min=8, calib="sensor"),
         "events": dict(events=dict(on=2, off=3, cap=16)), "prep": dict(), "resume_eager": dict(recal=64, recal_min=8)}


class Case:
    """One configuration: the model, the fleet's construction and its pushes, the same in every process."""

    def __init__(self, name, dev):
        self.name, self.dev, self.kw = name, dev, CASES[name]
        shape = MSL if name == "gaps_recal_sensor" else SHAPE        # (that case is calibrated on a resident series)
        self.n = shape[0]
        self.model, self.med_iqr, self.threshold, self.history = setup(dev, seed=3, shape=shape)
        self.prep = make_prep(dev) if name == "prep" else None
        if name == "events":
            self.threshold = torch.tensor([1e-9, 1.0, 1.5], dtype=torch.float64)     # unit 0: an episode always open
        script = RAW_PUSHES if self.prep is not None else PUSHES
        g = gen(17)
        self.pushes = []
        for i, (r, counts) in enumerate(script):
            if self.prep is not None:
                ticks = raw_ticks(g, r, torch.float64, dev)
            else:
                ticks = torch.rand((UNITS, r, self.n), generator=g).to(dev)
            if self.kw.get("gaps") and CUT - 2 <= i <= CUT + 1:
                ticks[1, :, 7] = float("nan")                        # a sensor of unit 1 missing across the cut
                ticks[2, 0, 9] = float("inf")
            self.pushes.append((ticks, counts))
        self.before, self.after = self.pushes[:CUT], self.pushes[CUT:]

    def build(self, use_graph=True):
        from gdn_amd import harness
        if self.name == "gaps_recal_sensor":                         # calibrated: calib_kept / calib_counts exist
            series = torch.rand((UNITS, self.n, 150), generator=gen(19))
            series[0, 3, 40:44] = float("nan")
            return harness.StreamFleet.from_calibration(self.model, series.to(self.dev), CHUNK, calib_gaps=True,
                                                        min_kept=16, top_m=TOP_M, log=LOG, wide=False,
                                                        use_graph=use_graph, **self.kw)
        return harness.StreamFleet(self.model, self.med_iqr, self.threshold, self.history, CHUNK, top_m=TOP_M, log=LOG,
                                   wide=False, use_graph=use_graph, prep=self.prep, **self.kw)


def take(fleet, pushes):
    """Push them; per push the outputs on every unit's real rows of the last cut (clones)."""
    rec = []
    for ticks, counts in pushes:
        got = fleet.push(ticks, counts)
        real = fleet.counts.tolist()
        rec.append([[t[u, :real[u]].clone() for u in range(fleet.units)] for t in got])
    return rec


def final(fleet):
    out = memory(fleet)
    out["host_counters"] = torch.tensor([fleet._handed, fleet._raw_handed, fleet.recals], dtype=torch.int64)
    if fleet.calib_kept is not None:
        out["calib_kept"] = torch.as_tensor(fleet.calib_kept, dtype=torch.int64).clone()
    return out


def assert_same_pushes(a, b):
    assert len(a) == len(b)
    for i, (pa, pb) in enumerate(zip(a, b)):
        for fa, fb, what in zip(pa, pb, ("top_scores", "top_sensors", "alarm")):
            for u, (x, y) in enumerate(zip(fa, fb)):
                assert same(x, y), (i, what, u)


@pytest.mark.parametrize("name", list(CASES))
def test_a_fleet_cut_by_save_and_load_writes_the_bits_of_the_uninterrupted_one(name, gpu_device, tmp_path):
    from gdn_amd import harness, ops
    case = Case(name, gpu_device)
    whole = case.build()
    rec_whole = take(whole, case.before)
    at_cut = final(whole)
    sd_in_passing = whole.state_dict()                               # in passing: it changes nothing
    assert_same_memory(final(whole), at_cut)
    rec_whole += take(whole, case.after)
    want = final(whole)

    first = case.build()
    take(first, case.before)
    if name == "prep":                                               # the cut falls where the open groups differ
        assert ops.fleet_prep_views(first.pend, UNITS, N, DOWN)[1][:, 0].tolist() == [0, 1, 2]
    if name == "events":
        assert int(first.events[0, 1]) == 1                          # unit 0's episode is open across the cut
    if name.startswith("gaps"):
        assert int(first.status_gaps()[1][1, 7]) > 0                 # unit 1's sensor 7 is missing at the cut
    if "recal_every" in case.kw:
        assert first.recals >= 1
    path = str(tmp_path / "fleet.npz")
    first.save(path)
    assert os.listdir(tmp_path) == ["fleet.npz"]
    sd = harness.read_stream_checkpoint(path)
    assert sorted(sd) == sorted(sd_in_passing)
    assert all(sd[k].tobytes() == np.asarray(sd_in_passing[k]).tobytes() for k in sd)
    assert int(sd["format"]) == harness.FLEET_CHECKPOINT_FORMAT and int(sd["units"]) == UNITS
    if name == "gaps_recal_sensor":
        assert sd["calib_kept"].shape == (UNITS,) and sd["calib_counts"].shape == (UNITS, case.n)

    second = harness.StreamFleet.load(path, case.model, prep=case.prep, use_graph=name != "resume_eager")
    assert_same_memory(final(second), at_cut)
    rec_second = take(second, case.after)
    assert_same_pushes(rec_second, rec_whole[CUT:])
    assert_same_memory(final(second), want)
    if name == "resume_eager":
        assert second.graph is None
    elif name == "prep":
        assert list(second._prep_graphs) == [torch.float64] and second.graph is None
    else:
        assert second.graph is not None

    # load_state_dict into the same fleet rewinds it: the pointers stay, the graph is captured again
    take(first, case.after)
    state_ptr = first.state.data_ptr()
    first.load_state_dict(sd)
    assert first.state.data_ptr() == state_ptr and first.graph is None and first._prep_graphs == {}
    assert_same_memory(final(first), at_cut)
    assert_same_pushes(take(first, case.after), rec_whole[CUT:])
    assert_same_memory(final(first), want)


def test_load_refuses_by_name_before_any_device_write(gpu_device, tmp_path):
    from gdn_amd import harness
    from gdn_amd.prep import Prep
    case = Case("prep", gpu_device)
    fleet = case.build()
    take(fleet, case.before)
    before = final(fleet)
    path = str(tmp_path / "fleet.npz")
    fleet.save(path)
    with pytest.raises(ValueError, match="fleet checkpoint: prep"):
        harness.StreamFleet.load(path, case.model)
    with pytest.raises(ValueError, match="prep_down"):
        harness.StreamFleet.load(path, case.model, prep=Prep(case.prep.table, case.prep.stats, DOWN + 1))
    moved = model_on(gpu_device)
    with torch.no_grad():
        moved.gnn_layers[0].bn.running_mean[0] += 0.5
    with pytest.raises(ValueError, match="check_model"):
        harness.StreamFleet.load(path, moved, prep=case.prep)
    assert harness.StreamFleet.load(path, moved, prep=case.prep, check_model=False).status()[0].tolist() == \
        fleet.status()[0].tolist()
    sd = harness.read_stream_checkpoint(path)
    bad = dict(sd, pending=np.array([0, DOWN, 0], dtype=np.int32))
    with pytest.raises(ValueError, match="pending"):
        fleet.load_state_dict(bad)
    other = Case("plain", gpu_device).build()
    with pytest.raises(ValueError, match="prep"):
        other.load_state_dict(sd, check_model=False)
    with pytest.raises(ValueError, match="units"):
        harness.StreamFleet(case.model, tables(gpu_device, gen(1), units=2), 1.0, case.history[:2].contiguous(), CHUNK,
                            top_m=TOP_M, log=LOG, wide=False, prep=case.prep).load_state_dict(sd, check_model=False)
    assert_same_memory(final(fleet), before)                         # the refusals wrote nothing
    # the detector keeps refusing a fleet's file (by the foreign key), and the fleet a detector's (no `units`)
    with pytest.raises(ValueError, match="stream checkpoint: "):
        harness.StreamDetector.load(path, case.model, prep=case.prep)
    det = harness.StreamDetector(case.model, case.med_iqr[0], 1.0, case.history[0].contiguous(), CHUNK, top_m=TOP_M,
                                 log=LOG, wide=False)
    det_path = str(tmp_path / "det.npz")
    det.save(det_path)
    with pytest.raises(ValueError, match="fleet checkpoint: key 'units' is missing"):
        harness.StreamFleet.load(det_path, case.model)


def _child(args, limit=120):
    """One fresh process per GPU step, under its own time limit; a non-zero exit ends the test."""
    done = subprocess.run([sys.executable, os.path.join(HERE, "_fleet_checkpoint_worker.py")] + args, timeout=limit,
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]


def test_saved_in_one_process_and_resumed_in_another(gpu_device, tmp_path):
    name = "prep"
    case = Case(name, gpu_device)
    whole = case.build()
    rec = take(whole, case.pushes)
    want = final(whole)
    ckpt, out = str(tmp_path / "fleet.npz"), str(tmp_path / "resumed.npz")
    _child(["save", name, ckpt])
    assert os.path.exists(ckpt)
    _child(["resume", name, ckpt, out])
    with np.load(out, allow_pickle=False) as z:
        got = {k: torch.from_numpy(z[k]) for k in z.files}
    for i in range(len(case.after)):
        for j, field in enumerate(("top_scores", "top_sensors", "alarm")):
            for u in range(UNITS):
                assert same(got[f"push{i}/{field}/{u}"], rec[CUT + i][j][u].cpu()), (i, field, u)
    assert sorted(k[6:] for k in got if k.startswith("final/")) == sorted(want)
    for k, v in want.items():
        assert same(got["final/" + k], v.cpu()), k
