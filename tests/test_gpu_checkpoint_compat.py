"""GPU suite of checkpoint compatibility: a checkpoint written by an earlier commit resumes bit for bit.
tests/golden/checkpoint_compat_<kind>_<calib>.npz hold, for a StreamDetector and a StreamFleet under tick and under
sensor calibration, the model's weights, a checkpoint saved in the middle of a stream (the log wrapped, a raw group open,
an episode open, one recalibrate() behind it), the raw ticks pushed after it, what those pushes returned and the final
state_dict() — all recorded by the commit named in the file's `written_by`.  The test loads the checkpoint, pushes the
same ticks and compares every output and every key by dtype, shape and bytes.

The recording is this module run as a program on the GPU, `python tests/test_gpu_checkpoint_compat.py OUT_DIR COMMIT`:
it uses the public API only, so the same code records at one commit and checks at a later one."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
KINDS, CALIBS = ("detector", "fleet"), ("tick", "sensor")
N, W, CHUNK, TOP_M, LOG, UNITS, DOWN, RECAL, CAP, MARGIN = 70, 5, 4, 2, 6, 3, 4, 64, 8, 1.5
# raw ticks per push after the save: the open group (2 raw ticks) is closed, one full chunk on a group boundary (the
# captured graph), a short push that leaves a group open; the fleet then takes a push in which unit 1 is silent
AFTER = [(2, None), (CHUNK * DOWN, None), (5, None), (6, [6, 0, 3])]
OPEN = 2                                 # raw ticks of the open group at the save


def _model(dev, weights=None):
    from _fleet_case import model_on
    model = model_on(dev)
    if weights is not None:
        model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in weights.items()})
    return model.eval()


def _raw(g, r, lead, spike=0.0):
    """Raw float64 ticks lead + [r, n] in engineering units (sensor i reads 50 + 10 i .. 150 + 10 i), `spike` added."""
    base = 50.0 + 10.0 * torch.arange(N, dtype=torch.float64)
    return torch.rand(lead + (r, N), generator=g, dtype=torch.float64) * 100.0 + base + spike


def _start(kind, calib, dev, model):
    """A running detector or fleet at the point of the save."""
    from _fleet_case import gen, make_prep, setup
    from gdn_amd import harness
    _, med_iqr, _, history = setup(dev)
    kw = dict(top_m=TOP_M, log=LOG, wide=False, gaps=True, recal=RECAL, recal_min=8, exclude_alarms=False, calib=calib,
              events=dict(on=2, off=2, cap=CAP), prep=make_prep(dev), recal_threshold=MARGIN)
    fleet = kind == "fleet"
    if fleet:
        obj = harness.StreamFleet(model, med_iqr, torch.full((UNITS,), 0.05, dtype=torch.float64), history, CHUNK, **kw)
    else:
        obj = harness.StreamDetector(model, med_iqr[0], 0.05, history[0].contiguous(), CHUNK, **kw)
    lead = (UNITS,) if fleet else ()
    g = gen(77)
    calm = _raw(g, 20 * DOWN, lead)                          # 20 model ticks, every one an alarm: the log wraps
    calm[..., 1 * DOWN:3 * DOWN, 3] = float("nan")           # model ticks 1 and 2: sensor 3 has no reading at all
    calm[..., 41, 7] = float("inf")                          # one missing raw reading inside a group
    for s, e in ((0, 16), (16, 23), (23, 48), (48, 80)):     # a full chunk, a short push, a split one, two full chunks
        obj.push(calm[..., s:e, :].contiguous().to(dev))
    obj.recalibrate()                                        # the table and (recal_threshold=) the threshold move
    obj.push(_raw(g, 5 * DOWN + OPEN, lead, spike=300.0).to(dev))    # far off: an episode opens; a raw group stays open
    return obj


def _push(obj, ticks, counts, dev):
    """One push; the returned views as host arrays, a fleet's rows at or beyond counts[u] (unspecified) zeroed."""
    if counts is None:
        out = obj.push(ticks.to(dev))
    else:
        out = obj.push(ticks.to(dev), counts)
    out = [t.detach().cpu().clone() for t in out]
    if hasattr(obj, "units"):
        real = obj.counts.cpu().tolist()
        for t in out:
            for u, c in enumerate(real):
                t[u, max(int(c), 0):] = 0
    return dict(zip(("top_scores", "top_sensors", "alarm"), (t.numpy() for t in out)))


def _after(kind, obj, ticks, dev, tmp_dir):
    """The pushes after the save and what is compared: {name: array}."""
    from gdn_amd import harness
    got = {}
    for i, (r, counts) in enumerate(AFTER if kind == "fleet" else AFTER[:3]):
        for k, v in _push(obj, ticks[i], counts, dev).items():
            got[f"out/{i}/{k}"] = v
    got.update({"final/" + k: np.asarray(v) for k, v in obj.state_dict().items()})
    if kind == "fleet":                                      # unit 1 leaves as a detector and comes back
        unit = obj.unit_state_dict(1)
        got.update({"unit/" + k: np.asarray(v) for k, v in unit.items()})
        path = os.path.join(tmp_dir, "unit.npz")
        harness.write_stream_checkpoint(path, unit)
        det = harness.StreamDetector.load(path, obj.model, prep=obj.unit_prep(1), device=dev)
        back = det.state_dict()
        got.update({"unit_detector/" + k: np.asarray(v) for k, v in back.items()})
        obj.load_unit(1, back)
        got.update({"adopted/" + k: np.asarray(v) for k, v in obj.state_dict().items()})
    return got


def _open_episodes(kind, obj):
    words = obj.events[:, :2] if kind == "fleet" else obj.events[None, :2]
    return words.cpu().tolist()


def _record(out_dir, commit):
    from _fleet_case import gen
    dev = torch.device("cuda:0")
    os.makedirs(out_dir, exist_ok=True)
    for kind in KINDS:
        for calib in CALIBS:
            model = _model(dev)
            obj = _start(kind, calib, dev, model)
            path = os.path.join(out_dir, f"checkpoint_compat_{kind}_{calib}.ckpt")
            obj.save(path)
            ckpt = dict(np.load(path, allow_pickle=False))
            print(kind, calib, "status", [t.tolist() if torch.is_tensor(t) else t for t in obj.status()[:3]],
                  "episodes (raised, open)", _open_episodes(kind, obj), "recals", obj.recals,
                  "threshold", obj.threshold.cpu().tolist(), "eligible", obj.ring_eligible.cpu().tolist(), flush=True)
            assert obj.recals == 1 and all(is_open for _, is_open in _open_episodes(kind, obj))
            assert int(np.min(ckpt["raw_pending" if kind == "detector" else "pending"])) == OPEN
            assert torch.isfinite(obj.threshold).all() and (obj.threshold.cpu() != 0.05).all()      # re-derived
            lead = (UNITS,) if kind == "fleet" else ()
            g = gen(78)
            ticks = [_raw(g, r, lead, spike=0.0 if i else 300.0) for i, (r, _) in enumerate(AFTER)]
            ticks[1][..., 3, 11] = float("nan")
            del obj
            from gdn_amd import harness
            cls = harness.StreamFleet if kind == "fleet" else harness.StreamDetector
            from _fleet_case import make_prep
            obj = cls.load(path, model, prep=make_prep(dev), device=dev)
            fix = {"written_by": np.array(commit)}
            fix.update({"model/" + k: v.detach().cpu().numpy() for k, v in model.state_dict().items()})
            fix.update({"ckpt/" + k: v for k, v in ckpt.items()})
            fix.update({f"ticks/{i}": t.numpy() for i, t in enumerate(ticks)})
            fix.update(_after(kind, obj, ticks, dev, out_dir))
            np.savez_compressed(os.path.join(out_dir, f"checkpoint_compat_{kind}_{calib}.npz"), **fix)
            os.unlink(path)
            if kind == "fleet":
                os.unlink(os.path.join(out_dir, "unit.npz"))
            print(kind, calib, "recorded", len(fix), "arrays", flush=True)


def _fixture(kind, calib):
    with np.load(os.path.join(GOLDEN, f"checkpoint_compat_{kind}_{calib}.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _group(fix, prefix):
    return {k[len(prefix):]: v for k, v in fix.items() if k.startswith(prefix)}


@pytest.mark.gpu
@pytest.mark.parametrize("calib", CALIBS)
@pytest.mark.parametrize("kind", KINDS)
def test_a_checkpoint_written_by_an_earlier_commit_resumes_bit_for_bit(kind, calib, gpu_device, tmp_path):
    from _fleet_case import make_prep
    from gdn_amd import harness
    dev = gpu_device
    fix = _fixture(kind, calib)
    assert len(str(fix["written_by"])) == 40                 # the commit that recorded it
    ckpt = _group(fix, "ckpt/")
    assert int(ckpt["recals"]) == 1 and int(ckpt["log"]) == LOG and int(ckpt["recal"]) == RECAL
    assert int(np.min(ckpt["raw_pending" if kind == "detector" else "pending"])) == OPEN
    model = _model(dev, _group(fix, "model/"))
    path = str(tmp_path / "parent.ckpt")
    np.savez(path + ".npz", **ckpt)                          # the file as the earlier commit's numpy.savez wrote it
    os.replace(path + ".npz", path)
    cls = harness.StreamFleet if kind == "fleet" else harness.StreamDetector
    obj = cls.load(path, model, prep=make_prep(dev), device=dev)
    ticks = [torch.from_numpy(fix[f"ticks/{i}"]) for i in range(len(AFTER))]
    got = _after(kind, obj, ticks, dev, str(tmp_path))
    want = {k: v for k, v in fix.items() if k.split("/")[0] in ("out", "final", "unit", "unit_detector", "adopted")}
    assert sorted(got) == sorted(want)
    for k, a in want.items():
        b = got[k]
        assert b.dtype == a.dtype and b.shape == a.shape, (k, b.dtype, b.shape, a.dtype, a.shape)
        assert b.tobytes() == a.tobytes(), k
    assert len(_group(want, "final/")) > 30 and any(k.startswith("out/2/") for k in want)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    _record(sys.argv[1], sys.argv[2])
