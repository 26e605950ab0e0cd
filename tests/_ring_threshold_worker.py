"""What tests/test_gpu_ring_threshold.py runs on both sides of a process boundary, and the child process itself:

    python tests/_ring_threshold_worker.py save   DET.npz FLEET.npz            part 0 of both streams, then save
    python tests/_ring_threshold_worker.py resume DET.npz FLEET.npz OUT.npz    load, part 1, the final memory

A StreamDetector and a StreamFleet of three units with a ring, episodes and recal_threshold; each part pushes ticks
(recal_every recalibrates on the way) and ends with an explicit recalibrate(), so there is a recalibration — table,
threshold and clear level — on each side of the cut.  The same seeds give the same model, tables and ticks in every
process.  The step runs under a time limit of its own."""
import faulthandler
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

LIMIT = 100          # seconds: a hung step ends this process (with a traceback), and with it the parent's test
UNITS, CHUNK = 3, 8
PARTS = ([8, 8, 5, 8], [8, 3, 8, 8, 8])


def build(kind, dev, recal_threshold=1.05, old_api=False):
    from _fleet_case import MSL, gen, model_on, tables
    from gdn_amd import harness
    n, w = MSL[:2]
    g = gen(11)
    kw = dict(top_m=2, log=8, wide=False, recal=64, recal_min=8, recal_every=24,
              events=dict(on=2, off=2, lo=2.0, cap=16))
    if not old_api:
        kw["recal_threshold"] = recal_threshold
    model = model_on(dev, MSL)
    if kind == "detector":
        return harness.StreamDetector(model, tables(dev, g, units=1, n=n)[0], 50.0,     # (never alarms at first)
                                      torch.rand((n, w + 2), generator=g).to(dev), CHUNK, **kw)
    return harness.StreamFleet(model, tables(dev, g, units=UNITS, n=n),
                               torch.tensor([4.0, 50.0, 60.0], dtype=torch.float64),
                               torch.rand((UNITS, n, w + 2), generator=g).to(dev), CHUNK, **kw)


def run(kind, obj, part, dev):
    """Part 0 | 1 of the stream: the pushes (part 1 at a higher level), then one recalibrate()."""
    from _fleet_case import gen
    g = gen(part, 23)
    for r in PARTS[part]:
        lead = () if kind == "detector" else (UNITS,)
        obj.push((torch.rand(lead + (r, obj.n), generator=g) + 0.3 * part).to(dev))
    obj.recalibrate()


def final(obj):
    names = ("state", "med_iqr", "threshold", "clear", "clear_frac", "ring_keys", "ring_keep", "events", "log_ticks",
             "log_sensors")
    return {k: getattr(obj, k).cpu().numpy() for k in names if getattr(obj, k, None) is not None}


def main():
    faulthandler.dump_traceback_later(LIMIT, exit=True)
    from gdn_amd import harness
    dev = torch.device("cuda:0")
    mode, paths = sys.argv[1], dict(zip(("detector", "fleet"), sys.argv[2:4]))
    if mode == "save":
        for kind, path in paths.items():
            obj = build(kind, dev)
            run(kind, obj, 0, dev)
            obj.save(path)
    elif mode == "resume":
        out = {}
        for kind, path in paths.items():
            obj = build(kind, dev)                                    # (for its model: the same seeds)
            cls = harness.StreamDetector if kind == "detector" else harness.StreamFleet
            loaded = cls.load(path, obj.model)
            assert loaded.recal_threshold == 1.05 and loaded.recals >= 1
            run(kind, loaded, 1, dev)
            out.update({f"{kind}/{k}": v for k, v in final(loaded).items()})
        np.savez(sys.argv[4], **out)
    else:
        raise SystemExit(f"unknown mode {mode!r}")
    torch.cuda.synchronize()
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()
