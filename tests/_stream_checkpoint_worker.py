"""Child process of tests/test_gpu_stream_checkpoint.py: one half of a stream that a process boundary cuts.

    python tests/_stream_checkpoint_worker.py save   CASE SETUP.npz CKPT         the pushes before the cut, then save
    python tests/_stream_checkpoint_worker.py resume CASE CKPT OUT.npz            load, the pushes after the cut

CASE names a configuration of the test module (the same seeds give the same model and ticks in every process);
SETUP.npz holds the parent's threshold and median / IQR table;
`resume` writes every push's top_scores / top_sensors / alarm / pred ("push<i>/...") and the detector's final memory
("final/...") for the parent to compare.  The step runs under a time limit of its own."""
import faulthandler
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

LIMIT = 100          # seconds: a hung step ends this process (with a traceback), and with it the parent's test


def main():
    faulthandler.dump_traceback_later(LIMIT, exit=True)
    from gdn_amd import harness
    from test_gpu_stream_checkpoint import Case, _final, _take
    mode, name = sys.argv[1], sys.argv[2]
    case = Case(name, torch.device("cuda:0"))
    if mode == "save":
        with np.load(sys.argv[3], allow_pickle=False) as z:
            det = case.build(float(z["threshold"]), med_iqr=torch.from_numpy(z["med_iqr"]).to(case.dev))
        _take(det, case.ticks, case.before)
        det.save(sys.argv[4])
    elif mode == "resume":
        det = harness.StreamDetector.load(sys.argv[3], case.model, prep=case.prep)
        rec = _take(det, case.ticks, case.after)
        out = {f"push{i}/{field}": r[j].cpu().numpy() for i, r in enumerate(rec)
               for j, field in enumerate(("top_scores", "top_sensors", "alarm", "pred"))}
        out.update({"final/" + k: v.cpu().numpy() for k, v in _final(det).items()})
        np.savez(sys.argv[4], **out)
    else:
        raise SystemExit(f"unknown mode {mode!r}")
    torch.cuda.synchronize()
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()
