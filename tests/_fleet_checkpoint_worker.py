"""Child process of tests/test_gpu_fleet_checkpoint.py: one half of a fleet stream that a process boundary cuts.

    python tests/_fleet_checkpoint_worker.py save   CASE CKPT             the pushes before the cut, then save
    python tests/_fleet_checkpoint_worker.py resume CASE CKPT OUT.npz     load, the pushes after the cut

CASE names a configuration of the test module (the same seeds give the same model, tables and ticks in every process);
`resume` writes every push's top_scores / top_sensors / alarm on each unit's real rows ("push<i>/<field>/<unit>") and
the fleet's final memory ("final/...") for the parent to compare.  The step runs under a time limit of its own."""
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
    from test_gpu_fleet_checkpoint import Case, final, take
    mode, name = sys.argv[1], sys.argv[2]
    case = Case(name, torch.device("cuda:0"))
    if mode == "save":
        fleet = case.build()
        take(fleet, case.before)
        fleet.save(sys.argv[3])
    elif mode == "resume":
        fleet = harness.StreamFleet.load(sys.argv[3], case.model, prep=case.prep)
        rec = take(fleet, case.after)
        out = {f"push{i}/{field}/{u}": r[j][u].cpu().numpy() for i, r in enumerate(rec)
               for j, field in enumerate(("top_scores", "top_sensors", "alarm")) for u in range(fleet.units)}
        out.update({"final/" + k: v.cpu().numpy() for k, v in final(fleet).items()})
        np.savez(sys.argv[4], **out)
    else:
        raise SystemExit(f"unknown mode {mode!r}")
    torch.cuda.synchronize()
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()
