"""Child process of tests/test_gpu_prep.py: runs `python -m gdn_amd.main`'s own entry (main.from_args(argv).run()) once
per argument list — the lists are separated by "--" — and saves every run's `stream_result` under the run's number.

    python tests/_prep_cli_worker.py OUT.npz <argv of run 0> -- <argv of run 1>"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from gdn_amd import main as cli
    out, rest = sys.argv[1], sys.argv[2:]
    runs, cur = [], []
    for a in rest:
        if a == "--":
            runs.append(cur)
            cur = []
        else:
            cur.append(a)
    runs.append(cur)
    saved = {}
    for i, argv in enumerate(runs):
        m = cli.from_args(argv)
        m.run()
        saved.update({f"{i}/{k}": np.asarray(v) for k, v in m.stream_result.items()})
    np.savez(out, **saved)


if __name__ == "__main__":
    main()
