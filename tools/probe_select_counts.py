"""Cost of per-sensor ranks in the select: gdn_score_select_counts with every count = the row length
against gdn_score_select(total = the row length) on the same keys.  HIP events, the two symbols alternated in one
process, five rounds of `reps` launches each, the best round per symbol.  Prints one line per shape."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdn_amd import ops  # noqa: E402


def timed(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps


def main(reps=20):
    dev = torch.device("cuda:0")
    for n, pitch in ((127, 32768), (16, 262144)):
        g = torch.Generator().manual_seed(n)
        pred, gt = torch.rand((pitch, n), generator=g).to(dev), torch.rand((pitch, n), generator=g).to(dev)
        keys = ops.score_keys(pred, gt, pitch)
        ws = ops.score_select_workspace(1, n, pitch, dev)
        counts = torch.full((n,), pitch, dtype=torch.int32, device=dev)
        a, b = torch.empty((n, 2), dtype=torch.float64, device=dev), torch.empty((n, 2), dtype=torch.float64, device=dev)
        plain = lambda: ops.score_select(keys, 1, n, pitch, pitch, ws, out=a)              # noqa: E731
        per_sensor = lambda: ops.score_select_counts(keys, 1, n, pitch, counts, 1, ws, out=b)   # noqa: E731
        plain(), per_sensor()
        torch.cuda.synchronize()
        assert torch.equal(a, b)
        rounds = [(timed(plain, reps), timed(per_sensor, reps)) for _ in range(5)]
        print(f"select n={n} pitch={pitch}: gdn_score_select best {min(r[0] for r in rounds):.1f} us (rounds "
              f"{' '.join(f'{r[0]:.1f}' for r in rounds)}); gdn_score_select_counts best "
              f"{min(r[1] for r in rounds):.1f} us (rounds {' '.join(f'{r[1]:.1f}' for r in rounds)})", flush=True)


if __name__ == "__main__":
    main()
