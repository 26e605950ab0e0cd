"""Step time of harness.SeriesEvaluator at the SWaT shape (n 127, w 15, k 30, d 64; 32768 scored ticks) with
gaps=False, with gaps=True on clean data and with gaps=True and about 1 % of the readings missing in bursts, plus the
one-off cost of gdn_series_fill.  Captured steps, HIP events around `steps` replays, the median of
`rounds` such timings per configuration, the configurations interleaved.
python3 tools/probe_series_gaps.py [ticks] [steps] [rounds]"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gdn_amd import GDN, harness, ops  # noqa: E402

t = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 7
n, w, k, d = 127, 15, 30, 64
dev = torch.device("cuda:0")
torch.manual_seed(0)
model = GDN([torch.zeros((2, 1), dtype=torch.long)], n, dim=d, input_dim=w, topk=k).to(dev).eval()
clean = torch.rand((n, w + t), device=dev)
gappy = clean.clone()
g = torch.Generator().manual_seed(1)
bursts = max(1, int(0.01 * n * t / 8))                              # bursts of 8 ticks on one sensor: ~1 % of the readings
at = torch.randint(w, w + t - 8, (bursts,), generator=g)
on = torch.randint(0, n, (bursts,), generator=g)
for a, s in zip(at.tolist(), on.tolist()):
    gappy[s, a:a + 8] = float("nan")
missing = float((~torch.isfinite(gappy[:, w:])).float().mean())


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


evs = {"gaps=False": harness.SeriesEvaluator(model, None, clean[:, w:].t().contiguous(), 512, series=clean, coalesce=64),
       "gaps=True, clean": harness.SeriesEvaluator(model, None, None, 512, series=clean, coalesce=64, gaps=True),
       "gaps=True, 1% missing": harness.SeriesEvaluator(model, None, None, 512, series=gappy, coalesce=64, gaps=True)}
for ev in evs.values():
    for _ in range(10):
        ev.step()
torch.cuda.synchronize()
times = {name: [] for name in evs}
for _ in range(rounds):
    for name, ev in evs.items():
        times[name].append(timed(ev.step))
for name, ev in evs.items():
    kept = "" if ev.kept is None else f"; kept {ev.kept} of {ev.t} ticks"
    print(f"step, {name}: median {statistics.median(times[name]):.1f} us (min {min(times[name]):.1f}, "
          f"max {max(times[name]):.1f}) over {rounds} x {steps} replays{kept}")
for _ in range(3):
    ops.series_fill(gappy, w)
fill = sorted(timed(lambda: ops.series_fill(gappy, w)) for _ in range(rounds))
print(f"gdn_series_fill (two launches and its allocations), {missing:.2%} missing: median {fill[len(fill) // 2]:.1f} us "
      f"(min {fill[0]:.1f}, max {fill[-1]:.1f})")
