"""Step time of harness.SeriesTrainer at the SWaT shape (n 127, w 15, k 30, d 64; 512-window captured steps) with
gaps=False, with gaps=True on a clean series and with gaps=True and about 1 % of the readings missing in bursts; the
one-off fill; the validation pass with and without the validity plane.  HIP events around `steps`
replays, the median of `rounds` such timings per configuration, the configurations interleaved.
python3 tools/probe_train_gaps.py [ticks] [steps] [rounds]"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gdn_amd import GDN, harness  # noqa: E402

t = int(sys.argv[1]) if len(sys.argv) > 1 else 47520
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 7
n, w, k, d, batch = 127, 15, 30, 64, 512
dev = torch.device("cuda:0")
clean = torch.rand((n, t), generator=torch.Generator().manual_seed(0)).to(dev)
gappy = clean.clone()
g = torch.Generator().manual_seed(1)
bursts = max(1, int(0.01 * n * (t - w) / 8))                        # bursts of 8 ticks on one sensor: ~1 % of the readings
for a, s in zip(torch.randint(w, t - 8, (bursts,), generator=g).tolist(), torch.randint(0, n, (bursts,), generator=g).tolist()):
    gappy[s, a:a + 8] = float("nan")
starts = torch.arange(w, t, 5)
starts = starts[: starts.numel() // batch * batch]
val = torch.arange(w, t, 5)[:4096]


def model():
    torch.manual_seed(0)
    return GDN([torch.zeros((2, 1), dtype=torch.long)], n, dim=d, input_dim=w, topk=k).to(dev)


def timed(fn, count):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(count):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / count


trainers = {"gaps=False": harness.SeriesTrainer(model(), clean, w, starts, batch),
            "gaps=True, clean": harness.SeriesTrainer(model(), clean, w, starts, batch, gaps=True),
            "gaps=True, 1% missing": harness.SeriesTrainer(model(), gappy, w, starts, batch, gaps=True)}
for tr in trainers.values():
    tr.epoch(torch.arange(batch * 4))                               # captures, then four replays
times = {name: [] for name in trainers}
for _ in range(rounds):
    for name, tr in trainers.items():
        # (the cursor is put back before every replay, so each one gathers the table's first windows: one memset
        # more per step, the same in all three)
        times[name].append(timed(lambda: (tr.cursor.zero_(), tr.step.step()), steps))
for name in trainers:
    print(f"step (with the cursor reset), {name}: median {statistics.median(times[name]):.1f} us (min {min(times[name]):.1f}, "
          f"max {max(times[name]):.1f}) over {rounds} x {steps} replays")
for _ in range(3):
    harness.fill_series(gappy, w)
fill = sorted(timed(lambda: harness.fill_series(gappy, w), 10) for _ in range(rounds))
print(f"fill_series (one host read, two launches and its allocations): median {fill[len(fill) // 2]:.1f} us "
      f"(min {fill[0]:.1f}, max {fill[-1]:.1f})")
held = trainers["gaps=True, 1% missing"]
net = model().eval()
passes = {"validate_series": lambda: harness.validate_series(net, held.series, val, batch, wide=False),
          "validate_series(valid=)": lambda: harness.validate_series(net, held.series, val, batch, wide=False, valid=held.valid)}
for fn in passes.values():
    fn()
vt = {name: [] for name in passes}
for _ in range(rounds):
    for name, fn in passes.items():
        vt[name].append(timed(fn, 5))
for name in passes:
    print(f"{name}, {val.numel()} windows: median {statistics.median(vt[name]):.1f} us (min {min(vt[name]):.1f}, "
          f"max {max(vt[name]):.1f})")
