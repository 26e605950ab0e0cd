"""Step time of harness.FleetEvaluator at the SWaT shape (n 127, w 15, k 30, d 64) with t scored ticks per unit and
U units, against U SeriesEvaluator(use_graph=True) steps replayed in a loop, plus construction + first step against
StreamFleet.from_calibration on the same data.  Host clock around `steps` calls that end in a device
synchronise (the loop of U replays is host work too), the median of `rounds` such timings, the configurations
interleaved.
python3 tools/probe_fleet_series.py [ticks] [steps] [rounds] [units ...]"""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gdn_amd import GDN, harness  # noqa: E402

t = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
fleets = [int(a) for a in sys.argv[4:]] or [16, 64, 256]
n, w, k, d, batch = 127, 15, 30, 64, 512
dev = torch.device("cuda:0")
torch.manual_seed(0)
model = GDN([torch.zeros((2, 1), dtype=torch.long)], n, dim=d, input_dim=w, topk=k).to(dev).eval()


def wall(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def line(name, ts):
    print(f"  {name}: median {statistics.median(ts):.3f} ms (min {min(ts):.3f}, max {max(ts):.3f}) over {len(ts)} x "
          f"{steps} steps", flush=True)


for units in fleets:
    print(f"U = {units}, t = {t}, n = {n}, batch = {batch}", flush=True)
    g = torch.Generator().manual_seed(units)
    clean = torch.rand((units, n, w + t), generator=g)
    gappy = clean.clone()
    hit = torch.rand(gappy.shape, generator=g) < 0.01
    hit[:, :, :w] = False
    gappy[hit] = float("nan")
    clean, gappy = clean.to(dev), gappy.to(dev)
    build = {}
    build["FleetEvaluator + first step"] = wall(lambda: harness.FleetEvaluator(model, clean, batch, use_graph=False).step())
    chunk = max(1, min(16, 4096 // units))
    build["StreamFleet.from_calibration"] = wall(lambda: harness.StreamFleet.from_calibration(model, clean, chunk,
                                                                                            batch=batch))
    fe = harness.FleetEvaluator(model, clean, batch, use_graph=False)
    fe.step()
    build["FleetEvaluator.fleet() after a step"] = wall(lambda: fe.fleet(chunk))
    del fe
    for name, ms in build.items():
        print(f"  {name}: {ms:.1f} ms (once, eager, host clock)", flush=True)
    plain = harness.FleetEvaluator(model, clean, batch)
    gaps = harness.FleetEvaluator(model, gappy, batch, gaps=True)
    solos = [harness.SeriesEvaluator(model, None, clean[u][:, w:].t().contiguous(), batch, series=clean[u])
             for u in range(units)]

    def loop():
        for ev in solos:
            ev.step()
    runs = {"FleetEvaluator.step()": plain.step, "FleetEvaluator.step(), gaps=True, 1% missing": gaps.step,
            f"{units} SeriesEvaluator.step() in a loop": loop}
    for fn in runs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    same = all(torch.equal(plain.anomaly[u].view(torch.int64), solos[u].anomaly.view(torch.int64)) for u in range(units))
    print(f"  the fleet step's anomaly equals the loop's bit for bit: {same}", flush=True)
    times = {name: [] for name in runs}
    for _ in range(rounds):
        for name, fn in runs.items():
            times[name].append(wall(fn, steps))
    for name, ts in times.items():
        line(name, ts)
    del plain, gaps, solos, runs
    torch.cuda.empty_cache()
