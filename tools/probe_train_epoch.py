"""What an epoch of training costs on the wall clock, and how much of it is the step: the SWaT shape (127 sensors,
W = 15, K = 30, d = 64) on a synthetic [127, 47 520] series at stride 5 (9 501 windows, 8 551 after the validation
block), batches of 512 and of the reference's default 128.

  (a) harness.train fed by main.IndexLoader (DataLoader over window indices, torch indexing, copies into the step's
      buffers, one replay per batch) — measured on the package under --parent-root (the parent commit, built there):
      this tree's code is never its own baseline
  (b) harness.train_series (the window table uploaded once per epoch, gather and bookkeeping inside the captured step)
  (c) back-to-back GraphedTrainStep.step() replays with no feeding: the floor; plus gdn_windows_gather and
      gdn_epoch_advance alone (HIP events, batch 512) as a share of it

(a) and (b) alternate, --runs times each, every run its own process.  A run times the loop with 1 and with 1 + E
epochs (each with its own capture) and reports the difference per epoch, with and without the validation loader: the
second difference is the validation pass.  Every epoch ends in the loop's own device-to-host read of its losses.

    python3 tools/probe_train_epoch.py --parent-root DIR [--runs 3] [--epochs 5]

Raw RESULT lines are what profiles/r06_train_epoch_*.txt keep."""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, W, K, D, T_RAW, STRIDE, VAL_RATIO = 127, 15, 30, 64, 47520, 5, 0.1
BATCHES = (512, 128)


def _opt(argv, name, default, cast=str):
    if name in argv:
        i = argv.index(name)
        val = cast(argv[i + 1])
        del argv[i:i + 2]
        return val
    return default


ARGV = sys.argv[1:]
CHILD = _opt(ARGV, "--child", "")
ROOT = os.path.abspath(_opt(ARGV, "--root", HERE))
PARENT = _opt(ARGV, "--parent-root", "")
RUNS = _opt(ARGV, "--runs", 3, int)
EPOCHS = _opt(ARGV, "--epochs", 5, int)


def spawn(mode, root):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--root", root, "--epochs", str(EPOCHS)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
    if run.returncode != 0 or not lines:
        sys.exit(f"child ({mode}) failed (rc {run.returncode}):\n{run.stdout[-2000:]}\n{run.stderr[-2000:]}")
    for ln in lines:
        print(ln, flush=True)
    return [json.loads(ln[len("RESULT "):]) for ln in lines]


if not CHILD:
    if not PARENT:
        sys.exit("--parent-root DIR (a built checkout of the parent commit) is needed: route (a) is measured there")
    rows = {"a": [], "b": []}
    for _ in range(RUNS):                       # alternate the two versions; this process never opens the GPU
        rows["a"] += spawn("a", os.path.abspath(PARENT))
        rows["b"] += spawn("b", HERE)
    floor = {r["batch"]: r for r in spawn("c", HERE)}
    for batch in BATCHES:
        a = [r for r in rows["a"] if r["batch"] == batch]
        b = [r for r in rows["b"] if r["batch"] == batch]
        c = floor[batch]
        fmt = lambda rs, key: " ".join(f"{r[key]:8.2f}" for r in rs)
        print(f"[epoch] batch {batch}: {a[0]['steps']} steps per epoch, floor (c) {c['step_us']:.1f} us per step = "
              f"{c['step_us'] * a[0]['steps'] / 1e3:.2f} ms per epoch")
        print(f"  (a) train + IndexLoader  ms/epoch {fmt(a, 'epoch_ms')}   validation ms {fmt(a, 'val_ms')}")
        print(f"  (b) train_series         ms/epoch {fmt(b, 'epoch_ms')}   validation ms {fmt(b, 'val_ms')}")
        print(f"  slowest (b) / fastest (a): {max(r['epoch_ms'] for r in b) / min(r['epoch_ms'] for r in a):.3f}; "
              f"(a) spread {max(r['epoch_ms'] for r in a) - min(r['epoch_ms'] for r in a):.2f} ms")
        if "gather_us" in c:
            print(f"  gdn_windows_gather {c['gather_us']:.2f} us, gdn_epoch_advance {c['advance_us']:.2f} us = "
                  f"{100 * (c['gather_us'] + c['advance_us']) / c['step_us']:.1f} % of a step")
    sys.exit(0)

# ------------------------------------------------------------------------------------------------ children
sys.path.insert(0, ROOT)
import random  # noqa: E402

import torch  # noqa: E402

import gdn_amd  # noqa: E402
from gdn_amd import GDN, harness  # noqa: E402
from gdn_amd.main import IndexLoader, SeriesWindows  # noqa: E402

dev = torch.device("cuda:0")
series = torch.rand((N, T_RAW), generator=torch.Generator().manual_seed(1)).to(dev)


def fresh(batch):
    """Model, windows and main.Main.get_loaders' pair from fixed seeds."""
    random.seed(0)
    torch.manual_seed(0)
    windows = SeriesWindows(series, torch.zeros(T_RAW, dtype=torch.float64, device=dev), W, STRIDE, "train")
    total = len(windows)
    use, val = int(total * (1 - VAL_RATIO)), int(total * VAL_RATIO)
    v0 = random.randrange(use)
    idx = torch.arange(total)
    train_idx, val_idx = torch.cat([idx[:v0], idx[v0 + val:]]), idx[v0:v0 + val]
    model = GDN([torch.zeros((2, 1), dtype=torch.long)], N, dim=D, input_dim=W, topk=K).to(dev)
    return (model, IndexLoader(windows, train_idx, batch, True, None), IndexLoader(windows, val_idx, batch, False, None),
            (len(train_idx) + batch - 1) // batch)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def loop(mode, epochs, batch, with_val):
    model, train_loader, val_loader, _steps = fresh(batch)
    cfg = {"epoch": epochs, "wide": False, "batch": batch}
    val = val_loader if with_val else None
    if mode == "a":
        return wall(lambda: harness.train(model, "", cfg, train_loader, val, use_graph=True))
    return wall(lambda: harness.train_series(model, "", cfg, series, W, train_loader, val))


if CHILD in ("a", "b"):
    loop(CHILD, 1, BATCHES[0], True)            # pre-roll: code objects, allocator, loader machinery
    for batch in BATCHES:
        steps = fresh(batch)[3]
        res = {}
        for with_val in (False, True):
            t1 = loop(CHILD, 1, batch, with_val)
            te = loop(CHILD, 1 + EPOCHS, batch, with_val)
            res[with_val] = (te - t1) / EPOCHS
        print("RESULT " + json.dumps({"route": CHILD, "package": os.path.dirname(gdn_amd.__file__), "batch": batch,
                                      "steps": steps, "epoch_ms": res[False], "step_us": res[False] * 1e3 / steps,
                                      "val_ms": res[True] - res[False]}), flush=True)
    sys.exit(0)

# (c) the floor, and the two new launches alone
from gdn_amd import ops  # noqa: E402

for batch in BATCHES:
    model, _tl, _vl, steps = fresh(batch)
    step = harness.GraphedTrainStep(model, batch, wide=False)
    step.x.uniform_()
    step.y.uniform_()
    for _ in range(20):
        step.step()
    best = min(wall(lambda: [step.step() for _ in range(steps * 4)]) for _ in range(3)) * 1e3 / (steps * 4)
    res = {"route": "c", "batch": batch, "steps": steps, "step_us": best}
    if batch == 512:
        table = torch.randint(W, T_RAW, (steps * batch,), generator=torch.Generator().manual_seed(2)).to(dev)
        cursor = torch.zeros((1,), dtype=torch.int64, device=dev)
        losses = torch.zeros((steps,), device=dev)

        def events(fn, reps=200):
            fn()
            torch.cuda.synchronize()
            best_us = 1e30
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                best_us = min(best_us, e0.elapsed_time(e1) * 1e3 / reps)
            return best_us

        res["gather_us"] = events(lambda: ops.windows_gather(series, table, batch, W, step.x, step.y, cursor=cursor))
        res["advance_us"] = events(lambda: ops.epoch_advance(step.loss, cursor, losses))
    print("RESULT " + json.dumps(res), flush=True)
