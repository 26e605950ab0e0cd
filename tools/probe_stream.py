"""What a push of the streaming detector costs: the SWaT shape (127 sensors, W = 15, K = 30, d = 64), pushes of 1, 16
and 512 ticks, a few thousand pushes after warm-up, HIP-event timed, every leg in a process of its own.

  (a) harness.StreamDetector.push: one copy into the chunk buffer + one replay of the captured graph
      (gdn_stream_windows -> forward_into -> gdn_stream_score -> gdn_stream_advance)
  (b) what the package offered before for the same result, eager: the ticks are appended to a resident series,
      GDN.forward_series runs over the new windows, gdn_score_smooth_topm scores them with first_tick and a 3-row
      pred / gt halo the host keeps between pushes
  (n) the three new launches of (a) alone, eager and back to back, as a share of (a)

    python3 tools/probe_stream.py [--pushes 3000] [--runs 3]

  --gaps: what missing readings cost instead of the legs above, same protocol —
  (g0) the push of (a), gaps=False   (g1) gaps=True on clean ticks   (g2) gaps=True with about 1 % of the readings NaN

  --recal R: what the calibration ring costs instead of the legs above, same protocol —
  (r0) the push of (a), recal=0   (r1) recal=R: the ring writer rides in the replay; after the timed pushes a second
  recalibrate() is timed on the host clock (the read of ring_keep, the select, a synchronisation)

Raw RESULT lines are what profiles/r07_stream_push.txt keeps."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, W, K, D = 127, 15, 30, 64
CHUNKS = (1, 16, 512)


def _opt(argv, name, default, cast=str):
    if name in argv:
        i = argv.index(name)
        val = cast(argv[i + 1])
        del argv[i:i + 2]
        return val
    return default


ARGV = sys.argv[1:]
CHILD = _opt(ARGV, "--child", "")
PUSHES = _opt(ARGV, "--pushes", 3000, int)
RUNS = _opt(ARGV, "--runs", 3, int)
GAPS = "--gaps" in ARGV
RECAL = _opt(ARGV, "--recal", 0, int)

if not CHILD and RECAL:
    rows = {"r0": [], "r1": []}
    for _ in range(RUNS):                       # alternate the legs; this process never opens the GPU
        for leg in rows:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, "--pushes", str(PUSHES), "--recal", str(RECAL)]
            run = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            lines = [ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
            if run.returncode != 0 or not lines:
                sys.exit(f"child ({leg}) failed (rc {run.returncode}):\n{run.stdout[-2000:]}\n{run.stderr[-2000:]}")
            for ln in lines:
                print(ln, flush=True)
            rows[leg] += [json.loads(ln[len("RESULT "):]) for ln in lines]
    for c in CHUNKS:
        r0, r1 = ([r["push_us"] for r in rows[leg] if r["chunk"] == c] for leg in rows)
        once = [r["recal_us"] for r in rows["r1"] if r["chunk"] == c]
        fmt = lambda v: " ".join(f"{x:8.1f}" for x in v)
        print(f"[stream recal] chunk {c:3d}: recal=0 {fmt(r0)} us | recal={RECAL} {fmt(r1)} us | fastest recal={RECAL} / "
              f"fastest recal=0 {min(r1) / min(r0):.3f} | one recalibrate() {fmt(once)} us")
    sys.exit(0)

if not CHILD and GAPS:
    rows = {"g0": [], "g1": [], "g2": []}
    for _ in range(RUNS):                       # alternate the legs; this process never opens the GPU
        for leg in rows:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, "--pushes", str(PUSHES)]
            run = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            lines = [ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
            if run.returncode != 0 or not lines:
                sys.exit(f"child ({leg}) failed (rc {run.returncode}):\n{run.stdout[-2000:]}\n{run.stderr[-2000:]}")
            for ln in lines:
                print(ln, flush=True)
            rows[leg] += [json.loads(ln[len("RESULT "):]) for ln in lines]
    for c in CHUNKS:
        g0, g1, g2 = ([r["push_us"] for r in rows[leg] if r["chunk"] == c] for leg in rows)
        fmt = lambda v: " ".join(f"{x:8.1f}" for x in v)
        print(f"[stream gaps] chunk {c:3d}: gaps=False {fmt(g0)} us | gaps=True clean {fmt(g1)} us | gaps=True 1 % "
              f"missing {fmt(g2)} us | fastest gaps=True clean / fastest gaps=False {min(g1) / min(g0):.3f}")
    sys.exit(0)

if not CHILD:
    rows = {"a": [], "b": [], "n": []}
    for _ in range(RUNS):                       # alternate the legs; this process never opens the GPU
        for leg in ("a", "b", "n"):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, "--pushes", str(PUSHES)]
            run = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            lines = [ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
            if run.returncode != 0 or not lines:
                sys.exit(f"child ({leg}) failed (rc {run.returncode}):\n{run.stdout[-2000:]}\n{run.stderr[-2000:]}")
            for ln in lines:
                print(ln, flush=True)
            rows[leg] += [json.loads(ln[len("RESULT "):]) for ln in lines]
    for c in CHUNKS:
        a, b, n = ([r["push_us"] for r in rows[leg] if r["chunk"] == c] for leg in ("a", "b", "n"))
        fmt = lambda v: " ".join(f"{x:8.1f}" for x in v)
        print(f"[stream] chunk {c:3d}: (a) replay {fmt(a)} us | (b) eager series + halo {fmt(b)} us | slowest (a) / "
              f"fastest (b) {max(a) / min(b):.3f} | new launches alone {fmt(n)} us = {100 * min(n) / min(a):.0f} % of (a)")
    sys.exit(0)

# ------------------------------------------------------------------------------------------------ children
sys.path.insert(0, HERE)
import torch  # noqa: E402

from gdn_amd import GDN, harness, ops  # noqa: E402

dev = torch.device("cuda:0")
torch.manual_seed(0)
model = GDN([torch.zeros((2, 1), dtype=torch.long)], N, dim=D, input_dim=W, topk=K).to(dev).eval()
med_iqr = torch.stack([torch.rand(N, dtype=torch.float64) * 0.1, torch.rand(N, dtype=torch.float64) * 0.2 + 0.05], 1).to(dev)
history = torch.rand((N, W), generator=torch.Generator().manual_seed(1)).to(dev)


def timed(push, pushes, warm=200):
    """us per push: `warm` pushes, then three windows of `pushes`, the best."""
    for i in range(warm):
        push(i)
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(pushes):
            push(i)
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / pushes)
    return best


for c in CHUNKS:
    pushes = max(200, PUSHES // (1 if c < 512 else 4))
    ticks = torch.rand((64, c, N), generator=torch.Generator().manual_seed(2)).to(dev)      # 64 different chunks, cycled
    extra = {}
    if CHILD in ("a", "g0", "r0"):
        det = harness.StreamDetector(model, med_iqr, 5.0, history, c, top_m=3)
        us = timed(lambda i: det.push(ticks[i & 63]), pushes)
    elif CHILD in ("g1", "g2"):
        if CHILD == "g2":
            ticks[torch.rand(ticks.shape, generator=torch.Generator().manual_seed(3)).to(dev) < 0.01] = float("nan")
        det = harness.StreamDetector(model, med_iqr, 5.0, history, c, top_m=3, gaps=True)
        us = timed(lambda i: det.push(ticks[i & 63]), pushes)
    elif CHILD == "r1":
        # exclude_alarms=False: the untrained model alarms at most ticks under this table; the writer's work is the same
        det = harness.StreamDetector(model, med_iqr, 5.0, history, c, top_m=3, recal=RECAL, recal_min=64,
                                     exclude_alarms=False)
        us = timed(lambda i: det.push(ticks[i & 63]), pushes)
        import time
        det.recalibrate()                                           # (the first call loads the select's kernels)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        kept = det.recalibrate()
        torch.cuda.synchronize()
        extra = {"recal": RECAL, "kept": kept, "recal_us": (time.perf_counter() - t0) * 1e6}
    elif CHILD == "n":
        det = harness.StreamDetector(model, med_iqr, 5.0, history, c, top_m=3, use_graph=False)
        det.push(ticks[0])

        def three(i):
            ops.stream_windows(det.state, det.chunk_buf, W, det.x)
            ops.stream_score(det.state, det.pred, det.chunk_buf, det.med_iqr, det.threshold, 3, det.top_scores,
                             det.top_sensors, det.alarm)
            ops.stream_advance(det.state, det.chunk_buf, det.pred, det.med_iqr, det.alarm, det.top_sensors, W, 3,
                               det.log_ticks, det.log_sensors)
        us = timed(three, pushes)
    else:
        # the resident series is a ring of 4096 chunks behind the history; the host keeps first_tick and the halo
        cap = 4096 if c < 512 else 64
        series = torch.zeros((N, W + cap * c), device=dev)
        series[:, :W] = history
        pred = torch.empty((c, N), device=dev)
        halo_p, halo_g = torch.zeros((3, N), device=dev), torch.zeros((3, N), device=dev)
        top_s = torch.empty((c, 3), dtype=torch.float64, device=dev)
        top_i = torch.empty((c, 3), dtype=torch.int32, device=dev)
        pos = {"tick": 0}

        def old(i):
            t = pos["tick"]
            at = (t % (cap * c))
            if at == 0 and t:                                       # wrap: the last window back to the front
                series[:, :W] = series[:, cap * c:cap * c + W]
            gt = ticks[i & 63]
            series[:, W + at:W + at + c] = gt.t()
            model.forward_series(series, at, c, out=pred, wide=False)
            ops.score_smooth_topm(pred, gt, med_iqr, 3, first_tick=t, halo_pred=halo_p if t else None,
                                  halo_gt=halo_g if t else None, top_scores=top_s, top_sensors=top_i)
            _flags = top_s[:, 0] > 5.0
            if c >= 3:
                halo_p.copy_(pred[-3:])
                halo_g.copy_(gt[-3:])
            else:
                halo_p.copy_(torch.cat([halo_p[c:], pred]))
                halo_g.copy_(torch.cat([halo_g[c:], gt]))
            pos["tick"] = t + c
        us = timed(old, pushes)
    print("RESULT " + json.dumps({"leg": CHILD, "chunk": c, "pushes": pushes, "push_us": us, **extra}), flush=True)
