"""MLP-head models (out_layer_num > 1) on the evaluation fast path: what folding the head into the OutLayer MLP's
first operand saves, and what the resident-series evaluator gains over minibatches of materialised windows.  HIP
events, best of 3 after a pre-roll, all four routes in one run:

  (a) gdn_head_fwd writing h2 + gdn_mlp_fwd reading it, back to back      — the reference for the kernel
  (b) gdn_head_mlp_fwd on the same z                                       — must equal (a) bit for bit (checked)
  (c) model(x) per 512 windows gathered from the series, predictions concatenated (the loop python -m gdn_amd.main
      ran for these models before forward_series took them), in a child process; `--route-c-root DIR` runs it on
      another checkout's package (the parent commit, built there) — GDN.forward is the same code in both
  (d) harness.SeriesEvaluator.step() on the raw series, HIP-graph replay (forward AND anomaly scores);
      (d') its forward_only()

    python3 tools/probe_mlp_fast_path.py [windows] [--route-c-root DIR]     (default 32768 windows, fewer where z
                                                                            would pass 4 GB)

Bytes from shapes: (a) moves z in, h2 out and h2 in again (3 * B * n * d * 4 bytes), (b) z only."""
import json
import os
import subprocess
import sys

SHAPES = [(127, 15, 30, 64, 256, 2), (512, 30, 64, 64, 256, 2)]       # (n, w, k, d, hidden, layers)
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args():
    argv = sys.argv[1:]
    root, child = HERE, False
    if "--route-c-root" in argv:
        i = argv.index("--route-c-root")
        root = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    if "--child" in argv:
        child = True
        argv.remove("--child")
    return (int(argv[0]) if argv else 32768), root, child


B, ROOT, CHILD = _args()
sys.path.insert(0, ROOT if CHILD else HERE)
sys.path.insert(0, os.path.join(ROOT if CHILD else HERE, "tests"))
import torch  # noqa: E402
from test_gpu_forward_parity import random_params  # noqa: E402

dev = torch.device("cuda:0")


def timed(fn, reps=3):
    fn()                                     # pre-roll: code objects, plans, cached buffers
    fn()
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / reps)
    return best          # us


def windows_of(n, d):
    return max(512, min(B, (4 * 10 ** 9) // (n * d * 4)))


def setup(n, w, k, d, hidden, layers):
    model = random_params(n, w, k, d, seed=0, out_layer_num=layers, inter=hidden).to(dev).eval()
    b = windows_of(n, d)
    series = torch.rand((n, b + w), generator=torch.Generator().manual_seed(1)).to(dev)
    return model, b, series


def route_c(model, b, series, w, batch=512):
    """main.py's loop for an MLP head before forward_series took it: IndexLoader -> SeriesWindows.batch -> model(x)."""
    model.operand_range = "narrow"          # (main.py leaves "auto": one host check per minibatch on top of this)
    offs = torch.arange(0, w, device=dev)

    def run():
        outs = []
        with torch.no_grad():
            for s in range(0, b, batch):
                at = torch.arange(s, min(b, s + batch), device=dev)
                x = series[:, at.view(-1, 1) + offs.view(1, -1)].permute(1, 0, 2).contiguous()
                outs.append(model(x, None))
        return torch.cat(outs)
    return timed(run, reps=1), run


if CHILD:
    import gdn_amd
    res = {"package": os.path.dirname(gdn_amd.__file__)}
    for shape in SHAPES:
        model, b, series = setup(*shape)
        t_c, _ = route_c(model, b, series, shape[1])
        res["n{}_w{}".format(*shape)] = t_c
        del model, series
        torch.cuda.empty_cache()
    print("ROUTE_C " + json.dumps(res), flush=True)
    sys.exit(0)

from gdn_amd import harness, ops  # noqa: E402

# (c) first, in a fresh child process (this one has not touched the GPU yet); the rest alternates in this process
child = subprocess.run([sys.executable, os.path.abspath(__file__), str(B), "--route-c-root", ROOT, "--child"],
                       capture_output=True, text=True, timeout=900)
line = [ln for ln in child.stdout.splitlines() if ln.startswith("ROUTE_C ")]
if child.returncode != 0 or not line:
    sys.exit(f"route (c) child failed (rc {child.returncode}):\n{child.stdout[-2000:]}\n{child.stderr[-2000:]}")
route_c_us = json.loads(line[0][len("ROUTE_C "):])
print(f"[mlp] route (c) measured on the package at {route_c_us['package']}", flush=True)

for shape in SHAPES:
    n, w, k, d, hidden, layers = shape
    model, b, series = setup(*shape)
    c = model._constants()
    emb = model.embedding.weight
    plan = ops.mlp_plan(model.out_layer, d)
    rows = b * n
    z = torch.randn((rows, d), generator=torch.Generator().manual_seed(2)).to(dev)
    zero_w, zero_b = torch.zeros((d,), device=dev), torch.zeros((1,), device=dev)
    out_a, out_b = torch.empty((rows,), device=dev), torch.empty((rows,), device=dev)
    h2 = torch.empty((rows, d), device=dev)
    head_out = torch.empty((b, n), device=dev)
    st = torch.cuda.current_stream().cuda_stream
    from gdn_amd import _lib

    def route_a():
        _lib.call("gdn_head_fwd", z.data_ptr(), emb.data_ptr(), c.bn1.data_ptr(), c.bn2.data_ptr(), zero_w.data_ptr(),
                  zero_b.data_ptr(), b, n, d, head_out.data_ptr(), h2.data_ptr(), st)
        ops.mlp_fwd(h2, plan, out=out_a)

    def route_b():
        ops.head_mlp_fwd(z, emb, c.bn1, c.bn2, plan, b, out=out_b)

    t_a, t_b = [], []
    for _ in range(2):                       # alternate the two versions
        t_a.append(timed(route_a))
        t_b.append(timed(route_b))
    t_a, t_b = min(t_a), min(t_b)
    t_head = timed(lambda: _lib.call("gdn_head_fwd", z.data_ptr(), emb.data_ptr(), c.bn1.data_ptr(), c.bn2.data_ptr(),
                                     zero_w.data_ptr(), zero_b.data_ptr(), b, n, d, head_out.data_ptr(), h2.data_ptr(), st))
    same = torch.equal(out_a, out_b)
    zbytes = rows * d * 4
    del z, h2, out_a, out_b, head_out
    torch.cuda.empty_cache()

    # (d) the evaluator on the raw series, graph replay; its predictions against route (c)'s loop in THIS tree
    y = series[:, w:].t().contiguous()
    ev = harness.SeriesEvaluator(model, None, y[:b], batch=512, use_graph=True, coalesce=8, series=series)
    t_d = timed(ev.step)
    t_df = timed(ev.forward_only)
    t_c_here, run_c = route_c(model, b, series, w)
    err = float((run_c() - ev.pred).abs().max())
    t_c = route_c_us["n{}_w{}".format(*shape)]
    print(f"[mlp] n={n} w={w} k={k} d={d} hidden={hidden} layers={layers} B={b}", flush=True)
    print(f"  (a) head + h2 + mlp   {t_a:9.1f} us   (gdn_head_fwd alone {t_head:.1f} us; {3 * zbytes / 1e9:.2f} GB moved)")
    print(f"  (b) gdn_head_mlp_fwd  {t_b:9.1f} us   = {t_a / t_b:.2f} x (a); z read at {zbytes / (t_b * 1e-6) / 1e12:.2f} TB/s; "
          f"bits equal (a): {same}")
    print(f"  (c) model(x) per 512  {t_c:9.1f} us   ({t_c_here:.1f} us in this tree)")
    print(f"  (d) evaluator step    {t_d:9.1f} us   = {t_c / t_d:.2f} x (c); forward only {t_df:.1f} us; "
          f"max|pred - (c)| = {err:.2e}", flush=True)
    print("RESULT " + json.dumps({"shape": shape, "windows": b, "a_us": t_a, "b_us": t_b, "head_us": t_head, "c_us": t_c,
                                  "c_here_us": t_c_here, "d_us": t_d, "d_forward_us": t_df, "bits_equal": same,
                                  "z_TBps": zbytes / (t_b * 1e-6) / 1e12, "pred_err_vs_c": err}), flush=True)
    assert same, "gdn_head_mlp_fwd differs from gdn_head_fwd + gdn_mlp_fwd"
    del model, series, ev, y
    torch.cuda.empty_cache()
