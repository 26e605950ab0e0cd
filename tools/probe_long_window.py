"""Windows longer than 64 ticks: per-kernel time of the staged eval forward (project -> aggregate -> head) and of
the whole eval forward, with HIP events, and the projection's achieved HBM rate against the 8 TB/s peak
(bytes = x read + xlin, s_i, s_j written: rows * (4 w + 4 d + 8)).

    python3 tools/probe_long_window.py [windows]          (default 32768 windows; shapes (n, w, k, d) below)

`rocprofv3 --kernel-trace --stats` on the same command gives the authoritative per-kernel table."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_gpu_forward_parity import random_params  # noqa: E402

from gdn_amd import ops  # noqa: E402

SHAPES = [(127, 65, 30, 64), (127, 100, 30, 64), (127, 256, 30, 64), (127, 1024, 30, 64), (700, 100, 30, 64)]
B = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
HBM_TBS = 8.0
dev = torch.device("cuda:0")


def timed(fn, reps=5):
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


for n, w, k, d in SHAPES:
    # windows per launch: at most ~3 GB of x
    b = max(1, min(B, (3 << 30) // (n * w * 4)))
    model = random_params(n, w, k, d, seed=0).to(dev).eval()
    model.operand_range = "narrow"
    gnn = model.gnn_layers[0].gnn
    lin = model.out_layer.mlp[0]
    x = torch.rand((b, n, w), device=dev)
    out = torch.empty((b, n), device=dev)
    c = model._constants()
    t_eval = timed(lambda: model.forward_into(x, out))
    xlin, s_i, s_j = ops.project_fwd(x, gnn.lin.weight, c.terms)
    t_proj = timed(lambda: ops.project_fwd(x, gnn.lin.weight, c.terms))
    t_agg = timed(lambda: ops.attn_aggregate_fwd(xlin, s_i, s_j, c.graph, gnn.bias, b, want_alpha=False))
    z, _ = ops.attn_aggregate_fwd(xlin, s_i, s_j, c.graph, gnn.bias, b, want_alpha=False)
    t_head = timed(lambda: ops.head_fwd(z, model.embedding.weight, c.bn1, c.bn2, lin.weight, lin.bias, b))
    rows = b * n
    moved = rows * (4 * w + 4 * d + 8)
    rate = moved / (t_proj * 1e-6) / 1e12
    tflops = 2.0 * rows * w * (d + 2) / (t_proj * 1e-6) / 1e12
    print(f"[long] n={n} w={w} k={k} d={d} B={b}: eval {b / (t_eval * 1e-6) / 1e6:.3f} M windows/s "
          f"({t_eval:.0f} us); project {t_proj:.0f} us, aggregate {t_agg:.0f} us, head {t_head:.0f} us", flush=True)
    print(f"[project] {moved / 1e9:.2f} GB moved: {rate:.2f} TB/s = {rate / HBM_TBS:.2f} of HBM peak, "
          f"{tflops:.1f} TF fp32 matrix work", flush=True)
    del model, x, out, xlin, s_i, s_j, z
    torch.cuda.empty_cache()
