"""Embedding widths other than 16 / 32 / 64 / 128: per-kernel times of the staged eval forward (project -> aggregate
-> head), the whole eval forward and one autograd training step (forward + backward, 512 windows), with HIP events
(best of 3).  The last shape runs at d = 64 on the existing large-form kernels in the same process, as the yardstick
of the gather.

    python3 tools/probe_any_width.py [windows]       (default 32768, fewer where xlin would pass 4 GB)

Bytes from shapes: projection = x read + xlin, s_i, s_j written (rows * (4 w + 4 d + 8)); gather = the source rows
the aggregate reads (rows * (k + 1) * 4 d, the self loop included)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_gpu_forward_parity import random_params  # noqa: E402

from gdn_amd import ops  # noqa: E402

SHAPES = [(127, 15, 30, 48), (127, 15, 30, 96), (127, 15, 30, 256), (1024, 30, 64, 96), (1024, 30, 64, 64)]
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
    b = max(1, min(B, (4 << 30) // (n * d * 4)))
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
    gathered = rows * (k + 1) * 4 * d
    print(f"[any] n={n} w={w} k={k} d={d} B={b}: eval {b / (t_eval * 1e-6) / 1e6:.3f} M windows/s ({t_eval:.0f} us); "
          f"project {t_proj:.0f} us, aggregate {t_agg:.0f} us, head {t_head:.0f} us", flush=True)
    print(f"[project] {moved / 1e9:.2f} GB moved: {moved / (t_proj * 1e-6) / 1e12:.2f} TB/s = "
          f"{moved / (t_proj * 1e-6) / 1e12 / HBM_TBS:.2f} of HBM peak", flush=True)
    print(f"[gather] {gathered / 1e9:.1f} GB of source rows: {gathered / (t_agg * 1e-6) / 1e12:.2f} TB/s", flush=True)
    del x, out, xlin, s_i, s_j, z
    torch.cuda.empty_cache()
    # one autograd training step (forward + backward, no optimizer) at 512 windows
    bt = 512
    model.train()
    model.dp = torch.nn.Dropout(0.0)
    xt, yt = torch.rand((bt, n, w), device=dev), torch.rand((bt, n), device=dev)

    def train_step():
        model.zero_grad(set_to_none=False)
        torch.nn.functional.mse_loss(model(xt, None), yt).backward()
    t_train = timed(train_step, reps=3)
    print(f"[train] B={bt}: {t_train:.0f} us per step = {bt / (t_train * 1e-6) / 1e3:.1f} k windows/s", flush=True)
    del model, xt, yt
    torch.cuda.empty_cache()
