"""Graphs beyond the LDS tile: windows/s and per-kernel time of the eval forward (project -> gather-aggregate ->
head) and of the autograd training step, and the gather kernel's achieved rate against its paper floor
(n * (k+1) * d * 4 gathered bytes per window at the L2 rate 16.8 TB/s; the Infinity Cache serves 8.6 TB/s).

    python3 tools/probe_large_graph.py [windows]          (default 4096 windows; shapes (n, w, k, d) below)

Per-kernel numbers come from events around single launches (after warm-up); `rocprofv3 --kernel-trace --stats`
on the same command gives the authoritative per-kernel table."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_gpu_forward_parity import random_params  # noqa: E402

from gdn_amd import harness, ops  # noqa: E402

SHAPES = [(1024, 30, 64, 64), (4096, 15, 30, 64)]
B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
L2_TBS, IC_TBS = 16.8, 8.6
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
    model = random_params(n, w, k, d, seed=0).to(dev).eval()
    gnn = model.gnn_layers[0].gnn
    lin = model.out_layer.mlp[0]
    x = torch.rand((B, n, w), generator=torch.Generator().manual_seed(0)).to(dev)
    out = torch.empty((B, n), device=dev)
    c = model._constants()
    t_eval = timed(lambda: model.forward_into(x, out))
    xlin, s_i, s_j = ops.project_fwd(x, gnn.lin.weight, c.terms)
    t_proj = timed(lambda: ops.project_fwd(x, gnn.lin.weight, c.terms))
    t_agg = timed(lambda: ops.attn_aggregate_fwd(xlin, s_i, s_j, c.graph, gnn.bias, B, want_alpha=False))
    z, _ = ops.attn_aggregate_fwd(xlin, s_i, s_j, c.graph, gnn.bias, B, want_alpha=False)
    t_head = timed(lambda: ops.head_fwd(z, model.embedding.weight, c.bn1, c.bn2, lin.weight, lin.bias, B))
    gathered = B * n * (k + 1) * d * 4
    rate = gathered / (t_agg * 1e-6) / 1e12
    print(f"[eval]  n={n} w={w} k={k} d={d} B={B}: {B / (t_eval * 1e-6) / 1e6:.3f} M windows/s ({t_eval:.0f} us); "
          f"project {t_proj:.0f} us, aggregate {t_agg:.0f} us, head {t_head:.0f} us", flush=True)
    print(f"[gather] {gathered / 1e9:.2f} GB gathered: {rate:.2f} TB/s = {rate / L2_TBS:.0%} of the L2 floor "
          f"({gathered / (L2_TBS * 1e12) * 1e6:.0f} us), {rate / IC_TBS:.0%} of the Infinity Cache rate", flush=True)
    del xlin, s_i, s_j, z
    # training: the autograd step (the native captured step does not take these shapes)
    model.train()
    model.dp = torch.nn.Dropout(0.0)
    model.operand_range = "narrow"
    tb = B
    step = harness.GraphedTrainStep(model, tb, use_graph=True)
    step.x.copy_(x[:tb])
    step.y.copy_(torch.rand((tb, n), device=dev))
    t_step = timed(step.step, reps=3)
    print(f"[train] n={n} B={tb}: {tb / (t_step * 1e-6) / 1e3:.1f} k windows/s ({t_step:.0f} us per step, "
          f"{type(step).__name__})", flush=True)
    xt = x[:tb].contiguous()
    xl, si, sj = ops.project_fwd(xt, gnn.lin.weight, c.terms)
    zt, alpha = ops.attn_aggregate_fwd(xl, si, sj, c.graph, gnn.bias, tb, want_alpha=True)
    dz = torch.randn_like(zt)
    c.graph.reverse()
    t_bwd = timed(lambda: ops.attn_aggregate_bwd(dz, xl, alpha, si, sj, c.graph, tb))
    print(f"[train] aggregate backward {t_bwd:.0f} us at B={tb}", flush=True)
    del model, step, x, out, xl, si, sj, zt, alpha, dz
    torch.cuda.empty_cache()
    time.sleep(0.1)
