"""sha256 of `GDN.forward` outputs on fixed seeds over the shapes of tests/test_gpu_fused_valu_trim.py, one line per
shape and one for all: run it once per library (GDN_HIP_LIB=... for another build) and compare the lines.
python3 tools/probe_fused_bits.py"""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_gpu_forward_parity import random_params  # noqa: E402
from test_gpu_fused_valu_trim import B_SMALL, B_UNEQUAL, CASES  # noqa: E402

dev = torch.device("cuda:0")
total = hashlib.sha256()
print({k: os.path.basename(v) for k, v in os.environ.items() if k.startswith("GDN_")})
for n, w, k, d, bf16 in CASES + [(127, 15, 48, 64, False), (64, 15, 15, 64, False)]:
    model = random_params(n, w, k, d, seed=181).to(dev).eval()
    x = torch.rand((B_UNEQUAL, n, w), generator=torch.Generator().manual_seed(182))
    x[:, :, 0] -= 0.5                                   # both signs
    xin = (x.bfloat16() if bf16 else x).to(dev)
    h = hashlib.sha256()
    with torch.no_grad():
        for b in (B_UNEQUAL, B_SMALL):
            out = model(xin[:b], None)
            into = model.forward_into(xin[:b], torch.empty((b, n), device=dev))
            torch.cuda.synchronize()
            for t in (out, into):
                h.update(t.cpu().numpy().tobytes())
    total.update(h.digest())
    print(f"n={n:3d} w={w:2d} k={k:2d} d={d:3d} {'bf16' if bf16 else 'fp32'}  {h.hexdigest()[:32]}  "
          f"sum {float(out.double().sum()):.9f}")
print("all", total.hexdigest())
