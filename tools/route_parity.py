"""One small launch per (stage, kernel family) cell of the staged graph layer on a GPU, fixed seed, batch 3; prints a
sha256 of every output tensor.  Host-side refactors of the dispatch must leave every line unchanged: run it on both
builds on the same machine and diff.  Uses only long-standing ops wrappers, so the same file runs on older trees."""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdn_amd import _lib, ops  # noqa: E402

B = 3
CELLS = (   # name, n, w, d, k, wide
    ("dense", 20, 8, 64, 6, False), ("dense_wide", 20, 8, 64, 6, True),
    ("tile_d16", 51, 5, 16, 5, False), ("tile_d128", 40, 30, 128, 16, False),
    ("tile_bwd_global_tables", 300, 15, 64, 30, False), ("large", 700, 15, 64, 30, False),
    ("long_dense_aggregate", 20, 100, 64, 6, False), ("any_width", 12, 4, 24, 3, False),
)
SERIES = ("dense", "long_dense_aggregate", "any_width")


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:24]


def cell(name, n, w, d, k, wide, dev):
    g = torch.Generator().manual_seed(1234)
    rnd = lambda *s, lo=-1.0, hi=1.0: (torch.rand(s, generator=g) * (hi - lo) + lo).to(dev)  # noqa: E731
    emb, lin_w = rnd(n, d), rnd(d, w, lo=-0.3, hi=0.3)
    att = [rnd(d, lo=-0.3, hi=0.3) for _ in range(4)]
    bias, x = rnd(d, lo=-0.1, hi=0.1), rnd(B, n, w, lo=0.0)
    graph = ops.topk_graph(emb, k)
    terms = ops.node_terms(lin_w, *att, emb)
    out = {}
    out["xlin"], out["s_i"], out["s_j"] = xlin, s_i, s_j = ops.project_fwd(x, lin_w, terms, wide=wide)
    out["z"], out["alpha"] = z, alpha = ops.attn_aggregate_fwd(xlin, s_i, s_j, graph, bias, B, want_alpha=True, wide=wide)
    out["z_no_alpha"], _ = ops.attn_aggregate_fwd(xlin, s_i, s_j, graph, bias, B, want_alpha=False, wide=wide)
    d_z = rnd(B * n, d)
    out["d_xlin"], out["d_si"], out["d_sj"], out["d_bias"] = d_xlin, d_si, d_sj, _ = \
        ops.attn_aggregate_bwd(d_z, xlin, alpha, s_i, s_j, graph, B, wide=wide)
    out["d_lin_w"], out["d_a"], out["d_c"] = d_lin_w, d_a, d_c = ops.project_bwd(x, d_xlin, d_si, d_sj, d)
    grads = ops.terms_bwd(lin_w, *att, emb, d_lin_w.clone(), d_a, d_c)
    for i, t in enumerate(grads if isinstance(grads, (tuple, list)) else (grads,)):
        out[f"terms_bwd_{i}"] = t
    bn1, bn2 = (torch.cat([rnd(d, lo=0.5, hi=1.5), rnd(d, lo=-0.2, hi=0.2)]) for _ in range(2))
    out["out"], _ = ops.head_fwd(z, emb, bn1, bn2, rnd(d), rnd(1), B)
    if name in SERIES:      # the series projection: windows first .. first + B - 1 of a raw series [n, T]
        series, first = rnd(n, w + B + 4, lo=0.0), 2
        for key in ("xlin", "s_i", "s_j"):
            out["series_" + key] = torch.empty_like(out[key])
        _lib.call("gdn_project_fwd_series", series.data_ptr(), series.shape[1], first, lin_w.data_ptr(), terms.data_ptr(),
                  B, n, w, d, out["series_xlin"].data_ptr(), out["series_s_i"].data_ptr(), out["series_s_j"].data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for key, t in out.items():
        print(f"{name} n={n} w={w} d={d} k={k} {key} {sha(t)}")


if __name__ == "__main__":
    for c in CELLS:
        cell(*c, torch.device("cuda:0"))
