"""Tensor-level wrappers over the C ABI (include/gdn_hip.h): PyTorch-ROCm tensors in,
tensors out.  torch is used for device memory and the current HIP stream only; all
arithmetic happens in libgdn_hip.so.  Every function raises if a tensor is not on a HIP
device — there is no CPU path.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _chk(t: torch.Tensor, dtype=torch.float32, name="tensor") -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.GdnHipError(f"{name} is on {t.device}: gdn_amd ops need a HIP device (no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _ptr(t):
    return None if t is None else t.data_ptr()


def nbr_pitch(k: int) -> int:
    return ((k + 1) + 15) & ~15


class SensorGraph:
    """Neighbour lists shared by every window (reference models/GDN.py:148-165 and
    models/graph_layer.py:61-63 in list form).  topk: [n,k] int64 = `learned_graph`."""

    def __init__(self, topk, nbr, deg, cos=None):
        self.topk, self.nbr, self.deg, self.cos = topk, nbr, deg, cos
        self.n, self.k = topk.shape
        self.pitch = nbr.shape[1]
        self._reverse = None
        self._ordered = False       # not built yet; None = shape outside the matrix-core kernels

    def nbr_ordered(self):
        """The neighbour lists with every row permuted inside its two halves for LDS bank spread
        (gdn_graph_bank_order), or `nbr` itself where the aggregate does not route to the matrix-core kernels.  For launches
        that do not hand alpha out in rank order.  Built on first use, once per graph."""
        if self._ordered is False:
            self._ordered = None
            if _lib.family(_lib.STAGE_AGGREGATE, self.n, 1, 64, self.k) == _lib.FAMILY_DENSE:
                out = torch.empty_like(self.nbr)
                out.copy_(self.nbr)                         # (padding rows / slots as in the original)
                _lib.call("gdn_graph_bank_order", _ptr(self.nbr), self.n, self.k, _ptr(out), _stream())
                self._ordered = out
        return self.nbr if self._ordered is None else self._ordered

    def reverse(self):
        """(rent[n, rpitch] u32, rlen[n] i32): per source, the (target << 16 | slot) entries that
        name it — the backward pass gathers through these.  Built on first use."""
        if self._reverse is None:
            rpitch = (self.n + 15) & ~15
            rent = torch.empty((self.n, rpitch), dtype=torch.int32, device=self.nbr.device)
            rlen = torch.empty((self.n,), dtype=torch.int32, device=self.nbr.device)
            _lib.call("gdn_graph_reverse", _ptr(self.nbr), _ptr(self.deg), self.n, self.k, _ptr(rent), _ptr(rlen),
                      _stream())
            self._reverse = (rent, rlen)
        return self._reverse


def topk_graph(emb: torch.Tensor, k: int, want_cos: bool = False) -> SensorGraph:
    emb = _chk(emb.detach(), name="embedding")            # graph is built on a detached copy (GDN.py:145)
    n, d = emb.shape
    dev = emb.device
    topk = torch.empty((n, k), dtype=torch.int64, device=dev)
    nbr = torch.empty((n, nbr_pitch(k)), dtype=torch.uint16, device=dev)
    deg = torch.empty((n,), dtype=torch.int32, device=dev)
    cos = torch.empty((n, n), dtype=torch.float32, device=dev) if want_cos else None
    _lib.call("gdn_topk_graph", _ptr(emb), n, d, k, _ptr(topk), _ptr(nbr), _ptr(deg), _ptr(cos), _stream())
    return SensorGraph(topk, nbr, deg, cos)


def graph_from_topk(topk: torch.Tensor) -> SensorGraph:
    topk = _chk(topk, torch.int64, "topk")
    n, k = topk.shape
    if k > 0 and (int(topk.min()) < 0 or int(topk.max()) >= n):     # caller data: one sync, once per graph
        raise ValueError(f"injected top-k table has entries outside [0, {n})")
    nbr = torch.empty((n, nbr_pitch(k)), dtype=torch.uint16, device=topk.device)
    deg = torch.empty((n,), dtype=torch.int32, device=topk.device)
    _lib.call("gdn_graph_from_topk", _ptr(topk), n, k, _ptr(nbr), _ptr(deg), _stream())
    return SensorGraph(topk, nbr, deg)


def terms_pitch(w: int) -> int:
    """P of the node-terms layout [a_i(P) | a_j(P) | c_i(n) | c_j(n)]: 64 up to w = 64, round_up(w, 64) above."""
    p = _lib.load().gdn_terms_pitch(w)
    if p == 0:
        raise _lib.GdnHipError(f"window length {w} is not supported (1 <= w <= 1024, include/gdn_hip.h)")
    return p


MAX_WIDTH = 256     # largest embedding width d (include/gdn_hip.h "Supported shapes")


def check_width(d: int) -> int:
    """The embedding width d, or GdnHipError when no kernel takes it (1 <= d <= 256).  Host only, no launch."""
    if not 1 <= d <= MAX_WIDTH:
        raise _lib.GdnHipError(f"embedding width {d} is not supported (1 <= d <= {MAX_WIDTH}, include/gdn_hip.h)")
    return d


def node_terms(lin_w, att_i, att_j, att_em_i, att_em_j, emb) -> torch.Tensor:
    lin_w = _chk(lin_w.detach(), name="lin.weight")
    d, w = lin_w.shape
    emb = _chk(emb.detach(), name="embedding")
    n = emb.shape[0]
    vs = [_chk(v.detach().reshape(-1), name="att") for v in (att_i, att_j, att_em_i, att_em_j)]
    out = torch.empty((2 * terms_pitch(w) + 2 * n,), dtype=torch.float32, device=emb.device)
    _lib.call("gdn_node_terms", _ptr(lin_w), *[_ptr(v) for v in vs], _ptr(emb), n, d, w, _ptr(out), _stream())
    return out


def bn_fold(bn: torch.nn.BatchNorm1d) -> torch.Tensor:
    c = bn.num_features
    out = torch.empty((2 * c,), dtype=torch.float32, device=bn.weight.device)
    _lib.call("gdn_bn_fold", _ptr(_chk(bn.weight.detach())), _ptr(_chk(bn.bias.detach())),
              _ptr(_chk(bn.running_mean)), _ptr(_chk(bn.running_var)), float(bn.eps), c, _ptr(out), _stream())
    return out


def _storage(t: torch.Tensor, name: str) -> str:
    """"" for fp32 tensors, "_bf16" for bfloat16 ones: the suffix of the C entry point (bf16 STORAGE of
    x / xlin / z, fp32 arithmetic — include/gdn_hip.h)."""
    if t.dtype == torch.bfloat16:
        return "_bf16"
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32 or bfloat16, got {t.dtype}")
    return ""


def project_fwd(x, lin_w, terms, wide: bool = False):
    """x[B,n,w] -> xlin[B*n,d], s_i[B*n], s_j[B*n]  (models/graph_layer.py:56 + logit scalars).
    bfloat16 x gives bfloat16 xlin (bf16 storage).  `wide`: the fp32 row-gather kernels at every shape (inputs
    beyond the 16-bit operand range of the matrix-core kernels, include/gdn_hip.h "range guard")."""
    sfx = _storage(x, "x")
    if wide and not sfx:
        sfx = "_wide"
    x = _chk(x, x.dtype, name="x")
    lin_w = _chk(lin_w.detach(), name="lin.weight")
    b, n, w = x.shape
    d = lin_w.shape[0]
    xlin = torch.empty((b * n, d), dtype=x.dtype, device=x.device)
    s_i = torch.empty((b * n,), dtype=torch.float32, device=x.device)
    s_j = torch.empty_like(s_i)
    _lib.call("gdn_project_fwd" + sfx, _ptr(x), _ptr(lin_w), _ptr(terms), b, n, w, d,
              _ptr(xlin), _ptr(s_i), _ptr(s_j), _stream())
    return xlin, s_i, s_j


def attn_aggregate_fwd(xlin, s_i, s_j, graph: SensorGraph, bias, batch: int, want_alpha: bool, wide: bool = False):
    """models/graph_layer.py:65-74,82-117 -> z[B*n,d] (+ dense alpha[B*n,pitch]).  Without alpha the lists come
    from the bank-ordered copy of the graph (same z; alpha, when asked for, is in rank order as documented)."""
    sfx = _storage(xlin, "xlin")
    if wide and not sfx:
        sfx = "_wide"
    xlin = _chk(xlin, xlin.dtype, name="xlin")
    bn, d = xlin.shape
    n = bn // batch
    z = torch.empty_like(xlin)
    alpha = torch.empty((bn, graph.pitch), dtype=torch.float32, device=xlin.device) if want_alpha else None
    flags = _lib.ROUTE_BF16 if sfx == "_bf16" else _lib.ROUTE_WIDE if wide else 0
    dense = _lib.family(_lib.STAGE_AGGREGATE, n, 1, d, graph.k, flags) == _lib.FAMILY_DENSE
    nbr = graph.nbr_ordered() if dense and not want_alpha else graph.nbr
    _lib.call("gdn_attn_aggregate_fwd" + sfx, _ptr(xlin), _ptr(_chk(s_i)), _ptr(_chk(s_j)), _ptr(nbr),
              _ptr(graph.deg), _ptr(_chk(bias.detach())), batch, n, d, graph.k, _ptr(z), _ptr(alpha), _stream())
    return z, alpha


def head_fwd(z, emb, bn1_affine, bn2_affine, out_w, out_b, batch: int, want_h2: bool = False):
    """Eval head: models/GDN.py:77-79,175-184 with out_layer_num == 1."""
    sfx = _storage(z, "z")
    z = _chk(z, z.dtype, name="z")
    bn, d = z.shape
    n = bn // batch
    out = torch.empty((batch, n), dtype=torch.float32, device=z.device)
    h2 = torch.empty((bn, d), dtype=torch.float32, device=z.device) if want_h2 else None
    _lib.call("gdn_head_fwd" + sfx, _ptr(z), _ptr(_chk(emb.detach())), _ptr(bn1_affine), _ptr(bn2_affine),
              _ptr(_chk(out_w.detach().reshape(-1))), _ptr(_chk(out_b.detach().reshape(-1))),
              batch, n, d, _ptr(out), _ptr(h2), _stream())
    return out, h2


def mlp_plan(out_layer, d_in: int):
    """Plan of the eval-mode OutLayer MLP (include/gdn_hip.h "OutLayer MLP"): (plan, hidden, layers), or None
    when the configuration is outside what gdn_mlp_fwd takes (hidden > 256)."""
    mods = list(out_layer.mlp)
    linears = [m for m in mods if isinstance(m, torch.nn.Linear)]
    bns = [m for m in mods if isinstance(m, torch.nn.BatchNorm1d)]
    layers = len(linears)
    if layers < 2 or any(not b.track_running_stats or not b.affine for b in bns):
        return None
    hidden = linears[0].out_features
    nbytes = _lib.load().gdn_mlp_plan_bytes(d_in, hidden, layers)
    if nbytes == 0:
        return None
    dev = linears[0].weight.device
    plan = torch.empty(((nbytes + 3) // 4,), dtype=torch.int32, device=dev)
    for i, (lin, bn) in enumerate(zip(linears[:-1], bns)):
        _lib.call("gdn_mlp_plan_layer", _ptr(_chk(lin.weight.detach())), _ptr(_chk(lin.bias.detach())),
                  _ptr(_chk(bn.weight.detach())), _ptr(_chk(bn.bias.detach())), _ptr(_chk(bn.running_mean)),
                  _ptr(_chk(bn.running_var)), float(bn.eps), d_in, hidden, layers, i, _ptr(plan), _stream())
    last = linears[-1]
    _lib.call("gdn_mlp_plan_out", _ptr(_chk(last.weight.detach().reshape(-1))), _ptr(_chk(last.bias.detach().reshape(-1))),
              d_in, hidden, layers, _ptr(plan), _stream())
    return plan, hidden, layers


def mlp_fwd(h2, plan_info, out: torch.Tensor | None = None):
    """h2[rows, d] -> out[rows]: OutLayer.forward (models/GDN.py:45-56) in eval mode."""
    plan, hidden, layers = plan_info
    h2 = _chk(h2, name="h2")
    rows, d_in = h2.shape
    if out is None:
        out = torch.empty((rows,), dtype=torch.float32, device=h2.device)
    _lib.call("gdn_mlp_fwd", _ptr(h2), _ptr(plan), rows, d_in, hidden, layers, _ptr(out), _stream())
    return out


def head_mlp_fwd(z, emb, bn1_affine, bn2_affine, plan_info, batch: int, out: torch.Tensor | None = None):
    """z[batch * n, d] -> out[batch * n]: the eval head (models/GDN.py:77-79,175-180) and the OutLayer MLP
    (:45-56) as one launch (gdn_head_mlp_fwd): the bits of mlp_fwd(head_fwd(z, ..., want_h2=True)[1]) without h2."""
    plan, hidden, layers = plan_info
    z = _chk(z, name="z")
    rows, d = z.shape
    if out is None:
        out = torch.empty((rows,), dtype=torch.float32, device=z.device)
    _lib.call("gdn_head_mlp_fwd", _ptr(z), _ptr(_chk(emb.detach())), _ptr(bn1_affine), _ptr(bn2_affine), _ptr(plan),
              batch, rows // batch, d, hidden, layers, _ptr(out), _stream())
    return out


def _bn_running(bn):
    """(momentum, running_mean, running_var, num_batches_tracked) pointers for the train-mode head."""
    if not bn.track_running_stats or bn.running_mean is None:
        return 0.0, None, None, None
    if bn.momentum is None:
        raise NotImplementedError("BatchNorm momentum=None (cumulative average) is not implemented")
    return float(bn.momentum), bn.running_mean, bn.running_var, bn.num_batches_tracked


def _mask_args(mask, numel: int, scale: float):
    """(fp32 multiplier pointer, byte keep-mask pointer, scale) for the train-mode head."""
    if mask is None:
        return None, None, 1.0
    if mask.numel() != numel:
        raise ValueError("dropout mask must have batch*n*d elements")
    if mask.dtype == torch.uint8:
        return None, _ptr(_chk(mask, dtype=torch.uint8, name="dropout keep mask")), float(scale)
    return _ptr(_chk(mask, name="dropout mask")), None, 1.0


def head_train_fwd(z, emb, bn1, bn2, lin_w, lin_b, mask, batch: int, mask_scale: float = 1.0):
    """Train-mode head (models/GDN.py:77-79,175-184, out_layer_num == 1): returns (out[B,n], stats).
    `mask`: fp32 multipliers [B*n, d] (0 or 1/(1-p)), or a uint8 keep mask (1/0) with `mask_scale` =
    1/(1-p), or None.  Updates the running statistics of the BatchNorm modules `bn1`, `bn2` in place."""
    z = _chk(z, name="z")
    bn, d = z.shape
    n = bn // batch
    out = torch.empty((batch, n), dtype=torch.float32, device=z.device)
    stats = torch.empty((_lib.load().gdn_head_train_stats_bytes(d) // 8,), dtype=torch.float64, device=z.device)
    mptr, kptr, kscale = _mask_args(mask, z.numel(), mask_scale)
    m1, rm1, rv1, nb1 = _bn_running(bn1)
    m2, rm2, rv2, nb2 = _bn_running(bn2)
    _lib.call("gdn_head_train_fwd", _ptr(z), _ptr(_chk(emb.detach())), _ptr(_chk(bn1.weight.detach())),
              _ptr(_chk(bn1.bias.detach())), _ptr(_chk(bn2.weight.detach())), _ptr(_chk(bn2.bias.detach())),
              _ptr(_chk(lin_w.detach().reshape(-1))), _ptr(_chk(lin_b.detach().reshape(-1))), mptr, kptr, kscale,
              batch, n, d, float(bn1.eps), float(bn2.eps), m1, m2, _ptr(rm1), _ptr(rv1), _ptr(nb1),
              _ptr(rm2), _ptr(rv2), _ptr(nb2), _ptr(stats), _ptr(out), _stream())
    return out, stats


def head_train_bwd(d_out, z, emb, bn1_w, bn1_b, bn2_w, bn2_b, lin_w, mask, stats, eps1: float, eps2: float,
                   batch: int, mask_scale: float = 1.0):
    """Gradients of head_train_fwd: (d_z, d_emb, d_bn1_w, d_bn1_b, d_bn2_w, d_bn2_b, d_lin_w, d_lin_b)."""
    d_out = _chk(d_out, name="d_out")
    bn, d = z.shape
    n = bn // batch
    dev = z.device
    ws = torch.empty((_lib.load().gdn_head_train_workspace_bytes(n, d) // 8,), dtype=torch.float64, device=dev)
    d_z = torch.empty_like(z)
    d_emb = torch.empty((n, d), dtype=torch.float32, device=dev)
    small = torch.empty((5 * d + 1,), dtype=torch.float32, device=dev)
    g1w, g1b, g2w, g2b, glw = (small[i * d:(i + 1) * d] for i in range(5))
    glb = small[5 * d:]
    mptr, kptr, kscale = _mask_args(mask, z.numel(), mask_scale)
    _lib.call("gdn_head_train_bwd", _ptr(d_out), _ptr(z), _ptr(_chk(emb)), _ptr(_chk(bn1_w)), _ptr(_chk(bn1_b)),
              _ptr(_chk(bn2_w)), _ptr(_chk(bn2_b)), _ptr(_chk(lin_w.reshape(-1))), mptr, kptr, kscale, _ptr(stats),
              batch, n, d, eps1, eps2, _ptr(ws), _ptr(d_z), _ptr(d_emb), _ptr(g1w), _ptr(g1b), _ptr(g2w),
              _ptr(g2b), _ptr(glw), _ptr(glb), _stream())
    return d_z, d_emb, g1w, g1b, g2w, g2b, glw, glb


def head_train_fwd_act(z, emb, bn1, bn2, mask, batch: int, mask_scale: float = 1.0):
    """Train-mode head in front of an OutLayer MLP (out_layer_num > 1): the passes of head_train_fwd ending at
    the [B*n, d] activation after dropout (models/GDN.py:182) instead of the fused Linear(d->1).
    Returns (act, stats)."""
    z = _chk(z, name="z")
    bn, d = z.shape
    n = bn // batch
    act = torch.empty_like(z)
    stats = torch.empty((_lib.load().gdn_head_train_stats_bytes(d) // 8,), dtype=torch.float64, device=z.device)
    mptr, kptr, kscale = _mask_args(mask, z.numel(), mask_scale)
    m1, rm1, rv1, nb1 = _bn_running(bn1)
    m2, rm2, rv2, nb2 = _bn_running(bn2)
    _lib.call("gdn_head_train_fwd_act", _ptr(z), _ptr(_chk(emb.detach())), _ptr(_chk(bn1.weight.detach())),
              _ptr(_chk(bn1.bias.detach())), _ptr(_chk(bn2.weight.detach())), _ptr(_chk(bn2.bias.detach())),
              mptr, kptr, kscale, None, 0.0, batch, n, d, float(bn1.eps), float(bn2.eps), m1, m2, _ptr(rm1), _ptr(rv1),
              _ptr(nb1), _ptr(rm2), _ptr(rv2), _ptr(nb2), _ptr(stats), _ptr(act), 0, _stream())
    return act, stats


def head_train_bwd_act(d_act, z, emb, bn1_w, bn1_b, bn2_w, bn2_b, mask, stats, eps1: float, eps2: float,
                       batch: int, mask_scale: float = 1.0):
    """Gradients of head_train_fwd_act: (d_z, d_emb, d_bn1_w, d_bn1_b, d_bn2_w, d_bn2_b)."""
    d_act = _chk(d_act, name="d_act")
    bn, d = z.shape
    n = bn // batch
    dev = z.device
    ws = torch.empty((_lib.load().gdn_head_train_workspace_bytes(n, d) // 8,), dtype=torch.float64, device=dev)
    d_z = torch.empty_like(z)
    d_emb = torch.empty((n, d), dtype=torch.float32, device=dev)
    small = torch.empty((4 * d,), dtype=torch.float32, device=dev)
    g1w, g1b, g2w, g2b = (small[i * d:(i + 1) * d] for i in range(4))
    mptr, kptr, kscale = _mask_args(mask, z.numel(), mask_scale)
    _lib.call("gdn_head_train_bwd_act", _ptr(d_act), _ptr(z), _ptr(_chk(emb)), _ptr(_chk(bn1_w)), _ptr(_chk(bn1_b)),
              _ptr(_chk(bn2_w)), _ptr(_chk(bn2_b)), mptr, kptr, kscale, None, 0.0, _ptr(stats), batch, n, d, eps1, eps2,
              _ptr(ws), _ptr(d_z), _ptr(d_emb), _ptr(g1w), _ptr(g1b), _ptr(g2w), _ptr(g2b), 0, _stream())
    return d_z, d_emb, g1w, g1b, g2w, g2b


def _ptr_array(tensors):
    """Host array of device pointers (None -> null) for the entry points that take one per layer."""
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def mlp_train_layers(out_layer):
    """[(Linear, BatchNorm1d), ...] of the hidden layers and the final Linear of a reference OutLayer
    (models/GDN.py:27-45), or None when its structure is not that."""
    mods = list(out_layer.mlp)
    if len(mods) < 4 or (len(mods) - 1) % 3 != 0:
        return None
    hidden = []
    for i in range(0, len(mods) - 1, 3):
        lin, bn, act = mods[i], mods[i + 1], mods[i + 2]
        if not (isinstance(lin, torch.nn.Linear) and isinstance(bn, torch.nn.BatchNorm1d) and
                isinstance(act, torch.nn.ReLU) and lin.bias is not None and bn.affine):
            return None
        if bn.track_running_stats and bn.momentum is None:
            return None
        hidden.append((lin, bn))
    last = mods[-1]
    if not isinstance(last, torch.nn.Linear) or last.out_features != 1 or last.bias is None:
        return None
    return hidden, last


def mlp_train_supported(out_layer, d_in: int, rows: int) -> bool:
    """True when gdn_mlp_train_fwd/bwd take this OutLayer: 2..8 layers, d_in (<= 256) a multiple of 4, hidden
    1..512, every hidden layer of the same width."""
    parts = mlp_train_layers(out_layer)
    if parts is None:
        return False
    hidden, _last = parts
    h = hidden[0][0].out_features
    if any(lin.out_features != h for lin, _ in hidden) or hidden[0][0].in_features != d_in:
        return False
    return _lib.load().gdn_mlp_train_saved_bytes(rows, d_in, h, len(hidden) + 1) > 0


def mlp_eval_wide_supported(out_layer, d_in: int) -> bool:
    """True when gdn_mlp_eval_fwd takes this OutLayer (eval mode, hidden up to 512, running
    statistics tracked): the path for widths beyond the one-launch chain (mlp_plan / mlp_fwd: hidden <= 256)."""
    parts = mlp_train_layers(out_layer)
    if parts is None:
        return False
    hidden, _last = parts
    h = hidden[0][0].out_features
    if any(lin.out_features != h for lin, _ in hidden) or hidden[0][0].in_features != d_in:
        return False
    if any(bn.running_mean is None or not bn.track_running_stats for _lin, bn in hidden):
        return False
    return _lib.load().gdn_mlp_eval_workspace_bytes(2, d_in, h, len(hidden) + 1) > 0


def mlp_fast_tail_supported(out_layer, d_in: int) -> bool:
    """True when one of the two eval tails takes this OutLayer (mlp_plan or mlp_eval_wide_supported), decided from the
    module's configuration and the library's size queries alone: no tensor is touched, no device is needed."""
    linears = [m for m in out_layer.mlp if isinstance(m, torch.nn.Linear)]
    bns = [m for m in out_layer.mlp if isinstance(m, torch.nn.BatchNorm1d)]
    planned = (len(linears) >= 2 and all(b.track_running_stats and b.affine for b in bns)
               and _lib.load().gdn_mlp_plan_bytes(d_in, linears[0].out_features, len(linears)) != 0)
    return planned or mlp_eval_wide_supported(out_layer, d_in)


def mlp_eval_wide_workspace(out_layer, rows: int, d_in: int, device) -> torch.Tensor:
    """Scratch of mlp_eval_wide for `rows` rows (gdn_mlp_eval_workspace_bytes): callers that run the same shape
    again and again keep it and pass it as `ws=`."""
    hidden, _last = mlp_train_layers(out_layer)
    nbytes = _lib.load().gdn_mlp_eval_workspace_bytes(rows, d_in, hidden[0][0].out_features, len(hidden) + 1)
    return torch.empty((nbytes,), dtype=torch.uint8, device=device)


def mlp_eval_wide(h2, out_layer, out: torch.Tensor | None = None, ws: torch.Tensor | None = None):
    """h2[rows, d] -> out[rows]: OutLayer.forward (models/GDN.py:45-56) in eval mode on the fp32 matrix-core GEMM
    kernels (gdn_mlp_eval_fwd).  `ws`: a workspace from mlp_eval_wide_workspace (allocated per call when None)."""
    h2 = _chk(h2, name="h2")
    rows, d_in = h2.shape
    hidden, last = mlp_train_layers(out_layer)
    h, layers = hidden[0][0].out_features, len(hidden) + 1
    if ws is None:
        ws = mlp_eval_wide_workspace(out_layer, rows, d_in, h2.device)
    if out is None:
        out = torch.empty((rows,), dtype=torch.float32, device=h2.device)
    params, running, eps = [], [], []
    for lin, bn in hidden:
        params += [_chk(lin.weight.detach()), _chk(lin.bias.detach()), _chk(bn.weight.detach()), _chk(bn.bias.detach())]
        running += [_chk(bn.running_mean), _chk(bn.running_var)]
        eps.append(float(bn.eps))
    _lib.call("gdn_mlp_eval_fwd", _ptr(h2), _ptr_array(params), _ptr_array(running), (ctypes.c_float * len(eps))(*eps),
              _ptr(_chk(last.weight.detach().reshape(-1))), _ptr(_chk(last.bias.detach().reshape(-1))),
              rows, d_in, h, layers, _ptr(ws), _ptr(out), _stream())
    return out


def mlp_train_fwd(act, out_layer):
    """Train-mode OutLayer MLP forward (models/GDN.py:47-56 under model.train(): Linear, batch-statistics
    BatchNorm, ReLU per hidden layer, then Linear(hidden->1)).  Returns (out[rows], saved); updates the
    BatchNorm running statistics in place."""
    act = _chk(act, name="act")
    rows, d_in = act.shape
    hidden, last = mlp_train_layers(out_layer)
    h, layers = hidden[0][0].out_features, len(hidden) + 1
    lib = _lib.load()
    saved = torch.empty((lib.gdn_mlp_train_saved_bytes(rows, d_in, h, layers),), dtype=torch.uint8, device=act.device)
    ws = torch.empty((lib.gdn_mlp_train_workspace_bytes(rows, d_in, h, layers),), dtype=torch.uint8, device=act.device)
    out = torch.empty((rows,), dtype=torch.float32, device=act.device)
    params, running, batches, eps, mom = [], [], [], [], []
    for lin, bn in hidden:
        params += [_chk(lin.weight.detach()), _chk(lin.bias.detach()), _chk(bn.weight.detach()), _chk(bn.bias.detach())]
        m, rm, rv, nb = _bn_running(bn)
        running += [rm, rv]
        batches.append(nb)
        eps.append(float(bn.eps))
        mom.append(m)
    _lib.call("gdn_mlp_train_fwd", _ptr(act), _ptr_array(params), _ptr_array(running), _ptr_array(batches),
              (ctypes.c_float * len(eps))(*eps), (ctypes.c_float * len(mom))(*mom),
              _ptr(_chk(last.weight.detach().reshape(-1))), _ptr(_chk(last.bias.detach().reshape(-1))),
              rows, d_in, h, layers, _ptr(saved), _ptr(ws), _ptr(out), _stream())
    return out, saved


def mlp_train_bwd(d_out, act, params, out_w, saved, d_in: int, hidden: int, layers: int):
    """Gradients of mlp_train_fwd.  `params` = [W, b, gamma, beta] * (layers-1).  Returns
    (d_act, [dW, db, dgamma, dbeta] * (layers-1), d_out_w[hidden], d_out_b[1])."""
    d_out = _chk(d_out.reshape(-1), name="d_out")
    rows = act.shape[0]
    dev = act.device
    ws = torch.empty((_lib.load().gdn_mlp_train_workspace_bytes(rows, d_in, hidden, layers),), dtype=torch.uint8, device=dev)
    grads = []
    for l in range(layers - 1):
        k = d_in if l == 0 else hidden
        grads += [torch.empty((hidden, k), dtype=torch.float32, device=dev)] + \
                 [torch.empty((hidden,), dtype=torch.float32, device=dev) for _ in range(3)]
    d_ow = torch.empty((hidden,), dtype=torch.float32, device=dev)
    d_ob = torch.empty((1,), dtype=torch.float32, device=dev)
    d_act = torch.empty_like(act)
    _lib.call("gdn_mlp_train_bwd", _ptr(d_out), _ptr(act), _ptr_array([_chk(p) for p in params]),
              _ptr(_chk(out_w.reshape(-1))), rows, d_in, hidden, layers, _ptr(saved), _ptr(ws), _ptr_array(grads),
              _ptr(d_ow), _ptr(d_ob), _ptr(d_act), _stream())
    return d_act, grads, d_ow, d_ob


def forward_fused(x, lin_w, terms, graph: SensorGraph, gnn_bias, emb, bn1_affine, bn2_affine, out_w, out_b,
                  out: torch.Tensor | None = None):
    """One launch from x[B,n,w] to out[B,n]: models/GDN.py:122-187 under model.eval().
    bfloat16 x selects the bf16-storage kernel."""
    sfx = _storage(x, "x")
    x = _chk(x, x.dtype, name="x")
    b, n, w = x.shape
    lin_w = _chk(lin_w.detach(), name="lin.weight")
    d = lin_w.shape[0]
    if out is None:
        out = torch.empty((b, n), dtype=torch.float32, device=x.device)
    _lib.call("gdn_forward_fused" + sfx, _ptr(x), _ptr(lin_w), _ptr(terms), _ptr(graph.nbr), _ptr(graph.deg),
              _ptr(_chk(gnn_bias.detach())), _ptr(_chk(emb.detach())), _ptr(bn1_affine), _ptr(bn2_affine),
              _ptr(_chk(out_w.detach().reshape(-1))), _ptr(_chk(out_b.detach().reshape(-1))),
              b, n, w, d, graph.k, _ptr(out), _stream())
    return out


def fused_plan(lin_w, terms, graph: SensorGraph, gnn_bias, emb, bn1_affine, bn2_affine, out_w, out_b,
               bf16_storage: bool = False):
    """Per-launch constants of the fused forward, precomputed (include/gdn_hip.h "plans"); None when the
    shape is not on the matrix-core path.  Rebuild after every parameter update."""
    lin_w = _chk(lin_w.detach(), name="lin.weight")
    d, w = lin_w.shape
    n = emb.shape[0]
    nbytes = _lib.load().gdn_fused_plan_bytes(n, w, d, graph.k, int(bf16_storage))
    if nbytes == 0 or _lib.family(_lib.STAGE_FUSED, n, w, d, graph.k) != _lib.FAMILY_DENSE:   # (GDN_FUSED_PATH=valu)
        return None
    plan = torch.empty(((nbytes + 3) // 4,), dtype=torch.int32, device=emb.device)
    _lib.call("gdn_fused_plan_build", _ptr(lin_w), _ptr(terms), _ptr(graph.nbr), _ptr(graph.deg),
              _ptr(_chk(gnn_bias.detach())), _ptr(_chk(emb.detach())), _ptr(bn1_affine), _ptr(bn2_affine),
              _ptr(_chk(out_w.detach().reshape(-1))), _ptr(_chk(out_b.detach().reshape(-1))),
              n, w, d, graph.k, int(bf16_storage), _ptr(plan), _stream())
    return plan


def fused_plan_limit(plan: torch.Tensor, n: int, w: int, d: int, k: int, bf16_storage: bool = False) -> torch.Tensor:
    """The plan's x limit (include/gdn_hip.h "range guard") as a 0-d float32 DEVICE tensor (a view of the plan:
    reading it on the host is a synchronisation, done once per resident series)."""
    off = _lib.load().gdn_fused_plan_limit_offset(n, w, d, k, int(bf16_storage))
    return plan[off // 4].view(torch.float32)


def forward_fused_series(series, first: int, batch: int, w: int, lin_w, terms, graph: SensorGraph, gnn_bias, emb,
                         bn1_affine, bn2_affine, out_w, out_b, out: torch.Tensor | None = None):
    """Fused eval forward of `batch` stride-1 windows read straight from series[n, T]
    (datasets/TimeDataset.py:46-49 without the w-fold copy)."""
    series = _chk(series, name="series")
    n, t_len = series.shape
    lin_w = _chk(lin_w.detach(), name="lin.weight")
    d = lin_w.shape[0]
    if out is None:
        out = torch.empty((batch, n), dtype=torch.float32, device=series.device)
    _lib.call("gdn_forward_fused_series", _ptr(series), t_len, first, _ptr(lin_w), _ptr(terms), _ptr(graph.nbr),
              _ptr(graph.deg), _ptr(_chk(gnn_bias.detach())), _ptr(_chk(emb.detach())), _ptr(bn1_affine),
              _ptr(bn2_affine), _ptr(_chk(out_w.detach().reshape(-1))), _ptr(_chk(out_b.detach().reshape(-1))),
              batch, n, w, d, graph.k, _ptr(out), _stream())
    return out


def attn_aggregate_bwd(d_z, xlin, alpha, s_i, s_j, graph: SensorGraph, batch: int, wide: bool = False):
    """Gradient of attn_aggregate_fwd w.r.t. xlin, s_i, s_j and bias."""
    d_z = _chk(d_z, name="d_z")
    bn, d = d_z.shape
    n = bn // batch
    d_xlin = torch.empty_like(d_z)
    d_si = torch.empty((bn,), dtype=torch.float32, device=d_z.device)
    d_sj = torch.empty_like(d_si)
    d_bias = torch.empty((d,), dtype=torch.float32, device=d_z.device)
    # the matrix-core backward (n <= 127, d = 64) does not read the reverse lists: they are not even built then
    rent, rlen = graph.reverse() if wide or _lib.load().gdn_attn_aggregate_bwd_uses_reverse(n, d, graph.k) else (None, None)
    # [ticket, zero on entry | d_bias partial rows | d_pi tables when they exceed LDS]: a fresh one per call, so
    # calls on different streams never share a ticket (NativeTrainStep owns one for its stream instead)
    nbytes = _lib.load().gdn_attn_aggregate_bwd_workspace_bytes(batch, n, d, graph.k)
    ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=d_z.device)
    ws[:4].zero_()
    _lib.call("gdn_attn_aggregate_bwd_wide" if wide else "gdn_attn_aggregate_bwd", _ptr(d_z), _ptr(_chk(xlin)),
              _ptr(_chk(alpha)), _ptr(_chk(s_i)),
              _ptr(_chk(s_j)), _ptr(graph.nbr), _ptr(rent), _ptr(rlen), batch, n, d, graph.k,
              _ptr(d_xlin), _ptr(d_si), _ptr(d_sj), _ptr(d_bias), _ptr(ws), _stream())
    return d_xlin, d_si, d_sj, d_bias


def project_bwd(x, d_xlin, d_si, d_sj, d: int):
    """Gradients of project_fwd: d_lin_w[d,w] (direct term), d_a[2,P] (P = terms_pitch(w)), d_c[2,n]."""
    x = _chk(x, name="x")
    b, n, w = x.shape
    ws = torch.empty((_lib.load().gdn_project_bwd_workspace_bytes(n, w, d) // 4,), dtype=torch.float32,
                     device=x.device)
    ap = terms_pitch(w)
    flat = torch.empty((d * w + 2 * ap + 2 * n,), dtype=torch.float32, device=x.device)
    d_lin_w, d_a, d_c = (flat[:d * w].view(d, w), flat[d * w:d * w + 2 * ap].view(2, ap),
                         flat[d * w + 2 * ap:].view(2, n))
    _lib.call("gdn_project_bwd", _ptr(x), _ptr(_chk(d_xlin)), _ptr(_chk(d_si)), _ptr(_chk(d_sj)),
              b, n, w, d, _ptr(ws), _ptr(d_lin_w), _ptr(d_a), _ptr(d_c), _stream())
    return d_lin_w, d_a, d_c


def mse_workspace(device) -> torch.Tensor:
    """Zeroed scratch for mse_loss_grad; allocate once and reuse (every call leaves it zeroed)."""
    return torch.zeros((_lib.load().gdn_mse_workspace_bytes() // 8,), dtype=torch.float64, device=device)


def mse_loss_grad(out, y, workspace, loss=None, d_out=None, valid=None, row_valid=None, m_out=None):
    """(loss, d_out): F.mse_loss(out, y, reduction='mean') (train.py:20-23) and d loss / d out.
    With `valid` [batch, n] uint8 and `row_valid` [batch] int32 (windows_gather's validity outputs) the mean runs over
    the observed targets only (gdn_mse_loss_grad_masked): d_out is exactly 0.0 at a masked target, whatever out / y
    hold there; no observed target: loss 0, d_out zeros.  `m_out`: optional int64 [] that receives their number."""
    out, y = _chk(out, name="out"), _chk(y, name="y")
    if out.shape != y.shape:
        raise ValueError(f"shape mismatch: {tuple(out.shape)} vs {tuple(y.shape)}")
    if loss is None:
        loss = torch.empty((), dtype=torch.float32, device=out.device)
    if d_out is None:
        d_out = torch.empty_like(out)
    if valid is None:
        if row_valid is not None or m_out is not None:
            raise ValueError("row_valid / m_out belong to the masked loss: give valid as well")
        _lib.call("gdn_mse_loss_grad", _ptr(out), _ptr(y), out.numel(), _ptr(workspace), _ptr(loss), _ptr(d_out),
                  _stream())
        return loss, d_out
    if out.dim() != 2:
        raise ValueError(f"the masked loss takes out / y [batch, n], got {tuple(out.shape)}")
    batch, n = out.shape
    valid = _valid_plane(valid, (batch, n), "valid")
    if row_valid is None:
        raise ValueError("valid needs row_valid [batch] int32, the per-window counts of the same gather")
    row_valid = _chk(row_valid, torch.int32, name="row_valid")
    if row_valid.numel() != batch:
        raise ValueError(f"row_valid: expected {batch} int32 counts, got {tuple(row_valid.shape)}")
    if m_out is not None:
        m_out = _chk(m_out, torch.int64, name="m_out")
    _lib.call("gdn_mse_loss_grad_masked", _ptr(out), _ptr(y), _ptr(valid), _ptr(row_valid), batch, n, _ptr(workspace),
              _ptr(loss), _ptr(d_out), _ptr(m_out), _stream())
    return loss, d_out


def terms_bwd(lin_w, att_i, att_j, att_em_i, att_em_j, emb, d_lin_w, d_a, d_c):
    """Chain rule through node_terms; d_lin_w (the direct term from project_bwd) is completed in place.
    Returns (d_lin_w, d_att_i, d_att_j, d_att_em_i, d_att_em_j, d_emb)."""
    d, w = lin_w.shape
    n = emb.shape[0]
    small = torch.empty((4 * d,), dtype=torch.float32, device=emb.device)
    d_emb = torch.empty((n, d), dtype=torch.float32, device=emb.device)
    _lib.call("gdn_terms_bwd", _ptr(_chk(lin_w)), _ptr(_chk(att_i)), _ptr(_chk(att_j)), _ptr(_chk(att_em_i)),
              _ptr(_chk(att_em_j)), _ptr(_chk(emb)), _ptr(d_a), _ptr(d_c), n, d, w, _ptr(d_lin_w),
              _ptr(small), _ptr(small[d:]), _ptr(small[2 * d:]), _ptr(small[3 * d:]), _ptr(d_emb), _stream())
    return (d_lin_w, small[:d].view_as(att_i), small[d:2 * d].view_as(att_j), small[2 * d:3 * d].view_as(att_em_i),
            small[3 * d:].view_as(att_em_j), d_emb)


def score_workspace(t: int, n: int, device) -> torch.Tensor:
    nbytes = _lib.load().gdn_score_workspace_bytes(t, n)
    return torch.empty(((nbytes + 7) // 8,), dtype=torch.float64, device=device)


def score_keys(pred, gt, pitch: int, out: torch.Tensor | None = None, keep=None, valid=None) -> torch.Tensor:
    """keys[n, pitch] float64 = |pred-gt| transposed (radix keys); slots t..pitch-1 = filler.  With `keep` [t] uint8
    (gdn_score_keys_keep) the filler is also in all n keys of every tick whose flag is 0; with `valid` [t, n] uint8
    (gdn_score_keys_valid) in the key of every (tick, sensor) whose byte is 0.  One of the two at the most."""
    pred, gt = _chk(pred, name="pred"), _chk(gt, name="gt")
    t, n = pred.shape
    if keep is not None and valid is not None:
        raise ValueError("score_keys: keep (whole ticks) and valid (single readings) exclude each other")
    if keep is not None:
        keep = _chk(keep, torch.uint8, "keep")
        if keep.numel() != t:
            raise ValueError(f"keep: one flag per tick is needed ({t}), got {keep.numel()}")
    if valid is not None:
        valid = _valid_plane(valid, pred.shape, "valid")
    keys = out if out is not None else torch.empty((n, pitch), dtype=torch.float64, device=pred.device)
    if keys.shape != (n, pitch) or keys.dtype != torch.float64 or not keys.is_contiguous():
        raise ValueError("keys buffer must be a contiguous float64 [n, pitch] tensor")
    if valid is not None:
        _lib.call("gdn_score_keys_valid", _ptr(pred), _ptr(gt), _ptr(valid), t, n, pitch, _ptr(keys), _stream())
    elif keep is None:
        _lib.call("gdn_score_keys", _ptr(pred), _ptr(gt), t, n, pitch, _ptr(keys), _stream())
    else:
        _lib.call("gdn_score_keys_keep", _ptr(pred), _ptr(gt), _ptr(keep), t, n, pitch, _ptr(keys), _stream())
    return keys


def score_select_workspace(blocks: int, n: int, pitch: int, device) -> torch.Tensor:
    nbytes = _lib.load().gdn_score_select_workspace_bytes(blocks, n, pitch)
    return torch.empty(((nbytes + 7) // 8,), dtype=torch.float64, device=device)


def score_select(keys, blocks: int, n: int, pitch: int, total: int, ws: torch.Tensor | None = None,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """Median / IQR per sensor over keys[blocks, n, pitch] holding `total` real keys per sensor.
    `ws` (score_select_workspace) and `out` [n, 2] float64 may be preallocated (no allocation per call)."""
    keys = _chk(keys, torch.float64, "keys")
    if ws is None:
        ws = score_select_workspace(blocks, n, pitch, keys.device)
    if out is None:
        out = torch.empty((n, 2), dtype=torch.float64, device=keys.device)
    _lib.call("gdn_score_select", _ptr(keys), blocks, n, pitch, total, _ptr(ws), _ptr(out), _stream())
    return out


def score_select_paths(keys, blocks: int, n: int, pitch: int, total: int):
    """score_select plus, per sensor, the path that settled its ranks: 0 = sample brackets of the one-workgroup
    select, 1 = digit passes (gdn_score_select_paths).  Returns (med_iqr[n, 2], path[n] int32)."""
    keys = _chk(keys, torch.float64, "keys")
    ws = score_select_workspace(blocks, n, pitch, keys.device)
    out = torch.empty((n, 2), dtype=torch.float64, device=keys.device)
    path = torch.full((n,), -1, dtype=torch.int32, device=keys.device)
    _lib.call("gdn_score_select_paths", _ptr(keys), blocks, n, pitch, total, _ptr(ws), _ptr(out), _ptr(path), _stream())
    return out, path


def score_key_counts(keys, blocks: int, n: int, pitch: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """counts[n] int32: per sensor, the slots of keys[blocks, n, pitch] that do not hold the filler
    (gdn_score_key_counts).  `out` may be a preallocated int32 [n] buffer."""
    keys = _chk(keys, torch.float64, "keys")
    if keys.numel() != blocks * n * pitch:
        raise ValueError(f"keys: expected {blocks} x {n} x {pitch} slots, got {keys.numel()}")
    if out is None:
        out = torch.empty((n,), dtype=torch.int32, device=keys.device)
    out = _chk(out, torch.int32, "counts")
    if out.numel() != n:
        raise ValueError(f"counts: one entry per sensor is needed ({n}), got {out.numel()}")
    _lib.call("gdn_score_key_counts", _ptr(keys), blocks, n, pitch, _ptr(out), _stream())
    return out


def score_select_counts(keys, blocks: int, n: int, pitch: int, counts, min_count: int = 1,
                        ws: torch.Tensor | None = None, out: torch.Tensor | None = None,
                        path: torch.Tensor | None = None) -> torch.Tensor:
    """score_select where sensor s has counts[s] real keys (int32 [n] on the device; gdn_score_select_counts): ranks
    and interpolation weights are formed per sensor on the device, nothing is read back.  The row of a sensor with
    fewer than max(min_count, 1) real keys is left as it is: pass `out` to decide what such a row holds (a fresh one
    is filled with NaN).  `path` (int32 [n]) takes the path per sensor as score_select_paths reports it."""
    keys = _chk(keys, torch.float64, "keys")
    counts = _chk(counts, torch.int32, "counts")
    if counts.numel() != n:
        raise ValueError(f"counts: one entry per sensor is needed ({n}), got {counts.numel()}")
    if ws is None:
        ws = score_select_workspace(blocks, n, pitch, keys.device)
    if out is None:
        out = torch.full((n, 2), float("nan"), dtype=torch.float64, device=keys.device)
    out = _chk(out, torch.float64, "med_iqr")
    if out.numel() != 2 * n:
        raise ValueError(f"med_iqr: expected [{n}, 2], got {tuple(out.shape)}")
    if path is not None:
        path = _chk(path, torch.int32, "path")
        if path.numel() != n:
            raise ValueError(f"path: one entry per sensor is needed ({n}), got {path.numel()}")
    _lib.call("gdn_score_select_counts", _ptr(keys), blocks, n, pitch, _ptr(counts), int(min_count), _ptr(ws),
              _ptr(out), _ptr(path), _stream())
    return out


def score_quantiles(pred, gt):
    """Per-sensor median and IQR of |pred-gt| over all ticks (util/data.py:75-82), float64.
    pred, gt: fp32 [t, n].  Returns med_iqr[n, 2]."""
    pred, gt = _chk(pred, name="pred"), _chk(gt, name="gt")
    t, n = pred.shape
    ws = score_workspace(t, n, pred.device)
    out = torch.empty((n, 2), dtype=torch.float64, device=pred.device)
    _lib.call("gdn_score_quantiles", _ptr(pred), _ptr(gt), t, n, _ptr(ws), _ptr(out), _stream())
    return out


def _valid_plane(valid, shape, name: str):
    valid = _chk(valid, torch.uint8, name)
    if tuple(valid.shape) != tuple(shape):
        raise ValueError(f"{name}: expected a uint8 plane of shape {tuple(shape)}, got {tuple(valid.shape)}")
    return valid


def _smooth_planes(pred, gt, valid, halo_valid):
    """pred, gt [t, n] fp32 and the optional validity plane `valid` [t, n] uint8 of the smooth launches, checked."""
    pred, gt = _chk(pred, name="pred"), _chk(gt, name="gt")
    if valid is not None:
        valid = _valid_plane(valid, pred.shape, "valid")
    elif halo_valid is not None:
        raise ValueError("halo_valid is the halo of the validity plane: give valid as well")
    return pred, gt, valid


def _smooth_call(name: str, pred, gt, med_iqr, first_tick: int, halo_pred, halo_gt, outputs, valid, halo_valid):
    """gdn_score_<name>, or gdn_score_<name>_gaps with (valid, halo_valid) behind the outputs when `valid` is given;
    the halos ([3, n], the three ticks before first_tick) are checked here."""
    t, n = pred.shape
    hp = None if halo_pred is None else _chk(halo_pred, name="halo_pred")
    hg = None if halo_gt is None else _chk(halo_gt, name="halo_gt")
    hv = None if halo_valid is None else _valid_plane(halo_valid, (3, n), "halo_valid")
    head = (_ptr(pred), _ptr(gt), _ptr(_chk(med_iqr, torch.float64)), t, n, first_tick, _ptr(hp), _ptr(hg), *outputs)
    if valid is None:
        _lib.call(f"gdn_score_{name}", *head, _stream())
    else:
        _lib.call(f"gdn_score_{name}_gaps", *head, _ptr(valid), _ptr(hv), _stream())


def score_smooth_max(pred, gt, med_iqr, want_scores: bool = True, first_tick: int = 0, halo_pred=None, halo_gt=None,
                     anomaly: torch.Tensor | None = None, valid=None, halo_valid=None):
    """evaluate.py:54-68 + the max over sensors of :131-139.  Returns (scores[n,t] | None, anomaly[t]);
    `anomaly` may be a preallocated float64 [t] buffer.  With the validity plane `valid` [t, n] uint8 of a filled `gt`
    (`halo_valid` [3, n] beside the halo) the normalised error of a missing reading is exactly 0.0 wherever it is used."""
    pred, gt, valid = _smooth_planes(pred, gt, valid, halo_valid)
    t, n = pred.shape
    scores = torch.empty((n, t), dtype=torch.float64, device=pred.device) if want_scores else None
    if anomaly is None:
        anomaly = torch.empty((t,), dtype=torch.float64, device=pred.device)
    _smooth_call("smooth_max", pred, gt, med_iqr, first_tick, halo_pred, halo_gt, (_ptr(scores), _ptr(anomaly)),
                 valid, halo_valid)
    return scores, anomaly


def score_smooth_topm(pred, gt, med_iqr, m: int, first_tick: int = 0, halo_pred=None, halo_gt=None,
                      top_scores: torch.Tensor | None = None, top_sensors: torch.Tensor | None = None,
                      valid=None, halo_valid=None):
    """score_smooth_max that keeps the `m` largest smoothed scores of every tick and their sensors (1 <= m <= 8,
    m <= n) instead of the maximum alone; the [n, t] table is never written.  Returns (top_scores[t, m] float64
    descending, top_sensors[t, m] int32; equal scores in ascending sensor order); both may be preallocated.
    `valid` / `halo_valid` as in score_smooth_max."""
    pred, gt, valid = _smooth_planes(pred, gt, valid, halo_valid)
    t, n = pred.shape
    if top_scores is None:
        top_scores = torch.empty((t, m), dtype=torch.float64, device=pred.device)
    if top_sensors is None:
        top_sensors = torch.empty((t, m), dtype=torch.int32, device=pred.device)
    if (top_scores.shape != (t, m) or top_scores.dtype != torch.float64 or not top_scores.is_contiguous()
            or top_sensors.shape != (t, m) or top_sensors.dtype != torch.int32 or not top_sensors.is_contiguous()):
        raise ValueError("top_scores / top_sensors must be contiguous [t, m] float64 / int32 tensors")
    _smooth_call("smooth_topm", pred, gt, med_iqr, first_tick, halo_pred, halo_gt,
                 (m, _ptr(top_scores), _ptr(top_sensors)), valid, halo_valid)
    return top_scores, top_sensors


# --------------------------------------------------------------------------- resident series with missing readings
def series_fill(raw, w: int):
    """Hold the missing readings (not finite: NaN, +inf, -inf) of `raw` [n, t_raw] fp32 at each sensor's latest earlier
    real one (gdn_series_fill; `raw` is not written, raw[:, :w] finite is the caller's duty).  Returns (filled
    [n, t_raw], gt [t, n] = filled[:, w:] time-major, valid [t, n] uint8, keep [t] uint8 = 1 where a tick is complete,
    counters [2, n] int64 = missing_total, missing_run over the t = t_raw - w scored ticks)."""
    raw = _chk(raw, name="series")
    if raw.dim() != 2:
        raise ValueError(f"expected the series [n, t_raw], got {tuple(raw.shape)}")
    n, t_raw = raw.shape
    nbytes = _lib.load().gdn_series_fill_workspace_bytes(n, t_raw)
    if nbytes <= 0 or w < 1 or t_raw <= w:
        raise _lib.GdnHipError(f"series fill: no kernel for n = {n}, t_raw = {t_raw}, w = {w} "
                               "(1 <= n <= 4096, w >= 1, t_raw > w)")
    dev, t = raw.device, t_raw - w
    ws = torch.empty((nbytes // 8,), dtype=torch.int64, device=dev)
    filled = torch.empty_like(raw)
    gt = torch.empty((t, n), dtype=torch.float32, device=dev)
    valid = torch.empty((t, n), dtype=torch.uint8, device=dev)
    keep = torch.empty((t,), dtype=torch.uint8, device=dev)
    counters = torch.empty((2, n), dtype=torch.int64, device=dev)
    _lib.call("gdn_series_fill", _ptr(raw), n, t_raw, w, _ptr(filled), _ptr(gt), _ptr(valid), _ptr(keep),
              _ptr(counters), _ptr(ws), _stream())
    return filled, gt, valid, keep, counters


def _attention_source(src: torch.Tensor, name: str) -> torch.Tensor:
    """The raw data of the attention entry points: fp32 on a HIP device.  They are fp32 throughout, so bf16 storage is
    refused by name (as CPU tensors are) instead of being converted behind the caller's back."""
    if not src.is_cuda:
        raise _lib.GdnHipError(f"{name} is on {src.device}: attention from raw data needs a HIP device (no CPU fallback)")
    if src.dtype == torch.bfloat16:
        raise _lib.GdnHipError(f"{name} is bfloat16: attention from raw data runs on fp32 storage only (bf16 storage "
                               "is not supported by gdn_attention_mean / gdn_attention_at)")
    if src.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32, got {src.dtype}")
    if src.dim() not in (2, 3):
        raise ValueError(f"{name}: expected the raw series [n, T] or windows [B, n, w], got {tuple(src.shape)}")
    return src if src.is_contiguous() else src.contiguous()


_attention_ws: dict = {}      # (device, stream) -> workspace of attention_mean, grown on demand


def _attention_workspace(nbytes: int, device) -> torch.Tensor:
    key = (device, _stream())
    ws = _attention_ws.get(key)
    if ws is None or ws.numel() * 8 < nbytes:
        ws = torch.empty(((nbytes + 7) // 8,), dtype=torch.float64, device=device)
        _attention_ws[key] = ws
    return ws


def attention_mean(src, terms, graph: SensorGraph, w: int, first: int = 0, batch: int | None = None, weights=None,
                   out: torch.Tensor | None = None) -> torch.Tensor:
    """Weighted mean of the attention rows over a run of windows, from raw data (include/gdn_hip.h "attention from
    raw data"): `src` is the raw series [n, T] (windows first .. first+batch-1, window b = columns first+b ..
    first+b+w-1) or windows [B, n, w].  weights [batch] fp32 or None (plain mean).  Returns mean[n, pitch] fp32 in
    the slot order of graph.nbr, padding 0; a weight sum that is not positive gives zeros.  Bitwise reproducible."""
    src = _attention_source(src, "series" if src.dim() == 2 else "x")
    if src.dim() == 2:
        n, t_raw = src.shape
        if batch is None:
            batch = t_raw - w + 1 - first
    else:
        if first != 0 or (batch is not None and batch != src.shape[0]):
            raise ValueError("windows [B, n, w] are averaged whole: first = 0, batch = B")
        batch, n, t_raw = src.shape[0], src.shape[1], 0
        if src.shape[2] != w:
            raise ValueError(f"windows of {src.shape[2]} ticks given to a model of window length {w}")
    if n != graph.n:
        raise ValueError(f"{n} sensors given to a graph of {graph.n}")
    if weights is not None:
        weights = _chk(weights, name="weights").reshape(-1)
        if weights.numel() != batch:
            raise ValueError(f"{weights.numel()} weights for {batch} windows")
    nbytes = _lib.load().gdn_attention_workspace_bytes(batch, n, w, graph.k)
    ws = _attention_workspace(max(nbytes, 8), src.device)
    if out is None:
        out = torch.empty((n, graph.pitch), dtype=torch.float32, device=src.device)
    _lib.call("gdn_attention_mean", _ptr(src), t_raw, first, _ptr(weights), _ptr(terms), _ptr(graph.nbr),
              _ptr(graph.deg), batch, n, w, graph.k, _ptr(ws), _ptr(out), _stream())
    return out


def attention_at(src, windows, sensors, terms, graph: SensorGraph, w: int, out: torch.Tensor | None = None,
                 check: bool = True) -> torch.Tensor:
    """One attention row per (window, sensor) pair from raw data: `src` as attention_mean's, windows [Q] = window
    indices (series: the window's first column), sensors [Q].  Returns alpha[Q, pitch] fp32.  `check`: compare the
    pairs with the data's extent on the host first (one synchronisation; the kernel itself writes zeros for a pair
    outside the data)."""
    src = _attention_source(src, "series" if src.dim() == 2 else "x")
    dev = src.device
    windows = torch.as_tensor(windows, device=dev).to(torch.int64).reshape(-1).contiguous()
    sensors = torch.as_tensor(sensors, device=dev).to(torch.int32).reshape(-1).contiguous()
    q = windows.numel()
    if sensors.numel() != q:
        raise ValueError(f"{q} windows but {sensors.numel()} sensors")
    if src.dim() == 2:
        n, t_raw = src.shape
        last = t_raw - w
    else:
        n, t_raw = src.shape[1], 0
        last = src.shape[0] - 1
        if src.shape[2] != w:
            raise ValueError(f"windows of {src.shape[2]} ticks given to a model of window length {w}")
    if n != graph.n:
        raise ValueError(f"{n} sensors given to a graph of {graph.n}")
    if out is None:
        out = torch.empty((q, graph.pitch), dtype=torch.float32, device=dev)
    if q == 0:
        return out
    if check:
        if int(windows.min()) < 0 or int(windows.max()) > last:
            raise ValueError(f"window indices outside [0, {last}]")
        if int(sensors.min()) < 0 or int(sensors.max()) >= n:
            raise ValueError(f"sensor indices outside [0, {n})")
    _lib.call("gdn_attention_at", _ptr(src), t_raw, _ptr(windows), _ptr(sensors), q, _ptr(terms), _ptr(graph.nbr),
              _ptr(graph.deg), n, w, graph.k, _ptr(out), _stream())
    return out


# --------------------------------------------------------------------------- epochs from the resident series
def check_window_table(starts: torch.Tensor, w: int, series_len: int) -> torch.Tensor:
    """A table of target ticks for windows_gather: int64, flat, every tick inside [w, series_len).  Looked at ONCE, when
    the table is uploaded (one synchronisation for a device tensor); the kernel itself writes zeros for a tick outside
    the data."""
    starts = torch.as_tensor(starts).to(torch.int64).reshape(-1)
    if starts.numel() and (int(starts.min()) < w or int(starts.max()) >= series_len):
        raise ValueError(f"target ticks outside [{w}, {series_len})")
    return starts


def windows_gather(series, starts, batch: int, w: int, x_out, y_out, first: int = 0, cursor=None, count: int | None = None,
                   valid=None, valid_out=None, row_valid=None):
    """x_out[b, i, :] = series[i, t-w : t], y_out[b, i] = series[i, t] with t = starts[first + cursor[0] * batch + b]
    (cursor None: starts[first + b]) for b < batch: datasets/TimeDataset.py's windows of a series [n, T] resident on the
    device.  `starts` int64 on the device (check_window_table), `count` = its valid entries (default: all); entries
    beyond it give windows of zeros.  x_out / y_out: contiguous fp32 with room for [batch, n, w] / [batch, n].
    With `valid` [T - w, n] uint8 (series_fill's plane of the filled `series`) the same launch also writes
    valid_out[b, :] = valid[t - w, :] (uint8, room for [batch, n]) and row_valid[b] = their sum (int32, room for
    [batch]); zeros for a window of zeros (gdn_windows_gather_gaps)."""
    series = _chk(series, name="series")
    if series.dim() != 2:
        raise ValueError(f"expected the raw series [n, T], got {tuple(series.shape)}")
    n, series_len = series.shape
    starts = _chk(starts, torch.int64, name="starts")
    if cursor is not None:
        cursor = _chk(cursor, torch.int64, name="cursor")
    for t, need, name in ((x_out, batch * n * w, "x_out"), (y_out, batch * n, "y_out")):
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < need:
            raise ValueError(f"{name}: a contiguous fp32 device tensor of at least {need} elements is needed")
    head = (_ptr(series), n, series_len, _ptr(starts), starts.numel() if count is None else count, _ptr(cursor), first,
            batch, w, _ptr(x_out), _ptr(y_out))
    if valid is None:
        if valid_out is not None or row_valid is not None:
            raise ValueError("valid_out / row_valid are cut from the validity plane: give valid as well")
        _lib.call("gdn_windows_gather", *head, _stream())
        return x_out, y_out
    valid = _valid_plane(valid, (series_len - w, n), "valid")
    if valid_out is None or row_valid is None:
        raise ValueError("valid needs valid_out (uint8, [batch, n]) and row_valid (int32, [batch]) to write into")
    for t, dtype, need, name in ((valid_out, torch.uint8, batch * n, "valid_out"), (row_valid, torch.int32, batch, "row_valid")):
        if not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or t.numel() < need:
            raise ValueError(f"{name}: a contiguous {dtype} device tensor of at least {need} elements is needed")
    _lib.call("gdn_windows_gather_gaps", *head, _ptr(valid), _ptr(valid_out), _ptr(row_valid), _stream())
    return x_out, y_out


def epoch_advance(loss, cursor, loss_table):
    """loss_table[cursor[0]] = loss (when the row exists); cursor[0] += 1.  One launch, stream-ordered after the step."""
    _lib.call("gdn_epoch_advance", _ptr(_chk(loss, name="loss")), _ptr(_chk(cursor, torch.int64, name="cursor")),
              _ptr(_chk(loss_table, name="loss_table")), loss_table.numel(), _stream())


def mse_batch_means(pred, y, batch: int, batch_means=None, mean=None, valid=None, batch_counts=None):
    """(batch_means [ceil(rows / batch)], mean []) float64: F.mse_loss of every logical minibatch of `batch` rows of
    pred / y [rows, n] (the last one ragged) and test.py's sum(losses) / len(losses).  Bitwise reproducible.
    With `valid` [rows, n] uint8 every minibatch's mean runs over its observed targets (0 when it has none), `mean` over
    the minibatches that have one (0 when none has), and the return is (batch_means, mean, batch_counts int64)
    (gdn_mse_batch_means_masked)."""
    pred, y = _chk(pred, name="pred"), _chk(y, name="y")
    if pred.shape != y.shape or pred.dim() != 2:
        raise ValueError(f"expected pred and y of one shape [rows, n], got {tuple(pred.shape)} and {tuple(y.shape)}")
    rows, n = pred.shape
    batches = (rows + batch - 1) // batch
    if batch_means is None:
        batch_means = torch.empty((batches,), dtype=torch.float64, device=pred.device)
    if mean is None:
        mean = torch.empty((), dtype=torch.float64, device=pred.device)
    if valid is None:
        if batch_counts is not None:
            raise ValueError("batch_counts belongs to the masked means: give valid as well")
        _lib.call("gdn_mse_batch_means", _ptr(pred), _ptr(y), rows, n, batch, _ptr(batch_means), _ptr(mean), None, _stream())
        return batch_means, mean
    valid = _valid_plane(valid, (rows, n), "valid")
    if batch_counts is None:
        batch_counts = torch.empty((batches,), dtype=torch.int64, device=pred.device)
    batch_counts = _chk(batch_counts, torch.int64, name="batch_counts")
    if batch_counts.numel() < batches or batch_means.numel() < batches:
        raise ValueError(f"batch_means / batch_counts: room for {batches} minibatches is needed")
    _lib.call("gdn_mse_batch_means_masked", _ptr(pred), _ptr(y), _ptr(valid), rows, n, batch, _ptr(batch_means),
              _ptr(batch_counts), _ptr(mean), None, _stream())
    return batch_means, mean, batch_counts


# --------------------------------------------------------------------------- streaming detector
def _stream_buf(t, dtype, need: int, name: str):
    if not t.is_cuda:
        raise _lib.GdnHipError(f"{name} is on {t.device}: gdn_amd ops need a HIP device (no CPU fallback)")
    if t.dtype != dtype or not t.is_contiguous() or t.numel() < need:
        raise ValueError(f"{name}: a contiguous {dtype} device tensor of at least {need} elements is needed")
    return t


def stream_state(history, w: int) -> torch.Tensor:
    """The device state of a stream (include/gdn_hip.h "streaming detector") that starts after `history` [n, h >= w]:
    an int64 tensor of gdn_stream_state_bytes(n, w) / 8 words, counters and carry zero, hist = history[:, -w:]."""
    history = _chk(history, name="history")
    if history.dim() != 2:
        raise ValueError(f"expected the history [n, h], got {tuple(history.shape)}")
    n, h = history.shape
    if h < w:
        raise ValueError(f"a history of {h} ticks is shorter than the window of {w}: buffer {w} ticks before streaming")
    nbytes = _lib.load().gdn_stream_state_bytes(n, w)
    if nbytes <= 0:
        raise _lib.GdnHipError(f"stream state: no kernel for n = {n}, w = {w} (1 <= n <= 4096, 1 <= w <= 1024)")
    state = torch.zeros((nbytes // 8,), dtype=torch.int64, device=history.device)       # (padding bytes compare equal)
    _lib.call("gdn_stream_init", _ptr(state), _ptr(history), h, n, w, _stream())
    return state


def stream_state_empty(n: int, w: int, device) -> torch.Tensor:
    """A stream state of gdn_stream_state_bytes(n, w) / 8 zero words that no history has seeded: the allocation a saved
    state is copied into (harness.StreamDetector.load).  No launch."""
    nbytes = _lib.load().gdn_stream_state_bytes(n, w)
    if nbytes <= 0:
        raise _lib.GdnHipError(f"stream state: no kernel for n = {n}, w = {w} (1 <= n <= 4096, 1 <= w <= 1024)")
    return torch.zeros((nbytes // 8,), dtype=torch.int64, device=device)


def stream_state_views(state, n: int, w: int):
    """(counters int64[3] = ticks, alarms, logged; carry float64 [3, n]; hist fp32 [n, w]): views of a stream state."""
    carry = state[4:4 + 3 * n].view(torch.float64).view(3, n)
    hist = state[4 + 3 * n:].view(torch.float32)[: n * w].view(n, w)
    return state[:3], carry, hist


def _stream_dims(state, chunk, count, w: int):
    chunk = _chk(chunk, name="chunk")
    if chunk.dim() != 2:
        raise ValueError(f"expected the chunk [c, n] (one row per tick), got {tuple(chunk.shape)}")
    c, n = chunk.shape
    count = c if count is None else int(count)
    _stream_buf(state, torch.int64, max(1, _lib.load().gdn_stream_state_bytes(n, w) // 8), "state")
    return chunk, c, n, count


def stream_windows(state, chunk, w: int, x_out, count: int | None = None):
    """x_out[b, i, :] = the w values of sensor i before tick b of `chunk` [c, n] (time-major), for b < count
    (default: all c rows): the head of a window from the state's hist, the rest from the chunk's earlier rows."""
    chunk, c, n, count = _stream_dims(state, chunk, count, w)
    _stream_buf(x_out, torch.float32, c * n * w, "x_out")
    _lib.call("gdn_stream_windows", _ptr(state), _ptr(chunk), c, count, n, w, _ptr(x_out), _stream())
    return x_out


def stream_score(state, pred, chunk, med_iqr, threshold, m: int, top_scores, top_sensors, alarm, count: int | None = None,
                 valid=None):
    """gdn_score_smooth_topm over `count` rows of pred / chunk [c, n] at the stream's position: first tick and the three
    values before the chunk come from the state.  alarm[b] = top_scores[b, 0] > threshold[0] (a float64 device scalar).
    With `valid` (stream_fill's plane of the filled `chunk`; gdn_stream_score_gaps) the normalised error of a missing
    reading is exactly 0.0 wherever it is used."""
    chunk, c, n, count = _stream_dims(state, chunk, count, 1)
    pred = _stream_buf(pred, torch.float32, c * n, "pred")
    if valid is not None:
        _stream_buf(valid, torch.uint8, c * n, "valid")
    _stream_buf(med_iqr, torch.float64, 2 * n, "med_iqr")
    _stream_buf(threshold, torch.float64, 1, "threshold")
    _stream_buf(top_scores, torch.float64, c * m, "top_scores")
    _stream_buf(top_sensors, torch.int32, c * m, "top_sensors")
    _stream_buf(alarm, torch.int32, c, "alarm")
    tail = (_ptr(med_iqr), _ptr(threshold), c, count, n, m, _ptr(top_scores), _ptr(top_sensors), _ptr(alarm), _stream())
    if valid is None:
        _lib.call("gdn_stream_score", _ptr(state), _ptr(pred), _ptr(chunk), *tail)
    else:
        _lib.call("gdn_stream_score_gaps", _ptr(state), _ptr(pred), _ptr(chunk), _ptr(valid), *tail)
    return top_scores, top_sensors, alarm


def stream_advance(state, chunk, pred, med_iqr, alarm, top_sensors, w: int, m: int, log_ticks=None, log_sensors=None,
                   count: int | None = None, valid=None, gap_chunk=None, gaps=None):
    """The one launch that writes the stream state: hist and carry rolled by `count` ticks, the counters on, every
    alarm appended to log_ticks [L] int64 / log_sensors [L, m] int32 in tick order (both None: no log).  With `valid`,
    `gap_chunk` (stream_fill's, of the filled `chunk`) and `gaps` [2, n] int64 (missing_total, missing_run), all three
    or none (gdn_stream_advance_gaps): carry entries of missing readings are 0.0 and `gaps` takes the push's gap_chunk."""
    with_gaps = valid is not None
    if (gap_chunk is not None) != with_gaps or (gaps is not None) != with_gaps:
        raise ValueError("give all of valid, gap_chunk and gaps, or none of them")
    chunk, c, n, count = _stream_dims(state, chunk, count, w)
    _stream_buf(pred, torch.float32, c * n, "pred")
    if with_gaps:
        _stream_buf(valid, torch.uint8, c * n, "valid")
        _stream_buf(gap_chunk, torch.int32, 2 * n, "gap_chunk")
    _stream_buf(med_iqr, torch.float64, 2 * n, "med_iqr")
    _stream_buf(alarm, torch.int32, c, "alarm")
    _stream_buf(top_sensors, torch.int32, c * m, "top_sensors")
    if with_gaps:
        _stream_buf(gaps, torch.int64, 2 * n, "gaps")
    if (log_ticks is None) != (log_sensors is None):
        raise ValueError("give both log_ticks and log_sensors, or neither")
    log_len = 0
    if log_ticks is not None:
        log_len = log_ticks.numel()
        _stream_buf(log_ticks, torch.int64, log_len, "log_ticks")
        _stream_buf(log_sensors, torch.int32, log_len * m, "log_sensors")
    tail = (_ptr(med_iqr), _ptr(alarm), _ptr(top_sensors), c, count, n, w, m, _ptr(log_ticks) if log_len else None,
            _ptr(log_sensors) if log_len else None, log_len)
    if with_gaps:
        _lib.call("gdn_stream_advance_gaps", _ptr(state), _ptr(chunk), _ptr(pred), _ptr(valid), _ptr(gap_chunk), *tail,
                  _ptr(gaps), _stream())
    else:
        _lib.call("gdn_stream_advance", _ptr(state), _ptr(chunk), _ptr(pred), *tail, _stream())


def stream_fill(state, raw_chunk, w: int, filled_chunk, valid, gap_chunk, count: int | None = None):
    """Hold missing readings (not finite: NaN, +inf, -inf) of `raw_chunk` [c, n] at each sensor's latest real reading —
    an earlier row of the chunk, else the state's hist[:, w - 1] — into `filled_chunk` [c, n]; valid [c, n] uint8 = 1
    for a real reading; gap_chunk [2, n] int32 = the push's missing readings and its trailing run of them per sensor.
    Rows >= count are not written."""
    raw_chunk, c, n, count = _stream_dims(state, raw_chunk, count, w)
    _stream_buf(filled_chunk, torch.float32, c * n, "filled_chunk")
    _stream_buf(valid, torch.uint8, c * n, "valid")
    _stream_buf(gap_chunk, torch.int32, 2 * n, "gap_chunk")
    if filled_chunk.data_ptr() == raw_chunk.data_ptr():
        raise ValueError("filled_chunk must not alias raw_chunk")
    _lib.call("gdn_stream_fill", _ptr(state), _ptr(raw_chunk), c, count, n, w, _ptr(filled_chunk), _ptr(valid),
              _ptr(gap_chunk), _stream())
    return filled_chunk, valid, gap_chunk


def stream_calib_ring(n: int, R: int, device):
    """An EMPTY calibration ring (include/gdn_hip.h "Rolling calibration") in one allocation of
    gdn_stream_calib_bytes(n, R): (ring_keys [n, R] float64, every key the filler pattern; ring_keep [R] uint8, zero)."""
    nbytes = _lib.load().gdn_stream_calib_bytes(n, R)
    if nbytes <= 0:
        raise _lib.GdnHipError(f"calibration ring: no kernel for n = {n}, R = {R} (1 <= n <= 4096, 64 <= R <= 2^20, "
                               "8 n R <= 2 GiB)")
    ring = torch.full((nbytes // 8,), -1, dtype=torch.int64, device=device)            # all ones: the filler
    ring_keys = ring[: n * R].view(torch.float64).view(n, R)
    ring_keep = ring[n * R:].view(torch.uint8)[:R]
    ring_keep.zero_()
    return ring_keys, ring_keep


def stream_calib_write(state, pred, chunk, alarm, ring_keys, ring_keep, exclude_alarms: bool = True,
                       count: int | None = None, valid=None, by_sensor: bool = False):
    """Row b < count of the push -> slot (state.ticks + b) mod R of the calibration ring: its keys |pred - chunk| and
    keep = 1, or the filler and keep = 0 when `exclude_alarms` and alarm[b] != 0.  After stream_score, before
    stream_advance.  Writes the ring only.  With `valid` (stream_fill's plane of the filled `chunk`;
    gdn_stream_calib_write_gaps) a tick with a missing reading in any sensor is not kept either; with `by_sensor` as
    well (gdn_stream_calib_write_sensor) such a tick is kept and only the keys of its missing readings are the filler."""
    if by_sensor and valid is None:
        raise ValueError("stream_calib_write: by_sensor needs the validity plane `valid`")
    chunk, c, n, count = _stream_dims(state, chunk, count, 1)
    _stream_buf(pred, torch.float32, c * n, "pred")
    _stream_buf(alarm, torch.int32, c, "alarm")
    if ring_keys.dim() != 2 or ring_keys.shape[0] != n:
        raise ValueError(f"ring_keys: expected [{n}, R], got {tuple(ring_keys.shape)}")
    R = ring_keys.shape[1]
    _stream_buf(ring_keys, torch.float64, n * R, "ring_keys")
    _stream_buf(ring_keep, torch.uint8, R, "ring_keep")
    tail = (c, count, n, R, int(bool(exclude_alarms)), _ptr(ring_keys), _ptr(ring_keep), _stream())
    if valid is None:
        _lib.call("gdn_stream_calib_write", _ptr(state), _ptr(pred), _ptr(chunk), _ptr(alarm), *tail)
    else:
        _stream_buf(valid, torch.uint8, c * n, "valid")
        name = "gdn_stream_calib_write_sensor" if by_sensor else "gdn_stream_calib_write_gaps"
        _lib.call(name, _ptr(state), _ptr(pred), _ptr(chunk), _ptr(alarm), _ptr(valid), *tail)
    return ring_keys, ring_keep


# --------------------------------------------------------------------------- streaming fleet
_FLEET_LIMITS = "1 <= units, units * c <= 4096, 1 <= n <= 4096, 1 <= w <= 1024"


def _fleet_state_words(units: int, n: int, w: int) -> int:
    nbytes = _lib.load().gdn_fleet_state_bytes(units, n, w)
    if nbytes <= 0:
        raise _lib.GdnHipError(f"fleet state: no kernel for units = {units}, n = {n}, w = {w} ({_FLEET_LIMITS})")
    return nbytes // 8


def fleet_state(history, w: int) -> torch.Tensor:
    """The device states of a fleet (include/gdn_hip.h "streaming fleet") whose units start after `history`
    [U, n, h >= w]: an int64 tensor [U, gdn_stream_state_bytes(n, w) / 8], row u the stream state of unit u (counters and
    carry zero, hist = history[u, :, -w:]) in the layout stream_state_views reads.  ONE launch."""
    history = _chk(history, name="history")
    if history.dim() != 3:
        raise ValueError(f"expected the history [U, n, h], got {tuple(history.shape)}")
    units, n, h = history.shape
    if h < w:
        raise ValueError(f"a history of {h} ticks is shorter than the window of {w}: buffer {w} ticks before streaming")
    words = _fleet_state_words(units, n, w)
    state = torch.zeros((units, words // units), dtype=torch.int64, device=history.device)
    _lib.call("gdn_fleet_init", _ptr(state), _ptr(history), h, units, n, w, _stream())
    return state


def fleet_state_empty(units: int, n: int, w: int, device) -> torch.Tensor:
    """Fleet states [U, gdn_stream_state_bytes(n, w) / 8] of zero words that no history has seeded: the allocation saved
    states are copied into (harness.StreamFleet.load).  No launch."""
    words = _fleet_state_words(units, n, w)
    return torch.zeros((units, words // units), dtype=torch.int64, device=device)


def fleet_state_views(state, units: int, n: int, w: int):
    """(counters int64 [U, 3] = ticks, alarms, logged; carry float64 [U, 3, n]; hist fp32 [U, n, w]): views of the
    states of a fleet.  Row u of each is what stream_state_views gives for unit u's slice."""
    state = state.view(units, -1)
    carry = state[:, 4:4 + 3 * n].view(torch.float64).view(units, 3, n)
    hist = state[:, 4 + 3 * n:].view(torch.float32)[:, : n * w].view(units, n, w)
    return state[:, :3], carry, hist


def _fleet_dims(state, chunk, counts, w: int):
    chunk = _chk(chunk, name="chunk")
    if chunk.dim() != 3:
        raise ValueError(f"expected the chunk [U, c, n] (one row per unit and tick), got {tuple(chunk.shape)}")
    units, c, n = chunk.shape
    _stream_buf(state, torch.int64, _fleet_state_words(units, n, w), "state")
    _stream_buf(counts, torch.int32, units, "counts")
    return chunk, units, c, n


def fleet_windows(state, chunk, counts, w: int, x_out):
    """x_out[u, b, i, :] = the w values of sensor i of unit u before tick b of `chunk` [U, c, n], for b < counts[u]
    (int32 [U] on the device, clamped to 0 .. c by the kernel): stream_windows per unit.  Rows b >= counts[u] are
    written as zeros: the forward's input never depends on an earlier push."""
    chunk, units, c, n = _fleet_dims(state, chunk, counts, w)
    _stream_buf(x_out, torch.float32, units * c * n * w, "x_out")
    _lib.call("gdn_fleet_windows", _ptr(state), _ptr(chunk), _ptr(counts), units, c, n, w, _ptr(x_out), _stream())
    return x_out


def fleet_fill(state, raw_chunk, counts, w: int, filled_chunk, valid, gap_chunk):
    """stream_fill per unit in one launch (gdn_fleet_fill): the missing readings (not finite) of rows b < counts[u] of
    `raw_chunk` [U, c, n] held at the unit's latest real reading — an earlier row of its chunk, else its own
    hist[:, w - 1] — into `filled_chunk` [U, c, n]; valid [U, c, n] uint8; gap_chunk [U, 2, n] int32.  Rows at or beyond
    counts[u] are neither read nor written; a unit with counts[u] == 0 writes nothing, gap_chunk included."""
    raw_chunk, units, c, n = _fleet_dims(state, raw_chunk, counts, w)
    _stream_buf(filled_chunk, torch.float32, units * c * n, "filled_chunk")
    _stream_buf(valid, torch.uint8, units * c * n, "valid")
    _stream_buf(gap_chunk, torch.int32, units * 2 * n, "gap_chunk")
    if filled_chunk.data_ptr() == raw_chunk.data_ptr():
        raise ValueError("filled_chunk must not alias raw_chunk")
    _lib.call("gdn_fleet_fill", _ptr(state), _ptr(raw_chunk), _ptr(counts), units, c, n, w, _ptr(filled_chunk),
              _ptr(valid), _ptr(gap_chunk), _stream())
    return filled_chunk, valid, gap_chunk


def fleet_score(state, pred, chunk, med_iqr, threshold, counts, w: int, m: int, top_scores, top_sensors, alarm,
                valid=None):
    """stream_score per unit in one launch: rows b < counts[u] of pred / chunk [U, c, n] at unit u's stream position,
    against med_iqr [U, n, 2] and threshold [U] (float64, device).  Rows b >= counts[u] of top_scores [U, c, m],
    top_sensors [U, c, m] and alarm [U, c] are not written.  `w` places the units' state blocks.  With `valid`
    (fleet_fill's plane of the filled `chunk`; gdn_fleet_score_gaps) the normalised error of a missing reading is 0.0."""
    chunk, units, c, n = _fleet_dims(state, chunk, counts, w)
    _stream_buf(pred, torch.float32, units * c * n, "pred")
    if valid is not None:
        _stream_buf(valid, torch.uint8, units * c * n, "valid")
    _stream_buf(med_iqr, torch.float64, units * 2 * n, "med_iqr")
    _stream_buf(threshold, torch.float64, units, "threshold")
    _stream_buf(top_scores, torch.float64, units * c * m, "top_scores")
    _stream_buf(top_sensors, torch.int32, units * c * m, "top_sensors")
    _stream_buf(alarm, torch.int32, units * c, "alarm")
    tail = (_ptr(med_iqr), _ptr(threshold), _ptr(counts), units, c, n, w, m, _ptr(top_scores), _ptr(top_sensors),
            _ptr(alarm), _stream())
    if valid is None:
        _lib.call("gdn_fleet_score", _ptr(state), _ptr(pred), _ptr(chunk), *tail)
    else:
        _lib.call("gdn_fleet_score_gaps", _ptr(state), _ptr(pred), _ptr(chunk), _ptr(valid), *tail)
    return top_scores, top_sensors, alarm


def fleet_advance(state, chunk, pred, med_iqr, alarm, top_sensors, counts, w: int, m: int, log_ticks=None,
                  log_sensors=None, valid=None, gap_chunk=None, gaps=None):
    """The one launch that writes the states of a fleet: stream_advance per unit with count = counts[u]; every alarm of
    unit u is appended to log_ticks [U, L] int64 / log_sensors [U, L, m] int32 in tick order (both None: no log).  A
    unit with counts[u] == 0 is left as it is, state and log.  With `valid`, `gap_chunk` (fleet_fill's, of the filled
    `chunk`) and `gaps` [U, 2, n] int64, all three or none (gdn_fleet_advance_gaps): stream_advance's gaps form per
    unit; a silent unit's gaps rows stay too."""
    with_gaps = valid is not None
    if (gap_chunk is not None) != with_gaps or (gaps is not None) != with_gaps:
        raise ValueError("give all of valid, gap_chunk and gaps, or none of them")
    chunk, units, c, n = _fleet_dims(state, chunk, counts, w)
    _stream_buf(pred, torch.float32, units * c * n, "pred")
    if with_gaps:
        _stream_buf(valid, torch.uint8, units * c * n, "valid")
        _stream_buf(gap_chunk, torch.int32, units * 2 * n, "gap_chunk")
        _stream_buf(gaps, torch.int64, units * 2 * n, "gaps")
    _stream_buf(med_iqr, torch.float64, units * 2 * n, "med_iqr")
    _stream_buf(alarm, torch.int32, units * c, "alarm")
    _stream_buf(top_sensors, torch.int32, units * c * m, "top_sensors")
    if (log_ticks is None) != (log_sensors is None):
        raise ValueError("give both log_ticks and log_sensors, or neither")
    log_len = 0
    if log_ticks is not None:
        if log_ticks.dim() != 2 or log_ticks.shape[0] != units:
            raise ValueError(f"log_ticks: expected [{units}, L], got {tuple(log_ticks.shape)}")
        log_len = log_ticks.shape[1]
        _stream_buf(log_ticks, torch.int64, units * log_len, "log_ticks")
        _stream_buf(log_sensors, torch.int32, units * log_len * m, "log_sensors")
    tail = (_ptr(med_iqr), _ptr(alarm), _ptr(top_sensors), _ptr(counts), units, c, n, w, m,
            _ptr(log_ticks) if log_len else None, _ptr(log_sensors) if log_len else None, log_len)
    if with_gaps:
        _lib.call("gdn_fleet_advance_gaps", _ptr(state), _ptr(chunk), _ptr(pred), _ptr(valid), _ptr(gap_chunk), *tail,
                  _ptr(gaps), _stream())
    else:
        _lib.call("gdn_fleet_advance", _ptr(state), _ptr(chunk), _ptr(pred), *tail, _stream())


def fleet_events_alloc(units: int, m: int, cap: int, device) -> torch.Tensor:
    """The events allocation of a fleet: int64 [U, gdn_stream_events_bytes(m, cap) / 8], zero (no tick seen); row u is
    what stream_events_alloc gives a single stream and stream_events_views reads."""
    nbytes = _lib.load().gdn_fleet_events_bytes(units, m, cap)
    if nbytes <= 0:
        raise _lib.GdnHipError(f"fleet events: no kernel for units = {units}, m = {m}, cap = {cap} (1 <= units <= 4096, "
                               "1 <= m <= 8, 0 <= cap <= 2^20)")
    return torch.zeros((units, nbytes // 8 // units), dtype=torch.int64, device=device)


def fleet_events(state, top_scores, top_sensors, threshold, clear, counts, n: int, w: int, on: int, off: int, cap: int,
                 events):
    """stream_events per unit in one launch (gdn_fleet_events): the episodes of rows b < counts[u] of top_scores /
    top_sensors [U, c, m] folded into unit u's row of `events` (fleet_events_alloc), raise level threshold[u], clear
    level clear[u] (float64 [U], device).  After fleet_score, before fleet_advance.  Reads the states (`n`, `w` place the
    units' blocks), writes `events` only; a unit with counts[u] == 0 keeps its row byte for byte."""
    if top_scores.dim() != 3:
        raise ValueError(f"expected top_scores [U, c, m], got {tuple(top_scores.shape)}")
    units, c, m = top_scores.shape
    _stream_buf(state, torch.int64, _fleet_state_words(units, n, w), "state")
    _stream_buf(counts, torch.int32, units, "counts")
    _stream_buf(top_scores, torch.float64, units * c * m, "top_scores")
    _stream_buf(top_sensors, torch.int32, units * c * m, "top_sensors")
    _stream_buf(threshold, torch.float64, units, "threshold")
    _stream_buf(clear, torch.float64, units, "clear")
    _stream_buf(events, torch.int64, max(1, _lib.load().gdn_fleet_events_bytes(units, m, cap) // 8), "events")
    _lib.call("gdn_fleet_events", _ptr(state), _ptr(top_scores), _ptr(top_sensors), _ptr(threshold), _ptr(clear),
              _ptr(counts), units, c, n, w, m, int(on), int(off), int(cap), _ptr(events), _stream())
    return events


_FLEET_RING_LIMITS = "1 <= units <= 4096, 1 <= n <= 4096, 64 <= R <= 2^20, 8 units n R <= 2 GiB"
FLEET_SELECT_ROWS = 65535           # rows one select call takes: its multi-pass route launches a grid (slices, rows)


def fleet_calib_ring(units: int, n: int, R: int, device):
    """The EMPTY calibration rings of a fleet (include/gdn_hip.h "Rolling calibration of a fleet") in one allocation of
    gdn_fleet_calib_bytes(units, n, R): (ring_keys [U, n, R] float64, every key the filler pattern; ring_keep [U, R]
    uint8, zero).  Unit u's slices are what stream_calib_ring gives a single stream."""
    nbytes = _lib.load().gdn_fleet_calib_bytes(units, n, R)
    if nbytes <= 0:
        raise _lib.GdnHipError(f"fleet calibration ring: no kernel for units = {units}, n = {n}, R = {R} "
                               f"({_FLEET_RING_LIMITS})")
    ring = torch.full((nbytes // 8,), -1, dtype=torch.int64, device=device)            # all ones: the filler
    ring_keys = ring[: units * n * R].view(torch.float64).view(units, n, R)
    ring_keep = ring[units * n * R:].view(torch.uint8)[: units * R].view(units, R)
    ring_keep.zero_()
    return ring_keys, ring_keep


def _fleet_ring_dims(ring_keys, ring_keep, units: int, n: int):
    if ring_keys.dim() != 3 or ring_keys.shape[:2] != (units, n):
        raise ValueError(f"ring_keys: expected [{units}, {n}, R], got {tuple(ring_keys.shape)}")
    R = ring_keys.shape[2]
    _stream_buf(ring_keys, torch.float64, units * n * R, "ring_keys")
    if ring_keep is not None:
        _stream_buf(ring_keep, torch.uint8, units * R, "ring_keep")
    return R


def fleet_calib_write(state, pred, chunk, alarm, counts, w: int, ring_keys, ring_keep, exclude_alarms: bool = True,
                      valid=None, by_sensor: bool = False):
    """stream_calib_write per unit in one launch (gdn_fleet_calib_write): row b < counts[u] of unit u -> slot
    (ticks_u + b) mod R of that unit's slices of ring_keys [U, n, R] / ring_keep [U, R].  After fleet_score (and
    fleet_events), before fleet_advance.  Writes the rings only; a unit with counts[u] == 0 has no byte of its ring
    touched.  `valid` (fleet_fill's plane of the filled `chunk`) and `by_sensor` pick gdn_fleet_calib_write_gaps /
    _sensor as stream_calib_write picks the single stream's."""
    if by_sensor and valid is None:
        raise ValueError("fleet_calib_write: by_sensor needs the validity plane `valid`")
    chunk, units, c, n = _fleet_dims(state, chunk, counts, w)
    _stream_buf(pred, torch.float32, units * c * n, "pred")
    _stream_buf(alarm, torch.int32, units * c, "alarm")
    R = _fleet_ring_dims(ring_keys, ring_keep, units, n)
    tail = (_ptr(counts), units, c, n, w, R, int(bool(exclude_alarms)), _ptr(ring_keys), _ptr(ring_keep), _stream())
    if valid is None:
        _lib.call("gdn_fleet_calib_write", _ptr(state), _ptr(pred), _ptr(chunk), _ptr(alarm), *tail)
    else:
        _stream_buf(valid, torch.uint8, units * c * n, "valid")
        name = "gdn_fleet_calib_write_sensor" if by_sensor else "gdn_fleet_calib_write_gaps"
        _lib.call(name, _ptr(state), _ptr(pred), _ptr(chunk), _ptr(alarm), _ptr(valid), *tail)
    return ring_keys, ring_keep


def fleet_ring_counts(ring_keys, ring_keep, counts, kept=None, select=None, by_sensor: bool = False):
    """The per-row counts score_select_counts takes over ring_keys [U, n, R] viewed as U * n sensors, into `counts`
    [U, n] int32 on the device (gdn_fleet_ring_counts); nothing is read back.  Tick calibration: kept [U] int32 = the sum
    of each unit's keep flags, broadcast over the unit's rows.  `by_sensor`: score_key_counts over the rings (every row's
    own real keys; `ring_keep` and `kept` are not used).  `select` [U] uint8 / bool on the device (None: every unit): a
    unit with select[u] == 0 gets counts 0 — the select then keeps its rows — and keeps kept[u]."""
    if ring_keys.dim() != 3:
        raise ValueError(f"ring_keys: expected [U, n, R], got {tuple(ring_keys.shape)}")
    units, n = ring_keys.shape[:2]
    R = _fleet_ring_dims(ring_keys, None if by_sensor else ring_keep, units, n)
    _stream_buf(counts, torch.int32, units * n, "counts")
    if select is not None:
        if select.dtype == torch.bool:
            select = select.view(torch.uint8)
        _stream_buf(select, torch.uint8, units, "select")
    if by_sensor:
        score_key_counts(ring_keys, 1, units * n, R, out=counts.view(-1)[: units * n])
        _lib.call("gdn_fleet_ring_counts", None, _ptr(select), units, n, R, _ptr(counts), None, _stream())
        return counts, None
    if kept is None:
        raise ValueError("fleet_ring_counts: tick calibration needs `kept` [U] int32")
    _stream_buf(kept, torch.int32, units, "kept")
    _lib.call("gdn_fleet_ring_counts", _ptr(ring_keep), _ptr(select), units, n, R, _ptr(counts), _ptr(kept), _stream())
    return counts, kept


def check_ring_margin(margin, name: str = "margin") -> float:
    """A threshold margin as a float: finite and > 0, else a ValueError that names `name`.  Host arithmetic only."""
    try:
        value = float(margin)
    except (TypeError, ValueError):
        raise ValueError(f"{name} = {margin!r}: a finite number > 0 (the factor on the ring's largest score)") from None
    if not (math.isfinite(value) and value > 0.0):
        raise ValueError(f"{name} = {margin!r}: a finite number > 0 (the factor on the ring's largest score)")
    return value


def fleet_ring_threshold_workspace(units: int, R: int, device) -> torch.Tensor:
    """The workspace of fleet_ring_threshold for `units` rings of R slots (gdn_fleet_ring_threshold_bytes)."""
    nbytes = _lib.load().gdn_fleet_ring_threshold_bytes(units, R)
    if nbytes <= 0:
        raise _lib.GdnHipError(f"ring threshold: no kernel for units = {units}, R = {R} ({_FLEET_RING_LIMITS})")
    return torch.empty((nbytes // 8,), dtype=torch.int64, device=device)


def fleet_ring_threshold(state, ring_keys, ring_keep, med_iqr, w: int, margin: float, min_eligible: int, ws, threshold,
                         peak, eligible, peak_slot, select=None, clear_frac=None, clear=None, by_sensor: bool = False):
    """Re-derive the thresholds from the rings under the tables in force (gdn_fleet_ring_threshold, include/gdn_hip.h
    "Threshold from the ring"): per unit the largest smoothed score among the eligible slots of ring_keys [U, n, R] /
    ring_keep [U, R] into `peak` [U] float64, their number into `eligible` [U] int32, the smallest slot of the peak into
    `peak_slot` [U] int32; threshold[u] = peak * margin in place for every unit with select[u] != 0 (None: all),
    eligible >= min_eligible and a finite peak > 0, and with `clear_frac` / `clear` [U] float64 (both or neither)
    clear[u] = threshold[u] * clear_frac[u] in the same step.  A single stream passes its tensors with a leading axis of
    one.  `by_sensor`: the rings were written by calib="sensor" (the filler in a key is a missing reading, error 0.0).
    Two launches, nothing is read back."""
    if ring_keys.dim() != 3:
        raise ValueError(f"ring_keys: expected [U, n, R], got {tuple(ring_keys.shape)}")
    margin = check_ring_margin(margin)
    if int(min_eligible) < 1:
        raise ValueError(f"min_eligible = {min_eligible}: at least one eligible slot")
    if (clear_frac is None) != (clear is None):
        raise ValueError("clear_frac and clear: both or neither")
    units, n = ring_keys.shape[:2]
    R = _fleet_ring_dims(ring_keys, ring_keep, units, n)
    _stream_buf(state, torch.int64, _fleet_state_words(units, n, w), "state")
    _stream_buf(med_iqr, torch.float64, units * n * 2, "med_iqr")
    _stream_buf(ws, torch.int64, max(1, _lib.load().gdn_fleet_ring_threshold_bytes(units, R) // 8), "ws")
    _stream_buf(threshold, torch.float64, units, "threshold")
    _stream_buf(peak, torch.float64, units, "peak")
    _stream_buf(eligible, torch.int32, units, "eligible")
    _stream_buf(peak_slot, torch.int32, units, "peak_slot")
    if select is not None:
        if select.dtype == torch.bool:
            select = select.view(torch.uint8)
        _stream_buf(select, torch.uint8, units, "select")
    if clear is not None:
        _stream_buf(clear_frac, torch.float64, units, "clear_frac")
        _stream_buf(clear, torch.float64, units, "clear")
    _lib.call("gdn_fleet_ring_threshold", _ptr(state), _ptr(ring_keys), _ptr(ring_keep), _ptr(med_iqr), _ptr(select),
              units, n, w, R, 2 if by_sensor else 0, margin, int(min_eligible), _ptr(ws), _ptr(threshold),
              _ptr(clear_frac), _ptr(clear), _ptr(peak), _ptr(eligible), _ptr(peak_slot), _stream())
    return threshold


def fleet_select_spans(units: int, n: int, limit: int = FLEET_SELECT_ROWS) -> list:
    """Cut the U * n rows of a fleet's rings into spans [(first unit, units)] of whole units with at most `limit` rows
    each (n <= limit): what one select call takes.  Host arithmetic only."""
    if units < 1 or n < 1 or n > limit:
        raise ValueError(f"units = {units}, n = {n}: at least one unit, and 1 <= n <= {limit} rows per unit")
    per = limit // n
    return [(u0, min(per, units - u0)) for u0 in range(0, units, per)]


def fleet_select_workspace(units: int, n: int, R: int, device) -> torch.Tensor:
    """One select workspace sized for the largest span of fleet_select_spans(units, n)."""
    most = max(k for _, k in fleet_select_spans(units, n))
    return score_select_workspace(1, most * n, R, device)


def fleet_select_counts(ring_keys, counts, min_count: int, ws, med_iqr):
    """med_iqr [U, n, 2] rewritten in place from ring_keys [U, n, R] with the per-row counts [U, n]: ONE
    score_select_counts per span of fleet_select_spans (one call up to 65535 rows), straight from the rings."""
    units, n, R = ring_keys.shape
    _stream_buf(med_iqr, torch.float64, units * n * 2, "med_iqr")
    _stream_buf(counts, torch.int32, units * n, "counts")
    for u0, k in fleet_select_spans(units, n):
        score_select_counts(ring_keys[u0:u0 + k], 1, k * n, R, counts[u0:u0 + k], min_count, ws,
                            out=med_iqr[u0:u0 + k])
    return med_iqr


# --------------------------------------------------------------------------- fleet series
FLEET_SERIES_LIMITS = "1 <= units <= 4096, 1 <= n <= 4096, t >= 1, 8 units n pitch <= 2 GiB"


def fleet_series_check(units: int, t: int, n: int, pitch: int | None = None) -> None:
    """The limits of the fleet-series launches (include/gdn_hip.h "Fleet series"), host arithmetic only."""
    pitch = t if pitch is None else pitch
    if not (1 <= units <= 4096 and 1 <= n <= 4096 and t >= 1 and pitch >= t and 8 * units * n * pitch <= 2 << 30):
        raise _lib.GdnHipError(f"fleet series: no kernel for units = {units}, t = {t}, n = {n}, pitch = {pitch} "
                               f"({FLEET_SERIES_LIMITS}, pitch >= t)")


def _fleet_planes(pred, gt, valid):
    """pred, gt [U, t, n] fp32 and the optional validity planes [U, t, n] uint8 of the fleet-series launches, checked."""
    pred, gt = _chk(pred, name="pred"), _chk(gt, name="gt")
    if pred.dim() != 3 or gt.shape != pred.shape:
        raise ValueError(f"expected pred and gt of one shape [U, t, n], got {tuple(pred.shape)} and {tuple(gt.shape)}")
    if valid is not None:
        valid = _valid_plane(valid, pred.shape, "valid")
    return pred, gt, valid


def fleet_series_keys(pred, gt, pitch: int, out: torch.Tensor | None = None, keep=None, valid=None) -> torch.Tensor:
    """keys [U, n, pitch] float64 of pred / gt [U, t, n] in ONE launch (gdn_fleet_series_keys): unit u's block is
    score_keys(pred[u], gt[u], pitch, keep=keep[u] / valid=valid[u]) bit for bit.  `keep` [U, t] uint8 or `valid`
    [U, t, n] uint8, one of the two at the most."""
    pred, gt, valid = _fleet_planes(pred, gt, valid)
    units, t, n = pred.shape
    if keep is not None and valid is not None:
        raise ValueError("fleet_series_keys: keep (whole ticks) and valid (single readings) exclude each other")
    if keep is not None:
        keep = _chk(keep, torch.uint8, "keep")
        if tuple(keep.shape) != (units, t):
            raise ValueError(f"keep: one flag per unit and tick is needed [{units}, {t}], got {tuple(keep.shape)}")
    fleet_series_check(units, t, n, pitch)
    keys = out if out is not None else torch.empty((units, n, pitch), dtype=torch.float64, device=pred.device)
    if keys.shape != (units, n, pitch) or keys.dtype != torch.float64 or not keys.is_contiguous():
        raise ValueError("keys buffer must be a contiguous float64 [U, n, pitch] tensor")
    _lib.call("gdn_fleet_series_keys", _ptr(pred), _ptr(gt), _ptr(keep), _ptr(valid), units, t, n, pitch, _ptr(keys),
              _stream())
    return keys


def _fleet_table(med_iqr, units: int, n: int):
    med_iqr = _chk(med_iqr, torch.float64, "med_iqr")
    if tuple(med_iqr.shape) != (units, n, 2):
        raise ValueError(f"med_iqr: expected [{units}, {n}, 2], got {tuple(med_iqr.shape)}")
    return med_iqr


def fleet_series_smooth_max(pred, gt, med_iqr, want_scores: bool = True, anomaly: torch.Tensor | None = None,
                            scores: torch.Tensor | None = None, valid=None):
    """score_smooth_max per unit in ONE launch (gdn_fleet_series_smooth_max / _gaps): pred, gt [U, t, n], med_iqr
    [U, n, 2]; every unit is a series of its own (first_tick = 0, nothing crosses a unit seam).  Returns (scores
    [U, n, t] | None, anomaly [U, t]); both may be preallocated.  `valid` [U, t, n] uint8 as in score_smooth_max."""
    pred, gt, valid = _fleet_planes(pred, gt, valid)
    units, t, n = pred.shape
    med_iqr = _fleet_table(med_iqr, units, n)
    fleet_series_check(units, t, n)
    if scores is None and want_scores:
        scores = torch.empty((units, n, t), dtype=torch.float64, device=pred.device)
    if anomaly is None:
        anomaly = torch.empty((units, t), dtype=torch.float64, device=pred.device)
    if scores is not None:
        _stream_buf(scores, torch.float64, units * n * t, "scores")
    _stream_buf(anomaly, torch.float64, units * t, "anomaly")
    head = (_ptr(pred), _ptr(gt), _ptr(med_iqr), units, t, n, _ptr(scores), _ptr(anomaly))
    if valid is None:
        _lib.call("gdn_fleet_series_smooth_max", *head, _stream())
    else:
        _lib.call("gdn_fleet_series_smooth_max_gaps", *head, _ptr(valid), _stream())
    return scores, anomaly


def fleet_series_smooth_topm(pred, gt, med_iqr, m: int, top_scores: torch.Tensor | None = None,
                             top_sensors: torch.Tensor | None = None, valid=None):
    """score_smooth_topm per unit in ONE launch (gdn_fleet_series_smooth_topm / _gaps): returns (top_scores [U, t, m]
    float64 descending, top_sensors [U, t, m] int32); both may be preallocated."""
    pred, gt, valid = _fleet_planes(pred, gt, valid)
    units, t, n = pred.shape
    med_iqr = _fleet_table(med_iqr, units, n)
    fleet_series_check(units, t, n)
    m = int(m)
    if top_scores is None:
        top_scores = torch.empty((units, t, m), dtype=torch.float64, device=pred.device)
    if top_sensors is None:
        top_sensors = torch.empty((units, t, m), dtype=torch.int32, device=pred.device)
    if (top_scores.shape != (units, t, m) or top_scores.dtype != torch.float64 or not top_scores.is_contiguous()
            or top_sensors.shape != (units, t, m) or top_sensors.dtype != torch.int32
            or not top_sensors.is_contiguous()):
        raise ValueError("top_scores / top_sensors must be contiguous [U, t, m] float64 / int32 tensors")
    head = (_ptr(pred), _ptr(gt), _ptr(med_iqr), units, t, n, m, _ptr(top_scores), _ptr(top_sensors))
    if valid is None:
        _lib.call("gdn_fleet_series_smooth_topm", *head, _stream())
    else:
        _lib.call("gdn_fleet_series_smooth_topm_gaps", *head, _ptr(valid), _stream())
    return top_scores, top_sensors


# --------------------------------------------------------------------------- raw readings
_PREP_MAX_DOWN = 64


def _prep_raw(raw, name: str = "raw"):
    """A raw tick-major block [t_raw, n], fp32 or float64, on the device: (tensor, t_raw, n, raw_f64)."""
    if not raw.is_cuda:
        raise _lib.GdnHipError(f"{name} is on {raw.device}: gdn_amd ops need a HIP device (no CPU fallback)")
    if raw.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{name}: expected {torch.float32} or {torch.float64}, got {raw.dtype}")
    if raw.dim() != 2 or raw.shape[0] < 1 or not 1 <= raw.shape[1] <= 4096:
        raise ValueError(f"expected {name} [t_raw >= 1, 1 <= n <= 4096] (one row per raw tick), got {tuple(raw.shape)}")
    raw = raw if raw.is_contiguous() else raw.contiguous()
    return raw, raw.shape[0], raw.shape[1], int(raw.dtype == torch.float64)


def _prep_down(down: int) -> int:
    if not 1 <= int(down) <= _PREP_MAX_DOWN:
        raise ValueError(f"down = {down}: a prepared tick is the median of 1 to {_PREP_MAX_DOWN} raw ticks")
    return int(down)


def _prep_table(table, n: int):
    table = _chk(table, torch.float64, name="table")
    if table.shape != (n, 2):
        raise ValueError(f"expected table of shape [{n}, 2] (scale, offset), got {tuple(table.shape)}")
    return table


def prep_stats(raw, out: torch.Tensor | None = None) -> torch.Tensor:
    """stats [n, 4] float64 = (min, max, mean, count) per sensor over the finite readings of `raw` [t_raw, n] (fp32 or
    float64, tick-major); all four 0 for a sensor with none (gdn_prep_stats: a fixed summation order)."""
    raw, t_raw, n, f64 = _prep_raw(raw)
    ws = torch.empty((_lib.load().gdn_prep_stats_workspace_bytes(t_raw, n) // 8,), dtype=torch.float64, device=raw.device)
    out = torch.empty((n, 4), dtype=torch.float64, device=raw.device) if out is None else out
    _stream_buf(out, torch.float64, 4 * n, "out")
    _lib.call("gdn_prep_stats", _ptr(raw), t_raw, n, f64, _ptr(ws), _ptr(out), _stream())
    return out


def prep_series(raw, table, down: int, fill=None, labels=None):
    """(series [n, T = t_raw // down] fp32, labels [T] float64 or None): every reading of `raw` [t_raw, n] normalised
    as x * table[i, 0] + table[i, 1] in float64, then the median of each group of `down` raw ticks (gdn_prep_series).
    `fill` [n] float64 replaces a missing (non-finite) reading before the normalisation; without it a missing reading
    is left out of its group's median and an empty group is NaN.  `labels` [t_raw] float64: rint(max) per group."""
    raw, t_raw, n, f64 = _prep_raw(raw)
    down = _prep_down(down)
    if t_raw < down:
        raise ValueError(f"t_raw = {t_raw} raw ticks are fewer than down = {down}: not one prepared tick")
    table = _prep_table(table, n)
    if fill is not None:
        fill = _chk(fill, torch.float64, name="fill")
        if fill.shape != (n,):
            raise ValueError(f"expected fill of shape [{n}], got {tuple(fill.shape)}")
    T = t_raw // down
    labels_out = None
    if labels is not None:
        labels = _chk(labels, torch.float64, name="labels")
        if labels.shape != (t_raw,):
            raise ValueError(f"expected labels of shape [{t_raw}], got {tuple(labels.shape)}")
        labels_out = torch.empty((T,), dtype=torch.float64, device=raw.device)
    series = torch.empty((n, T), dtype=torch.float32, device=raw.device)
    _lib.call("gdn_prep_series", _ptr(raw), t_raw, n, f64, _ptr(table), _ptr(fill), down, _ptr(labels), _ptr(series),
              _ptr(labels_out), _stream())
    return series, labels_out


def prep_ticks(raw, pend_in, pending: int, pend_out, down: int, table, out, rows: int | None = None) -> int:
    """The stream's front end (gdn_prep_ticks): the raw ticks [pend_in[:pending] | raw[:rows]] -> out[g, :] for g <
    (pending + rows) // down (tick-major fp32, `out` [c, n]) and the last (pending + rows) % down of them -> pend_out
    as float64.  pend_in / pend_out: distinct float64 planes of at least max(1, down - 1) rows of n.  `rows` (default:
    all of raw) lets a static staging buffer carry a shorter push.  Returns the number of completed groups."""
    raw, t_raw, n, f64 = _prep_raw(raw)
    down = _prep_down(down)
    rows = t_raw if rows is None else int(rows)
    if not 1 <= rows <= t_raw:
        raise ValueError(f"rows = {rows}: between 1 and the {t_raw} rows of raw")
    if not 0 <= int(pending) < down:
        raise ValueError(f"pending = {pending}: the raw ticks of an open group number 0 to down - 1 = {down - 1}")
    table = _prep_table(table, n)
    need = max(1, down - 1) * n
    _stream_buf(pend_in, torch.float64, need, "pend_in")
    _stream_buf(pend_out, torch.float64, need, "pend_out")
    if pend_in.data_ptr() == pend_out.data_ptr():
        raise ValueError("pend_out must not alias pend_in (alternate the two planes)")
    _stream_buf(out, torch.float32, 1, "out")
    if out.dim() != 2 or out.shape[1] != n:
        raise ValueError(f"expected out [c, {n}] (one row per prepared tick), got {tuple(out.shape)}")
    groups = (int(pending) + rows) // down
    if groups > out.shape[0]:
        raise ValueError(f"{pending} pending + {rows} raw ticks complete {groups} groups of {down}: more than the "
                         f"{out.shape[0]} rows of out")
    _lib.call("gdn_prep_ticks", _ptr(raw), rows, f64, _ptr(pend_in), int(pending), _ptr(pend_out), n, down, _ptr(table),
              _ptr(out), out.shape[0], _stream())
    return groups


_FLEET_PREP_LIMITS = "1 <= units <= 4096, 1 <= n <= 4096, 1 <= down <= 64"


def _fleet_prep_bytes(units: int, n: int, down: int) -> int:
    nbytes = _lib.load().gdn_fleet_prep_bytes(int(units), int(n), int(down))
    if nbytes <= 0:
        raise _lib.GdnHipError(f"fleet prep state: no kernel for units = {units}, n = {n}, down = {down} "
                               f"({_FLEET_PREP_LIMITS})")
    return nbytes


def fleet_prep_state(units: int, n: int, down: int, device) -> torch.Tensor:
    """The pending state of a fleet's raw-readings front end (include/gdn_hip.h "Raw readings of a fleet"): ONE zeroed
    allocation of gdn_fleet_prep_bytes(units, n, down) as int64 words — no unit holds a raw tick.  No launch."""
    return torch.zeros((_fleet_prep_bytes(units, n, down) // 8,), dtype=torch.int64, device=device)


def fleet_prep_views(pend, units: int, n: int, down: int):
    """(ticks [U, down, n] float64, pending [U, tiles] int32, tiles = ceil(n / 64)): views of a fleet's pending state.
    Unit u's open group is ticks[u, :pending[u, 0]]; all tiles of a unit hold the same count."""
    tiles = (n + 63) // 64
    words = units * down * n
    ticks = pend[:words].view(torch.float64).view(units, down, n)
    pending = pend[words:].view(torch.int32)[: units * tiles].view(units, tiles)
    return ticks, pending


def fleet_prep_ticks(raw, raw_counts, pend, down: int, table, out, counts):
    """gdn_prep_ticks per unit in ONE launch (gdn_fleet_prep_ticks): unit u's raw ticks [its open group | raw[u,
    :raw_counts[u]]] (`raw` [U, rows, n] fp32 or float64; raw_counts [U] int32 on the device, clamped to 0 .. rows by
    the kernel) -> out[u, g, :] for g < groups = (pending_u + raw_counts[u]) // down (`out` [U, c, n] fp32, rows
    <= c * down), counts[u] = groups, and the rest becomes the unit's open group in `pend` (fleet_prep_state), in
    place.  Rows of out at or beyond groups are not written; a unit with raw_counts[u] == 0 keeps its pending state.
    `table` [n, 2] float64 serves all units (gdn_fleet_prep_ticks); tables [U, n, 2] give every unit its own
    (gdn_fleet_prep_ticks_units: the same kernel body with a table stride)."""
    if not raw.is_cuda:
        raise _lib.GdnHipError(f"raw is on {raw.device}: gdn_amd ops need a HIP device (no CPU fallback)")
    if raw.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"raw: expected {torch.float32} or {torch.float64}, got {raw.dtype}")
    if raw.dim() != 3 or not raw.is_contiguous():
        raise ValueError(f"expected a contiguous raw [U, rows, n] (one row per unit and raw tick), got "
                         f"{tuple(raw.shape)}")
    units, rows, n = raw.shape
    down = _prep_down(down)
    per_unit = isinstance(table, torch.Tensor) and table.dim() == 3
    if per_unit:
        table = _chk(table, torch.float64, name="tables")
        if table.shape != (units, n, 2):
            raise ValueError(f"expected tables of shape [{units}, {n}, 2] (scale, offset per unit), got "
                             f"{tuple(table.shape)}")
    else:
        table = _prep_table(table, n)
    _stream_buf(out, torch.float32, 1, "out")
    if out.dim() != 3 or out.shape[0] != units or out.shape[2] != n:
        raise ValueError(f"expected out [{units}, c, {n}] (one row per unit and prepared tick), got {tuple(out.shape)}")
    c = out.shape[1]
    if not 1 <= rows <= c * down:
        raise ValueError(f"rows = {rows}: a launch carries 1 to c * down = {c * down} raw ticks per unit")
    _stream_buf(raw_counts, torch.int32, units, "raw_counts")
    _stream_buf(counts, torch.int32, units, "counts")
    _stream_buf(pend, torch.int64, _fleet_prep_bytes(units, n, down) // 8, "pend")
    _lib.call("gdn_fleet_prep_ticks_units" if per_unit else "gdn_fleet_prep_ticks", _ptr(raw), rows,
              int(raw.dtype == torch.float64), _ptr(raw_counts), _ptr(pend), units, c, n, down, _ptr(table), _ptr(out),
              _ptr(counts), _stream())
    return out


# --------------------------------------------------------------------------- alarm episodes
EPISODES_CARRY_WORDS = 20           # GDN_EPISODES_CARRY_BYTES / 8
_EPISODES_MAX_T, _EPISODES_MAX_E, _EPISODES_MAX_RUN = 1 << 26, 1 << 20, 4096


def episodes_check(hi, lo, on: int, off: int, cap: int) -> tuple:
    """(hi, lo, on, off, cap) as Python numbers, refused by name on the host: lo > hi or a NaN level, on / off outside
    1 .. 4096, cap outside 0 .. 2^20.  `lo=None` means hi; `hi=None` (a level that lives on the device) skips the
    comparison of the two."""
    on, off, cap = int(on), int(off), int(cap)
    if not 1 <= on <= _EPISODES_MAX_RUN:
        raise ValueError(f"on = {on}: an episode is raised after 1 to {_EPISODES_MAX_RUN} ticks above the level")
    if not 1 <= off <= _EPISODES_MAX_RUN:
        raise ValueError(f"off = {off}: an episode is cleared after 1 to {_EPISODES_MAX_RUN} ticks below the clear level")
    if not 0 <= cap <= _EPISODES_MAX_E:
        raise ValueError(f"cap = {cap}: the episode table keeps 0 to {_EPISODES_MAX_E} rows")
    if hi is not None:
        hi = float(hi)
        lo = hi if lo is None else float(lo)
        if hi != hi or lo != lo or lo > hi:
            raise ValueError(f"lo = {lo}, hi = {hi}: the clear level must be a number at or below the raise level")
    elif lo is not None:
        lo = float(lo)
        if lo != lo:
            raise ValueError(f"lo = {lo}: the clear level must be a number")
    return hi, lo, on, off, cap


def episodes_table(cap: int, m: int, device):
    """An empty episode table: (start, end, peak_tick int64 [cap], peak float64 [cap], sensors int32 [cap, m], count
    int64 [1])."""
    i64 = dict(dtype=torch.int64, device=device)
    return (torch.zeros((cap,), **i64), torch.full((cap,), -1, **i64), torch.zeros((cap,), **i64),
            torch.zeros((cap,), dtype=torch.float64, device=device),
            torch.zeros((cap, m), dtype=torch.int32, device=device), torch.zeros((1,), **i64))


def episodes_scan(scores, top_sensors, hi, lo=None, on: int = 1, off: int = 1, cap: int = 4096, first_tick: int = 0,
                  carry_in=None, carry_out=None, table=None, grid: int = 0):
    """gdn_episodes_scan: the episodes of `scores` [T] float64 with their sensors from `top_sensors` [T, m] int32, both
    on the device (include/gdn_hip.h "Alarm episodes").  Returns `table` = (start, end, peak_tick, peak, sensors,
    count) — a fresh one, or the one given: with `carry_in` (an int64 [20] device tensor a previous call wrote as its
    `carry_out`) the rows below the carried count stay and the scan goes on in the same table.  `grid` > 0 forces
    the grid of the tile launches (a diagnostic: the bits do not depend on it)."""
    scores = _chk(scores, torch.float64, "scores")
    top_sensors = _chk(top_sensors, torch.int32, "top_sensors")
    if scores.dim() != 1 or top_sensors.dim() != 2 or top_sensors.shape[0] != scores.shape[0]:
        raise ValueError(f"expected scores [T] and top_sensors [T, m], got {tuple(scores.shape)} and "
                         f"{tuple(top_sensors.shape)}")
    hi, lo, on, off, cap = episodes_check(hi, lo, on, off, cap)
    T, m = top_sensors.shape
    nbytes = _lib.load().gdn_episodes_workspace_bytes(T, cap)
    if nbytes <= 0 or not 1 <= m <= 8:
        raise _lib.GdnHipError(f"episodes: no kernel for T = {T}, m = {m}, cap = {cap} (1 <= T <= 2^26, 1 <= m <= 8, "
                               "0 <= cap <= 2^20)")
    if table is None:
        table = episodes_table(cap, m, scores.device)
    start, end, peak_tick, peak, sensors, count = table
    for t, dtype, need, name in ((start, torch.int64, cap, "start"), (end, torch.int64, cap, "end"),
                                 (peak_tick, torch.int64, cap, "peak_tick"), (peak, torch.float64, cap, "peak"),
                                 (sensors, torch.int32, cap * m, "sensors"), (count, torch.int64, 1, "count")):
        _stream_buf(t, dtype, need, name)
    for t, name in ((carry_in, "carry_in"), (carry_out, "carry_out")):
        if t is not None:
            _stream_buf(t, torch.int64, EPISODES_CARRY_WORDS, name)
    ws = torch.empty((nbytes // 8,), dtype=torch.int64, device=scores.device)
    head = (_ptr(scores), _ptr(top_sensors), T, m, hi, lo, on, off, int(first_tick), cap, _ptr(carry_in),
            _ptr(carry_out), _ptr(start) if cap else None, _ptr(end) if cap else None, _ptr(peak_tick) if cap else None,
            _ptr(peak) if cap else None, _ptr(sensors) if cap else None, _ptr(count), _ptr(ws))
    if grid:
        _lib.call("gdn_episodes_scan_grid", *head, int(grid), _stream())
    else:
        _lib.call("gdn_episodes_scan", *head, _stream())
    return table


def stream_events_alloc(m: int, cap: int, device) -> torch.Tensor:
    """The events allocation of a stream (gdn_stream_events_bytes(m, cap) / 8 int64 words, zero: no tick seen)."""
    nbytes = _lib.load().gdn_stream_events_bytes(m, cap)
    if nbytes <= 0:
        raise _lib.GdnHipError(f"stream events: no kernel for m = {m}, cap = {cap} (1 <= m <= 8, 0 <= cap <= 2^20)")
    return torch.zeros((nbytes // 8,), dtype=torch.int64, device=device)


def stream_events_views(events, m: int, cap: int):
    """(carry int64 [20], start, end, peak_tick int64 [cap], peak float64 [cap], sensors int32 [cap, m]): views of an
    events allocation."""
    h = EPISODES_CARRY_WORDS
    body = events[h:]
    return (events[:h], body[:cap], body[cap:2 * cap], body[2 * cap:3 * cap], body[3 * cap:4 * cap].view(torch.float64),
            body[4 * cap:].view(torch.int32)[:cap * m].view(cap, m))


def stream_events(state, top_scores, top_sensors, threshold, clear, on: int, off: int, cap: int, events,
                  count: int | None = None):
    """gdn_stream_events: the episodes of the push's `count` rows of top_scores [c, m] / top_sensors [c, m] folded into
    `events` (stream_events_alloc), raise level threshold[0], clear level clear[0] (float64 device scalars).  After
    stream_score, before stream_advance.  Reads the state, writes `events` only."""
    c, m = top_scores.shape
    count = c if count is None else int(count)
    _stream_buf(state, torch.int64, 4, "state")
    _stream_buf(top_scores, torch.float64, c * m, "top_scores")
    _stream_buf(top_sensors, torch.int32, c * m, "top_sensors")
    _stream_buf(threshold, torch.float64, 1, "threshold")
    _stream_buf(clear, torch.float64, 1, "clear")
    _stream_buf(events, torch.int64, max(1, _lib.load().gdn_stream_events_bytes(m, cap) // 8), "events")
    _lib.call("gdn_stream_events", _ptr(state), _ptr(top_scores), _ptr(top_sensors), _ptr(threshold), _ptr(clear), c,
              count, m, int(on), int(off), int(cap), _ptr(events), _stream())
    return events


# --------------------------------------------------------------------------- alarm tuning
ALARM_SWEEP_COUNTERS = ("episodes", "true_episodes", "incidents_hit", "delay_sum", "delay_max", "alarm_ticks",
                        "alarm_label_ticks", "open")
_ALARM_SWEEP_MAX_T, _ALARM_SWEEP_MAX_P = 1 << 26, 1 << 20


def alarm_sweep_check(hi, lo, on, off, ordered: bool = True) -> tuple:
    """(hi, lo float64 [P]; on, off int32 [P]) as host tensors: scalars and one-element sequences are broadcast to the
    longest of the four.  Refused by the field's name and the row: a NaN level, lo > hi, on / off outside 1 .. 4096,
    lengths that do not agree, no row or more than 2^20.  (The device marks such rows with -1 instead: the kernel does
    not validate.)  `ordered=False` lets lo > hi through: the rows of a grid of levels that the device is to mark."""
    cols = {}
    for name, value, dtype in (("hi", hi, torch.float64), ("lo", lo, torch.float64), ("on", on, torch.int64),
                               ("off", off, torch.int64)):
        exact = hasattr(value, "dtype") or dtype is torch.int64     # (a tensor or an array keeps its values; Python floats are float64)
        t = (torch.as_tensor(value) if exact else torch.as_tensor(value, dtype=torch.float64)).detach().cpu()
        if dtype is torch.int64 and (t.is_floating_point() or t.dtype is torch.bool):
            raise TypeError(f"{name}: whole numbers of ticks are needed, got {t.dtype}")
        if t.dim() > 1:
            raise ValueError(f"{name}: a scalar or a sequence is needed, got shape {tuple(t.shape)}")
        cols[name] = t.to(dtype).reshape(-1)
    P = max(c.numel() for c in cols.values())
    for name, c in cols.items():
        if c.numel() not in (1, P):
            raise ValueError(f"{name}: {c.numel()} values, the longest of hi, lo, on, off has {P}")
        cols[name] = c.expand(P).contiguous()
    if not 1 <= P <= _ALARM_SWEEP_MAX_P:
        raise ValueError(f"{P} settings: a sweep takes 1 to {_ALARM_SWEEP_MAX_P} rows")

    def first(mask):
        return int(torch.nonzero(mask)[0])
    for name in ("hi", "lo"):
        bad = cols[name] != cols[name]
        if bool(bad.any()):
            raise ValueError(f"{name}[{first(bad)}] = nan: the level must be a number")
    bad = cols["lo"] > cols["hi"]
    if ordered and bool(bad.any()):
        r = first(bad)
        raise ValueError(f"lo[{r}] = {float(cols['lo'][r])} lies above hi[{r}] = {float(cols['hi'][r])}: the clear level "
                         "must be at or below the raise level")
    for name in ("on", "off"):
        bad = (cols[name] < 1) | (cols[name] > _EPISODES_MAX_RUN)
        if bool(bad.any()):
            r = first(bad)
            raise ValueError(f"{name}[{r}] = {int(cols[name][r])}: 1 to {_EPISODES_MAX_RUN} ticks")
    return cols["hi"], cols["lo"], cols["on"].to(torch.int32), cols["off"].to(torch.int32)


def alarm_sweep(scores, labels, hi, lo, on, off, out=None):
    """gdn_alarm_sweep (include/gdn_hip.h "Alarm tuning"): scores [T] float64, labels [T] uint8, hi / lo [P] float64 and
    on / off [P] int32, all on the device -> counts [P, 8] int64 (ALARM_SWEEP_COUNTERS; -1 in a row that is not a
    setting).  ONE launch, no synchronisation.  `out`: a contiguous int64 device tensor of P * 8 elements to write."""
    scores = _chk(scores, torch.float64, "scores")
    labels = _chk(labels, torch.uint8, "labels")
    hi, lo = _chk(hi, torch.float64, "hi"), _chk(lo, torch.float64, "lo")
    on, off = _chk(on, torch.int32, "on"), _chk(off, torch.int32, "off")
    if scores.dim() != 1 or labels.shape != scores.shape:
        raise ValueError(f"expected scores [T] and labels [T], got {tuple(scores.shape)} and {tuple(labels.shape)}")
    if hi.dim() != 1:
        raise ValueError(f"expected hi [P], got {tuple(hi.shape)}")
    for t, name in ((lo, "lo"), (on, "on"), (off, "off")):
        if t.shape != hi.shape:
            raise ValueError(f"{name}: shape {tuple(t.shape)}, hi has {tuple(hi.shape)}")
    T, P = scores.shape[0], hi.shape[0]
    if not 1 <= T <= _ALARM_SWEEP_MAX_T or not 1 <= P <= _ALARM_SWEEP_MAX_P:
        raise _lib.GdnHipError(f"alarm sweep: no kernel for T = {T}, P = {P} (1 <= T <= 2^26, 1 <= P <= 2^20)")
    if out is None:
        out = torch.empty((P, 8), dtype=torch.int64, device=scores.device)
    else:
        _stream_buf(out, torch.int64, P * 8, "out")
    _lib.call("gdn_alarm_sweep", _ptr(scores), _ptr(labels), T, _ptr(hi), _ptr(lo), _ptr(on), _ptr(off), P, _ptr(out),
              _stream())
    return out
