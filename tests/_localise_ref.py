"""TEST INFRASTRUCTURE: the float64 yardstick of the localisation tests (numpy / torch-CPU).  tests/test_cpu_localise.py
pins it to oracle.score_oracle.full_err_scores and to oracle.gdn_oracle.forward(...)["att_weight_1"]."""
import numpy as np
import torch

NEG_SLOPE, SOFTMAX_EPS, SCORE_EPS = 0.2, 1e-16, 1e-2
TIE_REL = 1e-9          # scores closer than this (relative) may come in either order
SKIP_CAP = 0.01         # share of ticks (the first three excluded) an index comparison may skip


def scores_f64(pred, gt):
    """evaluate.py:48-68 for every sensor at once: [T, N] fp32 -> smoothed scores [N, T] float64."""
    delta = np.abs(np.asarray(pred, dtype=np.float64) - np.asarray(gt, dtype=np.float64))      # [T, N]
    med = np.median(delta, axis=0)
    rng = np.percentile(delta, 75, axis=0) - np.percentile(delta, 25, axis=0)
    a = ((delta - med) / (np.abs(rng) + SCORE_EPS)).T                                          # [N, T]
    out = np.zeros_like(a)
    out[:, 3:] = (((a[:, :-3] + a[:, 1:-2]) + a[:, 2:-1]) + a[:, 3:]) / 4.0                    # np.mean of 4: left to right
    return out


def topm(scores_nt, m):
    """Per tick the m largest scores, descending, equal scores by the lower sensor: (values [T, m], sensors [T, m])."""
    s = np.asarray(scores_nt, dtype=np.float64)
    idx = np.argsort(-s, axis=0, kind="stable")[:m]
    return np.take_along_axis(s, idx, axis=0).T.copy(), idx.T.copy()


def skippable_ticks(scores_nt, m):
    """Ticks whose order is not decided at TIE_REL: two adjacent scores among the oracle's m + 1 largest differ, but by
    no more than TIE_REL (relative); exactly equal scores are ordered by sensor and are not skipped.  The first three ticks (all scores 0) are not counted here: their sensors are
    checked exactly."""
    s = np.asarray(scores_nt, dtype=np.float64)
    top = -np.sort(-s, axis=0)[:min(m + 1, s.shape[0])]                                       # [m+1, T]
    a, b = top[:-1], top[1:]
    close = (a != b) & (np.abs(a - b) <= TIE_REL * np.maximum(np.abs(a), np.abs(b)))      # equal scores HAVE an order
    skip = close.any(axis=0) if len(a) else np.zeros(s.shape[1], dtype=bool)
    skip[:3] = False
    return skip


def skipped_share(skip):
    return float(skip[3:].mean()) if len(skip) > 3 else 0.0


def neighbours(graph):
    """[n, k] top-k table -> ([n, k+1] sources per slot: ranks without self, then self, -1 padding; deg [n])."""
    g = np.asarray(graph)
    n, k = g.shape
    nb = -np.ones((n, k + 1), dtype=np.int64)
    deg = np.zeros(n, dtype=np.int64)
    for i in range(n):
        row = g[i].astype(np.int64)
        srcs = row[row != i]                                  # (numpy, not a Python loop: 4096 x 1023 tables)
        nb[i, :len(srcs)] = srcs
        nb[i, len(srcs)] = i
        deg[i] = len(srcs) + 1
    return nb, deg


def attention_rows(params, x, graph, nb=None, targets=None):
    """Attention of every (window, target) from raw windows x[B, n, w], in float64: alpha[B, n, k+1] in the slot order
    of `neighbours` (padding 0).  s = x . (lin^T att) + emb . att_em (the separable form of models/graph_layer.py:
    91-104), LeakyReLU(0.2), max-subtract, exp, / (sum + 1e-16).
    `nb`: the lists themselves ([n, slots], -1 padding) where they do not come from `neighbours(graph)` (injected
    tables with repeats: tests/_graph_build_ref.py).  `targets` [B]: one target per window instead of all n: alpha
    [B, slots] (the rows gdn_attention_at returns)."""
    pre = "gnn_layers.0.gnn."
    lin = params[pre + "lin.weight"].double()
    emb = params["embedding.weight"].double()
    d = lin.shape[0]
    x = torch.as_tensor(x).double()
    s_i = x @ (lin.T @ params[pre + "att_i"].double().view(d)) + emb @ params[pre + "att_em_i"].double().view(d)
    s_j = x @ (lin.T @ params[pre + "att_j"].double().view(d)) + emb @ params[pre + "att_em_j"].double().view(d)
    if nb is None:
        nb, _ = neighbours(graph)
    nbt = torch.from_numpy(np.asarray(nb, dtype=np.int64))
    pad = nbt < 0
    if targets is None:
        logit = s_i.unsqueeze(-1) + s_j[:, nbt.clamp(min=0)]                                   # [B, n, k+1]
        pad = pad.unsqueeze(0)
    else:
        tg = torch.as_tensor(targets, dtype=torch.long)
        rows = torch.arange(x.shape[0])
        logit = s_i[rows, tg].unsqueeze(-1) + torch.gather(s_j, 1, nbt[tg].clamp(min=0))       # [B, k+1]
        pad = pad[tg]
    logit = torch.where(logit > 0, logit, logit * NEG_SLOPE)
    logit = logit.masked_fill(pad, float("-inf"))
    e = (logit - logit.max(dim=-1, keepdim=True).values).exp()
    return (e / (e.sum(dim=-1, keepdim=True) + SOFTMAX_EPS)).numpy(), nb


def attention_mean(alpha, weights=None):
    """sum_b w_b alpha_b / sum_b w_b in float64 (plain mean without weights; zeros for a zero weight sum)."""
    a = np.asarray(alpha, dtype=np.float64)
    if weights is None:
        return a.mean(axis=0)
    wt = np.asarray(weights, dtype=np.float64)
    tot = wt.sum()
    return np.tensordot(wt, a, axes=(0, 0)) / tot if tot > 0 else np.zeros(a.shape[1:])


def edge_order(alpha, deg):
    """alpha[B, n, k+1] -> the [E'] order of att_weight_1: non-self edges window / target / rank major, then one
    self-loop per (window, node)."""
    b, n, _ = alpha.shape
    slots = np.arange(alpha.shape[2])[None, :]
    nonself = slots < (deg[:, None] - 1)
    self_w = np.take_along_axis(alpha, np.broadcast_to((deg - 1)[None, :, None], (b, n, 1)), axis=2).reshape(-1)
    return np.concatenate((alpha[:, nonself].reshape(-1), self_w))


def windows_of(series, first, batch, w):
    """series [n, T] -> x[batch, n, w], window b = series[:, first+b : first+b+w]."""
    s = torch.as_tensor(series)
    idx = (first + torch.arange(batch)).view(-1, 1) + torch.arange(w).view(1, -1)
    return s[:, idx].permute(1, 0, 2).contiguous()


def seeded_scores(t, n, seed):
    """The seeded inputs of the top-m tests: predictions with heavy-tailed errors of a different scale per sensor."""
    g = np.random.default_rng(seed)
    gt = g.random((t, n), dtype=np.float32)
    err = 0.05 * g.standard_t(3, size=(t, n)).astype(np.float32) * (1 + 3 * g.random(n, dtype=np.float32))
    return (gt + err).astype(np.float32), gt
