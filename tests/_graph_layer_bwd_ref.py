"""TEST INFRASTRUCTURE: float64 CPU references of the three stages of the graph-layer backward, one per entry point
of include/gdn_hip.h (gdn_attn_aggregate_bwd[_wide], gdn_project_bwd[_partials], gdn_terms_bwd[_acc]), the reverse
lists gdn_graph_reverse builds for the first, and a hub graph whose reverse lists are as long as they can get.

The stages take their inputs as given (xlin, s_i, s_j, alpha's route; x and the three gradients; d_a and d_c), so a
comparison at a stage boundary has no kink problem: fp32 `s_i + s_j[j]` has the sign of the exact sum of the same two
fp32 numbers, and an exactly zero logit is zero on both sides.  tests/test_cpu_backward_stages_ref.py pins every
function here to _grad_check.staged_f64 at 1e-12.
"""
import torch
import torch.nn.functional as F

f64 = torch.float64
NEG_SLOPE = 0.2             # models/graph_layer.py:13
SOFTMAX_EPS = 1e-16         # torch_geometric.utils.softmax


def nbr_pitch(k):
    return ((k + 1) + 15) & ~15


def terms_pitch(w):
    """gdn_terms_pitch: 64 up to w = 64, round_up(w, 64) above."""
    return 64 if w <= 64 else (w + 63) & ~63


def nbr_of(topk):
    """gdn_graph_from_topk on the CPU: (nbr[n, pitch] int64, deg[n]) — a row's top-k entries other than the row itself in
    rank order, then the row itself, then padding = the sentinel n."""
    n, k = topk.shape
    nbr = torch.full((n, nbr_pitch(k)), n, dtype=torch.long)
    deg = torch.zeros((n,), dtype=torch.long)
    for i in range(n):
        src = [int(j) for j in topk[i] if int(j) != i] + [i]
        nbr[i, :len(src)] = torch.tensor(src)
        deg[i] = len(src)
    return nbr, deg


def aggregate_ref(xlin, s_i, s_j, bias, nbr, d_z):
    """models/graph_layer.py:65-117 in list form and its float64 autograd.  xlin, d_z: [b, n, d]; s_i, s_j: [b, n];
    bias: [d]; nbr: [n, pitch] integer lists, padding = n.  Returns (z[b, n, d], alpha[b, n, pitch] with 0 in the
    padding, d_xlin[b, n, d], d_si[b, n], d_sj[b, n], d_bias[d]), float64.
    The softmax runs over a row's valid slots only, /(sum + 1e-16); the LeakyReLU derivative at exactly 0 is the
    slope (torch's convention, the kernels' `pi > 0.f ? 1 : slope`)."""
    b, n, d = xlin.shape
    x64 = xlin.detach().to(f64).clone().requires_grad_(True)
    si64 = s_i.detach().to(f64).clone().requires_grad_(True)
    sj64 = s_j.detach().to(f64).clone().requires_grad_(True)
    b64 = bias.detach().to(f64).clone().requires_grad_(True)
    z, alpha = aggregate_fwd(x64, si64, sj64, b64, nbr)
    z.backward(d_z.detach().to(f64).view(b, n, d))
    return z.detach(), alpha.detach(), x64.grad, si64.grad, sj64.grad, b64.grad


def aggregate_fwd(xlin, s_i, s_j, bias, nbr):
    """The forward half of aggregate_ref in the dtype of its arguments (float64 there; float32 is the yardstick of the
    forward stage tests): (z[b, n, d], alpha[b, n, pitch]), differentiable."""
    nbr = nbr.long()
    n = xlin.shape[1]
    valid = nbr < n
    safe = nbr.clamp(max=n - 1)
    logit = F.leaky_relu(s_i.unsqueeze(-1) + s_j[:, safe], NEG_SLOPE)                # [b, n, pitch]
    logit = logit.masked_fill(~valid, float("-inf"))
    e = (logit - logit.max(dim=-1, keepdim=True).values).exp()                       # padding: exp(-inf) = 0
    alpha = e / (e.sum(dim=-1, keepdim=True) + SOFTMAX_EPS)
    return (alpha.unsqueeze(-1) * xlin[:, safe]).sum(dim=2) + bias, alpha


def project_bwd_ref(x, d_xlin, d_si, d_sj):
    """Float64 autograd of xlin = x lin^T, s_i = x a_i + c_i, s_j = x a_j + c_j (the three are linear in lin, a, c: the
    gradients do not depend on where they are taken).  x: [b, n, w]; d_xlin: [b, n, d]; d_si, d_sj: [b, n].
    Returns (d_lin_w[d, w], d_a[2, P] zero padded to P = gdn_terms_pitch(w), d_c[2, n])."""
    b, n, w = x.shape
    d = d_xlin.shape[-1]
    x64 = x.detach().to(f64)
    lin = torch.zeros((d, w), dtype=f64, requires_grad=True)
    a = torch.zeros((2, w), dtype=f64, requires_grad=True)
    c = torch.zeros((2, n), dtype=f64, requires_grad=True)
    outs = (x64 @ lin.T, x64 @ a[0] + c[0], x64 @ a[1] + c[1])
    seeds = (d_xlin.detach().to(f64).view(b, n, d), d_si.detach().to(f64).view(b, n), d_sj.detach().to(f64).view(b, n))
    d_lin, d_a, d_c = torch.autograd.grad(outs, (lin, a, c), seeds)
    d_a_pad = torch.zeros((2, terms_pitch(w)), dtype=f64)
    d_a_pad[:, :w] = d_a
    return d_lin, d_a_pad, d_c


def terms_bwd_ref(lin_w, att_i, att_j, att_em_i, att_em_j, emb, d_lin_w_direct, d_a, d_c, d_emb_in=None):
    """The six formulas at gdn_terms_bwd (include/gdn_hip.h), float64.  d_a: [2, >= w] (columns beyond w ignored),
    d_c: [2, n].  Returns (d_lin_w = direct + att_i (x) d_a[0] + att_j (x) d_a[1], d_att_i, d_att_j, d_att_em_i,
    d_att_em_j, d_emb = d_emb_in (0 when None) + d_c[0] (x) att_em_i + d_c[1] (x) att_em_j)."""
    lin = lin_w.detach().to(f64)
    d, w = lin.shape
    ai, aj, ei, ej = (t.detach().to(f64).reshape(d) for t in (att_i, att_j, att_em_i, att_em_j))
    em = emb.detach().to(f64)
    da = d_a.detach().to(f64)[:, :w]
    dc = d_c.detach().to(f64)
    d_lin = d_lin_w_direct.detach().to(f64) + torch.outer(ai, da[0]) + torch.outer(aj, da[1])
    d_emb = torch.outer(dc[0], ei) + torch.outer(dc[1], ej)
    if d_emb_in is not None:
        d_emb = d_emb_in.detach().to(f64) + d_emb
    return d_lin, lin @ da[0], lin @ da[1], em.T @ dc[0], em.T @ dc[1], d_emb


def hub_topk(n, k, seed):
    """[n, k] int64 top-k table of a plant with one hub: column 0 is sensor 0 in every row (its reverse list names
    every target: rlen[0] = n), the other k - 1 entries are distinct sensors other than 0 from a seeded generator.
    Odd rows contain their own index (deg = k), even rows other than 0 do not (deg = k + 1).  Sensor n - 1 appears in
    no row but its own list (rlen = 1)."""
    assert 1 <= k <= n - 2, (n, k)
    g = torch.Generator().manual_seed(seed)
    lone = n - 1
    out = torch.zeros((n, k), dtype=torch.long)
    for i in range(n):
        own = i % 2 == 1 and k >= 2
        perm = torch.randperm(n - 1, generator=g) + 1                      # the sensors other than 0, shuffled
        rest = perm[(perm != lone) & (perm != i)][:k - 1 - int(own)]
        if own:
            rest = torch.cat((rest, torch.tensor([i])))
            rest = rest[torch.randperm(k - 1, generator=g)]
        out[i, 1:] = rest
    return out


def reverse_ref(nbr, deg):
    """gdn_graph_reverse: per source j the sorted list of (target << 16 | slot) over the valid slots that name j."""
    n = nbr.shape[0]
    out = [[] for _ in range(n)]
    for i in range(n):
        for p in range(int(deg[i])):
            out[int(nbr[i, p])].append((i << 16) | p)
    return [sorted(r) for r in out]
