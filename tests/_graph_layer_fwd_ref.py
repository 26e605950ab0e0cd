"""TEST INFRASTRUCTURE: CPU references of the staged forward, one per entry point of include/gdn_hip.h (gdn_node_terms,
gdn_project_fwd[_wide|_series], gdn_attn_aggregate_fwd[_wide], gdn_head_fwd, gdn_bn_fold).

Every function takes its stage's inputs as given (project_ref a GIVEN node_terms, aggregate_ref given s_i / s_j, head_ref
given affine tables), so a stage is judged alone, and computes in `dtype`: float64 is the reference, float32 the
yardstick (what fp32 arithmetic of the same stage is from float64, tests/test_cpu_forward_stages_ref.py).  The graph
helpers and the softmax are the backward reference's (tests/_graph_layer_bwd_ref.py).
tests/test_cpu_forward_stages_ref.py pins the chain of these functions to oracle/gdn_oracle.py at 1e-12.
"""
import torch

import _graph_layer_bwd_ref as bwd
from _graph_layer_bwd_ref import hub_topk, nbr_of, nbr_pitch, terms_pitch  # noqa: F401  (one copy of the graph helpers)

f64 = torch.float64


def node_terms_ref(lin_w, att_i, att_j, att_em_i, att_em_j, emb, dtype=f64):
    """gdn_node_terms: [a_i(P) | a_j(P) | c_i(n) | c_j(n)], a = lin^T att zero padded to P = gdn_terms_pitch(w),
    c = emb . att_em.  lin_w: [d, w]; att*: d values each; emb: [n, d]."""
    lin, em = lin_w.detach().to(dtype), emb.detach().to(dtype)
    d, w = lin.shape
    ai, aj, ei, ej = (t.detach().to(dtype).reshape(d) for t in (att_i, att_j, att_em_i, att_em_j))
    a = torch.zeros((2, terms_pitch(w)), dtype=dtype)
    a[0, :w], a[1, :w] = lin.T @ ai, lin.T @ aj
    return torch.cat((a.reshape(-1), em @ ei, em @ ej))


def project_ref(x, lin_w, node_terms, dtype=f64):
    """gdn_project_fwd: x[b, n, w] -> (xlin[b, n, d] = x lin^T, s_i[b, n] = x . a_i + c_i[sensor], s_j likewise) from a
    GIVEN node_terms in gdn_node_terms' layout (the padding of a_* is not read)."""
    b, n, w = x.shape
    p = terms_pitch(w)
    x_, lin, t = x.detach().to(dtype), lin_w.detach().to(dtype), node_terms.detach().to(dtype).reshape(-1)
    assert t.numel() == 2 * p + 2 * n
    return x_ @ lin.T, x_ @ t[:w] + t[2 * p:2 * p + n], x_ @ t[p:p + w] + t[2 * p + n:]


def aggregate_ref(xlin, s_i, s_j, bias, nbr, dtype=f64):
    """gdn_attn_aggregate_fwd: the forward half of the backward reference — valid slots only, max-subtract,
    /(sum + 1e-16), padding exactly 0.  xlin: [b, n, d]; s_i, s_j: [b, n]; nbr: [n, pitch], padding = n.
    Returns (z[b, n, d], alpha[b, n, pitch])."""
    with torch.no_grad():
        return bwd.aggregate_fwd(xlin.detach().to(dtype), s_i.detach().to(dtype), s_j.detach().to(dtype),
                                 bias.detach().to(dtype), nbr)


def head_ref(z, emb, bn1_affine, bn2_affine, out_w, out_b, dtype=f64):
    """gdn_head_fwd: z[b, n, d] -> relu(z sc1 + sh1) * emb[row % n] -> h2 = relu(. sc2 + sh2) -> out = h2 . out_w + out_b.
    bn*_affine: [scale(d) | shift(d)] (gdn_bn_fold).  Returns (out[b, n], h2[b, n, d])."""
    d = z.shape[-1]
    a1, a2 = bn1_affine.detach().to(dtype).reshape(2, d), bn2_affine.detach().to(dtype).reshape(2, d)
    h = torch.relu(z.detach().to(dtype) * a1[0] + a1[1]) * emb.detach().to(dtype)
    h2 = torch.relu(h * a2[0] + a2[1])
    return h2 @ out_w.detach().to(dtype).reshape(d) + out_b.detach().to(dtype).reshape(()), h2


def bn_fold_ref(weight, bias, running_mean, running_var, eps, dtype=f64):
    """gdn_bn_fold: [scale(c) | shift(c)], scale = weight / sqrt(var + eps), shift = bias - mean scale (eps is the fp32
    number the entry point receives)."""
    wt, bs, mean, var = (t.detach().to(dtype) for t in (weight, bias, running_mean, running_var))
    scale = wt / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32).to(dtype))
    return torch.cat((scale, bs - mean * scale))
