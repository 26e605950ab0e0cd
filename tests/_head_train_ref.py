"""TEST INFRASTRUCTURE (CPU only): the train-mode head of gdn_head_train.hip restated in float64, the in-kernel dropout
draw, and the case tables of tests/test_gpu_head_train_stages.py.

`head_f64` is models/GDN.py:77-79,175-184 under model.train(), written out with plain tensor ops, forward AND
backward (no autograd, no nn.BatchNorm1d):

    y1 = BN1(z)   a1 = relu(y1)   h1 = a1 * emb[sensor]   y2 = BN2(h1)   a2 = relu(y2)   act = a2 * mask
    out = act @ lin_w + lin_b                                  (lin_w None: the `_act` form ends at `act`)

Both BatchNorms normalise by the statistics of the batch (all batch * n rows, biased variance) and move their running
estimates by `momentum` towards the batch mean and the UNBIASED batch variance; the counter goes up by one.
tests/test_cpu_head_train_ref.py pins it to a float64 nn.BatchNorm1d chain under autograd (`torch_chain`, 1e-12) and
to _grad_check.staged_f64.  `torch_chain` in float32 is the CPU float32 run the GPU tests size their bounds by.
"""
import numpy as np
import torch

from _grad_check import KINK_BAND

F64 = torch.float64
TILE, ANY = "TILE", "ANY"
GRADS_LIN = ("d_z", "d_emb", "d_bn1_w", "d_bn1_b", "d_bn2_w", "d_bn2_b", "d_lin_w", "d_lin_b")
GRADS_ACT = GRADS_LIN[:6]
RUNNING = ("rm1", "rv1", "rm2", "rv2")


# ---- the dropout draw ---------------------------------------------------------------------------------------------

def drop_threshold(p_drop):
    """gdn_head_train.hip drop_threshold: p arrives as a float32, (double)(float)p * 2^32, truncated, clamped."""
    t = float(np.float32(p_drop)) * 4294967296.0
    return 0 if t <= 0.0 else min(int(t), 4294967295)


def keep_scale(p_drop):
    """The multiplier of a kept element as the library forms it: 1.f / (1.f - p) in float32."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p_drop)))


def mix32_keep(seed, step, count, p_drop, device=None):
    """The in-kernel dropout draw (gdn_head_train.hip: gdn_mix32) restated: bool [count], True = element kept.  Element
    e of step t is dropped iff mix32(e, seed, t) < drop_threshold(p)."""
    M = 0xFFFFFFFF
    k0 = (seed & M) ^ (((step * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF) >> 32)
    k1 = ((seed >> 32) + ((step * 0x7F4A7C15) & M)) & M
    x = (torch.arange(count, dtype=torch.int64, device=device) * 0x9E3779B1 + k0) & M
    x = x ^ (x >> 16)
    x = (x * 0x85EBCA6B) & M
    x = x ^ (x >> 13)
    x = (x + k1) & M
    x = (x * 0xC2B2AE35) & M
    x = x ^ (x >> 16)
    return x >= drop_threshold(p_drop)


# ---- the cases ------------------------------------------------------------------------------------------------------

def _case(name, shape, family, padded, chunks, cell="", seed=None):
    return dict(id=name, shape=shape, family=family, padded=padded, chunks=chunks, cell=cell, seed=seed)


# (batch, n, d); `padded` = DP, the width the kernel is instantiated on; `chunks` = ceil(n / SLOTS), SLOTS = 1024 / DP
CASES = [
    _case("d16-ragged", (5, 70, 16), TILE, 16, 2, "2 chunks, the second with 6 live sensors"),
    _case("d32-one-extra", (2, 33, 32), TILE, 32, 2, "second chunk has 1 live sensor"),
    _case("d32-many-parts", (300, 5, 32), TILE, 32, 1, "batch parts capped at 64 in the embedding pass, more in the others"),
    _case("d64", (6, 127, 64), TILE, 64, 8),
    _case("d64-two-rows", (1, 2, 64), TILE, 64, 1, "the smallest legal batch * n"),
    _case("d128-one-sensor", (2, 1, 128), TILE, 128, 1, "n = 1"),
    _case("d64-n700", (9, 700, 64), TILE, 64, 44, "n * d beyond the LDS-resident embedding-gradient partial"),
    _case("d128", (3, 40, 128), TILE, 128, 5),
    _case("any-d1", (4, 9, 1), ANY, 16, 1),
    _case("any-d3", (3, 12, 3), ANY, 16, 1, "d % 4 != 0: scalar loads / stores"),
    _case("any-d24", (3, 20, 24), ANY, 32, 1, "float4 path with masked lane groups"),
    _case("any-d50", (2, 33, 50), ANY, 64, 3),
    _case("any-d100", (2, 17, 100), ANY, 128, 3),
    _case("any-d129", (2, 9, 129), ANY, 256, 3, "DP 256, odd"),
    _case("any-d256", (2, 6, 256), ANY, 256, 2, "DP 256, full"),
    _case("any-d200-ragged", (2, 130, 200), ANY, 256, 33, "33 chunks of 4 sensors, the last with 2"),
    # column 0 of z constant, column 1 dead behind BN1 (bias -10), column 2 of z = 1000 + 0.01 randn, column 3 of emb 0
    _case("edge-columns", (6, 40, 64), TILE, 64, 3, "variance 0, a dead channel, a mean that dwarfs the spread, emb = 0"),
]
BY_ID = {c["id"]: c for c in CASES}
# the cases every entry point runs on (the rest run with the plain pair only)
CORE = ("d16-ragged", "d64", "d64-two-rows", "d64-n700", "any-d3", "any-d50", "any-d129", "any-d200-ragged",
        "edge-columns")
# seeds: 2000 + index, except where that draw puts a pre-activation inside KINK_BAND (d64-n700: 1 element of 403 200)
SEEDS = {"d64-n700": 3006}

BN1_EPS, BN1_MOM = 1e-5, 0.1
BN2_EPS, BN2_MOM = 1e-3, 0.3
P_DROP = 0.2
COUNTER0 = 7


def seed_of(case):
    return SEEDS.get(case["id"], 2000 + [c["id"] for c in CASES].index(case["id"]))


def inputs(case):
    """CPU float32 inputs of a case from a seeded generator: z ~ 0.7 randn + 0.3, emb ~ randn, BN weights in [0.5, 1.5],
    BN biases 0.2 randn, lin_w 0.3 randn; running buffers at random values (var positive), counter 7; d_out / d_act /
    y ~ randn; a Bernoulli(0.8) keep mask (bytes) and its fp32 multiplier form."""
    b, n, d = case["shape"]
    g = torch.Generator().manual_seed(seed_of(case))
    rn = lambda *s: torch.randn(s, generator=g)
    ru = lambda *s: torch.rand(s, generator=g)
    t = dict(batch=b, n=n, d=d, z=rn(b * n, d) * 0.7 + 0.3, emb=rn(n, d))
    for name, eps, mom in (("bn1", BN1_EPS, BN1_MOM), ("bn2", BN2_EPS, BN2_MOM)):
        t[name] = dict(weight=ru(d) + 0.5, bias=rn(d) * 0.2, eps=eps, momentum=mom, running_mean=rn(d) * 0.5,
                       running_var=ru(d) + 0.5, batches=COUNTER0)
    t["lin_w"], t["lin_b"] = rn(d) * 0.3, rn(1)
    t["d_out"], t["d_act"], t["y"] = rn(b * n), rn(b * n, d), rn(b * n)
    t["keep"] = (ru(b * n, d) >= P_DROP).to(torch.uint8)
    t["mask"] = t["keep"].float() * keep_scale(P_DROP)
    if case["id"] == "edge-columns":
        t["z"][:, 0] = 0.75                                   # variance exactly 0: y1 = the bias, inv = 1 / sqrt(eps)
        t["bn1"]["bias"][0] = 0.8                             # ... behind a LIVE ReLU and an embedding away from 0, so
        t["emb"][:, 0] = torch.where(t["emb"][:, 0] < 0, -1.0, 1.0) * (t["emb"][:, 0].abs() + 0.5)   # gradients flow
        t["bn1"]["bias"][1] = -10.0                           # a1 = 0, h1 = 0: BN2 sees a dead channel
        t["z"][:, 2] = 1000.0 + 0.01 * rn(b * n)              # the mean dwarfs the spread
        # (y1 of that column carries the rounding of z - mean at 1000, ~3e-3 after the division by the spread: the
        #  bias keeps every pre-activation of the column that far and more from the kink)
        t["bn1"]["bias"][2] = 6.0
        t["emb"][:, 3] = 0.0
    return t


# ---- the head in plain tensor ops -------------------------------------------------------------------------------

def _bn(x, bn, dtype):
    rows = x.shape[0]
    mu = x.mean(0)
    var = ((x - mu) ** 2).mean(0)
    inv = 1.0 / torch.sqrt(var + bn["eps"])
    xh = (x - mu) * inv
    y = xh * bn["weight"].to(dtype) + bn["bias"].to(dtype)
    new = None
    if bn.get("running_mean") is not None:
        m = bn["momentum"]
        new = ((1 - m) * bn["running_mean"].to(dtype) + m * mu,
               (1 - m) * bn["running_var"].to(dtype) + m * var * rows / (rows - 1), bn["batches"] + 1)
    return y, xh, inv, new


def _bn_bwd(dy, xh, inv, weight):
    return weight * inv * (dy - dy.mean(0) - xh * (dy * xh).mean(0))


def head_f64(z, emb, bn1, bn2, mask, lin_w, lin_b, grad, batch, dtype=F64):
    """z [batch * n, d], emb [n, d]; bn1 / bn2: dicts of weight, bias, eps, momentum, running_mean, running_var, batches
    (running_mean None: not tracked); mask [batch * n, d] multipliers or None; lin_w [d] and lin_b [1], or both None for
    the `_act` form; grad: d_out [batch * n] (Linear form) or d_act [batch * n, d].
    Returns a dict: out or act, d_z, d_emb, d_bn1_w, d_bn1_b, d_bn2_w, d_bn2_b (, d_lin_w, d_lin_b), rm1 / rv1 / nbt1 /
    rm2 / rv2 / nbt2 after the call (None when not tracked), the pre-ReLU tensors y1, y2, live1 / live2 (where a
    gradient arrives at the ReLU: elsewhere either side of the kink gives the same result) and `scale`: for the tensors
    behind a BatchNorm backward, the same formula with every term taken by its magnitude (element by element) — what
    the result is measured against where dy - mean(dy) - xhat mean(dy xhat) cancels (two rows: to nearly 0)."""
    c = lambda v: None if v is None else v.detach().to(dtype)
    z, emb, mask, lin_w, lin_b, grad = c(z), c(emb), c(mask), c(lin_w), c(lin_b), c(grad)
    n, d = emb.shape
    e = emb.repeat(batch, 1)
    g1, g2 = bn1["weight"].to(dtype), bn2["weight"].to(dtype)
    y1, x1, inv1, new1 = _bn(z, bn1, dtype)
    a1 = torch.relu(y1)
    h1 = a1 * e
    y2, x2, inv2, new2 = _bn(h1, bn2, dtype)
    a2 = torch.relu(y2)
    act = a2 if mask is None else a2 * mask
    res = dict(y1=y1, y2=y2)
    if lin_w is None:
        res["act"] = act
        g_act = grad
    else:
        res["out"] = act @ lin_w + lin_b
        g_act = grad.view(-1, 1) * lin_w.view(1, d)
        res["d_lin_w"] = (grad.view(-1, 1) * act).sum(0)
        res["d_lin_b"] = grad.sum().view(1)
    d_a2 = g_act if mask is None else g_act * mask
    dy2 = d_a2 * (y2 > 0)
    res["d_bn2_b"], res["d_bn2_w"] = dy2.sum(0), (dy2 * x2).sum(0)
    dh1 = _bn_bwd(dy2, x2, inv2, g2)
    res["d_emb"] = (dh1 * a1).view(batch, n, d).sum(0)
    d_a1 = dh1 * e
    dy1 = d_a1 * (y1 > 0)
    res["d_bn1_b"], res["d_bn1_w"] = dy1.sum(0), (dy1 * x1).sum(0)
    res["d_z"] = _bn_bwd(dy1, x1, inv1, g1)
    res["live1"], res["live2"] = d_a1 != 0, d_a2 != 0
    for tag, new in (("1", new1), ("2", new2)):
        res["rm" + tag], res["rv" + tag], res["nbt" + tag] = new if new is not None else (None, None, None)
    # magnitudes of the uncancelled terms
    ab = torch.abs
    dh1_u = ab(g2 * inv2) * (ab(dy2) + ab(dy2).mean(0) + ab(x2) * ab(dy2 * x2).mean(0))
    dy1_u = dh1_u * ab(e) * (y1 > 0)
    d_z_u = ab(g1 * inv1) * (dy1_u + dy1_u.mean(0) + ab(x1) * (dy1_u * ab(x1)).mean(0))
    res["scale"] = dict(d_emb=(dh1_u * a1).view(batch, n, d).sum(0), d_bn1_b=dy1_u.sum(0),
                        d_bn1_w=(dy1_u * ab(x1)).sum(0), d_z=d_z_u)
    return res


def torch_chain(z, emb, bn1, bn2, mask, lin_w, lin_b, grad, batch, dtype=F64):
    """The same stage as a module chain: nn.BatchNorm1d x 2 in train mode built with the same momentum / eps / running
    buffers, the model's permutes (models/GDN.py:178-180), autograd for the gradients.  Keys as head_f64's."""
    n, d = emb.shape
    mods = []
    for bn in (bn1, bn2):
        track = bn.get("running_mean") is not None
        m = torch.nn.BatchNorm1d(d, eps=bn["eps"], momentum=bn["momentum"], track_running_stats=track).to(dtype)
        with torch.no_grad():
            m.weight.copy_(bn["weight"]); m.bias.copy_(bn["bias"])
            if track:
                m.running_mean.copy_(bn["running_mean"]); m.running_var.copy_(bn["running_var"])
                m.num_batches_tracked.fill_(bn["batches"])
        mods.append(m.train())
    m1, m2 = mods
    leaf = lambda v: v.detach().to(dtype).clone().requires_grad_(True)
    zz, ee = leaf(z), leaf(emb)
    h = torch.relu(m1(zz)).view(batch, n, d) * ee
    h = torch.relu(m2(h.permute(0, 2, 1))).permute(0, 2, 1).reshape(batch * n, d)
    act = h if mask is None else h * mask.to(dtype)
    res = {}
    if lin_w is None:
        res["act"] = act.detach()
        act.backward(grad.to(dtype))
    else:
        lin = torch.nn.Linear(d, 1).to(dtype)
        with torch.no_grad():
            lin.weight.copy_(lin_w.view(1, d)); lin.bias.copy_(lin_b)
        out = lin(act).view(-1)
        res["out"] = out.detach()
        out.backward(grad.to(dtype))
        res["d_lin_w"], res["d_lin_b"] = lin.weight.grad.view(d), lin.bias.grad
    res.update(d_z=zz.grad, d_emb=ee.grad, d_bn1_w=m1.weight.grad, d_bn1_b=m1.bias.grad, d_bn2_w=m2.weight.grad,
               d_bn2_b=m2.bias.grad)
    for tag, m in (("1", m1), ("2", m2)):
        track = m.running_mean is not None
        res["rm" + tag] = m.running_mean.detach() if track else None
        res["rv" + tag] = m.running_var.detach() if track else None
        res["nbt" + tag] = int(m.num_batches_tracked) if track else None
    return res


def kink_elements(y1, y2, live=None):
    """bool [rows, d]: elements whose derivative matters (`live` = (live1, live2) of head_f64; None: every element) and
    whose pre-activation in front of either ReLU lies inside _grad_check.KINK_BAND — fp32 may land on the other side."""
    l1, l2 = (True, True) if live is None else live
    return ((y1.abs() < KINK_BAND) & l1) | ((y2.abs() < KINK_BAND) & l2)
