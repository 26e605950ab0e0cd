"""TEST INFRASTRUCTURE: the float64 yardstick of training on a resident series with missing readings (numpy /
float64 torch), written from the contract of DESIGN §3.4c and not from the kernels.

1. Missing.  A reading is missing when (bits & 0x7f800000) == 0x7f800000.
2. Hold.  The series is filled ONCE (each missing reading at its sensor's latest earlier real one); every window and
   every target is cut from the filled series; raw[:, :w] must be real.
3. Masked loss.  For windows b with target ticks t_b: v[b, i] = valid[t_b - w, i], m = sum(v),
   loss = sum_{v=1} (out - y)^2 / m, d_out = 2 (out - y) / m where v = 1 and EXACTLY 0.0 where v = 0 (a select: what a
   masked slot holds never reaches either); m = 0: loss 0, d_out zeros.  Only the loss is masked.
4. With every v = 1 this is F.mse_loss(reduction='mean') and its gradient.
5. Validation.  A logical minibatch's loss is its masked mean; a minibatch without a real target is left out of
   sum(losses) / len(losses); none with a real target: 0.0."""
import numpy as np
import torch


def missing(raw):
    """Rule 1, on the bit pattern (NaN with any payload, +inf, -inf)."""
    bits = np.ascontiguousarray(raw, dtype=np.float32).view(np.uint32)
    return (bits & np.uint32(0x7f800000)) == np.uint32(0x7f800000)


def fill(raw, w):
    """Rule 2: raw [n, T] fp32 -> (filled [n, T] fp32, valid [T - w, n] uint8 time-major).  One column after the other."""
    raw = np.ascontiguousarray(raw, dtype=np.float32)
    gone = missing(raw)
    if gone[:, :w].any():
        raise ValueError("series: the first w ticks must be real readings (gaps)")
    filled = raw.copy()
    for c in range(w, raw.shape[1]):
        filled[:, c] = np.where(gone[:, c], filled[:, c - 1], raw[:, c])
    return filled, np.ascontiguousarray((~gone[:, w:]).T).astype(np.uint8)


def gather(filled, valid, ticks, w, batch=None):
    """(x [B, n, w] fp32, y [B, n] fp32, v [B, n] uint8, row_valid [B] int32) of target ticks `ticks` (B = `batch` or
    len(ticks)): windows and targets from the filled series, v = valid[t - w].  A window beyond `ticks`, or a tick
    outside [w, T), is zeros throughout."""
    filled = np.asarray(filled, dtype=np.float32)
    n, t_len = filled.shape
    ticks = [int(t) for t in np.asarray(ticks).reshape(-1)]
    b_all = len(ticks) if batch is None else batch
    x = np.zeros((b_all, n, w), dtype=np.float32)
    y = np.zeros((b_all, n), dtype=np.float32)
    v = np.zeros((b_all, n), dtype=np.uint8)
    for b, t in enumerate(ticks[:b_all]):
        if w <= t < t_len:
            x[b], y[b], v[b] = filled[:, t - w:t], filled[:, t], valid[t - w]
    return x, y, v, v.sum(axis=1).astype(np.int32)


def masked_loss(out, y, v):
    """Rule 3 in float64 with a loop-free select: (loss, d_out [B, n] float64, m)."""
    out, y, keep = np.asarray(out, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(v) != 0
    m = int(keep.sum())
    if m == 0:
        return 0.0, np.zeros(out.shape), 0
    diff = np.where(keep, out, 0.0) - np.where(keep, y, 0.0)       # masked slots replaced BEFORE the arithmetic
    return float((diff ** 2).sum() / m), 2.0 * diff / m, m


def masked_loss_loop(out, y, v):
    """Rule 3 as a plain float64 loop (the restatement's own check)."""
    out, y, v = np.asarray(out, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(v)
    total, m = 0.0, 0
    for idx in np.ndindex(out.shape):
        if v[idx]:
            total += (out[idx] - y[idx]) ** 2
            m += 1
    return (total / m if m else 0.0), m


def masked_loss_autograd(out, y, v):
    """Rule 3 through float64 autograd: (loss, d_out) of loss = sum(where(v, (out - y)^2, 0)) / m, on the CPU.  Masked
    slots are replaced BEFORE the arithmetic, so what they hold (nan, inf) reaches neither the loss nor the gradient."""
    keep = torch.as_tensor(np.asarray(v) != 0)
    o = torch.as_tensor(np.asarray(out, dtype=np.float64)).clone().requires_grad_(True)
    t = torch.as_tensor(np.asarray(y, dtype=np.float64))
    m = int(keep.sum())
    if m == 0:
        return 0.0, np.zeros(tuple(o.shape))
    zero = torch.zeros((), dtype=torch.float64)
    diff = torch.where(keep, o, zero) - torch.where(keep, t, zero)
    loss = (diff ** 2).sum() / m
    loss.backward()
    return float(loss.detach()), o.grad.numpy()


def masked_batch_means(pred, y, v, batch):
    """Rule 5: (batch_means float64 [ceil(rows / batch)], batch_counts int64, mean float64).  The difference is formed in
    fp32 (as F.mse_loss forms it in the tensors' type) and squared in float64."""
    pred, y, keep = np.asarray(pred, dtype=np.float32), np.asarray(y, dtype=np.float32), np.asarray(v) != 0
    means, counts = [], []
    for s in range(0, pred.shape[0], batch):
        k = keep[s:s + batch]
        with np.errstate(invalid="ignore", over="ignore"):
            diff = (pred[s:s + batch] - y[s:s + batch]).astype(np.float32)
        sq = np.where(k, np.where(k, diff, np.float32(0)).astype(np.float64) ** 2, 0.0)
        counts.append(int(k.sum()))
        means.append(sq.sum() / counts[-1] if counts[-1] else 0.0)
    means, counts = np.asarray(means, dtype=np.float64), np.asarray(counts, dtype=np.int64)
    used = counts > 0
    return means, counts, (float(means[used].sum() / used.sum()) if used.any() else 0.0)


def burst_series(clean, w, share, length, seed=0, keep_clear=()):
    """A copy of clean [n, T] fp32 with about `share` of the readings after tick w missing (NaN), in bursts of `length`
    ticks on one sensor; ticks in `keep_clear` stay real."""
    raw = np.array(clean, dtype=np.float32, copy=True)
    n, t_len = raw.shape
    rng = np.random.default_rng(seed)
    for _ in range(max(1, int(round(share * n * (t_len - w) / length)))):
        at = int(rng.integers(w, t_len - length + 1))
        raw[int(rng.integers(0, n)), at:at + length] = np.nan
    for t in keep_clear:
        raw[:, t] = np.asarray(clean)[:, t]
    return raw


def burst_mask(shape, share, length, seed=0):
    """[B, n] uint8 with about `share` zeros in runs of `length` along the flat index."""
    v = np.ones(int(np.prod(shape)), dtype=np.uint8)
    rng = np.random.default_rng(seed)
    for _ in range(max(1, int(round(share * v.size / length)))):
        at = int(rng.integers(0, max(1, v.size - length + 1)))
        v[at:at + length] = 0
    return v.reshape(shape)
