"""Float64 numpy restatement of the raw-readings front end (include/gdn_hip.h "Raw readings"): what
gdn_prep_stats / gdn_prep_series / gdn_prep_ticks and gdn_amd.prep.Prep must compute.  Raw data is tick-major
[t_raw, n]; a reading that is not finite is missing."""
import math

import numpy as np

EPS10 = 10.0 * np.finfo(np.float64).eps


def stats(raw):
    """[n, 4] float64 (min, max, mean, count) over the finite readings; zeros for a sensor with none.  The mean is
    the correctly rounded one (math.fsum)."""
    raw = np.asarray(raw, dtype=np.float64)
    out = np.zeros((raw.shape[1], 4))
    for i in range(raw.shape[1]):
        v = raw[np.isfinite(raw[:, i]), i]
        if v.size:
            out[i] = (v.min(), v.max(), fsum_mean(v), v.size)
    return out


def fsum_mean(v):
    return math.fsum(float(x) for x in v) / len(v)


def table(st):
    """MinMaxScaler(0, 1): scale = 1 / range (range = 1 below 10 eps), offset = 0 - min * scale."""
    rng = st[:, 1] - st[:, 0]
    rng = np.where(rng < EPS10, 1.0, rng)
    scale = 1.0 / rng
    return np.stack([scale, 0.0 - st[:, 0] * scale], axis=1)


def _median(v):
    """np.median spelled out: the middle value, or (lo + hi) / 2.0 of the middle pair; NaN for no value."""
    if v.size == 0:
        return np.nan
    s = np.sort(v)
    c = s.size
    return s[c // 2] if c % 2 else (s[c // 2 - 1] + s[c // 2]) / 2.0


def series(raw, tab, down, fill=None, labels=None):
    """(series [n, T] fp32, labels [T] float64 or None, filled [n, T] bool: the group held a filled reading)."""
    raw = np.asarray(raw, dtype=np.float64)
    t_raw, n = raw.shape
    T = t_raw // down
    gone = ~np.isfinite(raw)
    x = raw.copy()
    if fill is not None:
        x = np.where(gone, np.asarray(fill, dtype=np.float64)[None, :], x)
    ok = np.isfinite(x)
    v = np.where(ok, x, 0.0) * tab[None, :, 0]                       # two roundings: the product, then the sum
    v = v + tab[None, :, 1]
    out = np.empty((n, T), dtype=np.float32)
    filled = np.zeros((n, T), dtype=bool)
    for i in range(n):
        for g in range(T):
            rows = slice(g * down, (g + 1) * down)
            out[i, g] = np.float32(_median(v[rows, i][ok[rows, i]]))
            filled[i, g] = fill is not None and gone[rows, i].any()
    lab = None
    if labels is not None:
        lab = np.round(np.max(np.asarray(labels, dtype=np.float64)[:T * down].reshape(T, down), axis=1))
    return out, lab, filled


def raw_pushes(pending, r, down, chunk):
    """Brute force of harness.raw_push_plan: hand the raw ticks over one at a time.  A sub-push ends when `chunk`
    groups are complete or the ticks run out; (raw_rows, groups, new_pending, replayable)."""
    plan, rows, groups, open_ticks, start = [], 0, 0, pending, pending
    for _ in range(r):
        rows += 1
        open_ticks += 1
        if open_ticks == down:
            open_ticks, groups = 0, groups + 1
        if groups == chunk:
            plan.append((rows, groups, open_ticks, start == 0 and rows == chunk * down))
            rows, groups, start = 0, 0, open_ticks
    if rows:
        plan.append((rows, groups, open_ticks, False))
    return plan


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)


def assert_filled_rule(got, want64, filled):
    """The rule of the NaN pair: `got` [n, T] fp32 against the reference's float64 output.  Where the group holds no
    filled reading the bits are equal.  Elsewhere pandas' mean and a correctly rounded one differ far below half an
    fp32 ulp (a few float64 ulps of a value that is then scaled by at most 1 / range), so the two fp32 roundings are
    the same or neighbours: at most 1 fp32 ulp."""
    want = want64.astype(np.float32)
    assert np.array_equal(bits32(got)[~filled], bits32(want)[~filled])
    assert np.isfinite(got[filled]).all()
    assert (np.abs(bits32(got)[filled] - bits32(want)[filled]) <= 1).all()
