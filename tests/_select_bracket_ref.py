"""numpy restatement of the bracket path of select_onewg_kernel (gdn_amd/csrc/gdn_score.hip) and the inputs that the
CPU and GPU tests of it share.  Keys are the float64 bit patterns of |pred - gt| (non-negative: they order like
unsigned integers); FILLER marks a slot without a key."""
import numpy as np

S = 1024                 # BR_S
C = 2.62                 # BR_C
CAP2 = 1024              # ONE_CAP2
FILLER = np.uint64(0xFFFFFFFFFFFFFFFF)
NONE = 0xFFFF
T_CASES = [3000, 4 * S - 1, 4 * S, 4 * S + 1, 8191, 32768]     # 3000 and 4S-1: below the threshold (digit passes)


def ranks(t):
    """make_select_args: the six 0-based ranks (median lo/hi, q25 lo/hi, q75 lo/hi), gamma of the two percentiles."""
    pair = t % 2 == 0
    rk = [t // 2 - 1 if pair else (t - 1) // 2, t // 2 if pair else (t - 1) // 2]
    gamma = []
    for q in (0.25, 0.75):
        vi = t * q + (1.0 + q * (1.0 - 1.0 - 1.0)) - 1.0
        lo = int(np.floor(vi))
        rk += [min(max(lo, 0), t - 1), min(lo + 1, t - 1)]
        gamma.append(vi - np.floor(vi))
    return rk, gamma, pair


def med_iqr_from(vals, t):
    """write_result: numpy's median and 'linear' percentiles from the six order statistics."""
    _, gamma, pair = ranks(t)
    v = np.asarray(vals, dtype=np.uint64).view(np.float64)
    med = (v[0] + v[1]) / 2.0 if pair else v[0]
    qv = []
    for h in range(2):
        a, b, g = v[2 + 2 * h], v[3 + 2 * h], gamma[h]
        diff = b - a
        qv.append(b - diff * (1.0 - g) if g >= 0.5 else a + diff * g)
    return np.array([med, qv[1] - qv[0]])


def numpy_med_iqr(keys):
    keys = np.asarray(keys, dtype=np.float64)
    return np.array([np.median(keys), np.percentile(keys, 75) - np.percentile(keys, 25)])


def brackets(bits, total, c=C):
    """Steps 1-2: the sorted hi-word sample and the merged intervals.  None when the row does not try them."""
    slots = bits.size
    hi = (bits >> np.uint64(32)).astype(np.uint32)
    if total < 4 * S:
        return None
    smp = np.sort(hi[(np.arange(S, dtype=np.int64) * slots) // S])
    m = int((smp != 0xFFFFFFFF).sum())
    if m < S // 2:
        return None
    rk, _, _ = ranks(total)
    fm, ft = np.float32(m), np.float32(total)
    margin = int(np.float32(c) * np.sqrt(fm)) + 2
    lo, up = [], []
    for first in (2, 0, 4):                                   # q25, median, q75: ascending
        li = int(np.float32(rk[first]) * fm / ft) - margin
        ui = int(np.float32(rk[first + 1]) * fm / ft) + 1 + margin
        lo.append(0 if li < 0 else int(smp[li]))
        up.append(0x7FFFFFFF if ui >= m else int(smp[ui]))
    L, H, iv = [lo[0]], [up[0]], [0]
    for g in (1, 2):
        if lo[g] <= H[-1]:
            H[-1] = up[g]
        else:
            L.append(lo[g])
            H.append(up[g])
        iv.append(len(L) - 1)
    return hi, L, H, {0: iv[1], 1: iv[1], 2: 0, 3: 0, 4: iv[2], 5: iv[2]}


def emulate(bits, total, c=C):
    """Steps 1-5 for one row of slots (uint64 bit patterns).  Returns (six order statistics as uint64, path)."""
    bits = np.asarray(bits, dtype=np.uint64)
    rk, _, _ = ranks(total)

    def fallback():
        return np.sort(bits[bits != FILLER])[rk], 1

    br = brackets(bits, total, c)
    if br is None:
        return fallback()
    hi, L, H, iv_of = br
    h64 = hi.astype(np.int64)
    codes = np.full(bits.size, NONE, dtype=np.int64)
    below = []
    for i in reversed(range(len(L))):
        w = H[i] - L[i]
        sh = 0 if w < 512 else w.bit_length() - 9
        inside = (h64 >= L[i]) & (h64 <= H[i])
        codes[inside] = 512 * i + ((h64[inside] - L[i]) >> sh)
    for i in range(len(L)):
        below.append(int((h64 < L[i]).sum()))
    hist = np.bincount(codes[codes != NONE], minlength=3 * 512)
    code, rem = [], []
    for q in range(6):
        i = iv_of[q]
        h = hist[512 * i: 512 * i + 512]
        cum = np.cumsum(h)
        want = rk[q] - below[i]
        if want < 0 or want >= cum[-1]:
            return fallback()                                  # the rank lies outside its bracket
        b = int(np.searchsorted(cum, want, side="right"))
        code.append(512 * i + b)
        rem.append(want - int(cum[b] - h[b]))
    if int(np.isin(codes, code).sum()) > CAP2:
        return fallback()
    vals = [np.sort(bits[codes == code[q]])[rem[q]] for q in range(6)]
    return np.array(vals, dtype=np.uint64), 0


def to_bits(err32):
    """float32 errors -> the keys the keys kernel builds from pred = 0, gt = err: |0 - err| in float64."""
    return np.abs(0.0 - np.asarray(err32, dtype=np.float32).astype(np.float64)).view(np.uint64)


def sampled_slots(t):
    return (np.arange(S, dtype=np.int64) * t) // S


def make_cases(t, seed=0):
    """name -> float32 errors [t], one sensor each."""
    g = np.random.default_rng(1000 * seed + t)
    f32 = np.float32
    c = {}
    c["uniform"] = g.random(t).astype(f32)
    c["lognormal"] = np.exp(g.standard_normal(t)).astype(f32)
    c["uniform_small"] = (g.random(t) * 1e-3).astype(f32)
    c["ramp"] = (np.arange(t) * 1e-6).astype(f32)
    shift = g.random(t)
    shift[t // 2:] += 5.0
    c["level_shift"] = shift.astype(f32)
    eq = g.random(t).astype(f32)
    eq[sampled_slots(t)] = 0.5                                # the sample sees one value, the row has many
    c["sample_all_equal"] = eq
    c["all_equal"] = np.full(t, 0.25, dtype=f32)
    outlier = (g.random(t) * 1e-3).astype(f32)
    outlier[0] = 5e4
    c["outlier_at_slot_0"] = outlier
    # heavy ties exactly at a bracket edge: 1500 unsampled slots take the value of the sample key that bounds the
    # median bracket from below (found with the restatement of steps 1-2 on the untied row; the sample is unchanged)
    tied = g.random(t).astype(f32)
    br = brackets(to_bits(tied), t)
    if br is not None:
        _, L, _, iv_of = br
        smp_vals = np.sort(tied[sampled_slots(t)])
        edge = smp_vals[np.searchsorted((to_bits(smp_vals) >> np.uint64(32)).astype(np.int64), L[iv_of[0]])]
    else:
        edge = f32(0.4)
    free = np.setdiff1d(np.arange(t), sampled_slots(t))
    tied[g.choice(free, size=min(1500, free.size), replace=False)] = edge
    c["ties_at_bracket_edge"] = tied
    # two far clusters, the median pair straddling the gap (t even) or the median the last key of the low cluster
    low = (t + 1) // 2
    cl = np.concatenate([1e-30 * (1.0 + g.random(low)), 1e30 * (1.0 + g.random(t - low))])
    c["two_far_clusters"] = g.permutation(cl).astype(f32)
    c["denormals"] = (g.random(t) * 1e-38).astype(f32)
    c["hundred_binades"] = np.clip(np.exp(12.0 * g.standard_normal(t)), 1e-30, 1e30).astype(f32)
    return c


GROUPS = {
    "iid": ["uniform", "lognormal", "uniform_small"],
    "nonstationary": ["ramp", "level_shift", "sample_all_equal", "all_equal", "outlier_at_slot_0"],
    "edges": ["ties_at_bracket_edge", "two_far_clusters", "denormals", "hundred_binades"],
}
