"""numpy restatement of the bracket tiers of select_onewg_kernel (gdn_amd/csrc/gdn_score.hip): the one-span tier in
front of the three-interval tier of tests/_select_bracket_ref.py, whose inputs, sample and brackets it shares.

Tier rule (decided from the sorted sample alone, before any pass over the row): the one-span tier runs when its bin
shift is at most the smallest shift of the (used) intervals plus SPAN_SLACK and the span is wider than one hi word.
Why: a bin of the three-interval tier holds ~15 keys at its own shift; a span bin at most 4 x as wide keeps the six
ranks' bins far below CAP2 wherever the keys between the brackets are about as dense as inside them, and rows whose
brackets lie far apart (a level shift, two clusters: shifts 3 or more apart in the shared cases against <= 1 on every
i.i.d. row) do not pay for a pass that cannot settle them.  It falls through to the three-interval
tier when the rule rejects it, when a rank lies outside the span's histogram, or when more than CAP2 keys share the
ranks' bins; the three-interval tier falls back to the digit passes as before."""
import numpy as np

import _select_bracket_ref as ref
from _select_bracket_ref import FILLER, CAP2, GROUPS, T_CASES, make_cases, to_bits, brackets   # noqa: F401 (shared)

SPAN_BINS = 2048
SPAN_SLACK = 2
TIER_SPAN, TIER_INTERVALS, TIER_DIGITS = 0, 1, 2


def shift_for(width, bins):
    """smallest s with width >> s < bins (bins a power of two)"""
    return 0 if width < bins else width.bit_length() - (bins.bit_length() - 1)


def span_rule(L, H):
    """(L, H of the span, its shift, whether the one-span tier is chosen) from the merged intervals L[i], H[i]:
    the span runs from the lower edge of the q25 bracket (the first interval's) to the upper edge of the q75 bracket
    (the last interval's)."""
    lo, up = L[0], H[-1]
    s_span = shift_for(up - lo, SPAN_BINS)
    s_min = min(shift_for(H[i] - L[i], 512) for i in range(len(L)))
    return lo, up, s_span, up != lo and s_span <= s_min + SPAN_SLACK      # a span of one hi word separates nothing


def emulate(bits, total, c=ref.C):
    """One row of slots (uint64 bit patterns) -> (six order statistics as uint64, path, tier)."""
    bits = np.asarray(bits, dtype=np.uint64)

    def fall_through():
        vals, path = ref.emulate(bits, total, c)
        return vals, path, TIER_INTERVALS if path == 0 else TIER_DIGITS

    br = brackets(bits, total, c)
    if br is None:
        return fall_through()
    hi, L, H, _ = br
    lo, up, sh, chosen = span_rule(L, H)
    if not chosen:
        return fall_through()
    rk, _, _ = ref.ranks(total)
    h64 = hi.astype(np.int64)
    inside = (h64 >= lo) & (h64 <= up)                         # the filler (all ones) is above every span
    bins = np.full(bits.size, -1, dtype=np.int64)
    bins[inside] = (h64[inside] - lo) >> sh
    below = int((h64 < lo).sum())
    hist = np.bincount(bins[inside], minlength=SPAN_BINS)
    cum = np.cumsum(hist)
    code, rem = [], []
    for q in range(6):
        want = rk[q] - below
        if want < 0 or want >= cum[-1]:
            return fall_through()                              # the rank lies outside the span
        b = int(np.searchsorted(cum, want, side="right"))
        code.append(b)
        rem.append(want - int(cum[b] - hist[b]))
    # staging: three range tests, one per adjacent rank pair (the bins between a pair's two bins are empty)
    keep = np.zeros(bits.size, dtype=bool)
    for a in (2, 0, 4):
        keep |= (bins >= code[a]) & (bins <= code[a + 1])
    assert int(keep.sum()) == int(np.isin(bins, code).sum())
    if int(keep.sum()) > CAP2:
        return fall_through()
    vals = [np.sort(bits[bins == code[q]])[rem[q]] for q in range(6)]
    return np.array(vals, dtype=np.uint64), 0, TIER_SPAN


def extra_rows(t, seed=0):
    """name -> float32 errors [t]: rows beside the shared cases that the GPU test of the one-span tier also runs."""
    g = np.random.default_rng(7000 * seed + t)
    f32 = np.float32
    c = {}
    c["abs_normal"] = np.abs(g.standard_normal(t)).astype(f32)
    c["abs_uniform_difference"] = np.abs(g.random(t) - g.random(t)).astype(f32)
    act = (np.exp(g.standard_normal(t)) * 1e-3).astype(f32)    # an actuator: idle 40 % of the time, exact zeros
    act[g.random(t) < 0.4] = 0.0
    c["zeros_and_lognormal"] = act
    return c


def rank_past_the_span(t=32768, seed=3):
    """A row whose q75-hi rank lies just past the span's last bin: the strided sample sees uniform keys in [0, 1), but
    the unsampled slots hold so many small keys that every rank moves up; the keys above the sample's q75 bracket
    are placed so that rank q75-hi is the first key above H.  Returns float32 errors [t]."""
    g = np.random.default_rng(seed)
    err = g.random(t).astype(np.float32)
    bits = to_bits(err)
    hi, L, H, _ = brackets(bits, t)
    up = H[-1]
    rk, _, _ = ref.ranks(t)
    free = np.setdiff1d(np.arange(t), ref.sampled_slots(t))
    h64 = hi.astype(np.int64)
    # keys at or below H: exactly rk[5] of them must remain, so that rank rk[5] (0-based) is the first key above H
    at_or_below = int((h64 <= up).sum())
    move = at_or_below - rk[5]
    assert move > 0
    cand = free[h64[free] <= up]
    err[g.choice(cand, size=move, replace=False)] = np.float32(0.999)   # above H (H is a ~0.83 sample quantile)
    assert (to_bits(err)[ref.sampled_slots(t)] == bits[ref.sampled_slots(t)]).all()
    return err
