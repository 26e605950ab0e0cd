"""TEST INFRASTRUCTURE: the float64 yardstick of a resident series with missing readings (numpy), written from the
contract of DESIGN §3.5d and not from the kernels.  The series is raw [n, T_raw] fp32, t = T_raw - w ticks are scored,
tick j is column w + j.  A reading is missing when its exponent field is all ones; it is held at its sensor's latest
earlier real reading; its normalised error is exactly 0.0 wherever it is used; the median / IQR table comes from the
ticks whose n readings are all real.  Everything is the WHOLE-series form (no pushes, no carry):
tests/test_cpu_series_gaps.py pins it to tests/_stream_gaps_ref.py, the chunked form of the same rules."""
import numpy as np

from _stream_ref import SCORE_EPS

PATTERNS = ("a", "b", "c", "d", "e", "f")
LENGTHS = (37, 64, 65, 129, 300)
MIN_KEPT = 8


def missing(raw):
    """Rule 1, on the bit pattern: (bits & 0x7f800000) == 0x7f800000 (NaN with any payload, +inf, -inf)."""
    bits = np.ascontiguousarray(raw, dtype=np.float32).view(np.uint32)
    return (bits & np.uint32(0x7f800000)) == np.uint32(0x7f800000)


def fill(raw, w):
    """raw [n, T_raw] fp32 -> (filled [n, T_raw] fp32, gt [t, n] fp32, valid [t, n] bool, keep [t] bool,
    missing_total [n] int64, missing_run [n] int64); raw[:, :w] must be real.  One column after the other."""
    raw = np.ascontiguousarray(raw, dtype=np.float32)
    gone = missing(raw)
    if gone[:, :w].any():
        raise ValueError("series: the first w ticks must be real readings (gaps)")
    filled = raw.copy()
    run = np.zeros(raw.shape[0], dtype=np.int64)
    for c in range(w, raw.shape[1]):
        filled[:, c] = np.where(gone[:, c], filled[:, c - 1], raw[:, c])
        run = np.where(gone[:, c], run + 1, 0)
    valid = ~gone[:, w:].T
    return (filled, np.ascontiguousarray(filled[:, w:].T), np.ascontiguousarray(valid), valid.all(axis=1),
            gone[:, w:].sum(axis=1).astype(np.int64), run)


def table(pred, gt, keep):
    """Rule 4: med_iqr [n, 2] float64 = np.median and numpy-'linear' 75th - 25th percentile of |pred - gt| per sensor
    over the kept ticks (gdn_score_quantiles' arithmetic on the compacted rows)."""
    delta = np.abs(np.asarray(pred, dtype=np.float64) - np.asarray(gt, dtype=np.float64))[np.asarray(keep, dtype=bool)]
    q75, q25 = np.percentile(delta, [75, 25], axis=0)
    return np.stack([np.median(delta, axis=0), q75 - q25], axis=1)


def scores(pred, gt, valid, med_iqr, m=1):
    """Rule 3: (smoothed [n, t] float64, top values [t, m], top sensors [t, m]).  a = (|pred - gt| - med) / (|iqr| +
    eps), exactly 0.0 where the reading is missing; the mean of a tick and its three predecessors summed left to right;
    ticks 0 - 2 score 0; larger first, equal scores by the lower sensor."""
    mi = np.asarray(med_iqr, dtype=np.float64)
    delta = np.abs(np.asarray(pred, dtype=np.float64) - np.asarray(gt, dtype=np.float64))
    a = np.where(valid, (delta - mi[:, 0]) / (np.abs(mi[:, 1]) + SCORE_EPS), 0.0)
    sm = np.zeros(a.shape)
    sm[3:] = (((a[:-3] + a[1:-2]) + a[2:-1]) + a[3:]) / 4.0
    idx = np.argsort(-sm, axis=1, kind="stable")[:, :m]
    return sm.T.copy(), np.take_along_axis(sm, idx, axis=1), idx


def clean_series(n, w, t, seed=0):
    """[n, w + t] fp32 in [0, 1): the clean series every pattern is cut into."""
    return np.random.default_rng(1000 * seed + 7 * n + w + 31 * t).random((n, w + t)).astype(np.float32)


def with_pattern(clean, w, pattern, min_kept=MIN_KEPT):
    """The missing readings of the tests, one helper for all: a copy of clean [n, T_raw] with pattern
      a  no missing reading
      b  isolated readings: NaN, a NaN with a payload (and a negative one), +inf, -inf
      c  a run longer than w on one sensor
      d  a run of 140 ticks on one sensor that covers a whole 64-column block and the head of the next (t >= 300)
      e  one tick missing on every sensor
      f  missing at the first scored tick and at the last two (a trailing run)
    A pattern must leave at least `min_kept` complete ticks: checked here, on the CPU, as a condition on the inputs."""
    raw = np.array(clean, dtype=np.float32, copy=True)
    n, t_raw = raw.shape
    t = t_raw - w
    s = lambda j: j % n
    bits = raw.view(np.uint32)
    if pattern == "b":
        raw[s(0), w + 4] = np.nan
        bits[s(1), w + 9] = 0x7fc12345                               # a quiet NaN with a payload
        bits[s(1), w + 10] = 0x7f800001                              # a signalling pattern: the smallest mantissa
        bits[s(2), w + 17] = 0xffc00000                              # a negative NaN
        raw[s(3), w + 20] = np.inf
        raw[s(4), w + 26] = -np.inf
    elif pattern == "c":
        raw[s(2), w + 6:w + 6 + w + 3] = np.nan
    elif pattern == "d":
        assert t >= 300, "pattern d needs 300 scored ticks"
        raw[s(1), w + 70:w + 210] = np.nan
        assert (w + 70) <= 128 and (w + 210) > 192                   # block [128, 192) has no real reading of the sensor
    elif pattern == "e":
        raw[:, w + 11] = np.nan
        raw[s(3), w + 12] = np.inf                                   # (the tick after it too, on one sensor)
    elif pattern == "f":
        raw[s(0), w] = np.nan
        raw[s(4), w] = -np.inf
        raw[s(2), t_raw - 2:] = np.nan
        raw[s(0), t_raw - 1] = np.inf
    else:
        assert pattern == "a", pattern
    kept = int((~missing(raw)[:, w:]).all(axis=0).sum())
    assert kept >= min_kept, (pattern, kept, min_kept)
    assert not missing(raw)[:, :w].any()
    return raw


def bursts(clean, w, every=10, length=3, seed=0):
    """Bursts of `length` missing ticks on a random sensor, one about every `every` ticks: with 10 and 3 about 70 % of
    the ticks stay complete."""
    raw = np.array(clean, dtype=np.float32, copy=True)
    n, t_raw = raw.shape
    rng = np.random.default_rng(seed)
    for start in range(w + 2, t_raw - length, every):
        at = start + int(rng.integers(0, every - length))
        raw[int(rng.integers(0, n)), at:at + length] = np.nan
    return raw
