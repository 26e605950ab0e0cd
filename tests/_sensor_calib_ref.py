"""TEST INFRASTRUCTURE: the float64 yardstick of the calibration on each sensor's own readings (numpy), written from
the contract of DESIGN §3.5e and not from the kernels.  Hold and validity are those of tests/_series_gaps_ref.py
(imported); what changes is rule 4: sensor s's median / IQR row comes from the ticks at which SENSOR s reported, so
every sensor has its own count.  The ring is the `_sensor` write said in numpy: a tick excluded by its alarm leaves
the filler in all n keys and keep = 0, any other tick keep = 1, its keys where the reading is real and the filler
where it is missing."""
import numpy as np

from _series_gaps_ref import fill, missing, scores  # noqa: F401  (hold, validity and the score sweep: one source)
from _stream_recal_ref import keys_of

FILLER = np.uint64(0xffffffffffffffff)


def row(values):
    """(median, IQR) of one sensor's real errors: np.median and the 'linear' 75th - 25th percentile."""
    values = np.asarray(values, dtype=np.float64)
    q75, q25 = np.percentile(values, [75, 25], method="linear")
    return np.array([np.median(values), q75 - q25])


def table(pred, gt, valid, min_count=1, before=None):
    """med_iqr [n, 2] float64 and counts [n] int64.  pred, gt [t, n] fp32, valid [t, n] bool.  A sensor with fewer
    than max(min_count, 1) real readings keeps its row of `before` (NaN without one)."""
    delta = keys_of(pred, gt)
    valid = np.asarray(valid, dtype=bool)
    n = delta.shape[1]
    out = np.full((n, 2), np.nan) if before is None else np.array(before, dtype=np.float64, copy=True)
    counts = valid.sum(axis=0).astype(np.int64)
    for s in range(n):
        if counts[s] >= max(min_count, 1):
            out[s] = row(delta[valid[:, s], s])
    return out, counts


def table_of_keys(keys, min_count=1, before=None):
    """The same from a key plane [n, slots] float64 whose filler slots (all ones) do not count."""
    bits = np.ascontiguousarray(keys, dtype=np.float64).view(np.uint64)
    n = bits.shape[0]
    out = np.full((n, 2), np.nan) if before is None else np.array(before, dtype=np.float64, copy=True)
    real = bits != FILLER
    counts = real.sum(axis=1).astype(np.int64)
    for s in range(n):
        if counts[s] >= max(min_count, 1):
            out[s] = row(np.asarray(keys, dtype=np.float64)[s][real[s]])
    return out, counts


def keys_valid(pred, gt, valid, pitch):
    """gdn_score_keys_valid: [n, pitch] uint64 bit patterns."""
    delta = keys_of(pred, gt)
    t, n = delta.shape
    out = np.full((n, pitch), FILLER, dtype=np.uint64)
    real = np.ascontiguousarray(delta.T).view(np.uint64)
    real[~np.asarray(valid, dtype=bool).T] = FILLER
    out[:, :t] = real
    return out


class SensorRing:
    """The calibration ring under the `_sensor` write: tick j owns slot j mod R."""

    def __init__(self, n, R, exclude_alarms=True):
        self.n, self.R, self.exclude = n, R, exclude_alarms
        self.keys = np.full((n, R), FILLER, dtype=np.uint64)
        self.keep = np.zeros(R, dtype=np.uint8)
        self.ticks = 0

    def seed(self, pred, gt, valid):
        """from_calibration: the last s = min(R, t) ticks into slots R - s .. R - 1, every one kept."""
        s = min(self.R, np.asarray(pred).shape[0])
        self.keys[:, self.R - s:] = keys_valid(pred[-s:], gt[-s:], valid[-s:], s)
        self.keep[self.R - s:] = 1

    def push(self, pred, gt, alarm, valid):
        delta = keys_of(pred, gt).view(np.uint64)
        for b in range(delta.shape[0]):
            slot = (self.ticks + b) % self.R
            out = self.exclude and alarm[b] != 0
            self.keep[slot] = 0 if out else 1
            self.keys[:, slot] = FILLER if out else np.where(np.asarray(valid[b], dtype=bool), delta[b], FILLER)
        self.ticks += delta.shape[0]

    def table(self, min_count, before):
        return table_of_keys(self.keys.view(np.float64), min_count, before)


def motivating_mask(n=40, t=1500, share=0.1, seed=2025):
    """valid [t, n] bool: every reading dropped independently with probability `share`.  At n = 40, share = 0.1 a tick
    is complete with probability 0.9^40 = 0.0148: about 22 of 1500, while every sensor keeps about 1350."""
    return np.random.default_rng(seed).random((t, n)) >= share


def motivating_series(n=40, w=8, t=1500, share=0.1, seed=2025):
    """raw [n, w + t] fp32 in [0, 1) with NaN wherever motivating_mask drops the reading; the first w ticks are real."""
    raw = np.random.default_rng(seed + 1).random((n, w + t)).astype(np.float32)
    raw[:, w:][~motivating_mask(n, t, share, seed).T] = np.nan
    return raw
