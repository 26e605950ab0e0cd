"""The numpy yardstick of the threshold a calibration ring supports (include/gdn_hip.h "Threshold from
the ring"): the rule stated once, slot by slot, in float64 with separate roundings — what gdn_fleet_ring_threshold
must compute per unit.  No device, no project code."""
import numpy as np

FILLER = np.uint64(0xFFFFFFFFFFFFFFFF)          # gdn_sweep::FILLER: the key of a slot that holds no reading


def ring_errors(ring_keys, med_iqr, by_sensor: bool):
    """error[s, q] = (key - median_s) * (1 / (|iqr_s| + 1e-2)): the scorer's expression and its reciprocal-multiply;
    `by_sensor`: a key that is the filler bit pattern is a missing reading, error exactly 0.0."""
    keys = np.ascontiguousarray(ring_keys, dtype=np.float64)
    med = np.asarray(med_iqr, dtype=np.float64)[:, 0:1]
    inv_den = 1.0 / (np.abs(np.asarray(med_iqr, dtype=np.float64)[:, 1:2]) + 1e-2)
    with np.errstate(invalid="ignore"):
        err = (keys - med) * inv_den
    if by_sensor:
        err = np.where(keys.view(np.uint64) == FILLER, 0.0, err)
    return err


def ring_scores(ring_keys, med_iqr, by_sensor: bool):
    """score[q] = max over sensors of (((e[q-3] + e[q-2]) + e[q-1]) + e[q]) / 4.0, slots mod R; a NaN never wins (the
    maximum starts from -inf)."""
    e = ring_errors(ring_keys, med_iqr, by_sensor)
    with np.errstate(invalid="ignore"):
        sm = (((np.roll(e, 3, axis=1) + np.roll(e, 2, axis=1)) + np.roll(e, 1, axis=1)) + e) / 4.0
    return np.fmax.reduce(np.concatenate([np.full((1, sm.shape[1]), -np.inf), sm], axis=0), axis=0)


def ring_eligible(ring_keep, base: int):
    """eligible[q]: keep is 1 at q, q-1, q-2, q-3 (mod R) and (q - base) mod R >= 3."""
    k = np.asarray(ring_keep) != 0
    R = k.shape[0]
    age = (np.arange(R) - int(base)) % R
    return k & np.roll(k, 1) & np.roll(k, 2) & np.roll(k, 3) & (age >= 3)


def ring_peak(ring_keys, ring_keep, med_iqr, base: int, by_sensor: bool = False):
    """(peak, eligible, peak_slot) of one unit: the largest score of an eligible slot (-inf: none), how many slots are
    eligible, the smallest slot that attains the peak (-1: none does)."""
    score, ok = ring_scores(ring_keys, med_iqr, by_sensor), ring_eligible(ring_keep, base)
    if not ok.any():
        return -np.inf, 0, -1
    peak = float(np.max(score[ok]))
    at = np.nonzero(ok & (score == peak))[0]
    return peak, int(ok.sum()), int(at[0]) if at.size else -1


def ring_threshold(threshold, peak, eligible, margin: float, min_eligible: int, selected: bool = True):
    """The threshold after the step: peak * margin (one float64 multiply) iff the unit was selected, eligible >=
    min_eligible and peak is finite and > 0; else `threshold` as it was."""
    if selected and eligible >= min_eligible and np.isfinite(peak) and peak > 0:
        return float(np.float64(peak) * np.float64(margin))
    return float(threshold)
