"""TEST INFRASTRUCTURE: the float64 yardstick of the streaming detector's rolling calibration (numpy), written from the
contract of DESIGN §3.8c and not from the kernels.  A ring of R slots keeps |pred - gt| of the last R stream ticks:
tick t owns slot t mod R whatever else happens; a tick is kept unless it alarmed (exclude_alarms) or a reading of it
was missing; a tick that is not kept leaves the filler in its slot.  The table is the median / IQR per sensor of the
kept keys (np.median, numpy 'linear' percentiles).  A slot's bits are compared (`bits`): the filler is a NaN pattern."""
import numpy as np

import _stream_ref

FILLER_BITS = np.uint64(0xFFFFFFFFFFFFFFFF)


def keys_of(pred, gt):
    """[t, n] fp32 pair -> |pred - gt| [t, n] in float64: both widened first, one subtraction, one fabs."""
    return np.abs(np.asarray(pred, dtype=np.float32).astype(np.float64) - np.asarray(gt, dtype=np.float32).astype(np.float64))


def bits(keys):
    return np.ascontiguousarray(keys, dtype=np.float64).view(np.uint64)


def default_min_ticks(R):
    return max(64, R // 4)


class CalibRing:
    """ring_keys [n, R] float64 and ring_keep [R] uint8 of a stream that starts at tick 0, both empty at first."""

    def __init__(self, n, R, exclude_alarms=True, min_ticks=None):
        self.n, self.R, self.exclude_alarms = int(n), int(R), bool(exclude_alarms)
        self.min_ticks = default_min_ticks(self.R) if min_ticks is None else int(min_ticks)
        assert self.min_ticks <= self.R
        self.keys = np.full((self.n, self.R), FILLER_BITS, dtype=np.uint64).view(np.float64)
        self.keep = np.zeros(self.R, dtype=np.uint8)
        self.ticks = 0

    def seed(self, pred, gt):
        """The last s = min(R, t) rows of a period normal by declaration, oldest first, into slots R - s .. R - 1, all
        kept (the stream then overwrites the empty slots first and the oldest seeded tick last)."""
        k = keys_of(pred, gt)
        s = min(self.R, len(k))
        if s:
            self.keys[:, self.R - s:] = k[len(k) - s:].T
            self.keep[self.R - s:] = 1
        return s

    def push(self, pred, gt, alarm, valid=None):
        """One push: pred / gt [c, n] fp32 (gt = the filled chunk under gaps), alarm [c] (the flags the score launch
        of this push wrote), valid [c, n] bool or None.  c <= R.  One tick after the other: the definition."""
        k = keys_of(pred, gt)
        assert len(k) <= self.R and k.shape[1] == self.n
        alarm = np.asarray(alarm).reshape(-1)
        for b in range(len(k)):
            slot = self.ticks % self.R
            kept = not (self.exclude_alarms and alarm[b] != 0)
            if valid is not None and not np.asarray(valid[b], dtype=bool).all():
                kept = False
            if kept:
                self.keys[:, slot] = k[b]
            else:
                self.keys.view(np.uint64)[:, slot] = FILLER_BITS      # (written as bits: a NaN payload)
            self.keep[slot] = 1 if kept else 0
            self.ticks += 1

    def total(self):
        return int(self.keep.sum())

    def kept_keys(self):
        """[n, total] float64: the kept keys in slot order (a quantile does not care)."""
        return self.keys[:, self.keep != 0]

    def table(self):
        """med_iqr [n, 2] of the kept keys: np.median; np.percentile 75 - 25, 'linear'."""
        k = self.kept_keys()
        q = np.percentile(k, [25, 75], axis=1, method="linear")
        return np.stack([np.median(k, axis=1), q[1] - q[0]], axis=1)

    def recalibrate(self, med_iqr):
        """Contract point 4 on a table [n, 2] float64 in place: the kept ticks, or 0 and nothing written."""
        total = self.total()
        if total < self.min_ticks:
            return 0
        med_iqr[...] = self.table()
        return total


def brute_force(pred, gt, alarm, R, exclude_alarms=True, valid=None):
    """The ring after the whole stream pred / gt [T, n], said another way: of the last min(R, T) ticks, tick t sits in
    slot t mod R when it is kept, the filler when it is not; every other slot is empty.  (keys, keep)."""
    k = keys_of(pred, gt)
    T, n = k.shape
    keys = np.full((n, R), FILLER_BITS, dtype=np.uint64).view(np.float64)
    keep = np.zeros(R, dtype=np.uint8)
    dropped = np.zeros(T, dtype=bool)
    if exclude_alarms:
        dropped |= np.asarray(alarm).reshape(-1) != 0
    if valid is not None:
        dropped |= ~np.asarray(valid, dtype=bool).all(axis=1)
    for t in range(max(0, T - R), T):
        if not dropped[t]:
            keys[:, t % R] = k[t]
            keep[t % R] = 1
    return keys, keep


# The stage test of the ring write alone (test_gpu_stream_recal.py): ONE launch on a ring full of a sentinel, from a
# staged tick counter.  The shapes are the smallest at which the 64 x 64 tile can go wrong: one sensor, a full tile, one
# past it, two tiles and one; one row, one short of a tile, a full tile, one past it (a second workgroup).
SENTINEL_KEY, SENTINEL_KEEP = 123.0, 9
STAGE_N = (1, 64, 65, 129)
STAGE_COUNT_R = [(count, R) for R in (64, 130) for count in (1, 63, 64, 65) if count <= R]


def stage_ticks(count, R):
    """The staged tick counters: the ring's first slot, its last, and a second lap placed so that the push straddles
    the ring's end (slot R - (count + 1) // 2: a 64-row tile wraps inside)."""
    return (0, R - 1, 2 * R - (count + 1) // 2)


def stage_inputs(n, count, seed=0):
    """(pred, chunk [count, n] fp32, alarm [count] int32, valid [count, n] uint8) of one launch.  About one tick in
    four alarms and about one in three has a missing reading; then, by construction: the first row alarms and — from
    two rows on — has a missing reading (a broken tick), the last row does neither (a complete tick, no alarm)."""
    rng = np.random.default_rng(100003 * seed + 131 * n + count)
    pred, chunk = rng.random((count, n), dtype=np.float32), rng.random((count, n), dtype=np.float32)
    alarm = (rng.random(count) < 0.25).astype(np.int32)
    valid = (rng.random((count, n)) >= 1.0 - (2.0 / 3.0) ** (1.0 / n)).astype(np.uint8)
    alarm[0], valid[0, n // 2] = 1, 0
    alarm[count - 1], valid[count - 1] = 0, 1
    return pred, chunk, alarm, valid


def stage_ring(mode, n, R, ticks, exclude_alarms, pred, chunk, alarm, valid):
    """The ring after ONE push at stream tick `ticks` onto a ring full of the sentinel, `mode` "plain", "gaps" or
    "sensor" (tests/_sensor_calib_ref.py's ring): (keys [n, R] as uint64 bit patterns, keep [R] uint8)."""
    if mode == "sensor":
        import _sensor_calib_ref
        ring = _sensor_calib_ref.SensorRing(n, R, exclude_alarms)
        ring.keys[...] = bits(np.full((n, R), SENTINEL_KEY))
    else:
        ring = CalibRing(n, R, exclude_alarms=exclude_alarms)
        ring.keys[...] = SENTINEL_KEY
    ring.keep[...] = SENTINEL_KEEP
    ring.ticks = ticks
    if mode == "plain":
        ring.push(pred, chunk, alarm)
    else:
        ring.push(pred, chunk, alarm, valid.astype(bool))
    return bits(ring.keys.view(np.float64)), ring.keep


class SwitchedStreamRef(_stream_ref.StreamRef):
    """StreamRef whose table can be replaced between pushes: the carry keeps the normalised errors it holds (they were
    computed with the table in force at their tick), everything from the next push on uses the new table."""

    def switch(self, med_iqr):
        mi = np.asarray(med_iqr, dtype=np.float64)
        self.med, self.den = mi[:, 0].copy(), np.abs(mi[:, 1]) + _stream_ref.SCORE_EPS


def run_switched(delta, tables, chunk, m=1, threshold=np.inf):
    """The series delta [T, n] in pushes that never straddle a switch: `tables` = [(first tick, med_iqr), ..] with the
    first entry at tick 0; between two switches the ticks go in pushes of `chunk` through _stream_ref.run_chunked's
    loop.  (smoothed [T, n], top values, top sensors, flags, the ref)."""
    starts = [s for s, _ in tables] + [len(delta)]
    assert starts[0] == 0 and all(a < b for a, b in zip(starts, starts[1:]))
    ref = SwitchedStreamRef(tables[0][1], m, threshold)
    outs = []
    for (s, table), e in zip(tables, starts[1:]):
        ref.switch(table)
        outs += [ref.push(delta[t:min(e, t + chunk)]) for t in range(s, e, chunk)]
    sm, vals, idx, flags = (np.concatenate([o[j] for o in outs]) for j in range(4))
    return sm, vals, idx, flags, ref
