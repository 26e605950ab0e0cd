"""TEST INFRASTRUCTURE: the float64 yardstick of the streaming tests (numpy).  A chunked restatement of the reference's
scoring (evaluate.py:48-68) with a frozen median / IQR: the smoothing's three predecessors travel between chunks in a
carry, exactly what gdn_stream_score / gdn_stream_advance keep on the device.  tests/test_cpu_stream.py pins it to
oracle.score_oracle.full_err_scores: chunking with a carry is the batch arithmetic, bit for bit."""
import numpy as np

SCORE_EPS = 1e-2


class StreamRef:
    """med_iqr [n, 2] float64; top `m` sensors per tick; flags = top score > threshold (strict, NaN never)."""

    def __init__(self, med_iqr, m=1, threshold=np.inf):
        mi = np.asarray(med_iqr, dtype=np.float64)
        self.med, self.den = mi[:, 0], np.abs(mi[:, 1]) + SCORE_EPS
        self.m, self.threshold = int(m), float(threshold)
        self.carry = np.zeros((3, mi.shape[0]))            # normalised errors of the last three ticks, oldest first
        self.ticks = 0
        self.alarms = 0
        self.log = []                                      # (global tick, sensors [m]) of every alarm, in tick order

    def push(self, delta):
        """delta [c, n] = |pred - gt| of the chunk's ticks in float64 -> (smoothed [c, n], top values [c, m], top
        sensors [c, m], flags [c] bool)."""
        a = (np.asarray(delta, dtype=np.float64) - self.med) / self.den
        ext = np.vstack([self.carry, a])                   # row b + 3 = tick b of the chunk
        sm = (((ext[:-3] + ext[1:-2]) + ext[2:-1]) + ext[3:]) / 4.0      # np.mean of 4: left to right
        sm[np.arange(len(a)) + self.ticks < 3] = 0.0       # the first three ticks of the stream
        idx = np.argsort(-sm, axis=1, kind="stable")[:, :self.m]         # larger first, equal scores by the lower sensor
        vals = np.take_along_axis(sm, idx, axis=1)
        with np.errstate(invalid="ignore"):
            flags = vals[:, 0] > self.threshold
        for b in np.nonzero(flags)[0]:
            self.log.append((self.ticks + int(b), idx[b].copy()))
        self.carry = ext[-3:].copy()
        self.ticks += len(a)
        self.alarms += int(flags.sum())
        return sm, vals, idx, flags


def run_chunked(delta, med_iqr, chunk, m=1, threshold=np.inf):
    """The whole series [T, n] through a StreamRef in pushes of `chunk` (the last one ragged): (smoothed [n, T], top
    values [T, m], top sensors [T, m], flags [T], the StreamRef)."""
    ref = StreamRef(med_iqr, m, threshold)
    outs = [ref.push(delta[s:s + chunk]) for s in range(0, len(delta), chunk)]
    sm, vals, idx, flags = (np.concatenate([o[j] for o in outs]) for j in range(4))
    return sm.T.copy(), vals, idx, flags, ref
