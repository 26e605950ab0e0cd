"""TEST INFRASTRUCTURE: the float64 yardstick of the streaming detector's missing readings (numpy), written from the
contract of DESIGN §3.8b and not from the kernels.  A reading is missing when it is not finite; a missing reading is
held at the sensor's latest reading that was not missing; its normalised error is exactly 0.0 wherever it is used;
per sensor the readings missing so far and the run of missing readings that ends at the last tick are counted."""
import numpy as np

from _stream_ref import StreamRef


def ffill(raw, seed):
    """raw [c, n] fp32 (one row per tick), seed [n] fp32 = every sensor's latest real reading before the chunk ->
    (filled [c, n] fp32, valid [c, n] bool, missing [n] = missing readings of the chunk, trailing [n] = the run of
    missing readings that ends at the chunk's last row: c when every row is missing)."""
    raw = np.asarray(raw, dtype=np.float32)
    valid = np.isfinite(raw)
    filled = raw.copy()
    last = np.asarray(seed, dtype=np.float32).copy()
    trailing = np.zeros(raw.shape[1], dtype=np.int64)
    for b in range(raw.shape[0]):                          # the definition: one tick after the other
        last = np.where(valid[b], raw[b], last)
        filled[b] = last
        trailing = np.where(valid[b], 0, trailing + 1)
    return filled, valid, (~valid).sum(axis=0).astype(np.int64), trailing


class GapStreamRef(StreamRef):
    """StreamRef with a validity plane: the normalised error of a missing reading is 0.0 (the calibration median) in
    the smoothing, in the carry and therefore in the next three ticks' means; everything else is StreamRef's."""

    def __init__(self, med_iqr, m=1, threshold=np.inf):
        super().__init__(med_iqr, m, threshold)
        self.missing_total = np.zeros(len(self.med), dtype=np.int64)
        self.missing_run = np.zeros(len(self.med), dtype=np.int64)

    def push(self, delta, valid=None):
        """delta [c, n] = |pred - filled| in float64, valid [c, n] bool (None: every reading is real)."""
        delta = np.asarray(delta, dtype=np.float64)
        valid = np.ones(delta.shape, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
        # (med - med) / den is +0.0 for every finite med: the error of a missing reading, exactly
        out = super().push(np.where(valid, delta, self.med[None, :]))
        self.missing_total += (~valid).sum(axis=0)
        for row in valid:
            self.missing_run = np.where(row, 0, self.missing_run + 1)
        return out


def run_chunked(delta, valid, med_iqr, chunk, m=1, threshold=np.inf):
    """_stream_ref.run_chunked with the validity plane [T, n]."""
    ref = GapStreamRef(med_iqr, m, threshold)
    outs = [ref.push(delta[s:s + chunk], valid[s:s + chunk]) for s in range(0, len(delta), chunk)]
    sm, vals, idx, flags = (np.concatenate([o[j] for o in outs]) for j in range(4))
    return sm.T.copy(), vals, idx, flags, ref


def ffill_chunked(raw, seed, chunk):
    """The stream raw [T, n] filled push by push, each push seeded from the last filled row before it (hist[:, w-1]
    on the device): (filled [T, n], valid [T, n], missing_total [n], missing_run [n]) with the device's counter rule."""
    seed = np.asarray(seed, dtype=np.float32)
    total = np.zeros(raw.shape[1], dtype=np.int64)
    run = np.zeros(raw.shape[1], dtype=np.int64)
    filled, valid = [], []
    for s in range(0, len(raw), chunk):
        f, v, miss, trail = ffill(raw[s:s + chunk], seed)
        count = len(f)
        total += miss
        run = np.where(trail == count, run + count, trail)
        seed = f[-1]
        filled.append(f)
        valid.append(v)
    return np.concatenate(filled), np.concatenate(valid), total, run
