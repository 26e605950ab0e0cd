"""The definition of the alarm sweep's eight counters, written from the definition and deliberately NOT
as the streaming state machine of the kernel: the episode table of one setting comes from tests/_episodes_ref.py, the
incidents from the labels, and the two are matched by interval overlap with plain loops.  The only oracle of
tests/test_cpu_alarm_sweep.py and tests/test_gpu_alarm_sweep.py."""
import numpy as np

import _episodes_ref as episodes_ref

NAMES = ("episodes", "true_episodes", "incidents_hit", "delay_sum", "delay_max", "alarm_ticks", "alarm_label_ticks",
         "open")
MAX_RUN = 4096


def incidents(labels):
    """[(a, b)): the maximal runs of labelled (non-zero) ticks."""
    out, at = [], None
    for t, lab in enumerate(labels):
        if lab and at is None:
            at = t
        if not lab and at is not None:
            out.append((at, t))
            at = None
    if at is not None:
        out.append((at, len(labels)))
    return out


def spans(scores, hi, lo, on, off):
    """[(start, end)) of every episode of one setting; an episode open at the last tick ends at T.  Second value: open."""
    T = len(scores)
    table = episodes_ref.episodes(scores, np.zeros((T, 1), dtype=np.int32), hi, lo, on, off, T)
    assert table["count"] == len(table["start"])
    ends = [T if e < 0 else int(e) for e in table["end"]]
    return list(zip((int(s) for s in table["start"]), ends)), bool(len(ends) and table["end"][-1] < 0)


def valid(hi, lo, on, off):
    return bool(lo <= hi) and 1 <= on <= MAX_RUN and 1 <= off <= MAX_RUN


def counters(scores, labels, hi, lo, on, off, extra=None):
    """The eight counters of one setting.  `extra` (a dict) receives two figures the non-vacuity checks need: the sum
    over episodes of the incidents each overlaps, and the labelled ticks while `active` (from the raise to the clear)."""
    if not valid(hi, lo, on, off):
        return [-1] * 8
    labels = [1 if v else 0 for v in labels]
    T = len(scores)
    eps, is_open = spans(scores, hi, lo, on, off)
    incs = incidents(labels)
    true_episodes = sum(1 for s, e in eps if any(labels[s:e]))
    hit, delay_sum, delay_max, overlaps = 0, 0, 0, 0
    for a, b in incs:
        first = None
        for s, e in eps:
            if s < b and a < e:
                overlaps += 1
                if first is None:
                    first = (s, e)
        if first is not None:
            delay = max(0, first[0] + on - 1 - a)
            hit, delay_sum, delay_max = hit + 1, delay_sum + delay, max(delay_max, delay)
    if extra is not None:
        extra["overlaps"] = overlaps
        extra["active_label_ticks"] = sum(sum(labels[s + on - 1:(T if (k == len(eps) - 1 and is_open) else e + off - 1)])
                                          for k, (s, e) in enumerate(eps))
    return [len(eps), true_episodes, hit, delay_sum, delay_max, sum(e - s for s, e in eps),
            sum(sum(labels[s:e]) for s, e in eps), int(is_open)]


def sweep(scores, labels, hi, lo, on, off, extra=None):
    """counts [P, 8] int64 of P explicit rows; `extra`: a list that receives one dict per row."""
    rows = []
    for p in range(len(hi)):
        info = {} if extra is not None else None
        rows.append(counters(scores, labels, float(hi[p]), float(lo[p]), int(on[p]), int(off[p]), info))
        if extra is not None:
            extra.append(info)
    return np.array(rows, dtype=np.int64).reshape(len(hi), 8)
