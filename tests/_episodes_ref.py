"""The definition of an alarm episode as a sequential loop with an explicit carried state: the only
oracle of tests/test_cpu_episodes.py and tests/test_gpu_episodes.py.  Comparisons and copies only."""
import numpy as np


def new_state():
    return {"count": 0, "active": False, "run_hi": 0, "run_lo": 0, "cand": None, "open": None, "rows": []}


def run(scores, top_sensors, hi, lo, on, off, cap, first_tick=0, state=None):
    """Fold `scores` [T] / `top_sensors` [T, m] (ticks first_tick ..) into `state` (new_state() when None) and return
    it.  state["rows"]: the first `cap` episodes as dicts (start, end, peak, peak_tick, sensors), end = -1 while open;
    state["count"] counts all of them.  run_hi / run_lo saturate at on / off."""
    st = new_state() if state is None else state
    for i, s in enumerate(scores):
        t, sens = first_tick + i, np.array(top_sensors[i], dtype=np.int32)
        above, below = bool(s > hi), not bool(s > lo)
        st["run_hi"] = min(st["run_hi"] + 1, on) if above else 0
        st["run_lo"] = min(st["run_lo"] + 1, off) if below else 0
        if above and not st["active"]:                      # the peak so far of a run that has not raised yet
            if st["cand"] is None:
                st["cand"] = [s, t, sens]
            elif s > st["cand"][0]:
                st["cand"] = [s, t, sens]
        if not above:
            st["cand"] = None
        if not st["active"] and st["run_hi"] >= on:          # set: the episode opens
            st["active"] = True
            st["open"] = {"start": t - on + 1, "end": -1, "peak": st["cand"][0], "peak_tick": st["cand"][1],
                          "sensors": st["cand"][2]}
            st["cand"] = None
            if st["count"] < cap:
                st["rows"].append(st["open"])
            st["count"] += 1
        elif st["active"] and st["run_lo"] >= off:           # reset: it closes
            st["active"] = False
            st["open"]["end"] = t - off + 1
            st["open"] = None
        elif st["active"] and s > st["open"]["peak"]:
            st["open"].update(peak=s, peak_tick=t, sensors=sens)
    return st


def table(st, m):
    """state["rows"] as arrays: start, end, peak_tick int64; peak float64; sensors int32 [rows, m]; count."""
    rows = st["rows"]
    return {"start": np.array([r["start"] for r in rows], dtype=np.int64),
            "end": np.array([r["end"] for r in rows], dtype=np.int64),
            "peak": np.array([r["peak"] for r in rows], dtype=np.float64),
            "peak_tick": np.array([r["peak_tick"] for r in rows], dtype=np.int64),
            "sensors": np.array([r["sensors"] for r in rows], dtype=np.int32).reshape(len(rows), m),
            "count": st["count"]}


def episodes(scores, top_sensors, hi, lo, on, off, cap, first_tick=0):
    return table(run(scores, top_sensors, hi, lo, on, off, cap, first_tick), np.asarray(top_sensors).shape[1])


def same(a, b):
    """Two tables agree bit for bit (the peaks compared as their 64-bit patterns)."""
    return (a["count"] == b["count"] and all(np.array_equal(a[k], b[k]) for k in ("start", "end", "peak_tick", "sensors"))
            and np.array_equal(np.asarray(a["peak"]).view(np.int64), np.asarray(b["peak"]).view(np.int64)))
