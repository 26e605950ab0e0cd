"""GPU suite of the alarm sweep: gdn_alarm_sweep against the definition in tests/_alarm_sweep_ref.py.
Integer counts and comparisons only, so every comparison is exact.

The kernel's borders: a lane is a setting and a workgroup one wave, so P = 63, 64, 65, 130 are a partial wave, a full
one, one lane of a second and a partial third; it reads 8 ticks per iteration after the ticks that lead up to an 8-byte
aligned label, so T = 1 .. 9, 63 .. 65 walk the head, the body and the tail, and the labels are also handed over at
every byte offset."""
import functools

import numpy as np
import pytest
import torch

import _alarm_sweep_ref as ref
import _episodes_ref
from test_cpu_alarm_sweep import CASES

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 7, 8, 9, 63, 64, 65, 257, 1000)
ROWS = (1, 63, 64, 65, 130)
SEED = 3                                                    # chosen on the CPU: see _random_case's assertions
NAN, INF = float("nan"), float("inf")


def _settings(g, P):
    """P valid settings, mixed within a wave: hi among the score levels and between them, lo up to 2 below, on / off 1..6."""
    hi = g.integers(0, 8, size=P) / 2.0
    lo = hi - g.integers(0, 5, size=P) / 2.0
    return hi, lo, g.integers(1, 7, size=P).astype(np.int32), g.integers(1, 7, size=P).astype(np.int32)


def _labels(g, T, p=0.35):
    """Random runs of 1 .. 9 ticks, labelled with probability p."""
    lab, t = np.zeros(T, dtype=np.uint8), 0
    while t < T:
        run = int(g.integers(1, 10))
        if g.random() < p:
            lab[t:t + run] = 1
        t += run
    return lab


@functools.lru_cache(maxsize=None)
def _random_case(T):
    """(scores, labels, (hi, lo, on, off) of 130 rows, the oracle's counts [130, 8], its per-row extras): computed once
    per T; a test of P rows uses the first P."""
    g = np.random.default_rng(SEED * 1000 + T)
    s = g.integers(0, 5, size=T).astype(np.float64)          # a handful of levels: ties with hi and short runs are common
    lab = _labels(g, T)
    table = _settings(g, max(ROWS))
    extra = []
    want = ref.sweep(s, lab, *table, extra=extra)
    return s, lab, table, want, extra


def _sweep(dev, s, lab, hi, lo, on, off, label_offset=0):
    from gdn_amd import ops
    t = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(dev)
    room = torch.zeros((len(lab) + 8,), dtype=torch.uint8, device=dev)
    view = room[label_offset:label_offset + len(lab)]
    view.copy_(t(lab, torch.uint8))
    return ops.alarm_sweep(t(s, torch.float64), view, t(hi, torch.float64), t(lo, torch.float64), t(on, torch.int32),
                           t(off, torch.int32)).cpu().numpy()


@pytest.mark.parametrize("T", SIZES)
@pytest.mark.parametrize("P", ROWS)
def test_sweep_equals_the_definition_at_every_border_size(T, P, gpu_device):
    s, lab, table, want, _ = _random_case(T)
    got = _sweep(gpu_device, s, lab, *(c[:P] for c in table), label_offset=(T + P) % 8)
    assert got.shape == (P, 8) and got.dtype == np.int64
    bad = np.nonzero((got != want[:P]).any(axis=1))[0]
    assert bad.size == 0, (T, P, bad[:4], got[bad[:2]], want[bad[:2]])


def test_the_random_case_is_not_quiet():
    """On the oracle's results alone: the T = 1000 case walks every path the kernel has."""
    s, lab, table, want, extra = _random_case(1000)
    assert (want[:, 0] >= 2).sum() * 2 >= len(want)                                        # most settings raise twice
    assert any(row[2] < info["overlaps"] for row, info in zip(want, extra))                # the distinct-count path
    assert (want[:, 4] > 0).any() and (want[:, 7] == 1).any()                              # a delay; an open episode
    assert any(row[6] < info["active_label_ticks"] for row, info in zip(want, extra))      # the clearing-run path
    assert (want[:, 1] < want[:, 0]).any() and (want[:, 2] < len(ref.incidents(lab))).any()


def test_the_longest_delays_and_a_long_series(gpu_device):
    T = 10000
    g = np.random.default_rng(SEED)
    s = np.zeros(T)
    s[5000:5100] = 3.0
    s[9000:] = 3.0                                          # 1000 ticks: open for on <= 1000
    s[g.random(T) < 0.001] = 1.0                            # short breaks in the runs and in the quiet
    s[100:4300] = 3.0                                       # 4200 ticks above, unbroken: on = 4096 raises at tick 4195
    lab = _labels(g, T, 0.2)
    lab[90:120] = 1
    hi = np.array([2.0, 2.0, 2.0, 2.0, 0.5, 0.5, 2.0, 2.0])
    lo = np.array([2.0, 0.5, 2.0, 0.5, 0.5, 0.5, 2.0, -1.0])
    on = np.array([4096, 4096, 1, 1, 4096, 3, 100, 2], dtype=np.int32)
    off = np.array([4096, 1, 4096, 4096, 4096, 4096, 100, 7], dtype=np.int32)
    want = ref.sweep(s, lab, hi, lo, on, off)
    assert want[:, 0].min() >= 0 and (want[:2, 0] >= 1).all() and want[:, 4].max() >= 4000     # a delay near `on`
    assert np.array_equal(_sweep(gpu_device, s, lab, hi, lo, on, off, label_offset=5), want)


def test_special_scores_and_labels_at_both_ends(gpu_device):
    dev = gpu_device
    s = np.array([NAN, 3.0, INF, -INF, 0.0, -0.0, 0.0, 2.0, 2.0, NAN, NAN, 3.0, -0.0, INF, INF, 1.0, 2.0, -INF, 3.0, 3.0])
    T = len(s)
    first_last = np.zeros(T, dtype=np.uint8)
    first_last[:2], first_last[-3:] = 1, 1                  # an incident at tick 0 and one that ends at T - 1
    hi = np.array([0.0, 0.0, 2.0, 2.0, INF, -INF, 1.0, 0.0, 3.0])
    lo = np.array([0.0, -0.0, 2.0, 0.0, 0.0, -INF, -INF, -1.0, 2.0])
    on = np.array([1, 2, 1, 2, 1, 1, 1, 3, 1], dtype=np.int32)
    off = np.array([1, 1, 2, 2, 1, 1, 2, 1, 1], dtype=np.int32)
    for lab in (first_last, (np.arange(T) % 2).astype(np.uint8), ((np.arange(T) + 1) % 2).astype(np.uint8),
                np.ones(T, dtype=np.uint8), np.zeros(T, dtype=np.uint8)):
        want = ref.sweep(s, lab, hi, lo, on, off)
        assert np.array_equal(_sweep(dev, s, lab, hi, lo, on, off, label_offset=int(lab.sum()) % 8), want), lab
    assert want[0, 0] >= 2                                  # hi = 0.0: neither zero is above it, the others raise
    for name, (sc, lab, h, l, a, b, expect) in CASES.items():              # the hand-written cases, on the device
        got = _sweep(dev, np.array(sc, dtype=np.float64), np.array(lab, dtype=np.uint8), [h], [l], np.array([a], dtype=np.int32),
                     np.array([b], dtype=np.int32))
        assert got.tolist() == [expect], name
    # labels of value 255 and 2 are labelled ticks too
    s3, l3 = np.array([2.0, 0.0, 2.0]), np.array([255, 0, 2], dtype=np.uint8)
    assert _sweep(dev, s3, l3, [1.0], [1.0], np.array([1], dtype=np.int32), np.array([1], dtype=np.int32)).tolist() == [
        ref.counters(s3, l3, 1.0, 1.0, 1, 1)] == [[2, 2, 2, 0, 0, 2, 2, 1]]


def test_rows_that_are_no_settings_get_minus_one_and_leave_their_neighbours_alone(gpu_device):
    s, lab, table, want, _ = _random_case(257)
    hi, lo, on, off = (c[:130].copy() for c in table)
    lo[3] = hi[3] + 0.5                                     # lo > hi
    hi[64] = NAN
    lo[70] = NAN
    on[5], on[129] = 0, 4097
    off[63], off[100] = 4097, -1
    bad = [3, 5, 63, 64, 70, 100, 129]
    got = _sweep(gpu_device, s, lab, hi, lo, on, off)
    good = np.setdiff1d(np.arange(130), bad)
    assert (got[bad] == -1).all() and np.array_equal(got[good], want[good]) and (want[good] >= 0).all()


def test_the_report_of_the_archive_scan_aggregates_to_the_sweeps_rows(gpu_device):
    from gdn_amd import harness
    dev = gpu_device
    s, lab, table, want, _ = _random_case(1000)
    scores, labels = torch.from_numpy(s).to(dev), torch.from_numpy(lab).to(dev)
    sens = torch.zeros((len(s), 1), dtype=torch.int32, device=dev)
    rows = [int(r) for r in np.argsort(-want[:, 0], kind="stable")[:8]]                # the eight busiest settings
    hi, lo, on, off = (c[rows] for c in table)
    sweep = harness.alarm_sweep(scores, labels, hi, lo, on, off, product=False)
    assert np.array_equal(sweep.counts.cpu().numpy(), want[rows]) and int(sweep.incidents) == len(ref.incidents(lab))
    assert int(sweep.label_ticks) == int(lab.sum()) and int(sweep.ticks) == len(s)
    for j in range(8):
        table_j = harness.episodes(scores, sens, float(hi[j]), float(lo[j]), on=int(on[j]), off=int(off[j]), cap=1024)
        report = harness.episode_report(table_j, labels, int(on[j]))
        assert report.counters().tolist() == want[rows[j]].tolist(), j
        assert report.hit.sum().item() == want[rows[j], 2] and report.begin.shape[0] == len(ref.incidents(lab))
    with pytest.raises(ValueError, match="cap = 1"):
        harness.episode_report(harness.episodes(scores, sens, float(hi[0]), float(lo[0]), on=int(on[0]), off=int(off[0]),
                                                cap=1), labels, int(on[0]))


def test_an_evaluators_sweep_and_its_best_row_in_a_stream_detector(gpu_device):
    from gdn_amd import harness
    from test_gpu_episodes import MODELS, STREAM_T, _stream_case
    dev = gpu_device
    model, series, ev, hi0, lo0, _ = _stream_case("small", dev)
    w = MODELS["small"][1]
    scores = ev.top_scores[:, 0].cpu().numpy()
    lab = np.zeros(STREAM_T, dtype=np.float32)
    for j, t0 in enumerate(range(30, STREAM_T - 30, 45)):   # the planted excursions of the case, every other one labelled
        if j % 2 == 0:
            lab[t0 + 2:t0 + 6 + 2 * j] = 1.0
    his = [float(np.quantile(scores, q)) for q in (0.7, 0.8, 0.9, 0.95)]
    sweep = harness.alarm_sweep(ev, torch.from_numpy(lab), his, lo_frac=[1.0, 0.75], on=[1, 3], off=[1, 4])
    host = sweep.numpy()
    assert host["counts"].shape == (32, 8) and host["incidents"] == len(ref.incidents(lab)) >= 3
    want = ref.sweep(scores, lab, host["hi"], host["lo"], host["on"], host["off"])
    assert np.array_equal(host["counts"], want) and (want[:, 2] > 0).any()
    best = sweep.best(min_recall=0.5)
    f1 = sweep.f1().cpu().numpy()
    ok = (want[:, 0] >= 0) & (want[:, 2] >= 0.5 * host["incidents"])
    assert best["f1"] == f1[ok].max() > 0 and [best[k] for k in ref.NAMES] == want[best["row"]].tolist()
    det = harness.StreamDetector(model, ev.med_iqr, best["hi"], series[:, :w].contiguous(), 16, top_m=3,
                                 events=dict(on=best["on"], off=best["off"], lo=best["lo"], cap=64))
    stream = series[:, w:].t().contiguous()
    for a in range(0, STREAM_T, 16):
        det.push(stream[a:a + 16])
    assert det.episodes().numpy()["count"] == best["episodes"] >= 1


def test_entry_point_refusals_leave_counts_untouched(gpu_device):
    from gdn_amd import _lib, ops
    dev = gpu_device
    lib = _lib.load()
    T, P = 40, 5
    s = torch.rand((T,), dtype=torch.float64, device=dev)
    lab = (torch.rand((T,), device=dev) < 0.3).to(torch.uint8)
    hi = torch.full((P,), 0.5, dtype=torch.float64, device=dev)
    on = torch.ones((P,), dtype=torch.int32, device=dev)
    counts = torch.full((P, 8), -7, dtype=torch.int64, device=dev)

    def call(T=T, P=P, scores=s, labels=lab, hi=hi, lo=hi, on=on, off=on, counts=counts):
        ptr = lambda t: None if t is None else t.data_ptr()
        return lib.gdn_alarm_sweep(ptr(scores), ptr(labels), T, ptr(hi), ptr(lo), ptr(on), ptr(off), P, ptr(counts), None)
    ARG, UNSUPPORTED = -1, -3
    for name in ("scores", "labels", "hi", "lo", "on", "off", "counts"):
        assert call(**{name: None}) == ARG, name
    assert call(T=0) == UNSUPPORTED and call(T=(1 << 26) + 1) == UNSUPPORTED
    assert call(P=0) == UNSUPPORTED and call(P=(1 << 20) + 1) == UNSUPPORTED
    for kw, word in ((dict(scores=s.float()), "scores: expected torch.float64"), (dict(labels=lab.bool()), "labels: expected"),
                     (dict(on=on.long()), "on: expected torch.int32"), (dict(labels=lab[:-1]), "labels"),
                     (dict(lo=hi[:-1]), "lo: shape"), (dict(out=counts[:, :4]), "out")):
        args = dict(scores=s, labels=lab, hi=hi, lo=hi, on=on, off=on)
        args.update(kw)
        with pytest.raises((TypeError, ValueError), match=word):
            ops.alarm_sweep(**args)
    with pytest.raises(_lib.GdnHipError, match="scores is on cpu"):
        ops.alarm_sweep(s.cpu(), lab, hi, hi, on, on)
    torch.cuda.synchronize()
    assert bool((counts == -7).all())
    assert call() == 0                                      # and the same call with sound arguments runs
    torch.cuda.synchronize()
    want = ref.sweep(s.cpu().numpy(), lab.cpu().numpy(), [0.5] * P, [0.5] * P, [1] * P, [1] * P)
    assert np.array_equal(counts.cpu().numpy(), want)
    out = torch.zeros((P * 8,), dtype=torch.int64, device=dev)
    assert ops.alarm_sweep(s, lab, hi, hi, on, on, out=out) is out and np.array_equal(out.cpu().numpy().reshape(P, 8), want)
