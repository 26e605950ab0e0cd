"""CPU suite of the alarm sweep: the oracle against hand-written counters, the host-side refusals, the
settings table, `.best` on hand-made counts, the per-setting report on host tensors, the command line's flag checks and
the entry point's presence in the header and the built library.  No device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _alarm_sweep_ref as ref
import _episodes_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")

# name: (scores, labels, hi, lo, on, off, [episodes, true_episodes, incidents_hit, delay_sum, delay_max, alarm_ticks,
# alarm_label_ticks, open])
CASES = {
    # episodes [0, 1) and [2, 3) both lie inside the incident [0, 3): two true episodes, ONE incident
    "one incident under two episodes": ([2, 0, 2, 0], [1, 1, 1, 0], 1.0, 1.0, 1, 1, [2, 2, 1, 0, 0, 2, 2, 0]),
    # raised at 0; ticks 1-2 are the clearing run (off = 2): end = 1, the labelled ticks 1-2 are outside the span
    "labels inside the clearing run": ([2, 0, 0, 0], [0, 1, 1, 0], 1.0, 1.0, 1, 2, [1, 0, 0, 0, 0, 1, 0, 0]),
    # on = 3: span [0, 3) raised at tick 2; the incident [0, 1) ended before the raise: hit, delay 2 > its length 1
    "incident over before the raise": ([2, 2, 2, 0], [1, 0, 0, 0], 1.0, 1.0, 3, 1, [1, 1, 1, 2, 2, 3, 1, 0]),
    # raised at 2 (start 1); tick 3 is one below tick of off = 2: open, end = T = 4; incident [2, 4): delay 0
    "open at the last tick": ([0, 2, 2, 0], [0, 0, 1, 1], 1.0, 1.0, 2, 2, [1, 1, 1, 0, 0, 3, 2, 1]),
    "no incident": ([2, 0, 2, 2], [0, 0, 0, 0], 1.0, 1.0, 1, 1, [2, 0, 0, 0, 0, 3, 0, 1]),
    # one incident [0, 5); the episode [1, 3) is raised at 2; the lone above tick 4 never raises (on = 2)
    "labels all one": ([0, 2, 2, 0, 2], [1, 1, 1, 1, 1], 1.0, 1.0, 2, 1, [1, 1, 1, 2, 2, 2, 2, 0]),
    # deadband: 0.7 is neither above 1.0 nor at or below 0.5; NaN is below; s == hi is not above.  Spans [1, 6) and
    # [8, 9) (open); the incident [5, 7) is met by the first span's last tick only, after its raise: delay 0
    "deadband, NaN and a tie with hi": ([1.0, 2, 0.7, 0.4, 0.7, 0.7, NAN, 0.4, 2], [0, 1, 0, 0, 0, 1, 1, 0, 0],
                                        1.0, 0.5, 1, 2, [2, 1, 2, 0, 0, 6, 2, 1]),
    # two incidents inside one pre-raise run (on = 4): delays 3 - 0 and 3 - 2
    "two incidents before one raise": ([2, 2, 2, 2, 0], [1, 0, 1, 0, 0], 1.0, 1.0, 4, 1, [1, 1, 2, 4, 3, 4, 2, 0]),
    "not a setting": ([2, 0], [1, 0], 1.0, 2.0, 1, 1, [-1] * 8),
}


@pytest.mark.parametrize("name", list(CASES))
def test_the_oracle_gives_the_hand_written_counters(name):
    s, lab, hi, lo, on, off, want = CASES[name]
    assert ref.counters(np.array(s, dtype=np.float64), lab, hi, lo, on, off) == want
    assert len(ref.NAMES) == 8


def test_check_refuses_by_field_and_row_and_broadcasts():
    from gdn_amd import ops
    assert ops.ALARM_SWEEP_COUNTERS == ref.NAMES
    hi, lo, on, off = ops.alarm_sweep_check([1.0, 2.0, 3.0], 0.5, 2, [1, 2, 3])
    assert hi.dtype == lo.dtype == torch.float64 and on.dtype == off.dtype == torch.int32
    assert lo.tolist() == [0.5] * 3 and on.tolist() == [2] * 3 and off.tolist() == [1, 2, 3] and hi.is_contiguous()
    for args, word in ((([1.0, NAN], 0.0, 1, 1), r"hi\[1\] = nan"), (([1.0, 2.0], [0.0, NAN], 1, 1), r"lo\[1\] = nan"),
                       (([1.0, 2.0], [0.0, 2.5], 1, 1), r"lo\[1\] = 2.5 lies above hi\[1\] = 2.0"),
                       ((1.0, 1.0, [1, 0], 1), r"on\[1\] = 0"), ((1.0, 1.0, 1, [1, 1, 4097]), r"off\[2\] = 4097"),
                       (([1.0, 2.0], [1.0, 2.0, 3.0], 1, 1), "hi: 2 values"), (([], 1.0, 1, 1), "hi: 0 values"),
                       ((1.0, 1.0, [[1]], 1), "on: a scalar or a sequence")):
        with pytest.raises(ValueError, match=word):
            ops.alarm_sweep_check(*args)
    with pytest.raises(TypeError, match="on: whole numbers"):
        ops.alarm_sweep_check(1.0, 1.0, 1.5, 1)
    assert ops.alarm_sweep_check([1.0], [2.0], 1, 1, ordered=False)[1].tolist() == [2.0]
    cpu = torch.zeros((4,), dtype=torch.float64)
    with pytest.raises(Exception, match="scores is on cpu"):
        ops.alarm_sweep(cpu, cpu.to(torch.uint8), cpu, cpu, cpu.int(), cpu.int())


def test_table_product_explicit_rows_and_lo_frac():
    from gdn_amd import harness
    hi, lo, on, off = harness.alarm_sweep_table([1.0, 3.0], on=[1, 2], off=[5, 6, 7], lo_frac=[1.0, 0.3])
    assert hi.numel() == 2 * 2 * 2 * 3
    assert hi[:12].tolist() == [1.0] * 12 and off[:3].tolist() == [5, 6, 7] and on[:6].tolist() == [1, 1, 1, 2, 2, 2]
    frac = torch.tensor([1.0, 0.3], dtype=torch.float64)
    assert lo[6].item() == (torch.tensor(1.0, dtype=torch.float64) * frac[1]).item()       # the product is the level used
    assert lo[18].item() == (torch.tensor(3.0, dtype=torch.float64) * frac[1]).item() and lo[12].item() == 3.0
    hi, lo, on, off = harness.alarm_sweep_table([1.0, 3.0], lo=[0.5, 2.0])                  # absolute levels: 2.0 > 1.0 stays
    assert list(zip(hi.tolist(), lo.tolist())) == [(1.0, 0.5), (1.0, 2.0), (3.0, 0.5), (3.0, 2.0)]
    assert on.tolist() == off.tolist() == [1] * 4
    hi, lo, on, off = harness.alarm_sweep_table([1.0, 3.0])
    assert lo.tolist() == [1.0, 3.0]
    hi, lo, on, off = harness.alarm_sweep_table([1.0, 3.0], on=[2, 4], off=3, product=False, lo_frac=0.5)
    assert lo.tolist() == [0.5, 1.5] and on.tolist() == [2, 4] and off.tolist() == [3, 3]
    with pytest.raises(ValueError, match=r"lo\[0\] = 2.0 lies above"):
        harness.alarm_sweep_table([1.0], lo=[2.0], product=False)
    with pytest.raises(ValueError, match=r"on\[1\] = 5000"):
        harness.alarm_sweep_table([1.0], on=[1, 5000])
    with pytest.raises(ValueError, match=r"lo_frac\[0\] = nan"):
        harness.alarm_sweep_table([1.0], lo_frac=[NAN])
    with pytest.raises(ValueError, match="one way"):
        harness.alarm_sweep_table([1.0], lo=[1.0], lo_frac=[1.0])
    with pytest.raises(Exception, match="HIP device"):
        harness.alarm_sweep(torch.zeros((4,), dtype=torch.float64), torch.zeros((4,)), [1.0])


def _hand_sweep(rows, incidents):
    from gdn_amd import harness
    P = len(rows)
    i64 = lambda v: torch.tensor([v], dtype=torch.int64)
    return harness.AlarmSweep(torch.arange(P, dtype=torch.float64) + 1.0, torch.arange(P, dtype=torch.float64),
                              torch.full((P,), 2, dtype=torch.int32), torch.full((P,), 3, dtype=torch.int32),
                              torch.tensor(rows, dtype=torch.int64), i64(incidents), i64(40), i64(100))


def test_best_orders_by_f1_then_delay_then_alarm_ticks_then_row():
    #        ep te ih dsum dmax at alt open            I = 4
    rows = [[-1] * 8,                                  # not a setting
            [4, 4, 4, 9, 5, 30, 20, 0],                # F1 1.0, delay_sum 9
            [4, 4, 4, 6, 5, 31, 20, 0],                # F1 1.0, delay_sum 6, alarm_ticks 31
            [4, 4, 4, 6, 5, 28, 20, 0],                # F1 1.0, delay_sum 6, alarm_ticks 28   <- best
            [4, 4, 4, 6, 5, 28, 20, 0],                # the same again: the lower row wins
            [8, 4, 4, 0, 0, 10, 9, 0],                 # F1 2*4*4 / (4*4 + 4*8) = 2/3
            [2, 2, 2, 0, 0, 5, 5, 1],                  # recall 0.5: F1 2*2*2 / (2*4 + 2*2) = 2/3, delay 0
            [0, 0, 0, 0, 0, 0, 0, 0]]                  # nothing raised: F1 0
    sweep = _hand_sweep(rows, 4)
    assert sweep.f1().tolist() == [0.0, 1.0, 1.0, 1.0, 1.0, 2 * 4 * 4 / (4 * 4 + 4 * 8), 2 * 2 * 2 / (2 * 4 + 2 * 2), 0.0]
    best = sweep.best()
    assert best["row"] == 3 and best["f1"] == 1.0 and (best["hi"], best["lo"], best["on"], best["off"]) == (4.0, 3.0, 2, 3)
    assert [best[k] for k in ref.NAMES] == rows[3]
    # mean delay <= 1 leaves rows 5-7: rows 5 and 6 tie on F1 and on delay_sum, row 6 has fewer alarm ticks ...
    assert sweep.best(max_delay=1.0)["row"] == 6
    assert sweep.best(max_delay=1.0, min_recall=1.0)["row"] == 5     # ... but hits half the incidents only
    with pytest.raises(ValueError, match="min_recall = 1.0 within max_delay = 0.5"):
        _hand_sweep(rows[:5], 4).best(min_recall=1.0, max_delay=0.5)
    with pytest.raises(ValueError, match="none of the 1 settings"):
        _hand_sweep(rows[:1], 4).best()
    assert _hand_sweep(rows[7:], 0).best()["f1"] == 0.0                # no incident at all: every valid row qualifies
    host = sweep.numpy()
    assert host["counts"].tolist() == rows and host["incidents"] == 4 and host["ticks"] == 100 and host["label_ticks"] == 40
    assert host["hi"].tolist() == sweep.hi.tolist() and host["on"].dtype == np.int32


def _episodes_of(s, hi, lo, on, off, cap):
    from gdn_amd import harness
    t = _episodes_ref.episodes(s, np.zeros((len(s), 1), dtype=np.int32), hi, lo, on, off, cap)
    pad = lambda a, fill, dtype: torch.cat([torch.from_numpy(a), torch.full((cap - len(a),), fill, dtype=dtype)])
    return harness.Episodes(pad(t["start"], 0, torch.int64), pad(t["end"], -1, torch.int64), pad(t["peak"], 0.0, torch.float64),
                            pad(t["peak_tick"], 0, torch.int64), torch.zeros((cap, 1), dtype=torch.int32),
                            torch.tensor([t["count"]], dtype=torch.int64))


def test_episode_report_aggregates_are_the_counters_on_host_tensors():
    from gdn_amd import harness
    for name, (s, lab, hi, lo, on, off, want) in CASES.items():
        if want[0] < 0:
            continue
        rep = harness.episode_report(_episodes_of(np.array(s, dtype=np.float64), hi, lo, on, off, 8), torch.tensor(lab), on)
        assert rep.counters().tolist() == want, name
    s, lab, hi, lo, on, off, want = CASES["deadband, NaN and a tie with hi"]
    rep = harness.episode_report(_episodes_of(np.array(s), hi, lo, on, off, 8), torch.tensor(lab, dtype=torch.float32), on)
    assert rep.begin.tolist() == [1, 5] and rep.end.tolist() == [2, 7] and rep.hit.tolist() == [True, True]
    assert rep.episode.tolist() == [0, 0] and rep.delay.tolist() == [0, 0]
    assert rep.spans.tolist() == [[1, 6], [8, 9]] and rep.label_ticks.tolist() == [2, 0] and rep.true.tolist() == [True, False]
    g = np.random.default_rng(5)
    for trial in range(40):
        T = int(g.integers(1, 120))
        s = g.integers(0, 5, size=T).astype(np.float64)
        lab = (g.random(T) < 0.5).astype(np.uint8) if trial % 2 else np.repeat(g.random(T // 5 + 1) < 0.4, 5)[:T].astype(np.uint8)
        hi, lo, on, off = float(g.integers(0, 4)), float(g.integers(-1, 1)), int(g.integers(1, 6)), int(g.integers(1, 6))
        rep = harness.episode_report(_episodes_of(s, hi, lo, on, off, T), torch.from_numpy(lab), on)
        assert rep.counters().tolist() == ref.counters(s, lab, hi, lo, on, off), trial
    with pytest.raises(ValueError, match="cap = 1"):
        harness.episode_report(_episodes_of(np.array([2.0, 0, 2, 0]), 1.0, 1.0, 1, 1, 1), torch.zeros(4), 1)


def test_the_command_line_flags():
    from gdn_amd import main
    for flags, word in ((["-tune_hi_steps", "8"], "-tune_hi_steps needs -tune_alarm"),
                        (["-tune_on", "1,2"], "-tune_on needs -tune_alarm"), (["-tune_off", "3"], "-tune_off needs -tune_alarm"),
                        (["-tune_alarm", "o.npz", "-tune_on", "1,x"], "-tune_on '1,x'"),
                        (["-tune_alarm", "o.npz", "-tune_off", "0"], "-tune_off '0'"),
                        (["-tune_alarm", "o.npz", "-tune_hi_steps", "0"], "-tune_hi_steps 0")):
        with pytest.raises(ValueError, match=word):
            main.from_args(flags)
    hi, on, off = main.tune_alarm_grid(torch.arange(400, dtype=torch.float64), 32, main.TUNE_ON, main.TUNE_OFF)
    assert hi.numel() == 32 and hi[0] == 0 and hi[-1] == 399 and on == [1, 2, 3, 5, 10] and off == [1, 5, 10, 30]
    assert main.tune_alarm_grid(torch.ones(400, dtype=torch.float64), 32, "2", "3")[0].tolist() == [1.0]
    assert main.TUNE_LO_FRAC == (1.0, 0.9, 0.75, 0.5)


def test_a_test_file_without_labels_is_refused_by_name(tmp_path):
    from gdn_amd import main
    (tmp_path / "plain.csv").write_text("timestamp,a,b\n0,1.0,2.0\n1,1.5,2.5\n")
    (tmp_path / "labelled.csv").write_text("timestamp,a,b,attack\n0,1.0,2.0,0\n1,1.5,2.5,1\n")
    with pytest.raises(ValueError, match="-tune_alarm needs labels: .*plain.csv has no `attack` column"):
        main.check_attack_column(str(tmp_path / "plain.csv"))
    main.check_attack_column(str(tmp_path / "labelled.csv"))


def test_the_header_declares_the_entry_point_and_the_library_exports_it():
    from gdn_amd import _lib
    header = open(os.path.join(ROOT, "include", "gdn_hip.h")).read()
    assert re.search(r"int gdn_alarm_sweep\(const double\* scores, const uint8_t\* labels, long long T,", header)
    assert "gdn_alarm_sweep" in _lib.SIGNATURES and len(_lib.SIGNATURES["gdn_alarm_sweep"]) == 10
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "gdn_alarm_sweep")
    assert _lib.load().gdn_abi_version() == _lib.ABI_VERSION == 23      # additive: the version does not move
