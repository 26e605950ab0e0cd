"""CPU suite of the calibration on each sensor's own readings: tests/_sensor_calib_ref.py against
hand-worked rows, the refusals and their messages, the argument rules of calib="sensor", and the motivating case (40
sensors each dropping a tenth of their readings: hardly a complete tick, plenty of readings per sensor)."""
import numpy as np
import pytest
import torch

import _sensor_calib_ref as cref
import _series_gaps_ref as sref

F32 = np.float32


def _plane(columns, t):
    """gt [t, n] fp32 (pred = 0) and valid [t, n] from per-sensor lists of real errors, placed at the FIRST ticks of
    odd sensors and the LAST ticks of even ones; the rest is missing and holds a large value that must not count."""
    n = len(columns)
    gt, valid = np.full((t, n), 1e6, dtype=F32), np.zeros((t, n), dtype=bool)
    for s, vals in enumerate(columns):
        at = slice(0, len(vals)) if s % 2 else slice(t - len(vals), t)
        gt[at, s] = np.asarray(vals, dtype=F32)
        valid[at, s] = True
    return np.zeros((t, n), dtype=F32), gt, valid


def test_hand_worked_rows_of_one_to_five_readings_and_ties():
    # (errors exact in fp32, unsorted) -> (median, q75 - q25) worked by hand with numpy's 'linear' rule:
    # virtual index (c - 1) q, the two neighbours and the fraction
    cases = [
        ([4.0], 4.0, 0.0),                                   # count 1: every rank is the one value
        ([8.0, 2.0], 5.0, (2.0 + 6.0 * 0.75) - (2.0 + 6.0 * 0.25)),            # 2: indices 0.25 / 0.75 -> 3.5 .. 6.5
        ([1.0, 16.0, 4.0], 4.0, (4.0 + 12.0 * 0.5) - (1.0 + 3.0 * 0.5)),      # 3: indices 0.5 / 1.5 -> 2.5 .. 10
        ([8.0, 1.0, 2.0, 4.0], 3.0, (4.0 + 4.0 * 0.25) - (1.0 + 1.0 * 0.75)), # 4: indices 0.75 / 2.25 -> 1.75 .. 5
        ([16.0, 1.0, 8.0, 2.0, 4.0], 4.0, 8.0 - 2.0),                          # 5: indices 1 / 3 exactly
        ([2.0, 2.0, 2.0, 5.0, 2.0, 2.0], 2.0, 0.0),                            # ties: indices 1.25 / 3.75 inside the 2s
        ([3.0, 1.0, 3.0, 1.0], 2.0, (3.0 + 0.0 * 0.25) - (1.0 + 0.0 * 0.75)), # ties at both ends, even count
    ]
    pred, gt, valid = _plane([c[0] for c in cases], 9)
    got, counts = cref.table(pred, gt, valid)
    assert counts.tolist() == [len(c[0]) for c in cases]
    for s, (_vals, med, iqr) in enumerate(cases):
        assert got[s, 0] == med and got[s, 1] == iqr, (s, got[s], med, iqr)
    # the same through the key plane, the filler scattered as the validity plane says
    keys = cref.keys_valid(pred, gt, valid, 12).view(np.float64)
    again, counts2 = cref.table_of_keys(keys)
    assert np.array_equal(again, got) and np.array_equal(counts2, counts)
    assert (cref.keys_valid(pred, gt, valid, 12)[:, 9:] == cref.FILLER).all()


def test_a_sensor_below_min_count_keeps_its_row_and_an_empty_one_always_does():
    pred, gt, valid = _plane([[1.0, 2.0, 3.0], [5.0], []], 4)
    before = np.array([[-1.0, -2.0], [-3.0, -4.0], [-5.0, -6.0]])
    got, counts = cref.table(pred, gt, valid, min_count=2, before=before)
    assert counts.tolist() == [3, 1, 0]
    assert got[0].tolist() == [2.0, 1.0] and np.array_equal(got[1:], before[1:])
    got, _ = cref.table(pred, gt, valid, min_count=0, before=before)
    assert got[1].tolist() == [5.0, 0.0] and np.array_equal(got[2], before[2])


def test_the_ring_keeps_a_tick_with_missing_readings_and_drops_an_alarmed_one():
    n, R = 3, 4
    ring = cref.SensorRing(n, R)
    gt = np.arange(1, 19, dtype=F32).reshape(6, n)
    valid = np.ones((6, n), dtype=bool)
    valid[:, 2] = False                                       # a dead sensor
    valid[1, 0] = False
    alarm = np.array([0, 0, 1, 0, 0, 0])
    ring.push(np.zeros((4, n), dtype=F32), gt[:4], alarm[:4], valid[:4])
    ring.push(np.zeros((2, n), dtype=F32), gt[4:], alarm[4:], valid[4:])
    assert ring.keep.tolist() == [1, 1, 0, 1]                 # ticks 4, 5, 2 (alarmed), 3
    want = np.array([[13.0, 16.0, np.nan, 10.0], [14.0, 17.0, np.nan, 11.0]])
    got = ring.keys.view(np.float64)
    assert np.array_equal(got[:2][:, [0, 1, 3]], want[:, [0, 1, 3]])
    assert (ring.keys[:, 2] == cref.FILLER).all() and (ring.keys[2] == cref.FILLER).all()
    before = np.full((n, 2), 7.0)
    table, counts = ring.table(2, before)
    assert counts.tolist() == [3, 3, 0] and table[0].tolist() == [13.0, 3.0] and np.array_equal(table[2], before[2])


def test_the_motivating_case_has_hardly_a_complete_tick_and_plenty_of_readings_per_sensor():
    """n = 40, t = 1500, every reading dropped with probability 0.1: 0.9^40 * 1500 = 22 complete ticks are expected, so
    calib="tick" with min_kept = 64 must refuse, while every sensor keeps about 1350 readings."""
    valid = cref.motivating_mask()
    complete = int(valid.all(axis=1).sum())
    print(f"complete ticks {complete} of 1500 (expectation {1500 * 0.9 ** 40:.1f}); per-sensor counts "
          f"{valid.sum(axis=0).min()} .. {valid.sum(axis=0).max()}")
    assert valid.shape == (1500, 40) and complete < 64 and abs(complete - 22) <= 14      # 3 sigma of Binomial(1500, .0148)
    assert valid.sum(axis=0).min() >= 64
    raw = cref.motivating_series()
    _filled, _gt, v, keep, total, _run = sref.fill(raw, 8)
    assert np.array_equal(v, valid) and int(keep.sum()) == complete
    assert np.array_equal(1500 - total, valid.sum(axis=0))


def test_the_refusal_names_min_kept_the_sensors_and_their_counts():
    from gdn_amd import harness
    counts = torch.tensor([100, 3, 100, 0] + [5] * 10, dtype=torch.int32)
    msg = harness.too_few_readings(counts, 64, 1500)
    assert "min_kept = 64" in msg and "[1, 3, 4, 5, 6, 7, 8, 9]" in msg and "[3, 0, 5, 5, 5, 5, 5, 5]" in msg
    assert "1500" in msg


def test_calib_sensor_is_refused_without_gaps_or_a_ring_and_an_unknown_rule_by_name():
    from gdn_amd import harness
    series = torch.zeros((3, 40))
    with pytest.raises(ValueError, match=r"calib='sensor'.*gaps=True"):
        harness.SeriesEvaluator(None, None, None, 64, series=series, calib="sensor")
    with pytest.raises(ValueError, match=r"calib = 'row'"):
        harness.SeriesEvaluator(None, None, None, 64, series=series, gaps=True, calib="row")
    for kw in (dict(gaps=True), dict(recal=64), dict()):
        with pytest.raises(ValueError, match=r"(?s)calib='sensor'.*gaps=True.*recal=R"):
            harness.StreamDetector(None, None, 1.0, series, 8, calib="sensor", **kw)
    with pytest.raises(ValueError, match=r"calib = 'row'"):
        harness.StreamDetector(None, None, 1.0, series, 8, calib="row")
    with pytest.raises(ValueError, match=r"(?s)calib='sensor'.*calib_gaps=True"):
        harness.StreamDetector.from_calibration(None, series, 8, gaps=True, recal=64, calib="sensor")


def test_the_command_line_refuses_calib_by_sensor_outside_its_three_flags():
    from gdn_amd import main as cli
    args = cli.build_parser().parse_args(["-stream", "16", "-stream_gaps", "-stream_calib_gaps", "-calib_by_sensor"])
    assert args.calib_by_sensor
    cli.check_calib_by_sensor(True, True, True, True)
    cli.check_calib_by_sensor(False, False, False, False)
    for flags in ((False, True, True), (True, False, True), (True, True, False)):
        with pytest.raises(ValueError, match=r"-calib_by_sensor needs -stream C -stream_gaps -stream_calib_gaps"):
            cli.check_calib_by_sensor(True, *flags)
    assert not cli.build_parser().parse_args([]).calib_by_sensor


def test_the_wrappers_refuse_on_host_facts():
    from gdn_amd import ops
    with pytest.raises(ValueError, match="by_sensor needs the validity plane"):
        ops.stream_calib_write(None, None, None, None, None, None, by_sensor=True)
