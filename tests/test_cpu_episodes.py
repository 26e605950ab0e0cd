"""CPU suite of the alarm episodes: the reference's own properties, the host-side refusals, the
checkpoint's key rules on plain dicts and the command line's flag checks.  No device."""
import numpy as np
import pytest
import torch

import _episodes_ref as ref
from test_cpu_stream_checkpoint import M, N, _dict, _expect


def _series(T, seed, m=3, n=40):
    g = np.random.default_rng(seed)
    s = g.standard_normal(T).cumsum() * 0.3 + g.standard_normal(T)
    s[g.random(T) < 0.02] = np.nan
    return s, g.integers(0, n, size=(T, m), dtype=np.int32)


def _runs_of(flags):
    """[(start, end)) of the maximal runs of True; the last one open (-1) when it reaches the end."""
    out, at = [], None
    for t, f in enumerate(flags):
        if f and at is None:
            at = t
        if not f and at is not None:
            out.append((at, t))
            at = None
    return out + ([(at, -1)] if at is not None else [])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_on_off_one_and_equal_levels_give_the_runs_of_the_alarm_flag(seed):
    s, sens = _series(500, seed)
    hi = float(np.nanquantile(s, 0.7))
    got = ref.episodes(s, sens, hi, hi, 1, 1, 4096)
    runs = _runs_of(s > hi)                                  # the alarm rule: strict, a NaN score is not above
    assert len(runs) >= 3 and got["count"] == len(runs)
    assert list(zip(got["start"].tolist(), got["end"].tolist())) == runs
    for j, (a, b) in enumerate(runs):
        seg = s[a:(b if b >= 0 else len(s))]
        assert got["peak"][j] == np.nanmax(seg) and got["peak_tick"][j] == a + int(np.nanargmax(seg))
        assert np.array_equal(got["sensors"][j], sens[got["peak_tick"][j]])


@pytest.mark.parametrize("on,off,gap", [(1, 1, 0.0), (3, 5, 0.5), (64, 2, 0.2), (7, 7, 0.0)])
def test_the_carried_state_form_does_not_depend_on_where_the_series_is_cut(on, off, gap):
    s, sens = _series(700, on + off)
    hi = float(np.nanquantile(s, 0.6))
    whole = ref.episodes(s, sens, hi, hi - gap, on, off, 6, first_tick=11)
    g = np.random.default_rng(3)
    for cuts in ([1], [350], list(range(1, 700, 37)), sorted(g.integers(1, 700, size=12).tolist())):
        st, at = None, 0
        for c in cuts + [700]:
            if c > at:
                st = ref.run(s[at:c], sens[at:c], hi, hi - gap, on, off, 6, first_tick=11 + at, state=st)
            at = max(at, c)
        assert ref.same(ref.table(st, 3), whole), cuts
    assert np.all((whole["end"] > whole["start"]) | (whole["end"] == -1))
    assert whole["count"] >= len(whole["start"]) and len(whole["start"]) <= 6


def test_on_delay_deadband_off_delay_first_peak_and_the_count_beyond_cap():
    hi, lo = 1.0, 0.5
    #            0    1    2    3    4    5    6    7    8    9    10   11   12   13   14   15
    s = np.array([2.0, 2.0, 0.0, 2.0, 3.0, 3.0, 0.7, 0.4, 0.7, 0.4, 0.4, 2.0, np.nan, np.nan, 5.0, 5.0])
    sens = np.arange(16, dtype=np.int32).reshape(16, 1)
    got = ref.episodes(s, sens, hi, lo, 3, 2, 4096)
    # ticks 0-1: two above, on = 3: no raise.  3-5 raise at 5, start 3; 6, 8 sit in the deadband, 7 alone is one below
    # tick (off = 2): no clear; 9-10 clear at 10, end 9.  11 alone; 12-13 NaN are below; 14-15: two above only.
    assert got["count"] == 1 and got["start"].tolist() == [3] and got["end"].tolist() == [9]
    assert got["peak"].tolist() == [3.0] and got["peak_tick"].tolist() == [4] and got["sensors"].tolist() == [[4]]
    got = ref.episodes(s, sens, hi, lo, 2, 2, 1)
    # on = 2: 0-1 raise; tick 2 alone does not clear, so the episode runs on to 9; 14-15 raise a second one, beyond cap
    assert got["count"] == 2 and got["start"].tolist() == [0] and got["end"].tolist() == [9]
    assert got["peak_tick"].tolist() == [4]
    got = ref.episodes(s, sens, hi, lo, 2, 1, 4096)
    assert list(zip(got["start"].tolist(), got["end"].tolist())) == [(0, 2), (3, 7), (14, -1)]
    assert got["peak_tick"].tolist() == [0, 4, 14]
    assert ref.episodes(s, sens, hi, lo, 2, 1, 0)["count"] == 3 and ref.episodes(s, sens, 9.0, 9.0, 1, 1, 8)["count"] == 0


def test_host_side_refusals_name_their_argument():
    from gdn_amd import harness, ops
    s = torch.zeros((4,), dtype=torch.float64)
    sens = torch.zeros((4, 1), dtype=torch.int32)
    for kw, word in ((dict(hi=1.0, lo=2.0), "clear level"), (dict(hi=float("nan")), "clear level"),
                     (dict(hi=1.0, on=0), "on = 0"), (dict(hi=1.0, off=4097), "off = 4097"),
                     (dict(hi=1.0, cap=-1), "cap = -1"), (dict(hi=1.0, first_tick=-2), "first_tick")):
        with pytest.raises(ValueError, match=word):
            harness.episodes(s, sens, **kw)
    with pytest.raises(ValueError, match="hi"):
        harness.episodes(s, sens)
    assert ops.episodes_check(2.0, None, 1, 1, 0) == (2.0, 2.0, 1, 1, 0)
    with pytest.raises(ValueError, match="unknown key 'hi'"):
        harness.events_config(dict(hi=1.0), 1)
    with pytest.raises(ValueError, match="on = 0"):
        harness.events_config(dict(on=0), 1)
    assert harness.events_config(dict(off=4), 3) == {"on": 1, "off": 4, "cap": 4096, "m": 3, "lo": None}

    class NoTopM(harness.SeriesEvaluator):
        def __init__(self):
            self.top_m = 0
    with pytest.raises(ValueError, match="top_m"):
        harness.episodes(NoTopM(), 1.0)


def _with_events(sd, on=3, off=5, cap=16, m=M):
    from gdn_amd import harness
    sd = dict(sd)
    sd["events"] = np.zeros((harness.events_bytes(m, cap),), dtype=np.uint8)
    sd["events_cfg"] = np.array([on, off, cap, m], dtype=np.int64)
    sd["events_lo"] = np.array([0.25])
    return sd


def test_checkpoint_keys_events_off_is_the_file_it_was_and_events_on_adds_three():
    from gdn_amd import _lib, harness
    assert _lib.load().gdn_stream_events_bytes(M, 16) == harness.events_bytes(M, 16) == 160 + 32 * 16 + 4 * 16 * M
    assert _lib.load().gdn_stream_events_bytes(1, 3) == harness.events_bytes(1, 3) == 272
    assert _lib.load().gdn_stream_events_bytes(9, 3) == 0 and _lib.load().gdn_stream_events_bytes(1, (1 << 20) + 1) == 0
    plain = _dict()
    assert harness.stream_checkpoint_events(plain) is None
    harness.stream_checkpoint_check(plain, dict(_expect(), events=None))
    on = _with_events(plain)
    assert set(on) - set(plain) == {"events", "events_cfg", "events_lo"}
    assert harness.stream_checkpoint_events(on) == {"on": 3, "off": 5, "cap": 16, "m": M, "lo": 0.25}
    mine = {"on": 3, "off": 5, "cap": 16, "m": M}
    harness.stream_checkpoint_check(on, dict(_expect(), events=mine))
    harness.stream_checkpoint_check(on, _expect())           # load(): the detector is built from the file
    assert int(on["format"]) == harness.STREAM_CHECKPOINT_FORMAT == int(plain["format"])


@pytest.mark.parametrize("case", ["file_without", "file_with", "on", "off", "cap", "m", "truncated", "bytes", "cfg_range"])
def test_checkpoint_refusals_name_the_events_field(case):
    from gdn_amd import harness
    mine = {"on": 3, "off": 5, "cap": 16, "m": M}
    sd, expect, word = _with_events(_dict()), dict(_expect(), events=mine), None
    if case == "file_without":
        sd, word = _dict(), "events: the detector was saved without"
    elif case == "file_with":
        expect, word = dict(_expect(), events=None), "events: the detector was saved with"
    elif case in ("on", "off", "cap"):
        expect, word = dict(_expect(), events=dict(mine, **{case: mine[case] + 1})), rf"events\.{case} = "
    elif case == "m":
        sd, word = _with_events(_dict(), m=M - 1), r"events\.m = "
    elif case == "truncated":
        del sd["events_lo"]
        word = "without the rest of events"
    elif case == "bytes":
        sd["events"] = sd["events"][:-8]
        word = "'events' must be uint8"
    elif case == "cfg_range":
        sd["events_cfg"] = np.array([0, 5, 16, M], dtype=np.int64)
        word = "events_cfg"
    with pytest.raises(ValueError, match=word):
        harness.stream_checkpoint_check(sd, expect)


def test_the_episode_flags_need_a_stream():
    from gdn_amd import main
    for flags, word in ((["-stream_on", "3"], "-stream_on needs -stream C"), (["-stream_off", "2"], "-stream_off needs -stream C"),
                        (["-stream_clear", "0.5"], "-stream_clear needs -stream C"),
                        (["-stream_events", "out.npz"], "-stream_events needs -stream C")):
        with pytest.raises(ValueError, match=word):
            main.from_args(flags)
    assert main.stream_events_config(None, None, None, "") is None
    assert main.stream_events_config(3, None, None, "") == {"on": 3, "off": 1, "lo": None}
    assert main.stream_events_config(None, None, 0.5, "x.npz") == {"on": 1, "off": 1, "lo": 0.5}
    main.check_stream_events(True, True, True, True, True)
