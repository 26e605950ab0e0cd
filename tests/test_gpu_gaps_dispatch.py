"""GPU suite of the optional validity arguments: every folded wrapper of gdn_amd.ops calls
the plain symbol without them and the `_gaps` / `_keep` symbol with them, once, with the argument list of the binding
and the bits of a direct call; a partial set of optional arguments is refused before any launch; and a step of
StreamDetector / SeriesEvaluator issues exactly the launches written out below, with and without gaps.
n = 5, t = 40, w = 5, chunk = 8, m = 2, R = 64 everywhere."""
import pytest
import torch

from test_gpu_series_gaps import _evaluator, _plain
from test_gpu_stream import _detector, _model, _table

pytestmark = pytest.mark.gpu

N, T, W, CHUNK, M, R = 5, 40, 5, 8, 2, 64
MODEL = (N, W, 3, 16)
NAN = float("nan")
STEP = ("gdn_score_", "gdn_stream_", "gdn_series_")


class _Calls:
    def __init__(self, real):
        self.real, self.seen = real, []

    def __call__(self, name, *args):
        self.seen.append((name, len(args)))
        return self.real(name, *args)

    def step(self, start=0):
        return [name for name, _ in self.seen[start:] if name.startswith(STEP)]


@pytest.fixture
def calls(monkeypatch):
    from gdn_amd import _lib
    rec = _Calls(_lib.call)
    monkeypatch.setattr(_lib, "call", rec)
    return rec


def _bits(t):
    return t.contiguous().view({8: torch.int64, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def _same(got, want):
    return all(torch.equal(_bits(g), _bits(w)) for g, w in zip(got, want))


def _once(calls, name):
    """The wrapper made ONE call, of `name`, with as many arguments as the binding declares."""
    from gdn_amd import _lib
    assert calls.seen == [(name, len(_lib.SIGNATURES[name]))], calls.seen
    calls.seen.clear()


def _series(dev, seed=0):
    """pred, gt [T, N] fp32, valid [T, N] uint8 with missing readings (one whole tick among them), keep [T] uint8, the
    table and the three ticks before tick 0 (pred, gt, valid)."""
    g = torch.Generator().manual_seed(seed)
    pred, gt = torch.rand((T, N), generator=g).to(dev), torch.rand((T, N), generator=g).to(dev)
    valid = torch.ones((T, N), dtype=torch.uint8)
    valid[4, 1] = valid[5, 1] = valid[17, 0] = valid[39, 4] = 0
    valid[20, :] = 0
    keep = valid.min(dim=1).values.contiguous()
    halo = (torch.rand((3, N), generator=g).to(dev), torch.rand((3, N), generator=g).to(dev),
            torch.tensor([[1, 1, 0, 1, 1], [1, 1, 1, 1, 1], [0, 1, 1, 1, 1]], dtype=torch.uint8).to(dev))
    return pred, gt, valid.to(dev), keep.to(dev), _table(N, dev), halo


def _push(dev, calls, seed=0):
    """A stream state after W ticks of history and the buffers of one push of CHUNK ticks, filled by gdn_stream_fill."""
    from gdn_amd import ops
    g = torch.Generator().manual_seed(seed + 1)
    state = ops.stream_state(torch.rand((N, W), generator=g).to(dev), W)
    raw = torch.rand((CHUNK, N), generator=g)
    raw[0, 2] = raw[3, 0] = raw[4, 0] = raw[7, 4] = NAN
    raw[5, :] = NAN
    chunk = torch.zeros((CHUNK, N), device=dev)
    valid = torch.zeros((CHUNK, N), dtype=torch.uint8, device=dev)
    gap_chunk = torch.zeros((2, N), dtype=torch.int32, device=dev)
    ops.stream_fill(state, raw.to(dev), W, chunk, valid, gap_chunk)
    pred = torch.rand((CHUNK, N), generator=g).to(dev)
    threshold = torch.tensor([0.5], dtype=torch.float64, device=dev)
    calls.seen.clear()
    return state, chunk, valid, gap_chunk, pred, _table(N, dev), threshold


def _top(dev, rows):
    return (torch.zeros((rows, M), dtype=torch.float64, device=dev), torch.zeros((rows, M), dtype=torch.int32, device=dev),
            torch.zeros((rows,), dtype=torch.int32, device=dev))


def _st():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ 1. the six wrappers
@pytest.mark.parametrize("with_keep", [False, True])
def test_score_keys_dispatch(with_keep, calls, gpu_device):
    from gdn_amd import ops
    pred, gt, _, keep, _, _ = _series(gpu_device)
    pitch = T + 8
    got = ops.score_keys(pred, gt, pitch, keep=keep if with_keep else None)
    want = torch.zeros_like(got)
    if with_keep:
        _once(calls, "gdn_score_keys_keep")
        calls.real("gdn_score_keys_keep", pred.data_ptr(), gt.data_ptr(), keep.data_ptr(), T, N, pitch, want.data_ptr(),
                   _st())
    else:
        _once(calls, "gdn_score_keys")
        calls.real("gdn_score_keys", pred.data_ptr(), gt.data_ptr(), T, N, pitch, want.data_ptr(), _st())
    assert _same([got], [want])


@pytest.mark.parametrize("first", [0, 3])
@pytest.mark.parametrize("with_valid", [False, True])
def test_score_smooth_max_dispatch(with_valid, first, calls, gpu_device):
    from gdn_amd import ops
    dev = gpu_device
    pred, gt, valid, _, med_iqr, (hp, hg, hv) = _series(dev)
    if not first:
        hp = hg = hv = None
    kw = dict(valid=valid, halo_valid=hv) if with_valid else {}
    got = ops.score_smooth_max(pred, gt, med_iqr, first_tick=first, halo_pred=hp, halo_gt=hg, **kw)
    name = "gdn_score_smooth_max_gaps" if with_valid else "gdn_score_smooth_max"
    _once(calls, name)
    want = (torch.zeros((N, T), dtype=torch.float64, device=dev), torch.zeros((T,), dtype=torch.float64, device=dev))
    ptr = ops._ptr
    tail = (valid.data_ptr(), ptr(hv)) if with_valid else ()
    calls.real(name, pred.data_ptr(), gt.data_ptr(), med_iqr.data_ptr(), T, N, first, ptr(hp), ptr(hg), want[0].data_ptr(),
               want[1].data_ptr(), *tail, _st())
    assert _same(got, want)


@pytest.mark.parametrize("first", [0, 3])
@pytest.mark.parametrize("with_valid", [False, True])
def test_score_smooth_topm_dispatch(with_valid, first, calls, gpu_device):
    from gdn_amd import ops
    dev = gpu_device
    pred, gt, valid, _, med_iqr, (hp, hg, hv) = _series(dev)
    if not first:
        hp = hg = hv = None
    kw = dict(valid=valid, halo_valid=hv) if with_valid else {}
    got = ops.score_smooth_topm(pred, gt, med_iqr, M, first_tick=first, halo_pred=hp, halo_gt=hg, **kw)
    name = "gdn_score_smooth_topm_gaps" if with_valid else "gdn_score_smooth_topm"
    _once(calls, name)
    want = _top(dev, T)[:2]
    ptr = ops._ptr
    tail = (valid.data_ptr(), ptr(hv)) if with_valid else ()
    calls.real(name, pred.data_ptr(), gt.data_ptr(), med_iqr.data_ptr(), T, N, first, ptr(hp), ptr(hg), M,
               want[0].data_ptr(), want[1].data_ptr(), *tail, _st())
    assert _same(got, want)


@pytest.mark.parametrize("count", [CHUNK, 3])
@pytest.mark.parametrize("with_valid", [False, True])
def test_stream_score_dispatch(with_valid, count, calls, gpu_device):
    from gdn_amd import ops
    dev = gpu_device
    state, chunk, valid, _, pred, med_iqr, thr = _push(dev, calls)
    got, want = _top(dev, CHUNK), _top(dev, CHUNK)
    ops.stream_score(state, pred, chunk, med_iqr, thr, M, *got, count=count, valid=valid if with_valid else None)
    head = (state.data_ptr(), pred.data_ptr(), chunk.data_ptr())
    tail = (med_iqr.data_ptr(), thr.data_ptr(), CHUNK, count, N, M, *(b.data_ptr() for b in want), _st())
    if with_valid:
        _once(calls, "gdn_stream_score_gaps")
        calls.real("gdn_stream_score_gaps", *head, valid.data_ptr(), *tail)
    else:
        _once(calls, "gdn_stream_score")
        calls.real("gdn_stream_score", *head, *tail)
    assert _same(got, want)


@pytest.mark.parametrize("exclude", [True, False])
@pytest.mark.parametrize("with_valid", [False, True])
def test_stream_calib_write_dispatch(with_valid, exclude, calls, gpu_device):
    from gdn_amd import ops
    dev = gpu_device
    state, chunk, valid, _, pred, _, _ = _push(dev, calls)
    alarm = torch.tensor([0, 1, 0, 0, 0, 0, 1, 0], dtype=torch.int32, device=dev)
    got, want = ops.stream_calib_ring(N, R, dev), ops.stream_calib_ring(N, R, dev)
    ops.stream_calib_write(state, pred, chunk, alarm, *got, exclude_alarms=exclude, valid=valid if with_valid else None)
    head = (state.data_ptr(), pred.data_ptr(), chunk.data_ptr(), alarm.data_ptr())
    tail = (CHUNK, CHUNK, N, R, int(exclude), want[0].data_ptr(), want[1].data_ptr(), _st())
    if with_valid:
        _once(calls, "gdn_stream_calib_write_gaps")
        calls.real("gdn_stream_calib_write_gaps", *head, valid.data_ptr(), *tail)
    else:
        _once(calls, "gdn_stream_calib_write")
        calls.real("gdn_stream_calib_write", *head, *tail)
    assert _same(got, want) and int(got[1].sum()) > 0


@pytest.mark.parametrize("log", [True, False])
@pytest.mark.parametrize("with_gaps", [False, True])
def test_stream_advance_dispatch(with_gaps, log, calls, gpu_device):
    from gdn_amd import ops
    dev = gpu_device
    state, chunk, valid, gap_chunk, pred, med_iqr, _ = _push(dev, calls)
    alarm = torch.tensor([0, 1, 0, 0, 0, 0, 1, 0], dtype=torch.int32, device=dev)
    sensors = torch.tensor([[0, 1], [2, 3], [4, 0], [1, 2], [3, 4], [0, 2], [1, 3], [2, 4]], dtype=torch.int32, device=dev)

    def buffers():
        return (state.clone(), torch.zeros((16,), dtype=torch.int64, device=dev),
                torch.zeros((16, M), dtype=torch.int32, device=dev), torch.ones((2, N), dtype=torch.int64, device=dev))
    got, want = buffers(), buffers()
    kw = dict(valid=valid, gap_chunk=gap_chunk, gaps=got[3]) if with_gaps else {}
    ops.stream_advance(got[0], chunk, pred, med_iqr, alarm, sensors, W, M, *(got[1:3] if log else ()), **kw)
    tail = (med_iqr.data_ptr(), alarm.data_ptr(), sensors.data_ptr(), CHUNK, CHUNK, N, W, M,
            want[1].data_ptr() if log else None, want[2].data_ptr() if log else None, 16 if log else 0)
    if with_gaps:
        _once(calls, "gdn_stream_advance_gaps")
        calls.real("gdn_stream_advance_gaps", want[0].data_ptr(), chunk.data_ptr(), pred.data_ptr(), valid.data_ptr(),
                   gap_chunk.data_ptr(), *tail, want[3].data_ptr(), _st())
    else:
        _once(calls, "gdn_stream_advance")
        calls.real("gdn_stream_advance", want[0].data_ptr(), chunk.data_ptr(), pred.data_ptr(), *tail, _st())
    assert _same(got, want)
    assert not torch.equal(got[0], state) and int(got[0][0]) == CHUNK            # the state moved by the push
    assert torch.equal(got[3], torch.ones_like(got[3])) != with_gaps            # `gaps` is written with gaps only


# ------------------------------------------------------------------------------------------------ 2. partial sets
def test_a_partial_set_of_optional_arguments_is_refused_before_any_launch(calls, gpu_device):
    from gdn_amd import ops
    dev = gpu_device
    pred, gt, _, _, med_iqr, (hp, hg, hv) = _series(dev)
    state, chunk, valid, gap_chunk, cpred, table, _ = _push(dev, calls)
    gaps = torch.zeros((2, N), dtype=torch.int64, device=dev)
    _, sensors, alarm = _top(dev, CHUNK)
    with pytest.raises(ValueError, match="valid"):
        ops.score_smooth_max(pred, gt, med_iqr, first_tick=3, halo_pred=hp, halo_gt=hg, halo_valid=hv)
    with pytest.raises(ValueError, match="valid"):
        ops.score_smooth_topm(pred, gt, med_iqr, M, first_tick=3, halo_pred=hp, halo_gt=hg, halo_valid=hv)
    full = dict(valid=valid, gap_chunk=gap_chunk, gaps=gaps)
    for given in (("valid",), ("gap_chunk",), ("gaps",), ("valid", "gap_chunk"), ("valid", "gaps"), ("gap_chunk", "gaps")):
        before = state.clone()
        with pytest.raises(ValueError, match="valid, gap_chunk and gaps"):
            ops.stream_advance(state, chunk, cpred, table, alarm, sensors, W, M, **{key: full[key] for key in given})
        assert torch.equal(state, before), given
    assert calls.seen == []


# ------------------------------------------------------------------------------------------------ 3. launch sequences
def _stream_series(seed=0):
    return torch.rand((N, W + CHUNK), generator=torch.Generator().manual_seed(seed + 3))


@pytest.mark.parametrize("recal", [0, R])
def test_a_plain_push_issues_the_launches_it_always_did(recal, calls, gpu_device):
    dev = gpu_device
    s = _stream_series()
    det = _detector(_model(dev, *MODEL), s, W, CHUNK, dev, use_graph=False, top_m=M, recal=recal)
    start = len(calls.seen)
    det.push(s[:, W:].t().contiguous().to(dev))
    want = ["gdn_stream_windows", "gdn_stream_score"] + ["gdn_stream_calib_write"] * bool(recal) + ["gdn_stream_advance"]
    assert calls.step(start) == want
    assert det.status()[0] == CHUNK


@pytest.mark.parametrize("recal", [0, R])
def test_a_gaps_push_issues_the_gaps_launches(recal, calls, gpu_device):
    dev = gpu_device
    s = _stream_series()
    ticks = s[:, W:].t().contiguous()
    ticks[2, 1] = ticks[3, 1] = ticks[6, 4] = NAN
    det = _detector(_model(dev, *MODEL), s, W, CHUNK, dev, use_graph=False, top_m=M, recal=recal, gaps=True)
    start = len(calls.seen)
    det.push(ticks.to(dev))
    want = (["gdn_stream_fill", "gdn_stream_windows", "gdn_stream_score_gaps"]
            + ["gdn_stream_calib_write_gaps"] * bool(recal) + ["gdn_stream_advance_gaps"])
    assert calls.step(start) == want
    assert det.status()[0] == CHUNK and det.status_gaps()[0].tolist() == [0, 2, 0, 0, 1]


@pytest.mark.parametrize("top_m", [0, M])
@pytest.mark.parametrize("gaps", [False, True])
def test_an_evaluator_step_issues_the_launches_it_always_did(gaps, top_m, calls, gpu_device):
    dev = gpu_device
    series = torch.rand((N, W + T), generator=torch.Generator().manual_seed(5))
    model = _model(dev, *MODEL)
    if gaps:
        series[1, W + 4] = series[1, W + 5] = series[3, W + 30] = NAN
        ev = _evaluator(model, series.to(dev), top_m=top_m)
        assert [name for name, _ in calls.seen if name.startswith("gdn_series_")] == ["gdn_series_fill"]
        table = ["gdn_score_keys_keep", "gdn_score_select"]
    else:
        ev = _plain(model, series.to(dev), W, top_m=top_m)
        table = ["gdn_score_quantiles"]
    start = len(calls.seen)
    anomaly = ev.step()
    sweep = ("gdn_score_smooth_topm" if top_m else "gdn_score_smooth_max") + ("_gaps" if gaps else "")
    assert calls.step(start) == table + [sweep]
    assert anomaly.shape == (T,) and bool(torch.isfinite(anomaly).all())
