"""Which C entry points an eval forward launches, per public entry and model state (DESIGN.md "Eval routes").

`_lib.call` is wrapped to record symbol names; every row runs its public entry once to warm constants and plans, then
records a second call and asserts the exact list.  The output of that call is also compared bit for bit with the same
model evaluated through ANOTHER public entry, which takes another Python path: forward_into against `model(x)`,
`model(x)` against forward_into, forward_series against forward_into on the materialised windows.  Only public
entry points are used.  (Since the single dispatcher all three entries pass through GDN._eval_forward, so these
equalities mostly compare a route with itself: they show that the entries agree, as they did before it; what shows
that a route is RIGHT are the symbol lists here and the float64-oracle tests of the other GPU files.)  B = T = 3
windows at the smallest shape that reaches each route; the route's precondition is asserted with gdn_tile_fits /
gdn_fused_plan_bytes."""
import functools

import pytest
import torch

from test_gpu_forward_parity import random_params
from test_gpu_fused_reordered import CASES as REORDERED_CASES

pytestmark = pytest.mark.gpu

B = 3
REFUSED = "GdnHipError, nothing launched"
PLAN, GATED, KEYS = "gdn_forward_fused_plan", "gdn_forward_fused_gated", "gdn_forward_fused_plan_keys"
S_PLAN, S_GATED, S_KEYS = ("gdn_forward_fused_series_plan", "gdn_forward_fused_series_gated",
                           "gdn_forward_fused_series_plan_keys")
PROJECT, PROJECT_WIDE, PROJECT_SERIES = "gdn_project_fwd", "gdn_project_fwd_wide", "gdn_project_fwd_series"
AGG, AGG_WIDE, HEAD, HEAD_MLP, MLP_EVAL = ("gdn_attn_aggregate_fwd", "gdn_attn_aggregate_fwd_wide", "gdn_head_fwd",
                                           "gdn_head_mlp_fwd", "gdn_mlp_eval_fwd")


def _lib_fns():
    from gdn_amd import _lib
    return _lib.load()


def _tile_without_plan(d=16):
    lib = _lib_fns()
    n = next(n for n in range(128, 4097) if lib.gdn_tile_fits(n, 4, d, 3) == 1 and lib.gdn_fused_plan_bytes(n, 4, d, 3, 0) == 0)
    return n, 4, 3, d


# name -> ((n, w, k, d), OutLayer layers, hidden); "planned": the smallest parametrised shape of test_gpu_fused_reordered
SHAPES = {
    "planned": (min(REORDERED_CASES, key=lambda c: c[0] * c[1] * c[3])[:4], 1, 256),
    "tile": (_tile_without_plan, 1, 256),
    # the plan-less series kernel projects on the matrix cores only (d >= 32): at d = 16 gdn_forward_fused_series
    # answers GDN_ERR_UNSUPPORTED, before and after the dispatcher; its row runs at the smallest width it takes
    "tile32": (functools.partial(_tile_without_plan, 32), 1, 256),
    "long": ((8, 65, 3, 16), 1, 256),
    "width": ((8, 4, 3, 24), 1, 256),
    "mlp": ((12, 4, 3, 16), 2, 32),
    "mlpwide": ((12, 4, 3, 16), 2, 260),
    # the same two heads beyond the tile (long window), where both projections share one arithmetic: see NOT_BITWISE
    "mlplong": ((12, 65, 3, 16), 2, 32),
    "mlpwidelong": ((12, 65, 3, 16), 2, 260),
}


@functools.lru_cache(maxsize=None)
def _setup(name, dev):
    shape, layers, hidden = SHAPES[name]
    n, w, k, d = shape() if callable(shape) else shape
    lib = _lib_fns()
    fits = lib.gdn_tile_fits(n, w, d, k)
    plan_bytes = [lib.gdn_fused_plan_bytes(n, w, d, k, bf16) for bf16 in (0, 1)]
    if name == "planned":
        assert fits == 1 and min(plan_bytes) > 0
    elif name in ("tile", "tile32"):
        assert n > 127 and fits == 1 and plan_bytes == [0, 0]
    elif name in ("long", "width", "mlplong", "mlpwidelong"):
        assert fits == 0
    else:
        assert fits == 1        # (gdn_project_fwd_wide is launched only where the tile fits)
    model = random_params(n, w, k, d, seed=91, out_layer_num=layers, inter=hidden).to(dev).eval()
    if layers > 1:
        assert model.mlp_fast_path_supported()
    series = torch.rand((n, B + w), generator=torch.Generator().manual_seed(92))
    x = series.unfold(1, w, 1)[:, :B].permute(1, 0, 2).contiguous()
    return model, x.to(dev), series.to(dev)


class _Spy:
    def __init__(self, monkeypatch):
        from gdn_amd import _lib
        self.names, real = [], _lib.call

        def call(name, *args):
            self.names.append(name)
            return real(name, *args)
        monkeypatch.setattr(_lib, "call", call)

    def second_call(self, fn):
        """fn() once to warm, then again: (result, symbols of the second call)."""
        fn()
        torch.cuda.synchronize()
        del self.names[:]
        out = fn()
        torch.cuda.synchronize()
        return out, list(self.names)

    def refused(self, fn):
        from gdn_amd import _lib
        for _ in range(2):      # the first call of a model as well: a refusal builds no plan on the way
            del self.names[:]
            with pytest.raises(_lib.GdnHipError):
                fn()
            assert self.names == []


_KEY_ROWS = {}


def _run(model, entry, x, series, wide=False, keys=False, mode=None):
    """One eval forward of the B windows through a public entry; `mode`: operand_range for entry 'model'."""
    n = x.shape[1]
    dev = x.device
    k = None
    if keys:    # the key rows are passed as a raw pointer: they stay in _KEY_ROWS, alive while the launch writes them
        rows = _KEY_ROWS.setdefault((n, dev), torch.zeros((n, B), dtype=torch.float64, device=dev))
        k = (torch.rand((B, n), generator=torch.Generator().manual_seed(93)).to(dev), rows.data_ptr(), B)
    if entry == "into":
        return model.forward_into(x, torch.empty((B, n), device=dev), keys=k, wide=wide)
    if entry == "series":
        return model.forward_series(series, 0, B, keys=k, wide=wide)
    before = model.operand_range
    model.operand_range = mode
    try:
        with torch.no_grad():
            return model(x, None)
    finally:
        model.operand_range = before


ROWS = [    # (shape, entry, options, symbols of the second call)
    ("planned", "into", {}, [PLAN]),
    ("planned", "model", {"mode": "auto"}, [PLAN, GATED]),
    ("planned", "model", {"mode": "narrow"}, [PLAN]),
    ("planned", "into", {"wide": True}, [GATED]),
    ("planned", "model", {"mode": "wide"}, [GATED]),
    ("planned", "into", {"keys": True}, [KEYS]),
    ("planned", "into", {"bf16": True}, [PLAN]),
    ("planned", "into", {"bf16": True, "wide": True}, [PLAN]),
    ("planned", "model", {"bf16": True, "mode": "auto"}, [PLAN]),
    ("tile", "into", {}, ["gdn_forward_fused"]),
    ("tile", "into", {"bf16": True}, ["gdn_forward_fused_bf16"]),
    ("tile", "into", {"wide": True}, [GATED]),
    ("tile", "into", {"keys": True}, REFUSED),
    ("long", "into", {}, [PROJECT, AGG, HEAD]),
    ("long", "into", {"wide": True}, [PROJECT, AGG_WIDE, HEAD]),
    ("long", "into", {"bf16": True}, REFUSED),
    ("long", "into", {"keys": True}, REFUSED),
    ("width", "into", {}, [PROJECT, AGG, HEAD]),
    ("width", "into", {"wide": True}, [PROJECT, AGG_WIDE, HEAD]),
    ("width", "into", {"bf16": True}, REFUSED),
    ("width", "into", {"keys": True}, REFUSED),
    ("planned", "series", {}, [S_PLAN]),
    ("planned", "series", {"keys": True}, [S_KEYS]),
    ("planned", "series", {"wide": True}, [S_GATED]),
    ("tile32", "series", {}, ["gdn_forward_fused_series"]),
    ("long", "series", {}, [PROJECT_SERIES, AGG, HEAD]),
    ("long", "series", {"wide": True}, [PROJECT_SERIES, AGG_WIDE, HEAD]),
    ("width", "series", {}, [PROJECT_SERIES, AGG, HEAD]),
    ("width", "series", {"wide": True}, [PROJECT_SERIES, AGG_WIDE, HEAD]),
    ("mlp", "into", {}, [PROJECT, AGG, HEAD_MLP]),
    ("mlp", "into", {"wide": True}, [PROJECT_WIDE, AGG_WIDE, HEAD_MLP]),
    ("mlpwide", "into", {}, [PROJECT, AGG, HEAD, MLP_EVAL]),
    ("mlp", "series", {}, [PROJECT_SERIES, AGG, HEAD_MLP]),
    ("mlpwide", "series", {}, [PROJECT_SERIES, AGG, HEAD, MLP_EVAL]),
    ("mlplong", "series", {}, [PROJECT_SERIES, AGG, HEAD_MLP]),
    ("mlpwidelong", "series", {}, [PROJECT_SERIES, AGG, HEAD, MLP_EVAL]),
    ("mlp", "into", {"bf16": True}, REFUSED),
    ("mlp", "into", {"keys": True}, REFUSED),
    ("mlp", "series", {"keys": True}, REFUSED),
    ("mlpwide", "into", {"bf16": True}, REFUSED),
    ("mlpwide", "into", {"keys": True}, REFUSED),
]


# Where the tile fits, gdn_project_fwd (windows) and gdn_project_fwd_series (the fp32 streaming projection) sum in
# different orders, so a series forward of an MLP-head model is not the bits of forward_into there — on the commit before
# the dispatcher either (test_gpu_mlp_fast_path.py holds both to float64 at atol 2e-6, rtol 1e-5 for that reason).  These
# rows are held to twice that bar against each other; the bit-for-bit comparison of the two MLP tails from a series is
# made by the "mlplong" / "mlpwidelong" rows, beyond the tile, where the two projections are one arithmetic.
NOT_BITWISE = {("mlp", "series"), ("mlpwide", "series")}


@pytest.mark.parametrize("what", ["keys", "bf16"])
def test_first_refusal_of_an_mlp_head_model_builds_nothing(what, gpu_device, monkeypatch):
    """A model nobody has evaluated yet: the refusal comes before the OutLayer plan is allocated or built."""
    from gdn_amd import _lib
    n, w, k, d = SHAPES["mlp"][0]
    model = random_params(n, w, k, d, seed=96, out_layer_num=2, inter=32).to(gpu_device).eval()
    model._constants()
    x = torch.rand((B, n, w), device=gpu_device)
    series = torch.rand((n, B + w), device=gpu_device)
    if what == "bf16":
        x, series = x.to(torch.bfloat16), series.to(torch.bfloat16)
    spy = _Spy(monkeypatch)
    for entry in ("into", "series"):
        with pytest.raises(_lib.GdnHipError):
            _run(model, entry, x, series, keys=what == "keys")
    assert spy.names == [] and model._constants().mlp is False


def test_plan_less_series_kernel_refuses_width_16(gpu_device, monkeypatch):
    """forward_series on the tile-without-plan shape at d = 16 reaches gdn_forward_fused_series, which refuses it."""
    from gdn_amd import _lib
    model, x, series = _setup("tile", gpu_device)
    spy = _Spy(monkeypatch)
    for _ in range(2):
        del spy.names[:]
        with pytest.raises(_lib.GdnHipError, match="gdn_forward_fused_series failed: GDN_ERR_UNSUPPORTED"):
            _run(model, "series", x, series)
    assert spy.names == ["gdn_forward_fused_series"]


@pytest.mark.parametrize("shape,entry,opts,expected", ROWS,
                         ids=["-".join([s, e] + [f"{k}={v}" for k, v in o.items()]) for s, e, o, _ in ROWS])
def test_launch_sequence_of_the_second_call(shape, entry, opts, expected, gpu_device, monkeypatch):
    model, x, series = _setup(shape, gpu_device)
    opts = dict(opts)
    if opts.pop("bf16", False):
        x = x.to(torch.bfloat16)
    spy = _Spy(monkeypatch)
    if expected == REFUSED:
        spy.refused(lambda: _run(model, entry, x, series, **opts))
        return
    out, names = spy.second_call(lambda: _run(model, entry, x, series, **opts))
    print(f"{shape} {entry} {opts}: {names}")
    assert names == expected
    # the same windows through another public entry, on another Python path
    wide = opts.get("wide", False) or opts.get("mode") == "wide"
    if entry == "into":
        other = _run(model, "model", x, series, mode="wide" if wide else "narrow")
    else:
        other = _run(model, "into", x, series, wide=wide)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0
    print(f"   max |difference| to the other entry: {float((out - other).abs().max()):.3e}")
    if (shape, entry) in NOT_BITWISE:
        torch.testing.assert_close(out, other, atol=4e-6, rtol=2e-5)
    else:
        assert torch.equal(out, other)


def test_graphed_evaluator_equals_the_eager_one(gpu_device):
    """The dispatcher is capture-safe: T = 7 ticks in batches of 3 on the planned shape, windows and series."""
    from gdn_amd import harness
    model, _, _ = _setup("planned", gpu_device)
    n, w = model.embedding.weight.shape[0], model.gnn_layers[0].gnn.lin.weight.shape[1]
    t = 7
    series = torch.rand((n, t + w), generator=torch.Generator().manual_seed(94)).to(gpu_device)
    xs = series.unfold(1, w, 1)[:, :t].permute(1, 0, 2).contiguous()
    y = series[:, w:].t().contiguous()
    for kw in ({"x_all": xs}, {"x_all": None, "series": series}):
        preds = []
        for use_graph in (True, False):
            ev = harness.SeriesEvaluator(model, y_all=y, batch=3, use_graph=use_graph, **kw)
            ev.step()
            torch.cuda.synchronize()
            preds.append(ev.pred.clone())
        assert float(preds[0].abs().max()) > 0 and torch.equal(preds[0], preds[1])


@pytest.mark.parametrize("scale", [1.0, 1.0e5], ids=["below", "above"])
def test_one_range_decision_for_windows_and_series(scale, gpu_device):
    """SeriesEvaluator.wide comes out the same from windows and from the series of the same data."""
    from gdn_amd import harness
    model, _, _ = _setup("planned", gpu_device)
    assert model.operand_range == "auto"
    n, w = model.embedding.weight.shape[0], model.gnn_layers[0].gnn.lin.weight.shape[1]
    t = 7
    series = (torch.rand((n, t + w), generator=torch.Generator().manual_seed(95)) * scale).to(gpu_device)
    xs = series.unfold(1, w, 1)[:, :t].permute(1, 0, 2).contiguous()
    y = series[:, w:].t().contiguous()
    from_windows = harness.SeriesEvaluator(model, xs, y, batch=3, use_graph=False).wide
    from_series = harness.SeriesEvaluator(model, None, y, batch=3, use_graph=False, series=series).wide
    assert from_windows is from_series is (scale > 1.0)
