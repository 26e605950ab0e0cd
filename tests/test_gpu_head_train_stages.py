"""The train-mode head stage by stage: every entry point of gdn_head_train.hip against a float64 reference of the same
stage (tests/_head_train_ref.py: head_f64), at the four tile widths and at the run-time widths of the ANY template,
and the bit claims of include/gdn_hip.h about them.

  (a) gdn_head_train_fwd / _bwd (fp32 mask, byte keep mask, no mask), _fwd_rng / _bwd_rng (the in-kernel draw, p = 0.2),
      _fwd_rng_mse (loss and d_out folded in), _fwd_act / _bwd_act (mask, keep, draw, none) against float64: out / act,
      every gradient, BOTH BatchNorms' running mean, running variance and counter.  BN1: eps 1e-5, momentum 0.1; BN2:
      eps 1e-3, momentum 0.3; running buffers start at random values, the counter at 7.
  (b) _rng = plain + the draw as a byte mask; buffers_zeroed = 1 = 0 and leaves stats / the workspace sums zero;
      buffers_zeroed | 2 + gdn_project_bwd_partials + gdn_train_finish = _bwd_rng + gdn_project_bwd; _rng_mse =
      _rng + gdn_mse_loss_grad; two calls give the same bits.  All with torch.equal on every output.
  (c) refusals, all before any launch (the outputs and `stats` keep their fill).  The `_act` entry points take no
      lin_w / lin_b / out at all, so "`_act` with lin_w given" cannot be written against the C ABI; the converse (the
      Linear form without lin_w, lin_b or out; `_act` without act / d_act) is refused.

BOUNDS.  Ceilings: gradients _grad_check.TOL_MAX (2e-5 of the tensor's largest entry) and TOL_ELEM (1e-2 per element,
the element clamped at 1e-3 of the largest); out / act |d| <= 2e-5 + 1e-5 |want|; running statistics 1e-6 of the
tensor's largest entry; d_z element by element outside kink_elements (the seeds leave none).  Every (case, mask,
tensor) is a cell; edge-columns is judged in PARTS (`SPLIT`): column 0 (variance 0: its gradients carry 1 / sqrt(eps)),
column 2 (the mean dwarfs the spread) and the other 62 columns (the dead channel and the emb = 0 column among them),
each against its own largest entry and float32 figure; a part that is exactly 0 in float64 (d_bn1_w of column 0) must
be exactly 0.  A cell's float32 figure is the error of torch float32 CPU autograd of the same stage on the same inputs
(_head_train_ref.torch_chain: nn.BatchNorm1d x 2) against head_f64.  The bound is the smaller of the ceiling and 4 x
that figure (the factor covers another summation order).
FLOOR, a departure from the issue's rule: the figure is not taken below 2^-24 of the cell's uncancelled terms
(head_f64's `scale`: the same formula with every term by its magnitude; the largest entry where nothing cancels) — a
float32 CPU result closer than half an ulp of its terms is luck (exact hits would give a bound of 0).  It never lifts a
bound over its ceiling.  Cells that are inside their bound ONLY through the floor are marked in the -s output and
listed under MEASURED.
CANCELLATION CELLS are NAMED (`CANCELLATION`), not detected: only there, and only where torch float32 itself is beyond
the ceiling, the bound is 4 x the figure, per tensor only (the elements of a cancelled tensor have no scale of their
own).  Anywhere else a float32 figure beyond the ceiling changes nothing: the ceiling stays (marked in the output).
  d64-two-rows, d128-one-sensor   d_z, rm2, rv2: BatchNorm backward over two rows, dy - mean(dy) - xhat mean(dy xhat)
                                  cancels to ~eps / var of its terms (d_z is 1e-3 of them); two-row BN2 statistics
  edge-columns                    column 2 of every per-column tensor, and out / the fused d_out, which mix the
                                  columns: z - mean at 1000 carries 3e-5 of rounding into a spread of 0.01;
                                  d_bn1_b of column 0: a1 is constant there, h1 = a1 emb lies in the span BN2's backward
                                  removes, sum(dh1 emb) cancels to 5e-6 of its terms

MEASURED on the MI355X (worst hip / bound over an entry point's cells per family, with that cell's figures: hip error,
torch float32 CPU figure, bound; every test prints its own with -s; the whole file, 84 tests, takes 8-11 s):
  gdn_head_train_fwd / _bwd      TILE 0.78  d128-one-sensor d_bn1_w   2.60e-6   fp32 8.28e-7   bound 3.31e-6
                                 ANY  0.79  any-d1 d_lin_w            2.02e-7   fp32 6.39e-8   bound 2.56e-7
  _fwd_rng / _bwd_rng            TILE 0.40  d64-two-rows out          8.2e-3 of the ceiling   fp32 5.2e-3   bound 2.1e-2
                                 ANY  0.46  any-d3 d_emb              1.72e-7   fp32 9.03e-8   bound 3.76e-7
  _fwd_rng_mse                   TILE 0.60  d64-two-rows d_out        1.42e-7   fp32 5.76e-8   bound 2.38e-7
                                 ANY  0.55  any-d129 loss             1.1e-2 of the ceiling   fp32 5.0e-3   bound 2.1e-2
  _fwd_act / _bwd_act            TILE 0.43  d64-two-rows d_bn2_w      1.24e-7   fp32 7.25e-8   bound 2.90e-7
                                 ANY  0.78  any-d3 d_bn2_w            1.86e-7   fp32 4.12e-8   bound 2.38e-7
Inside the bound through the FLOOR only (hip > 4 x torch float32), all of them, per tensor:
  act  any-d3 draw d_bn2_w    1.86e-7  against 4 x 4.12e-8 (floor bound 2.38e-7)
  act  any-d3 keep d_bn1_b    3.18e-7  against 4 x 3.19e-8 (floor bound 2.71e-6: a column sum, 11 x its largest entry in terms)
and per element (ceiling 1e-2; hip, 4 x float32 would be): act any-d200-ragged keep d_bn2_w 3.7e-5 (3.5e-5), act any-d3
draw d_emb 1.6e-6 (1.4e-6), act any-d3 keep d_bn1_b 3.2e-7 (2.6e-7), plain any-d1 mask d_z 3.5e-6 (2.9e-6), plain any-d100
mask d_lin_w 4.1e-5 (2.4e-5), plain any-d200-ragged none d_bn1_b 4.5e-5 (4.3e-5), plain d64-n700 none d_bn2_w 2.2e-5 (8.6e-6).
Cancellation cells: d64-two-rows d_z 1.6e-6 against torch float32's 2.75e-5; d128-one-sensor d_z 2.07e-4 against 2.07e-4.
edge-columns in parts: column 2 and out 0.07-0.08 of 4 x float32 in every cell (d_z[col2] 3.2e-4 against float32's
1.1e-3, rv2[col2] 6.6e-4 against 2.3e-3, out 2.3 of the ceiling against 7.9; worst 0.25); columns 0 and the other 62
under the ordinary bounds, worst 0.38 (rv2[rest] 9.1e-8, bound 2.4e-7): d_z[rest] 1.4e-7 (float32 2.1e-7, bound 8.2e-7),
d_z[col0] 1.0e-7 (float32 5.7e-6, bound = the ceiling), d_bn1_w[col0] exactly 0.  rm2 / rv2 of column 0 are the cells
where torch float32 (1.5e-6 / 3.9e-6) is beyond the ceiling without being named: the ceiling 1e-6 stayed, hip 4.9e-8 /
2.6e-8.  Every bit claim of (b) held as the header states it, but one:
FOUND: gdn_head_train_fwd_rng_mse left its per-workgroup loss partials in the mse workspace (only the ticket word went
back to 0), where the workspace is documented as zero-filled once and reusable.  The next call overwrites every partial
it reads, so no result was wrong; the last workgroup now stores 0 over each partial after reading it (both kernel
templates), and the header says that the whole workspace is left zero.  Regression case:
test_fused_loss_equals_the_separate_loss_launch[d64].
"""
import ctypes
import functools

import pytest
import torch

import _head_train_ref as ref
from _grad_check import TOL_ELEM, TOL_MAX, rel_err
from gdn_amd import _lib, ops

pytestmark = pytest.mark.gpu

F64 = torch.float64
SEED, STEP = (5 << 32) | 424242, 3           # the draw's key: both halves of the seed in use
HALF_ULP = 2.0 ** -24
CEIL = dict(q=1.0, rel=1e-6, max=TOL_MAX, elem=TOL_ELEM, zero=0.0)
ERR_ARG, ERR_UNSUPPORTED = -1, -3
WORST = {}                                    # entry / family -> (hip / bound, hip, float32 figure, bound, cell)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


# ---- device buffers and argument lists -----------------------------------------------------------------------------

class Bufs:
    """Inputs of a case on the device, fresh running buffers, outputs filled with NaN, `stats` / workspace filled with
    NaN unless given (buffers_zeroed = 0 must zero-fill what it sums into by itself)."""

    def __init__(self, t, device, track=True, stats=None, ws=None, step=STEP):
        lib = _lib.load()
        self.batch, self.n, self.d = t["batch"], t["n"], t["d"]
        rows, d, n = self.batch * self.n, self.d, self.n
        dev = lambda v: v.to(device).contiguous()
        f32 = dict(dtype=torch.float32, device=device)
        nan = lambda *s: torch.full(s, float("nan"), **f32)
        self.z, self.emb, self.lin_w, self.lin_b = dev(t["z"]), dev(t["emb"]), dev(t["lin_w"]), dev(t["lin_b"])
        self.g1, self.b1, self.g2, self.b2 = (dev(t[bn][key]) for bn in ("bn1", "bn2") for key in ("weight", "bias"))
        self.eps = (t["bn1"]["eps"], t["bn2"]["eps"])
        self.mom = (t["bn1"]["momentum"], t["bn2"]["momentum"]) if track else (0.0, 0.0)
        self.d_out, self.d_act, self.y = dev(t["d_out"]), dev(t["d_act"]), dev(t["y"])
        self.mask, self.keep, self.keep_scale = dev(t["mask"]), dev(t["keep"]), ref.keep_scale(ref.P_DROP)
        self.rng = torch.tensor([SEED, step], dtype=torch.int64, device=device)
        self.run = [None] * 6
        if track:
            self.run = [x for bn in ("bn1", "bn2") for x in (
                dev(t[bn]["running_mean"].clone()), dev(t[bn]["running_var"].clone()),
                torch.tensor([t[bn]["batches"]], dtype=torch.int64, device=device))]
        self.stats = stats if stats is not None else torch.full((lib.gdn_head_train_stats_bytes(d) // 8,), float("nan"),
                                                                dtype=F64, device=device)
        self.ws = ws if ws is not None else torch.full((lib.gdn_head_train_workspace_bytes(n, d) // 8,), float("nan"),
                                                       dtype=F64, device=device)
        self.out, self.act, self.d_z, self.d_emb = nan(rows), nan(rows, d), nan(rows, d), nan(n, d)
        self.small = [nan(d) for _ in range(5)] + [nan(1)]          # d_bn1_w, d_bn1_b, d_bn2_w, d_bn2_b, d_lin_w, d_lin_b
        self.loss, self.mse_d_out = nan(1), nan(rows)
        self.mse_ws = torch.zeros((lib.gdn_head_mse_workspace_bytes() // 8,), dtype=F64, device=device)

    def mask_args(self, source, p):
        """mask, keep, keep_scale, rng_seed_step, p_drop"""
        return dict(mask=[ptr(self.mask), None, 1.0, None, 0.0], keep=[None, ptr(self.keep), self.keep_scale, None, 0.0],
                    none=[None, None, 1.0, None, 0.0], draw=[None, None, 1.0, ptr(self.rng), p])[source]

    def forward(self, entry, source="draw", zeroed=0, p=ref.P_DROP):
        """(entry point, arguments) of the forward; attributes set to None go in as null pointers."""
        head = [ptr(v) for v in (self.z, self.emb, self.g1, self.b1, self.g2, self.b2)]
        dims = [self.batch, self.n, self.d, *self.eps, *self.mom] + [ptr(v) for v in self.run]
        lin = [ptr(self.lin_w), ptr(self.lin_b)]
        if entry == "plain":
            return "gdn_head_train_fwd", head + lin + self.mask_args(source, p)[:3] + dims + [ptr(self.stats), ptr(self.out), _stream()]
        if entry == "rng":
            return "gdn_head_train_fwd_rng", head + lin + [ptr(self.rng), p] + dims + [ptr(self.stats), ptr(self.out), zeroed, _stream()]
        if entry == "rng_mse":
            return "gdn_head_train_fwd_rng_mse", head + lin + [ptr(self.rng), p] + dims + [
                ptr(self.stats), ptr(self.out), ptr(self.y), ptr(self.mse_ws), ptr(self.loss), ptr(self.mse_d_out), zeroed, _stream()]
        assert entry == "act"
        return "gdn_head_train_fwd_act", head + self.mask_args(source, p) + dims + [ptr(self.stats), ptr(self.act), zeroed, _stream()]

    def backward(self, entry, source="draw", zeroed=0, p=ref.P_DROP):
        head = [ptr(v) for v in (self.z, self.emb, self.g1, self.b1, self.g2, self.b2)]
        dims = [ptr(self.stats), self.batch, self.n, self.d, *self.eps, ptr(self.ws)]
        outs = [ptr(self.d_z), ptr(self.d_emb)] + [ptr(v) for v in self.small]
        if entry == "plain":
            return "gdn_head_train_bwd", [ptr(self.d_out)] + head + [ptr(self.lin_w)] + self.mask_args(source, p)[:3] + dims + outs + [_stream()]
        if entry in ("rng", "rng_mse"):
            return "gdn_head_train_bwd_rng", [ptr(self.d_out)] + head + [ptr(self.lin_w), ptr(self.rng), p] + dims + outs + [zeroed, _stream()]
        assert entry == "act"
        return "gdn_head_train_bwd_act", [ptr(self.d_act)] + head + self.mask_args(source, p) + dims + outs[:6] + [zeroed, _stream()]

    def run_both(self, entry, source="draw", zeroed=0, p=ref.P_DROP):
        _lib.call(*_flat(self.forward(entry, source, zeroed, p)))
        _lib.call(*_flat(self.backward(entry, source, zeroed, p)))
        return self.collect(entry)

    def collect(self, entry, backward=True):
        torch.cuda.synchronize()
        got = {"act" if entry == "act" else "out": (self.act if entry == "act" else self.out).cpu()}
        if backward:
            names = ref.GRADS_ACT if entry == "act" else ref.GRADS_LIN
            got.update(zip(names, [v.cpu() for v in [self.d_z, self.d_emb] + self.small]))
        for i, key in enumerate(("rm1", "rv1", "nbt1", "rm2", "rv2", "nbt2")):
            got[key] = None if self.run[i] is None else self.run[i].cpu()
        if entry == "rng_mse":
            got["loss"], got["mse_d_out"] = self.loss.cpu(), self.mse_d_out.cpu()
        return got


def _flat(name_args):
    return (name_args[0], *name_args[1])


def rc_of(name_args):
    """The entry point's return code (no exception): for the refusals."""
    return getattr(_lib.load(), name_args[0])(*name_args[1])


def sums_words(n, d):
    """fp64 words of the sums block at the head of the workspace: the byte count is affine in n."""
    ws = _lib.load().gdn_head_train_workspace_bytes
    return (ws(n, d) - n * (ws(2, d) - ws(1, d))) // 8


def is_zero(t):
    return not bool(t.view(torch.int64).any())


def same_bits(a, b, what):
    keys = [k for k in a if a[k] is not None]
    assert keys and set(keys) == {k for k in b if b[k] is not None}, what
    differ = [k for k in keys if not torch.equal(a[k], b[k])]
    assert not differ, (what, differ)
    assert all(bool(torch.isfinite(a[k]).all()) for k in keys if a[k].is_floating_point()), what


# ---- the float64 reference, the float32 figures and the comparison ----------------------------------------------

def draw_mask(t, p=ref.P_DROP, step=STEP):
    keep = ref.mix32_keep(SEED, step, t["z"].numel(), p).view(t["z"].shape)
    return keep, keep.float() * ref.keep_scale(p)


def _with_mse(res, y):
    if "out" in res:
        df = res["out"] - y.to(res["out"].dtype)
        res["loss"], res["mse_d_out"] = (df * df).mean().view(1), 2.0 * df / df.numel()
    return res


def _metrics(name, got, want, kink):
    got = got.detach().cpu().to(F64).reshape(want.shape)
    if name == "d_z" and bool(kink.any()):
        got, want = got.masked_fill(kink, 0.0), want.masked_fill(kink, 0.0)
    diff = (got - want).abs()
    if not bool(want.any()):                          # exactly 0 in float64 (xhat = 0 in the variance-0 column): exactly 0
        return dict(zero=float(diff.max()))
    if name in ("out", "act", "loss"):
        return dict(q=float((diff / (2e-5 + 1e-5 * want.abs())).max()))
    if name in ref.RUNNING:
        return dict(rel=float(diff.max() / want.abs().max()))
    elem, top_rel, _top = rel_err(got, want)
    return dict(max=top_rel, elem=elem)


# edge-columns is judged in parts: the variance-0 column (its gradients carry 1 / sqrt(eps) = 316), the column whose
# mean dwarfs its spread, and the other 62 (the dead channel and the emb = 0 column among them) each against their own
# largest entry, so that column 2's float32 noise and column 0's size do not hide the rest
SPLIT = {"edge-columns": (("col0", (0,)), ("col2", (2,)))}
PER_COLUMN = ("act",) + ref.GRADS_LIN[:7] + ref.RUNNING
# the cancellation cells, by name: only here may a bound pass its ceiling (and only where torch float32 does)
_TWO_ROWS = frozenset(("d_z", "rm2", "rv2"))
CANCELLATION = {"d64-two-rows": _TWO_ROWS, "d128-one-sensor": _TWO_ROWS,
                # (d_bn1_b[col0]: in the variance-0 column a1 is constant, so h1 = a1 emb lies in the span that BN2's
                #  backward removes: sum(dh1 emb) cancels to ~eps2 / var2 of its terms, 1e-3 of an ordinary column's)
                "edge-columns": frozenset(("out", "mse_d_out", "d_bn1_b[col0]")) | {f"{nm}[col2]" for nm in PER_COLUMN}}


def parts(case_id, name, x):
    """[(label, tensor)]: the tensor as a whole, or its column groups where the case is judged in parts."""
    groups = SPLIT.get(case_id)
    if not groups or name not in PER_COLUMN:
        return [(name, x)]
    listed = [c for _lab, cols in groups for c in cols]
    rest = [c for c in range(x.shape[-1]) if c not in listed]
    return [(f"{name}[{lab}]", x[..., list(cols)]) for lab, cols in groups] + [(f"{name}[rest]", x[..., rest])]


@functools.lru_cache(maxsize=None)
def reference(case_id, form, maskkind):
    """(head_f64's results, kink elements, {cell label: {measure: (torch float32 figure, floor)}}, the inputs):
    computed once per (case, form, mask)."""
    t = ref.inputs(ref.BY_ID[case_id])
    mask = dict(bern=t["mask"], none=None, draw=draw_mask(t)[1])[maskkind]
    lin = (t["lin_w"], t["lin_b"]) if form == "lin" else (None, None)
    args = (t["z"], t["emb"], t["bn1"], t["bn2"], mask, *lin, t["d_out"] if form == "lin" else t["d_act"], t["batch"])
    want = _with_mse(ref.head_f64(*args), t["y"])
    kink = ref.kink_elements(want["y1"], want["y2"], (want["live1"], want["live2"]))
    names = [k for k in want if k.startswith(("d_", "rm", "rv")) or k in ("out", "act", "loss", "mse_d_out")]
    res = _with_mse(ref.torch_chain(*args, dtype=torch.float32), t["y"])
    fig = {}
    for name in names:
        scale = want["scale"].get(name, want[name].abs())
        cells = zip(parts(case_id, name, want[name]), parts(case_id, name, res[name].reshape(want[name].shape)),
                    parts(case_id, name, scale), parts(case_id, name, kink if name == "d_z" else scale))
        for (label, w), (_l, r), (_s, sc), (_k, kk) in cells:
            top = float(w.abs().max())
            if top == 0.0:
                assert case_id in SPLIT, (case_id, label)
                fig[label] = dict(zero=(0.0, 0.0))
                continue
            unc = max(float(sc.max()), top) / top                        # uncancelled terms / largest entry
            floor = dict(zero=0.0, q=HALF_ULP * top / (2e-5 + 1e-5 * top), rel=HALF_ULP, max=HALF_ULP * unc, elem=1e3 * HALF_ULP * unc)
            fig[label] = {key: (v, floor[key]) for key, v in _metrics(name, r, w, kk).items()}
    return want, kink, fig, t


def bound_of(fig32, floor, key, named):
    """The smaller of the ceiling and 4 x the float32 figure (not below the format's floor); in a NAMED cancellation
    cell where float32 itself is beyond the ceiling: 4 x the figure."""
    figure = max(fig32, floor)
    return 4.0 * figure if named and fig32 > CEIL[key] else min(CEIL[key], 4.0 * figure)


def judge(case, entry, source, got, names):
    form = "act" if entry == "act" else "lin"
    maskkind = dict(mask="bern", keep="bern", none="none", draw="draw")[source]
    want, kink, fig, _t = reference(case["id"], form, maskkind)
    tag = f"{entry}/{case['family']}"
    fails = []
    for name in names:
        if want[name] is None:
            assert got[name] is None
            continue
        g = got[name].detach().cpu().reshape(want[name].shape)
        cells = zip(parts(case["id"], name, want[name]), parts(case["id"], name, g),
                    parts(case["id"], name, kink if name == "d_z" else want[name]))
        for (label, w), (_l, gg), (_k, kk) in cells:
            named = label in CANCELLATION.get(case["id"], ())
            cancelled = named and "max" in fig[label] and fig[label]["max"][0] > CEIL["max"]
            for key, v in _metrics(name, gg, w, kk).items():
                if key == "elem" and cancelled:
                    continue
                f32, floor = fig[label][key]
                bd = bound_of(f32, floor, key, named)
                ratio = (v / bd if bd > 0 else 0.0 if v == 0 else float("inf")) if v == v else float("inf")
                cell = f"{case['id']} {source} {label}.{key}"
                note = "  (cancellation cell)" if named and f32 > CEIL[key] else ""
                if not note and v > min(CEIL[key], 4.0 * f32):
                    note = "  (inside the bound by the 2^-24 floor only)"
                if not named and f32 > CEIL[key]:
                    note += "  (torch float32 is beyond the ceiling; the ceiling stays)"
                print(f"[head-stages] {tag:12s} {cell:46s} hip {v:9.2e}  fp32 {f32:9.2e}  bound {bd:9.2e}"
                      f"  hip/bound {ratio:5.2f}{note}")
                if ratio > WORST.get(tag, (-1.0,))[0]:
                    WORST[tag] = (ratio, v, f32, bd, cell)
                if not v <= bd:
                    fails.append((cell, v, bd))
    w = WORST[tag]
    print(f"[head-stages] {tag:12s} worst so far: hip/bound {w[0]:.2f} (hip {w[1]:.2e}, fp32 {w[2]:.2e}, bound {w[3]:.2e}) at {w[4]}")
    for key in ("nbt1", "nbt2"):
        assert (got[key] is None) == (want[key] is None) and (got[key] is None or int(got[key]) == want[key] == ref.COUNTER0 + 1), key
    assert not fails, fails


# ---- (a) against float64 -------------------------------------------------------------------------------------------

def _runs():
    core = [ref.BY_ID[name] for name in ref.CORE]
    runs = [("plain", "mask", c["id"]) for c in ref.CASES]
    runs += [("plain", ("keep", "none")[i % 2], c["id"]) for i, c in enumerate(core)]
    runs += [("rng", "draw", c["id"]) for c in core] + [("rng_mse", "draw", c["id"]) for c in core]
    runs += [("act", "draw", c["id"]) for c in core]
    runs += [("act", ("mask", "keep", "none")[i % 3], c["id"]) for i, c in enumerate(core)]
    return runs


RUNS = _runs()


def test_every_entry_point_and_mask_source_has_a_tile_and_an_any_cell():
    cells = {(e, s, ref.BY_ID[c]["family"]) for e, s, c in RUNS}
    pairs = [("plain", "mask"), ("plain", "keep"), ("plain", "none"), ("rng", "draw"), ("rng_mse", "draw"), ("act", "mask"),
             ("act", "keep"), ("act", "draw"), ("act", "none")]
    assert all((e, s, fam) in cells for e, s in pairs for fam in (ref.TILE, ref.ANY))
    for entry in ("plain", "rng", "rng_mse", "act"):
        assert set(ref.CORE) <= {c for e, _s, c in RUNS if e == entry}
    assert {c["id"] for c in ref.CASES} == {c for e, _s, c in RUNS if e == "plain"}


@pytest.mark.parametrize("entry,source,name", RUNS, ids=["-".join(r) for r in RUNS])
def test_head_against_float64(entry, source, name, gpu_device):
    """out / act, every gradient, both BatchNorms' running statistics and counters; for _rng_mse also loss and d_out
    (its backward is gdn_head_train_bwd_rng: judged in the `rng` runs)."""
    case = ref.BY_ID[name]
    t = ref.inputs(case)
    b = Bufs(t, gpu_device)
    if entry == "rng_mse":
        _lib.call(*_flat(b.forward(entry)))
        got = b.collect(entry, backward=False)
        names = ("out", "loss", "mse_d_out") + ref.RUNNING
    else:
        got = b.run_both(entry, source)
        names = (("act",) + ref.GRADS_ACT if entry == "act" else ("out",) + ref.GRADS_LIN) + ref.RUNNING
    for key in names:
        assert bool(torch.isfinite(got[key]).all()), (name, key)         # edge-columns included: no NaN, no inf
    judge(case, entry, source, got, names)


@pytest.mark.parametrize("name", ["d64", "any-d50"])
def test_without_running_statistics_nothing_else_changes(name, gpu_device):
    """track_running_stats off: null running_mean / running_var / batches pointers; out and every gradient keep their bits."""
    t = ref.inputs(ref.BY_ID[name])
    for entry, source in (("plain", "mask"), ("act", "draw")):
        tracked = Bufs(t, gpu_device).run_both(entry, source)
        bare = Bufs(t, gpu_device, track=False).run_both(entry, source)
        assert all(bare[key] is None for key in ref.RUNNING + ("nbt1", "nbt2"))
        same_bits({k: v for k, v in tracked.items() if k[:2] not in ("rm", "rv", "nb")}, bare, (name, entry))


# ---- (b) bit claims ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["d16-ragged", "any-d3", "any-d129"])
def test_the_drawn_mask_equals_the_same_mask_read_from_bytes(name, gpu_device):
    """_rng / _act-with-draw at (seed, step, p) = the plain / _act entry points fed mix32_keep as a byte mask with
    keep_scale = float32(1 / (1 - p)): at d % 4 != 0 this pins the draw's element index to row * d + column (the real
    width, not the padded one).  p = 0 draws nothing: the plain call without a mask."""
    t = ref.inputs(ref.BY_ID[name])
    keep, _m = draw_mask(t)
    assert 0.6 < float(keep.float().mean()) < 0.95
    for drawn, fed in (("rng", "plain"), ("act", "act")):
        a = Bufs(t, gpu_device).run_both(drawn, "draw")
        b = Bufs(t, gpu_device)
        b.keep = keep.to(torch.uint8).to(gpu_device)
        same_bits(a, b.run_both(fed, "keep"), (name, drawn))
    same_bits(Bufs(t, gpu_device).run_both("rng", "draw", p=0.0), Bufs(t, gpu_device).run_both("plain", "none"), (name, "p = 0"))


@pytest.mark.parametrize("entry", ["rng", "act"])
@pytest.mark.parametrize("name", ["d64", "any-d50", "any-d200-ragged"])
def test_buffers_zeroed_equals_self_zeroing_and_leaves_the_buffers_zero(name, entry, gpu_device):
    """buffers_zeroed = 1 on zero-filled stats / workspace = buffers_zeroed = 0; after the backward every word of
    `stats` and of the workspace's sums block is 0 again; a second step (t + 1) on the same buffers = one on fresh ones."""
    lib = _lib.load()
    t = ref.inputs(ref.BY_ID[name])
    n, d = t["n"], t["d"]
    stats = torch.zeros((lib.gdn_head_train_stats_bytes(d) // 8,), dtype=F64, device=gpu_device)
    ws = torch.zeros((lib.gdn_head_train_workspace_bytes(n, d) // 8,), dtype=F64, device=gpu_device)
    words = sums_words(n, d)
    assert 0 < words < ws.numel()
    for step in (STEP, STEP + 1):
        kept = Bufs(t, gpu_device, stats=stats, ws=ws, step=step).run_both(entry, "draw", zeroed=1)
        fresh = Bufs(t, gpu_device, step=step).run_both(entry, "draw", zeroed=0)
        same_bits(kept, fresh, (name, entry, step))
        assert is_zero(stats), (name, entry, step, "stats")
        assert is_zero(ws[:words]), (name, entry, step, "workspace sums")
    first = Bufs(t, gpu_device, step=STEP).run_both(entry, "draw")
    assert not torch.equal(first["d_z"], fresh["d_z"])                     # another step, another mask


@pytest.mark.parametrize("name,w", [("d16-ragged", 5), ("d128", 33), ("d16-ragged", 33), ("d128", 5)])
def test_deferred_finish_equals_the_separate_launches(name, w, gpu_device):
    """gdn_head_train_bwd_rng with buffers_zeroed | 2, gdn_project_bwd_partials, gdn_train_finish = gdn_head_train_bwd_rng
    + gdn_project_bwd: every head gradient, d_proj_w, d_a, d_c, and the zeroed state of stats / workspace."""
    lib = _lib.load()
    t = ref.inputs(ref.BY_ID[name])
    batch, n, d = t["batch"], t["n"], t["d"]
    g = torch.Generator().manual_seed(w + d)
    x = torch.rand((batch, n, w), generator=g).to(gpu_device)
    d_xlin = torch.randn((batch * n, d), generator=g).to(gpu_device)
    d_si, d_sj = (torch.randn((batch * n,), generator=g).to(gpu_device) for _ in range(2))
    ap = ops.terms_pitch(w)
    assert ap == 64
    outs = {}
    for form in ("separate", "deferred"):
        stats = torch.zeros((lib.gdn_head_train_stats_bytes(d) // 8,), dtype=F64, device=gpu_device)
        ws = torch.zeros((lib.gdn_head_train_workspace_bytes(n, d) // 8,), dtype=F64, device=gpu_device)
        pws = torch.empty((lib.gdn_project_bwd_workspace_bytes(n, w, d) // 4,), device=gpu_device)
        proj = [torch.full(s, float("nan"), device=gpu_device) for s in ((d, w), (2, ap), (2, n))]
        b = Bufs(t, gpu_device, stats=stats, ws=ws)
        _lib.call(*_flat(b.forward("rng", zeroed=1)))
        pin = [ptr(v) for v in (x, d_xlin, d_si, d_sj)] + [batch, n, w, d, ptr(pws)]
        if form == "separate":
            _lib.call(*_flat(b.backward("rng", zeroed=1)))
            _lib.call("gdn_project_bwd", *pin, *[ptr(v) for v in proj], _stream())
        else:
            _lib.call(*_flat(b.backward("rng", zeroed=3)))
            rows = ctypes.c_int(0)
            _lib.call("gdn_project_bwd_partials", *pin, ctypes.byref(rows), _stream())
            assert rows.value > 0
            _lib.call("gdn_train_finish", ptr(ws), ptr(stats), 1, batch, n, d, ptr(b.d_emb), *[ptr(v) for v in b.small],
                      ptr(pws), rows.value, w, *[ptr(v) for v in proj], _stream())
        got = b.collect("rng")
        got.update(d_proj_w=proj[0].cpu(), d_a=proj[1].cpu(), d_c=proj[2].cpu())
        assert is_zero(stats) and is_zero(ws[:sums_words(n, d)]), form
        outs[form] = got
    same_bits(outs["separate"], outs["deferred"], (name, w))
    assert float(outs["deferred"]["d_proj_w"].abs().max()) > 0 and float(outs["deferred"]["d_emb"].abs().max()) > 0


def test_train_finish_refuses_other_widths_and_long_windows(gpu_device):
    """gdn_train_finish takes the four tile widths and w <= 64 only: GDN_ERR_UNSUPPORTED before any launch."""
    lib = _lib.load()
    scratch = torch.full((1 << 18,), 3.0, device=gpu_device)
    p = scratch.data_ptr()
    for d, w in ((50, 5), (64, 65), (256, 5)):
        rc = lib.gdn_train_finish(p, p, 1, 2, 9, d, p, p, p, p, p, p, p, p, 1, w, p, p, p, _stream())
        assert rc == ERR_UNSUPPORTED, (d, w, rc)
    torch.cuda.synchronize()
    assert bool((scratch == 3.0).all())


@pytest.mark.parametrize("name", ["d64", "any-d50"])
def test_fused_loss_equals_the_separate_loss_launch(name, gpu_device):
    """_rng_mse: out = _rng's bits; d_out = gdn_mse_loss_grad's bits on that out; loss within 1e-7 of it; the mse
    workspace is all zero afterwards and a second call on it gives the same bits."""
    t = ref.inputs(ref.BY_ID[name])
    plain = Bufs(t, gpu_device)
    _lib.call(*_flat(plain.forward("rng")))
    want = plain.collect("rng", backward=False)
    loss, d_out = ops.mse_loss_grad(plain.out, plain.y, ops.mse_workspace(gpu_device))
    fused = Bufs(t, gpu_device)
    _lib.call(*_flat(fused.forward("rng_mse")))
    got = fused.collect("rng_mse", backward=False)
    assert is_zero(fused.mse_ws)
    assert torch.equal(got["out"], want["out"]) and torch.equal(got["mse_d_out"], d_out.cpu())
    assert all(torch.equal(got[k], want[k]) for k in ref.RUNNING + ("nbt1", "nbt2"))
    assert abs(float(got["loss"]) - float(loss)) < 1e-7
    again = Bufs(t, gpu_device)
    again.mse_ws = fused.mse_ws
    _lib.call(*_flat(again.forward("rng_mse")))
    same_bits(got, again.collect("rng_mse", backward=False), name)
    assert is_zero(fused.mse_ws)


@pytest.mark.parametrize("name", ["d32-many-parts", "any-d200-ragged"])
def test_two_calls_give_the_same_bits(name, gpu_device):
    """The sums across workgroups are exact (integer atomics): the same inputs give the same bits in every output."""
    t = ref.inputs(ref.BY_ID[name])
    for entry, source in (("plain", "mask"), ("rng", "draw"), ("act", "keep")):
        first, second = (Bufs(t, gpu_device).run_both(entry, source) for _ in range(2))
        same_bits(first, second, (name, entry))


# ---- (c) refusals --------------------------------------------------------------------------------------------------

ENTRIES = (("plain", "mask"), ("rng", "draw"), ("rng_mse", "draw"), ("act", "draw"), ("act", "mask"))


def _refused(b, want_rc, what, entries=ENTRIES, p=ref.P_DROP):
    """Both directions of every entry point return `want_rc` (None: any error) and launch nothing: outputs and stats
    keep their NaN fill (the memset of stats is a launch too)."""
    for entry, source in entries:
        for name_args in (b.forward(entry, source, p=p), b.backward(entry, source, p=p)):
            rc = rc_of(name_args)
            assert rc == want_rc if want_rc is not None else rc in (ERR_ARG, ERR_UNSUPPORTED), (what, name_args[0], rc)
    torch.cuda.synchronize()
    for v in [b.out, b.act, b.d_z, b.d_emb, b.stats, b.ws, b.loss, b.mse_d_out] + b.small:
        assert bool(torch.isnan(v).all()), what
    assert all(r is None or int(r[0]) == ref.COUNTER0 for r in b.run[2::3])


def test_refusals_come_before_any_launch(gpu_device):
    t = ref.inputs(ref.BY_ID["d64"])
    fresh = lambda: Bufs(t, gpu_device)
    b = fresh()
    b.batch, b.n = 1, 1                                   # one value per channel: torch raises, so does every form
    _refused(b, ERR_ARG, "batch * n = 1")
    for d in (0, 257):
        b = fresh()
        b.d = d
        _refused(b, None, f"d = {d}")
    for p in (1.0, -0.25):
        _refused(fresh(), ERR_ARG, f"p_drop = {p}", entries=ENTRIES[1:4], p=p)
    # the Linear form without lin_w / lin_b / out / d_out, the `_act` form without act / d_act
    for attr, entries in (("lin_w", ENTRIES[:3]), ("d_out", ENTRIES[:1]), ("d_act", ENTRIES[3:])):
        b = fresh()
        setattr(b, attr, None)
        dirs = [b.backward(e, s) for e, s in entries] + ([b.forward(e, s) for e, s in entries] if attr == "lin_w" else [])
        assert all(rc_of(na) == ERR_ARG for na in dirs), attr
    for attr, entry in (("lin_b", "plain"), ("out", "plain"), ("out", "rng"), ("act", "act"), ("y", "rng_mse"), ("rng", "rng")):
        b = fresh()
        setattr(b, attr, None)
        assert rc_of(b.forward(entry, "mask" if entry == "plain" else "draw")) == ERR_ARG, (attr, entry)
        torch.cuda.synchronize()
        assert bool(torch.isnan(b.stats).all()), (attr, entry)
