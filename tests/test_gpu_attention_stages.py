"""Attention from raw data form by form: gdn_attention_mean dispatches on the list pitch to seven instantiations
<L, NS> of gdn_attention_mean_kernel (L lanes per target, NS slots per lane; gdn_amd/csrc/gdn_attention.hip), and
gdn_attention_at stages up to 1024 logits per row.  One cell per form at the smallest shape that launches it, on graphs
from ops.graph_from_topk with INJECTED tables (tests/_graph_build_ref.attention_table), so that one graph holds rows
with self absent (deg = k + 1, = pitch where k + 1 is a multiple of 16), rows with self present (deg = k), rows
shortened by repeats and one row that is only self (deg = 1).  A case id names its form: `L64-NS4-n260-k255-w7`.

Per cell, at batches of 1, 3, 67 and 130 windows (one short step, a step tail with cnt % 4 != 0, several workgroups):
  mean and weighted mean (weights with zeros) against float64 (tests/_localise_ref.attention_rows / attention_mean,
  a chunk of windows at a time) at the project's bar ATT_ATOL, ATT_RTOL = 2e-6, 1e-5; an all-zero weight vector gives
  exact zeros; every row sums to 1 within 1e-5; the slots beyond deg are exactly 0.0 over the whole pitch;
  gdn_attention_at on 48 (window, sensor) pairs (both ends of the series, sensors 0 and n - 1, the only-self row, a
  full row) against the same reference, pairs outside the data give rows of zeros;
  the series and the windows addressing give the same bits from both entry points, and so does a second call;
  the guard words around `mean` and `alpha` are untouched.
Two more cells run the accumulate path (`runs_per > 1`, `*cell + acc`): n = 4096 with k = 511 (batch 29) and k = 1023
(batch 11), where the 64 MiB budget of partial blocks allows 4 and 2 workgroups for 10 and 4 steps: asserted from
gdn_attention_workspace_bytes, so a change of the budget cannot silently un-test the path.
Every test prints the worst |hip - float64| / (ATT_ATOL + ATT_RTOL |float64|) of its form so far (-s).

MEASURED on the MI355X (worst ratio per form over its cells, mean, weighted mean and gdn_attention_at; the file takes
8 s, its longest test 2.5 s at n = 1100, k = 1023):
  <16,1> 0.009   <32,1> 0.027 (attention_at at w = 100)   <64,1> 0.018   <64,2> 0.022   <64,4> 0.011   <64,8> 0.014
  <64,16> 0.011; the accumulate cells 0.008 (k = 511) and 0.011 (k = 1023).
Every form meets the project's bar as it stands, so no cell has a bound of its own and no fp32 restatement of the
kernel was needed.  FOUND: nothing: every bit claim held (addressings, second call, exact zeros)."""
import numpy as np
import pytest
import torch

import _graph_build_ref as gref
import _localise_ref as lref
from gdn_amd import _lib, ops
from test_gpu_forward_stages import Guarded
from test_gpu_localise import ATT_ATOL, ATT_RTOL, _model, _series

pytestmark = pytest.mark.gpu

D = 16                       # the embedding width: the attention kernels see it through the node terms only
FIRST = 5                    # first window of every run of the series addressing
BATCHES = (1, 3, 67, 130)
PAIRS = 48
REF_BYTES = 100e6            # float64 reference arrays stay below this (a few of them live at a time)

# (L, NS, n, k, w): the form gdn_attention_mean launches at pitch(k); k = 32 and k = 63 are the two ends of <64,1>;
# w = 100 puts a_i / a_j at the terms pitch 128
FORM_CELLS = [(16, 1, 20, 15, 7), (32, 1, 40, 31, 7), (64, 1, 70, 32, 7), (64, 1, 70, 63, 7), (64, 2, 130, 127, 7),
              (64, 4, 260, 255, 7), (64, 8, 520, 511, 7), (64, 16, 1100, 1023, 7), (32, 1, 40, 31, 100)]
# (L, NS, n, k, w, batch): the accumulate path
ACC_CELLS = [(64, 8, 4096, 511, 7, 29), (64, 16, 4096, 1023, 7, 11)]
WORST = {}                   # form -> worst ratio seen in this session


def _id(cell):
    return "L{}-NS{}-n{}-k{}-w{}".format(*cell[:5]) + (f"-b{cell[5]}" if len(cell) > 5 else "")


def form_of_pitch(pitch):
    """The dispatch of gdn_attention_mean."""
    for limit, form in ((16, (16, 1)), (32, (32, 1)), (64, (64, 1)), (128, (64, 2)), (256, (64, 4)), (512, (64, 8))):
        if pitch <= limit:
            return form
    return (64, 16)


def _note(form, ratio):
    key = "<{},{}>".format(*form)
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"[att-stages] {key:8s} ratio {ratio:9.2e}   worst so far {WORST[key]:9.2e}")


def _ratio(got, want):
    return float((np.abs(got - want) / (ATT_ATOL + ATT_RTOL * np.abs(want))).max())


def _weights(batch):
    g = torch.Generator().manual_seed(31)
    wt = 0.25 + torch.rand((batch,), generator=g)
    wt[torch.arange(batch) % 3 == 1] = 0.0
    return wt


class Cell:
    """Parameters, series, graph (device and host lists) and node terms of one cell."""

    def __init__(self, n, k, w, windows, dev):
        self.n, self.k, self.w, self.dev = n, k, w, dev
        self.pitch = gref.pitch_of(k)
        _, self.params = _model(n, w, k, D, "cpu")
        self.series = _series(n, FIRST + windows + w + 2)
        self.table, self.kinds = gref.attention_table(n, k)
        self.graph = ops.graph_from_topk(torch.from_numpy(self.table).to(dev))
        nbr, self.deg = gref.lists_from_table(self.table)
        np.testing.assert_array_equal(self.graph.deg.cpu().numpy(), self.deg)
        np.testing.assert_array_equal(self.graph.nbr.view(torch.int16).cpu().numpy().astype(np.int64) & 0xFFFF, nbr)
        self.nb = gref.with_padding(nbr, n)                          # [n, pitch], -1 padding
        assert self.deg[self.kinds["lone"]] == 1 and (self.deg[self.kinds["absent"]] == k + 1).all()
        assert (self.deg[self.kinds["present"]] == k).all() and (self.deg[self.kinds["short"]] < k).all()
        p = {key: v.to(dev) for key, v in self.params.items()}
        pre = "gnn_layers.0.gnn."
        self.terms = ops.node_terms(p[pre + "lin.weight"], p[pre + "att_i"], p[pre + "att_j"], p[pre + "att_em_i"],
                                    p[pre + "att_em_j"], p["embedding.weight"])
        assert self.terms.numel() == 2 * ops.terms_pitch(w) + 2 * n

    def reference_means(self, batches, weights):
        """{batch: (plain, weighted)} float64 means over windows FIRST .. FIRST + batch - 1, the attention rows
        computed once, a chunk of windows at a time."""
        top = max(batches)
        chunk = max(1, int(REF_BYTES // (self.n * self.pitch * 8)))
        wt = weights.double().numpy()
        acc = {b: [np.zeros((self.n, self.pitch)), np.zeros((self.n, self.pitch))] for b in batches}
        for s in range(0, top, chunk):
            e = min(top, s + chunk)
            alpha, _ = lref.attention_rows(self.params, lref.windows_of(self.series, FIRST + s, e - s, self.w), None,
                                           nb=self.nb)
            for b in batches:
                hi = min(e, b)
                if hi > s:
                    acc[b][0] += alpha[:hi - s].sum(axis=0)
                    acc[b][1] += np.tensordot(wt[s:hi], alpha[:hi - s], axes=(0, 0))
        return {b: (acc[b][0] / b, acc[b][1] / wt[:b].sum()) for b in batches}


def _mean(cell, src, batch, weights=None, first=0):
    g = Guarded((cell.n, cell.pitch), cell.dev)
    out = ops.attention_mean(src, cell.terms, cell.graph, cell.w, first=first, batch=batch, weights=weights, out=g.out)
    torch.cuda.synchronize()
    assert g.intact(), "gdn_attention_mean wrote outside mean[n, pitch]"
    assert g.written(), "gdn_attention_mean left cells of mean[n, pitch] unwritten"
    return out


def check_means(cell, form, batches):
    dev, n = cell.dev, cell.n
    wt = _weights(max(batches))
    assert float(wt[0]) > 0 and float(wt[1]) == 0
    want = cell.reference_means(batches, wt)
    sd = cell.series.to(dev)
    pad = np.arange(cell.pitch)[None, :] >= cell.deg[:, None]
    for b in batches:
        wb = wt[:b].contiguous().to(dev)
        plain = _mean(cell, sd, b, first=FIRST)
        masked = _mean(cell, sd, b, weights=wb, first=FIRST)
        for name, got, exp in (("plain", plain, want[b][0]), ("weighted", masked, want[b][1])):
            got_np = got.cpu().numpy().astype(np.float64)
            ratio = _ratio(got_np, exp)
            print(f"[att-stages]   n={n} k={cell.k} w={cell.w} windows={b} {name}: max |hip - float64| = "
                  f"{np.abs(got_np - exp).max():.2e}")
            _note(form, ratio)
            np.testing.assert_allclose(got_np, exp, atol=ATT_ATOL, rtol=ATT_RTOL)
            np.testing.assert_allclose(got_np.sum(axis=1), 1.0, atol=1e-5)
            assert (got_np[pad] == 0).all()                         # exactly 0.0 beyond deg, over the whole pitch
        assert float(plain[cell.kinds["lone"], 0]) == 1.0            # the only-self row: one slot, weight 1
        # the same bits: a second call, and the windows addressing
        assert torch.equal(_mean(cell, sd, b, weights=wb, first=FIRST), masked)
        xw = lref.windows_of(cell.series, FIRST, b, cell.w).to(dev)
        assert torch.equal(_mean(cell, xw, b), plain)
        assert torch.equal(_mean(cell, xw, b, weights=wb), masked)
        zero = _mean(cell, sd, b, weights=torch.zeros((b,), device=dev), first=FIRST)
        assert not zero.any()


def _at(cell, src, windows, sensors, check=True):
    q = len(windows)
    g = Guarded((q, cell.pitch), cell.dev)
    out = ops.attention_at(src, torch.as_tensor(windows), torch.as_tensor(sensors), cell.terms, cell.graph, cell.w,
                           out=g.out, check=check)
    torch.cuda.synchronize()
    assert g.intact(), "gdn_attention_at wrote outside alpha[q, pitch]"
    assert g.written(), "gdn_attention_at left cells of alpha[q, pitch] unwritten"
    return out


def check_at(cell, form):
    n, w, dev = cell.n, cell.w, cell.dev
    g = np.random.default_rng(3)
    last = cell.series.shape[1] - w
    windows = np.sort(g.integers(0, last + 1, size=PAIRS))
    windows[0], windows[-1] = 0, last                                # both ends of the series
    sensors = g.integers(0, n, size=PAIRS)
    sensors[:4] = (0, n - 1, cell.kinds["lone"], cell.kinds["absent"][0])
    sensors[-1] = cell.kinds["absent"][-1]
    sd = cell.series.to(dev)
    got = _at(cell, sd, windows, sensors)
    x = torch.stack([cell.series[:, b:b + w] for b in windows])      # [q, n, w]
    want, _ = lref.attention_rows(cell.params, x, None, nb=cell.nb, targets=sensors)
    got_np = got.cpu().numpy().astype(np.float64)
    print(f"[att-stages]   n={n} k={cell.k} w={w} attention_at: max |hip - float64| = {np.abs(got_np - want).max():.2e}")
    _note(form, _ratio(got_np, want))
    np.testing.assert_allclose(got_np, want, atol=ATT_ATOL, rtol=ATT_RTOL)
    np.testing.assert_allclose(got_np.sum(axis=1), 1.0, atol=1e-5)
    pad = np.arange(cell.pitch)[None, :] >= cell.deg[sensors][:, None]
    assert (got_np[pad] == 0).all()
    assert got_np[2, 0] == 1.0 and cell.deg[sensors[3]] == cell.k + 1
    # the same bits: a second call, and the windows addressing
    assert torch.equal(_at(cell, sd, windows, sensors), got)
    xd = x.to(dev)
    assert torch.equal(_at(cell, xd, np.arange(PAIRS), sensors), got)
    # pairs outside the data: rows of zeros, the pair beside them untouched
    out = _at(cell, sd, [-1, last + 1, 0, 0, int(windows[5])], [0, 0, -1, n, int(sensors[5])], check=False)
    assert not out[:4].any() and torch.equal(out[4], got[5])
    out = _at(cell, xd, [-1, 0, 0, 5], [0, -1, n, int(sensors[5])], check=False)
    assert not out[:3].any() and torch.equal(out[3], got[5])


@pytest.mark.parametrize("cell", FORM_CELLS, ids=[_id(c) for c in FORM_CELLS])
def test_attention_form_against_float64(cell, gpu_device):
    L, NS, n, k, w = cell
    assert form_of_pitch(gref.pitch_of(k)) == (L, NS)
    c = Cell(n, k, w, max(BATCHES), gpu_device)
    if (k + 1) % 16 == 0:
        assert (c.deg[c.kinds["absent"]] == c.pitch).all()           # full rows: no padding slot
    check_means(c, (L, NS), BATCHES)
    check_at(c, (L, NS))


@pytest.mark.parametrize("cell", ACC_CELLS, ids=[_id(c) for c in ACC_CELLS])
def test_attention_accumulate_path_against_float64(cell, gpu_device):
    """Fewer partial blocks than steps: a workgroup runs several steps and adds into its own block (`*cell + acc`),
    the last workgroup runs out of windows before its last step (cnt <= 0)."""
    L, NS, n, k, w, batch = cell
    pitch = gref.pitch_of(k)
    assert form_of_pitch(pitch) == (L, NS)
    run = min(64, (128 * 1024) // (8 * (n | 1)))                     # windows staged per step (mean_plan)
    runs = -(-batch // run)
    parts = _lib.load().gdn_attention_workspace_bytes(batch, n, w, k) // (n * pitch * 8)
    assert 1 <= parts < runs, (parts, runs)
    c = Cell(n, k, w, batch, gpu_device)
    check_means(c, (L, NS), (batch,))
    check_at(c, (L, NS))
