"""The graph build stage by stage: gdn_topk_graph, gdn_topk_graph_terms and gdn_graph_from_topk
(gdn_amd/csrc/gdn_graph.hip) at both rank-count branches (n <= 128: P = 256 / n partial counts per candidate summed
with atomicAdd; n >= 129: one thread per candidate), both row readers (float4; scalar where d % 4 != 0), the borders
of k and of the list pitch, ties, NaN rows and caller tables.  A case id names its branch and reader:
`<why>-n<n>-d<d>-k<k>-<atomicP<P>|thread>-<float4|scalar>`.

Every learned-graph case makes three assertions, none of which a near-tie between fp32 and float64 can flip:
  1  cos_out against float64 (oracle/gdn_oracle.cosine_matrix), atol 1e-6, NaN in the same places;
  2  topk_idx is the first k of a stable host sort of cos_out's own rows (tests/_graph_build_ref.rank_rows: descending,
     NaN first, equal values by index), and as a SET it is float64's top-k on the rows whose k-th and (k+1)-th float64
     cosines lie more than 1e-5 apart;
  3  nbr (all `pitch` slots, sentinel n beyond deg) and deg are tests/_localise_ref.neighbours(topk_idx).
Every case runs a second time into buffers with 64 guard words on both sides: the same bits, guards untouched.
The caller tables of gdn_graph_from_topk go through _lib.call (ops.graph_from_topk refuses entries outside [0, n) on
the host: tested on its own) against the list rule restated in tests/_graph_build_ref.lists_from_table, and through
gdn_graph_reverse against the reference of test_reverse_lists_against_the_reference.
Every test prints the worst |cos - float64| / 1e-6 of its branch and reader so far (-s).

MEASURED on the MI355X (worst |cos - float64| / 1e-6; the file takes 10 s, its longest tests 1.4 s at n = 4096, most
of it the host sort):  atomic/float4 0.22   atomic/scalar 0.21   thread/float4 0.24   thread/scalar 0.21.
FOUND: nothing: ranking, lists, deg, sentinels and guards were exact in every case."""
import numpy as np
import pytest
import torch

import _graph_build_ref as gref
import _localise_ref as lref
from _graph_layer_bwd_ref import reverse_ref
from gdn_amd import _lib, ops
from test_gpu_forward_stages import GUARD, PATTERN
from test_gpu_train_parity import check_graph_and_terms_single_launch

pytestmark = pytest.mark.gpu

COS_ATOL = 1e-6              # the bar of test_learned_graph_is_a_descending_topk_of_the_cosine_matrix
WORST = {}                   # branch / reader -> worst |cos - float64| / COS_ATOL seen in this session


def _note(n, d, ratio):
    key = f"{gref.branch_of(n).rstrip('0123456789')}/{gref.reader_of(d)}"
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"[graph-stages] {key:16s} n={n} d={d} ratio {ratio:9.2e}   worst so far {WORST[key]:9.2e}")


class Guarded:
    """An output of `dtype` cut from the middle of a buffer filled with PATTERN: GUARD elements in front and behind."""

    def __init__(self, shape, dtype, device):
        self.numel = int(np.prod(shape))
        size = torch.empty((), dtype=dtype).element_size()
        raw = {2: torch.int16, 4: torch.int32, 8: torch.int64}[size]
        self.fill = PATTERN if size >= 4 else ((PATTERN & 0xFFFF) ^ 0x8000) - 0x8000      # 0xa5a5 as an int16
        self.buf = torch.full((self.numel + 2 * GUARD,), self.fill, dtype=raw, device=device)
        self.out = self.buf[GUARD:GUARD + self.numel].view(shape)      # the raw integer view of the output
        self.ptr = self.out.data_ptr()

    def intact(self):
        edge = torch.cat((self.buf[:GUARD], self.buf[-GUARD:]))
        return bool((edge == self.fill).all())


def guarded_topk_graph(emb, k):
    """gdn_topk_graph into guarded buffers -> (topk int64, nbr int16 bits, deg int32, cos int32 bits), checked."""
    n, d = emb.shape
    dev = emb.device
    outs = dict(topk=Guarded((n, k), torch.int64, dev), nbr=Guarded((n, ops.nbr_pitch(k)), torch.int16, dev),
                deg=Guarded((n,), torch.int32, dev), cos=Guarded((n, n), torch.float32, dev))
    _lib.call("gdn_topk_graph", emb.data_ptr(), n, d, k, outs["topk"].ptr, outs["nbr"].ptr, outs["deg"].ptr,
              outs["cos"].ptr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for key, g in outs.items():
        assert g.intact(), f"gdn_topk_graph n={n} d={d} k={k}: {key} wrote outside its buffer"
    return {key: g.out for key, g in outs.items()}


def build(emb, k):
    """ops.topk_graph(emb, k, want_cos=True), then the guarded run of the same call: the same bits.  -> numpy."""
    graph = ops.topk_graph(emb, k, want_cos=True)
    again = guarded_topk_graph(emb, k)
    assert torch.equal(again["topk"], graph.topk) and torch.equal(again["deg"], graph.deg)
    assert torch.equal(again["nbr"], graph.nbr.view(torch.int16))
    assert torch.equal(again["cos"], graph.cos.view(torch.int32))
    return (graph.cos.cpu().numpy(), graph.topk.cpu().numpy(),
            graph.nbr.view(torch.int16).cpu().numpy().astype(np.int64) & 0xFFFF, graph.deg.cpu().numpy().astype(np.int64))


def check_graph(emb_cpu, k, device, cos64=None):
    """The three assertions of the module docstring.  -> (cos, topk, nbr, deg) as numpy."""
    n, d = emb_cpu.shape
    cos, topk, nbr, deg = build(emb_cpu.to(device), k)
    # 1: cosines against float64, NaN in the same places
    if cos64 is None:
        cos64 = gref.gdn_oracle.cosine_matrix(emb_cpu.to(gref.F64)).numpy()
    assert np.array_equal(np.isnan(cos), np.isnan(cos64))
    finite = ~np.isnan(cos64)
    err = float(np.abs(cos[finite] - cos64[finite]).max()) if finite.any() else 0.0
    _note(n, d, err / COS_ATOL)
    np.testing.assert_allclose(cos[finite], cos64[finite], atol=COS_ATOL, rtol=0)
    # 2: the ranking is an exact function of cos_out; as a set it is float64's where float64 decides
    np.testing.assert_array_equal(topk, gref.rank_rows(cos)[:, :k])
    clear, sets = gref.clear_rows(emb_cpu, k)
    clear = clear.numpy()
    np.testing.assert_array_equal(np.sort(topk, axis=1)[clear], np.sort(sets.numpy(), axis=1)[clear])
    # 3: the lists are an exact function of the table, over the whole pitch
    nb, want_deg = lref.neighbours(topk)
    assert nbr.shape == (n, gref.pitch_of(k))
    np.testing.assert_array_equal(deg, want_deg)
    np.testing.assert_array_equal(nbr, gref.with_sentinel(nb, n, k))
    return cos, topk, nbr, deg, clear


# ---- random embeddings: n edges, k edges, widths ------------------------------------------------------------------

@pytest.mark.parametrize("case", gref.RANDOM_CASES, ids=[c["id"] for c in gref.RANDOM_CASES])
def test_graph_build_on_random_embeddings(case, gpu_device):
    """gref.N_EDGES / K_EDGES / WIDTHS say what each case is there for; tests/test_cpu_graph_attention_refs.py holds
    the share of float64-decided rows of every one of them at 0.9 or more."""
    n, d, k = case["n"], case["d"], case["k"]
    emb = gref.embedding(n, d, case["seed"])
    _cos, topk, _nbr, deg, clear = check_graph(emb, k, gpu_device, cos64=gref.cosine_f64(n, d, case["seed"]))
    assert clear.mean() >= 0.9
    own = (topk == np.arange(n)[:, None]).any(axis=1)
    np.testing.assert_array_equal(deg, np.where(own, k, k + 1))
    if k == n:
        assert (deg == n).all()                                   # every sensor listed, self moved last


# ---- ties ---------------------------------------------------------------------------------------------------------

def test_groups_of_identical_rows_rank_by_index(gpu_device):
    """Integer-valued embeddings (every fp32 product and sum exact) with 2, 3 and 7 identical rows: equal cosines bit
    for bit, ranked by index.  The rows scaled by 2 have the same cosine up to rounding only: they are held to the
    three assertions, not to an order known beforehand."""
    emb = torch.from_numpy(gref.tie_embedding())
    for k in (5, 16, 59):
        cos, topk, _nbr, _deg, _clear = check_graph(emb, k, gpu_device)
        for grp in gref.GROUPS:
            cols = cos[:, list(grp)].view(np.int32)
            assert (cols == cols[:, :1]).all()
        assert gref.groups_in_order(topk, gref.GROUPS)


@pytest.mark.parametrize("n,k", gref.IDENTICAL_CASES)
def test_all_rows_identical(n, k, gpu_device):
    """Every cosine is the same number: every target's top-k is 0 .. k-1; targets i >= k are not in their own top-k
    (deg = k + 1, self last); at n = 40 the counts are split over P = 6 parts, at n = 200 they are not."""
    _cos, topk, nbr, deg, _clear = check_graph(torch.from_numpy(gref.identical_embedding(n)), k, gpu_device)
    np.testing.assert_array_equal(topk, np.tile(np.arange(k), (n, 1)))
    np.testing.assert_array_equal(deg, np.where(np.arange(n) < k, k, k + 1))
    np.testing.assert_array_equal(nbr[np.arange(n), deg - 1], np.arange(n))


@pytest.mark.parametrize("n,zeros", gref.ZERO_CASES, ids=[f"n{n}-zeros{len(z)}" for n, z in gref.ZERO_CASES])
def test_zero_norm_rows(n, zeros, gpu_device):
    """GDN.py:152 has no epsilon: a zero target row is all NaN (ranked by index), a zero source is NaN in every row
    (ranked first, NaN ties by index)."""
    k = 6
    cos, topk, _nbr, _deg, _clear = check_graph(torch.from_numpy(gref.zero_row_embedding(n, zeros)), k, gpu_device)
    assert np.isnan(cos[list(zeros)]).all() and np.isnan(cos[:, list(zeros)]).all()
    assert int(np.isnan(cos).sum()) == 2 * len(zeros) * n - len(zeros) ** 2
    assert gref.zero_rows_expected(topk, zeros, n, k)


# ---- the same bits from two calls -------------------------------------------------------------------------------

@pytest.mark.parametrize("case", gref.TWICE, ids=[c["id"] for c in gref.TWICE])
def test_two_calls_give_the_same_bits(case, gpu_device):
    """n = 100: the atomicAdd branch (integer counts: the order of the additions cannot matter); n = 300: the other."""
    emb = gref.embedding(case["n"], case["d"], case["seed"]).to(gpu_device)
    a, b = guarded_topk_graph(emb, case["k"]), guarded_topk_graph(emb, case["k"])
    for key in a:
        assert torch.equal(a[key], b[key]), key


# ---- gdn_topk_graph_terms -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,d,k,w", gref.TERMS_SHAPES,
                         ids=[f"n{n}-d{d}-k{k}-w{w}-{gref.branch_of(n)}" for n, d, k, w in gref.TERMS_SHAPES])
def test_graph_and_terms_single_launch_at_the_branch_borders(n, d, k, w, gpu_device):
    """The one-launch form has the bits of gdn_topk_graph (topk_idx, nbr, deg) and of gdn_node_terms: the check of
    test_graph_and_terms_single_launch_equals_the_two_entry_points at n = 27, 128 | 129 and 600."""
    check_graph_and_terms_single_launch(n, k, d, w, gpu_device)


def test_graph_and_terms_single_launch_refuses_a_width_off_the_float4_reader(gpu_device):
    n, d, k, w = 27, 50, 5, 5
    buf = torch.zeros((4096,), dtype=torch.float32, device=gpu_device)
    idx = torch.zeros((4096,), dtype=torch.int64, device=gpu_device)
    with pytest.raises(_lib.GdnHipError, match="GDN_ERR_UNSUPPORTED"):
        _lib.call("gdn_topk_graph_terms", buf.data_ptr(), n, d, k, idx.data_ptr(), idx.data_ptr(), idx.data_ptr(),
                  *[buf.data_ptr()] * 5, w, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)


# ---- gdn_graph_from_topk on caller tables ---------------------------------------------------------------------------

TABLES = gref.injected_tables()


@pytest.mark.parametrize("name", list(TABLES))
def test_lists_from_a_caller_table(name, gpu_device):
    """Repeats dropped (the first kept), entries outside [0, n) dropped, self moved last, the sentinel beyond deg; then
    the reverse lists of the same graph against the reference."""
    table = TABLES[name]
    n, k = table.shape
    topk = torch.from_numpy(table).to(gpu_device)
    nbr_g = Guarded((n, ops.nbr_pitch(k)), torch.int16, gpu_device)
    deg_g = Guarded((n,), torch.int32, gpu_device)
    _lib.call("gdn_graph_from_topk", topk.data_ptr(), n, k, nbr_g.ptr, deg_g.ptr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert nbr_g.intact() and deg_g.intact()
    nbr = nbr_g.out.cpu().numpy().astype(np.int64) & 0xFFFF
    deg = deg_g.out.cpu().numpy().astype(np.int64)
    want_nbr, want_deg = gref.lists_from_table(table)
    np.testing.assert_array_equal(deg, want_deg)
    np.testing.assert_array_equal(nbr, want_nbr)
    if name == "only-self":
        assert (deg[[0, 7, 19]] == 1).all()
    if name == "outside":
        assert (deg[[5, 6]] == 1).all()
    if name.endswith("deg16"):
        assert (deg == 16).all() and nbr.shape[1] == 16
    if name.endswith("deg1024"):
        assert (deg == 1024).all() and nbr.shape[1] == 1024
    graph = ops.SensorGraph(topk, nbr_g.out.view(torch.uint16), deg_g.out)
    rent, rlen = graph.reverse()
    rent, rlen = rent.cpu().numpy().astype(np.int64) & 0xffffffff, rlen.cpu().numpy()
    want = reverse_ref(want_nbr, want_deg)
    assert rlen.tolist() == [len(r) for r in want]
    for j in range(n):
        assert rent[j, :len(want[j])].tolist() == want[j], j


def test_the_python_wrapper_refuses_entries_outside_the_graph(gpu_device):
    table = torch.from_numpy(TABLES["self-positions"]).to(gpu_device)
    for bad in (-1, table.shape[0]):
        t = table.clone()
        t[3, 2] = bad
        with pytest.raises(ValueError, match="outside"):
            ops.graph_from_topk(t)
    graph = ops.graph_from_topk(table)
    want_nbr, want_deg = gref.lists_from_table(TABLES["self-positions"])
    np.testing.assert_array_equal(graph.deg.cpu().numpy(), want_deg)
    np.testing.assert_array_equal(graph.nbr.view(torch.int16).cpu().numpy().astype(np.int64) & 0xFFFF, want_nbr)
