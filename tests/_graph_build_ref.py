"""TEST INFRASTRUCTURE: host restatements of the graph build (gdn_topk_graph, gdn_graph_from_topk in
gdn_amd/csrc/gdn_graph.hip) and the case tables shared by tests/test_gpu_graph_stages.py,
tests/test_gpu_attention_stages.py and tests/test_cpu_graph_attention_refs.py (which pins the restatements to
oracle/gdn_oracle.py and tests/_localise_ref.py on the golden model cases).  numpy / torch-CPU only."""
import functools

import numpy as np
import torch

from oracle import gdn_oracle

F64 = torch.float64
GAP = 1e-5                # float64 gap between the k-th and (k+1)-th cosine above which a row's top-k SET is decided


def pitch_of(k):
    return ((k + 1) + 15) & ~15


# ---- the ranking rule -------------------------------------------------------------------------------------------
def rank_rows(cos):
    """[n, m] cosines -> [n, m] column indices of every row in the library's order (gdn_graph.hip `ranks_before`):
    descending, NaN ranks highest, equal values (and NaN among themselves) in ascending index: a stable sort."""
    c = np.asarray(cos)
    assert not np.isinf(c).any()                       # a cosine is finite or NaN (0 / 0): +inf is free for the NaNs
    key = np.where(np.isnan(c), np.inf, c)
    return np.argsort(-key, axis=1, kind="stable")


def clear_rows(emb, k, gap=GAP):
    """float64 cosine ranking: (rows whose k-th / (k+1)-th gap exceeds `gap`, the top-k sets).  With k = n there is no
    (k+1)-th entry: every row without a NaN is decided."""
    cos = gdn_oracle.cosine_matrix(emb.to(F64))
    srt = torch.sort(cos, dim=1, descending=True)
    if k >= cos.shape[1]:
        return ~torch.isnan(cos).any(dim=1), srt.indices[:, :k]
    return (srt.values[:, k - 1] - srt.values[:, k]) > gap, srt.indices[:, :k]


def cosine_of_integers(emb):
    """Cosine matrix of integer-valued embeddings, element by element in float64 (exact dot products and squared
    norms): identical source rows give bitwise identical entries, zero rows give NaN: ties a host can rank."""
    e = np.asarray(emb, dtype=np.float64)
    assert (e == np.round(e)).all()
    dots = e @ e.T
    nrm = np.sqrt((e * e).sum(axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        return dots / (nrm[:, None] * nrm[None, :])


# ---- the list rule ----------------------------------------------------------------------------------------------
def lists_from_table(table, n=None):
    """The rule of include/gdn_hip.h for a caller's [n, k] table: keep the first occurrence of an entry, drop entries
    outside [0, n), strip self, append self, pad with the sentinel n.  -> (nbr [n, pitch] int64, deg [n])."""
    t = np.asarray(table, dtype=np.int64)
    n = t.shape[0] if n is None else n
    nbr = np.full((t.shape[0], pitch_of(t.shape[1])), n, dtype=np.int64)
    deg = np.zeros(t.shape[0], dtype=np.int64)
    for i, row in enumerate(t):
        row = row[(row >= 0) & (row < n) & (row != i)]
        first = np.sort(np.unique(row, return_index=True)[1])
        kept = np.append(row[first], i)
        nbr[i, :len(kept)] = kept
        deg[i] = len(kept)
    return nbr, deg


def with_sentinel(nb, n, k):
    """_localise_ref.neighbours' lists ([n, k+1], -1 padding) at the device's pitch with the sentinel n."""
    out = np.full((nb.shape[0], pitch_of(k)), n, dtype=np.int64)
    out[:, :nb.shape[1]] = np.where(nb < 0, n, nb)
    return out


def with_padding(nbr, n):
    """The device's lists (sentinel n) with _localise_ref's -1 padding."""
    nbr = np.asarray(nbr, dtype=np.int64)
    return np.where(nbr >= n, -1, nbr)


# ---- the cases of the graph build -------------------------------------------------------------------------------
def branch_of(n):
    """The rank-count branch of graph_row: P = 256 / n partial counts per candidate (atomicAdd) up to n = 128, one
    thread per candidate beyond."""
    return f"atomicP{256 // n}" if n <= 128 else "thread"


def reader_of(d):
    return "float4" if d % 4 == 0 else "scalar"


def _case(why, n, d, k, seed):
    return dict(id=f"{why}-n{n}-d{d}-k{k}-{branch_of(n)}-{reader_of(d)}", n=n, d=d, k=k, seed=seed, why=why)


# n edges at d = 64, k = min(n, 5): the two rank-count branches and their borders (P = 256, 128, 85 | 3 (3 x 29 > 85:
# the ragged last part), 2 | 2, 2 | 1 at 129), the strided candidate loop at n > 256, the cap
N_EDGES = [_case("n-edge", n, 64, min(n, 5), 100 + n)
           for n in (1, 2, 3, 85, 86, 127, 128, 129, 255, 256, 257, 700, 4096)]
# k edges: one slot, every sensor listed, the pitch borders 16 | 32 and 64 | 80, the widest list (pitch 1024)
K_EDGES = [_case("k1", 27, 16, 1, 201), _case("k-equals-n", 27, 16, 27, 202), _case("k-equals-n", 128, 16, 128, 203),
           _case("k-equals-n", 300, 16, 300, 204), _case("pitch16-full", 40, 16, 15, 205),
           _case("pitch32", 40, 16, 16, 206), _case("pitch64-full", 130, 64, 63, 207),
           _case("pitch80", 130, 64, 64, 208), _case("k1023-equals-n", 1023, 16, 1023, 209),
           _case("k1023", 1024, 16, 1023, 210), _case("k1023", 4096, 16, 1023, 211)]
# widths: d % 4 != 0 reads the rows column by column, d % 4 == 0 as float4; both at both rank-count branches
WIDTHS = [_case("width", n, d, 5 if n == 27 else 20, 300 + d + n)
          for d in (3, 50, 129, 254, 4, 16, 128, 256) for n in (27, 200)]
RANDOM_CASES = N_EDGES + K_EDGES + WIDTHS
TWICE = [_case("twice", 100, 64, 10, 401), _case("twice", 300, 64, 10, 402)]      # the same bits from two calls
TERMS_SHAPES = [(27, 16, 5, 5), (128, 64, 30, 15), (129, 64, 30, 64), (600, 32, 20, 30)]    # (n, d, k, w)


@functools.lru_cache(maxsize=None)
def embedding(n, d, seed):
    return torch.randn((n, d), generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=4)
def cosine_f64(n, d, seed):
    """The float64 cosine matrix of a seeded embedding: computed once, shared by the cases on it, never written."""
    return gdn_oracle.cosine_matrix(embedding(n, d, seed).to(F64)).numpy()


def clear_share(case):
    clear, _ = clear_rows(embedding(case["n"], case["d"], case["seed"]), case["k"])
    return float(clear.float().mean())


# ---- tie inputs (integer valued: every product and sum below 2^24 is exact in fp32) ----------------------------
GROUPS = ((3, 17), (5, 6, 40), (10, 11, 20, 21, 30, 50, 59))       # identical rows: 2, 3 and 7 of them
SCALED = (2, 25, 33)                                               # row 25 = row 33 = 2 x row 2


def tie_embedding(n=60, d=8, seed=7):
    g = np.random.default_rng(seed)
    emb = g.integers(-4, 5, size=(n, d)).astype(np.float32)
    emb[(emb == 0).all(axis=1), 0] = 1.0
    for grp in GROUPS:
        emb[list(grp[1:])] = emb[grp[0]]
    emb[list(SCALED[1:])] = 2.0 * emb[SCALED[0]]
    return emb


def identical_embedding(n, d=8):
    return np.tile(np.arange(1, d + 1, dtype=np.float32) - 3.0, (n, 1))


def zero_row_embedding(n, zeros, d=8, seed=9):
    g = np.random.default_rng(seed + n)
    emb = g.integers(-4, 5, size=(n, d)).astype(np.float32)
    emb[(emb == 0).all(axis=1), 0] = 1.0
    emb[list(zeros)] = 0.0
    return emb


ZERO_CASES = [(27, (13,)), (27, (0, 13, 26)), (150, (77,)), (150, (5, 77, 149))]
IDENTICAL_CASES = [(40, 7), (200, 30)]


def groups_in_order(topk, groups):
    """Rows of a tie group have the same cosine to every target: wherever one of them is in a top-k row, every lower
    index of its group is there too, and they stand in ascending index."""
    for row in np.asarray(topk):
        where = {int(j): r for r, j in enumerate(row)}
        for grp in groups:
            ranks = [where.get(j) for j in grp]
            seen = [r for r in ranks if r is not None]
            if ranks[:len(seen)] != seen or seen != sorted(seen):
                return False
    return True


def zero_rows_expected(topk, zeros, n, k):
    """A zero target row is all NaN: ranked by index.  A zero source is NaN in every row: it ranks first, by index."""
    topk = np.asarray(topk)
    zs = sorted(zeros)
    for i in range(n):
        if i in zs:
            if topk[i].tolist() != list(range(k)):
                return False
        elif topk[i, :min(k, len(zs))].tolist() != zs[:k]:
            return False
    return True


# ---- caller tables for gdn_graph_from_topk ----------------------------------------------------------------------
def _distinct_others(g, n, i, count):
    """`count` distinct sensors other than i."""
    pick = g.choice(n - 1, size=count, replace=False)
    return pick + (pick >= i)


def injected_tables():
    """name -> [n, k] int64 table (caller data: repeats, self anywhere, entries outside [0, n))."""
    g = np.random.default_rng(17)
    out = {}
    out["repeats"] = g.integers(0, 50, size=(50, 12))                               # random, with repeats
    t = np.stack([_distinct_others(g, 30, i, 9) for i in range(30)])                 # self at rank 0 / middle / last
    for i in range(30):
        if i % 4 != 3:
            t[i, (0, 4, 8)[i % 4]] = i
    out["self-positions"] = t
    t = np.stack([_distinct_others(g, 20, i, 6) for i in range(20)])                 # rows that are all self
    t[[0, 7, 19]] = np.array([0, 7, 19])[:, None]
    out["only-self"] = t
    t = g.integers(0, 33, size=(33, 10))                                             # entries -1 and n: dropped
    t[g.random(t.shape) < 0.2] = -1
    t[g.random(t.shape) < 0.2] = 33
    t[5], t[6] = -1, 33                                                              # nothing kept but self
    out["outside"] = t
    out["k15-no-self-deg16"] = np.stack([_distinct_others(g, 40, i, 15) for i in range(40)])
    out["k1023-no-self-deg1024"] = np.stack([_distinct_others(g, 1100, i, 1023) for i in range(1100)])
    return {name: np.ascontiguousarray(t, dtype=np.int64) for name, t in out.items()}


# ---- injected tables of the attention cells ---------------------------------------------------------------------
def attention_table(n, k, seed=23):
    """[n, k] table whose lists vary inside one graph: row i % 4 == 0 has k distinct others (self absent: deg = k + 1,
    = pitch where k + 1 is a multiple of 16), == 1 has self among k distinct entries (deg = k), == 2 draws its entries
    with repeats from a few sensors (a short list), == 3 as 0; row n // 2 is only self (deg = 1).
    -> (table, dict of the rows by kind)."""
    assert k <= n - 1
    g = np.random.default_rng(seed + n + k)
    t = np.zeros((n, k), dtype=np.int64)
    for i in range(n):
        kind = i % 4
        if kind == 2:
            pool = g.integers(0, n, size=1 + int(g.integers(0, min(k, 9))))
            t[i] = pool[g.integers(0, len(pool), size=k)]
        else:
            t[i] = _distinct_others(g, n, i, k)
            if kind == 1:
                t[i, int(g.integers(0, k))] = i
    lone = n // 2
    t[lone] = lone
    kinds = dict(absent=[i for i in range(n) if i % 4 in (0, 3) and i != lone],
                 present=[i for i in range(n) if i % 4 == 1 and i != lone],
                 short=[i for i in range(n) if i % 4 == 2 and i != lone], lone=lone)
    return t, kinds
