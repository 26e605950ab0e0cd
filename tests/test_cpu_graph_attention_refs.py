"""CPU side of tests/test_gpu_graph_stages.py and tests/test_gpu_attention_stages.py: the host restatements of
tests/_graph_build_ref.py pinned to oracle/gdn_oracle.py and tests/_localise_ref.py on the golden model cases, the
rows the tie / NaN / all-identical inputs must give, the share of float64-decided rows of every random-embedding case,
and the host refusals of the graph and attention entry points (decided before any launch: fake pointers, no device).
The refusals tests/test_cpu_localise.py already holds (w outside 1 .. 1024, k = 0, windows past the series, its own
n / k corners) are not repeated here; the attention corners below are the ones next to the widest form."""
import numpy as np
import pytest
import torch

import _graph_build_ref as gref
import _localise_ref as lref
from conftest import MODEL_CASES, load_golden, meta
from oracle import gdn_oracle

GDN_ERR_ARG, GDN_ERR_UNSUPPORTED = -1, -3
FAKE = 4096          # a non-null, 16-byte aligned address that is never dereferenced on the host


# ---- the restatements on the golden model cases -------------------------------------------------------------------

@pytest.mark.parametrize("case", MODEL_CASES)
def test_ranking_restatement_equals_the_oracle(case):
    data, p = load_golden(case)
    k = meta(data)["k"]
    cos = gdn_oracle.cosine_matrix(p["embedding.weight"].double())
    want = torch.topk(cos, k, dim=-1)
    got = gref.rank_rows(cos.numpy())[:, :k]
    np.testing.assert_array_equal(np.take_along_axis(cos.numpy(), got, axis=1), want.values.numpy())
    srt = np.take_along_axis(cos.numpy(), gref.rank_rows(cos.numpy())[:, :k + 1], axis=1)
    untied = (np.diff(srt, axis=1) != 0).all(axis=1)            # torch.topk leaves the order of ties open
    assert untied.any()
    np.testing.assert_array_equal(got[untied], want.indices.numpy()[untied])
    np.testing.assert_array_equal(got[untied], gdn_oracle.learned_graph(p["embedding.weight"].double(), k).numpy()[untied])
    tied = got[~untied]                                          # ours: equal values in ascending index
    vals = np.take_along_axis(cos.numpy()[~untied], tied, axis=1)
    assert (np.diff(tied, axis=1)[np.diff(vals, axis=1) == 0] > 0).all()


@pytest.mark.parametrize("case", MODEL_CASES)
def test_list_restatement_equals_the_localise_helper(case):
    data, _ = load_golden(case)
    m = meta(data)
    graph = data["learned_graph"]
    nb, deg = lref.neighbours(graph)
    nbr, deg2 = gref.lists_from_table(graph)
    np.testing.assert_array_equal(deg2, deg)
    np.testing.assert_array_equal(nbr, gref.with_sentinel(nb, m["n"], m["k"]))
    np.testing.assert_array_equal(gref.with_padding(nbr, m["n"])[:, :m["k"] + 1], nb)
    assert nbr.shape[1] == gref.pitch_of(m["k"]) and nbr.shape[1] % 16 == 0


@pytest.mark.parametrize("name", list(gref.injected_tables()))
def test_list_restatement_follows_the_rule_word_by_word(name):
    table = gref.injected_tables()[name]
    n, k = table.shape
    nbr, deg = gref.lists_from_table(table)
    for i in range(0, n, max(1, n // 40)):
        kept = []
        for j in table[i].tolist():
            if 0 <= j < n and j != i and j not in kept:
                kept.append(j)
        kept.append(i)
        assert deg[i] == len(kept) and nbr[i, :len(kept)].tolist() == kept and (nbr[i, len(kept):] == n).all()
    if name.startswith("k15"):
        assert (deg == 16).all() and nbr.shape[1] == 16
    if name.startswith("k1023"):
        assert (deg == 1024).all() and nbr.shape[1] == 1024


def test_attention_tables_hold_every_kind_of_row():
    for n, k in ((20, 15), (70, 32), (1100, 1023)):
        table, kinds = gref.attention_table(n, k)
        assert table.min() >= 0 and table.max() < n
        _, deg = gref.lists_from_table(table)
        assert deg[kinds["lone"]] == 1 and (deg[kinds["absent"]] == k + 1).all() and (deg[kinds["present"]] == k).all()
        assert (deg[kinds["short"]] < k).all() and min(len(kinds[key]) for key in ("absent", "present", "short")) >= 3


def test_targets_of_the_attention_helper_pick_rows_of_the_full_answer():
    data, p = load_golden("msl_demo_w5_k5")
    x, graph = torch.from_numpy(data["x"]), data["learned_graph"]
    alpha, nb = lref.attention_rows(p, x, graph)
    again, _ = lref.attention_rows(p, x, None, nb=nb)
    np.testing.assert_array_equal(again, alpha)
    tg = np.arange(x.shape[0]) % graph.shape[0]
    rows, _ = lref.attention_rows(p, x, graph, targets=tg)
    np.testing.assert_allclose(rows, alpha[np.arange(x.shape[0]), tg], atol=1e-15, rtol=0)


# ---- the rows the tie inputs must give ----------------------------------------------------------------------------

def _host_graph(emb, k):
    cos = gref.cosine_of_integers(emb)
    topk = gref.rank_rows(cos)[:, :k]
    return cos, topk, lref.neighbours(topk)


def test_tie_groups_rank_by_index_on_the_host():
    emb = gref.tie_embedding()
    for grp in gref.GROUPS:
        assert (emb[list(grp)] == emb[grp[0]]).all()
    assert (emb[list(gref.SCALED[1:])] == 2 * emb[gref.SCALED[0]]).all()
    for k in (5, 16, 59):
        cos, topk, _ = _host_graph(emb, k)
        for grp in gref.GROUPS:
            assert (cos[:, list(grp)] == cos[:, [grp[0]]]).all()
        assert gref.groups_in_order(topk, gref.GROUPS)
    swapped = topk.copy()
    row = np.flatnonzero((topk == 3).any(axis=1) & (topk == 17).any(axis=1))[0]
    a, b = np.flatnonzero(topk[row] == 3)[0], np.flatnonzero(topk[row] == 17)[0]
    swapped[row, a], swapped[row, b] = 17, 3
    assert not gref.groups_in_order(swapped, gref.GROUPS)        # the check can fail


@pytest.mark.parametrize("n,k", gref.IDENTICAL_CASES)
def test_identical_rows_list_the_first_k_sensors_on_the_host(n, k):
    _cos, topk, (nb, deg) = _host_graph(gref.identical_embedding(n), k)
    np.testing.assert_array_equal(topk, np.tile(np.arange(k), (n, 1)))
    np.testing.assert_array_equal(deg, np.where(np.arange(n) < k, k, k + 1))
    np.testing.assert_array_equal(nb[np.arange(n), deg - 1], np.arange(n))


@pytest.mark.parametrize("n,zeros", gref.ZERO_CASES, ids=[f"n{n}-zeros{len(z)}" for n, z in gref.ZERO_CASES])
def test_zero_rows_rank_first_and_by_index_on_the_host(n, zeros):
    emb = gref.zero_row_embedding(n, zeros)
    assert ((emb == 0).all(axis=1) == np.isin(np.arange(n), zeros)).all()
    cos, topk, _ = _host_graph(emb, 6)
    assert np.array_equal(np.isnan(cos), np.isnan(gdn_oracle.cosine_matrix(torch.from_numpy(emb).double()).numpy()))
    assert gref.zero_rows_expected(topk, zeros, n, 6)
    assert not gref.zero_rows_expected(topk[:, ::-1], zeros, n, 6)


# ---- the random cases leave the set check something to check ------------------------------------------------------

@pytest.mark.parametrize("case", gref.RANDOM_CASES, ids=[c["id"] for c in gref.RANDOM_CASES])
def test_random_cases_have_a_clear_float64_gap_on_most_rows(case):
    assert case["k"] <= case["n"] and case["id"].count(gref.branch_of(case["n"])) == 1
    assert gref.clear_share(case) >= 0.9


def test_case_tables_cover_what_the_issue_lists():
    ns = [c["n"] for c in gref.N_EDGES]
    assert ns == [1, 2, 3, 85, 86, 127, 128, 129, 255, 256, 257, 700, 4096]
    assert all(c["d"] == 64 and c["k"] == min(c["n"], 5) for c in gref.N_EDGES)
    assert {(c["n"], c["k"]) for c in gref.K_EDGES} == {(27, 1), (27, 27), (128, 128), (300, 300), (40, 15), (40, 16),
                                                        (130, 63), (130, 64), (1023, 1023), (1024, 1023), (4096, 1023)}
    assert {(c["n"], c["d"]) for c in gref.WIDTHS} == {(n, d) for n in (27, 200) for d in (3, 50, 129, 254, 4, 16, 128, 256)}
    assert gref.branch_of(85) == "atomicP3" and 3 * 29 > 85 and gref.branch_of(128) == "atomicP2"
    assert gref.branch_of(129) == "thread" and gref.reader_of(254) == "scalar" and gref.reader_of(256) == "float4"


# ---- host refusals --------------------------------------------------------------------------------------------------

def _topk_graph(n=127, d=64, k=30):
    from gdn_amd import _lib
    return _lib.load().gdn_topk_graph(FAKE, n, d, k, FAKE, FAKE, FAKE, FAKE, None)


def _topk_graph_terms(n=127, d=64, k=30, w=15):
    from gdn_amd import _lib
    return _lib.load().gdn_topk_graph_terms(FAKE, n, d, k, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, w, FAKE, None)


def _from_topk(n=127, k=30, **_):
    from gdn_amd import _lib
    return _lib.load().gdn_graph_from_topk(FAKE, n, k, FAKE, FAKE, None)


ENVELOPE = [dict(n=4097), dict(n=27, k=28), dict(n=2000, k=1024)]


@pytest.mark.parametrize("shape", ENVELOPE, ids=["n4097", "k_is_n_plus_1", "k_plus_1_is_1025"])
def test_graph_entry_points_refuse_shapes_outside_the_envelope(shape):
    assert _topk_graph(**shape) == GDN_ERR_UNSUPPORTED
    assert _topk_graph_terms(**shape) == GDN_ERR_UNSUPPORTED
    assert _from_topk(**shape) == GDN_ERR_UNSUPPORTED


def test_graph_entry_points_refuse_a_width_no_reader_takes():
    assert _topk_graph(d=257) == GDN_ERR_UNSUPPORTED             # d % 4 != 0 beyond the scalar reader's 256
    assert _topk_graph_terms(d=257) == GDN_ERR_UNSUPPORTED
    assert _topk_graph_terms(d=50) == GDN_ERR_UNSUPPORTED        # the one-launch form has the float4 reader only
    assert _topk_graph_terms(w=65) == GDN_ERR_UNSUPPORTED
    from gdn_amd import _lib
    assert _lib.load().gdn_topk_graph(None, 127, 64, 30, FAKE, FAKE, FAKE, None, None) == GDN_ERR_ARG
    assert _lib.load().gdn_graph_from_topk(FAKE, 127, 0, FAKE, FAKE, None) == GDN_ERR_ARG


@pytest.mark.parametrize("shape", [dict(n=4097, k=1023), dict(n=1023, k=1024), dict(n=4096, k=1024)],
                         ids=["n4097_k1023", "k_is_n_plus_1_is_1024", "n4096_k1024"])
def test_attention_entry_points_refuse_the_corners_beyond_the_widest_form(shape):
    from gdn_amd import _lib
    lib = _lib.load()
    n, k = shape["n"], shape["k"]
    assert lib.gdn_attention_mean(FAKE, 2000, 0, None, FAKE, FAKE, FAKE, 8, n, 7, k, FAKE, FAKE, None) == GDN_ERR_UNSUPPORTED
    assert lib.gdn_attention_mean(FAKE, 0, 0, None, FAKE, FAKE, FAKE, 8, n, 7, k, FAKE, FAKE, None) == GDN_ERR_UNSUPPORTED
    assert lib.gdn_attention_at(FAKE, 2000, FAKE, FAKE, 4, FAKE, FAKE, FAKE, n, 7, k, FAKE, None) == GDN_ERR_UNSUPPORTED
    assert lib.gdn_attention_workspace_bytes(8, n, 7, k) == 0
    assert lib.gdn_attention_mean(FAKE, 0, 2, None, FAKE, FAKE, FAKE, 8, 4096, 7, 1023, FAKE, FAKE, None) == GDN_ERR_ARG


def test_accumulate_cells_have_fewer_partial_blocks_than_steps():
    """Host only: what test_attention_accumulate_path_against_float64 asserts before it launches."""
    from gdn_amd import _lib
    from test_gpu_attention_stages import ACC_CELLS, FORM_CELLS, form_of_pitch
    for L, NS, n, k, w, batch in ACC_CELLS:
        run = min(64, (128 * 1024) // (8 * (n | 1)))
        parts = _lib.load().gdn_attention_workspace_bytes(batch, n, w, k) // (n * gref.pitch_of(k) * 8)
        assert 1 <= parts < -(-batch // run)
    assert {form_of_pitch(gref.pitch_of(c[3])) for c in FORM_CELLS} == {(16, 1), (32, 1), (64, 1), (64, 2), (64, 4),
                                                                       (64, 8), (64, 16)}
    assert all(form_of_pitch(gref.pitch_of(c[3])) == c[:2] for c in FORM_CELLS + ACC_CELLS)
