"""The bracket tiers of the one-workgroup quantile select (gdn_score.hip, select_onewg_kernel) restated in numpy
(tests/_select_span_ref.py: the one-span tier in front of the three-interval tier of tests/_select_bracket_ref.py)
against np.median / np.percentile and against the three-interval restatement's path on the shared inputs."""
import numpy as np
import pytest

import _select_bracket_ref as ref
import _select_span_ref as span


def _check(bits, total, c=ref.C):
    vals, path, tier = span.emulate(bits, total, c)
    real = bits[bits != ref.FILLER].view(np.float64)
    np.testing.assert_array_equal(ref.med_iqr_from(vals, total), ref.numpy_med_iqr(real))
    assert (path == 1) == (tier == span.TIER_DIGITS)
    return path, tier


@pytest.mark.parametrize("t", ref.T_CASES)
def test_restated_tiers_on_the_shared_inputs(t):
    for name, err in ref.make_cases(t).items():
        bits = ref.to_bits(err)
        path, tier = _check(bits, t)
        # no row that the three-interval tier settles on its brackets falls to the digit passes (nor the reverse)
        assert path == ref.emulate(bits, t)[1], name
        if t >= 4 * ref.S and name in ref.GROUPS["iid"]:
            assert tier == span.TIER_SPAN, name


@pytest.mark.parametrize("t", [4 * ref.S, 8191, 20000, 32768])
def test_restated_tiers_on_the_extra_rows_of_the_gpu_test(t):
    rows = span.extra_rows(t)
    assert _check(ref.to_bits(rows["abs_normal"]), t)[1] == span.TIER_SPAN
    assert _check(ref.to_bits(rows["abs_uniform_difference"]), t)[1] == span.TIER_SPAN
    # 40 % exact zeros: the q25 pair sits among ~0.4 t equal keys, far more than CAP2 candidates in any bin
    assert _check(ref.to_bits(rows["zeros_and_lognormal"]), t)[1] == span.TIER_DIGITS


def test_restated_tiers_on_200_random_rows():
    g = np.random.default_rng(11)
    tiers = [0, 0, 0]
    for seed in range(200):
        t = int(g.integers(4 * ref.S, 32769))
        kind = seed % 4
        err = (g.random(t), np.exp(g.standard_normal(t)), g.gamma(2.0, 0.6, t), np.round(g.random(t), 2))[kind]
        bits = ref.to_bits(err.astype(np.float32))
        tiers[_check(bits, t)[1]] += 1
        tiers[_check(bits, t, c=0.02)[1]] += 1      # a margin far too small: ranks outside the span and the brackets
    assert tiers[span.TIER_SPAN] >= 150 and tiers[span.TIER_DIGITS] >= 50, tiers


def test_a_rank_just_past_the_last_bin_of_the_span_falls_through():
    err = span.rank_past_the_span()
    bits = ref.to_bits(err)
    t = err.size
    hi, L, H, _ = ref.brackets(bits, t)
    lo, up, sh, chosen = span.span_rule(L, H)
    assert chosen
    rk, _, _ = ref.ranks(t)
    srt = np.sort(hi.astype(np.int64))
    assert srt[rk[4]] <= up < srt[rk[5]]            # q75-lo is the last key of the span, q75-hi the first key past it
    assert _check(bits, t)[1] != span.TIER_SPAN


@pytest.mark.parametrize("total", [20000, 5000])
def test_restated_tiers_with_the_filler_scattered_over_the_slots(total):
    g = np.random.default_rng(total)
    bits = np.full(32768, ref.FILLER, dtype=np.uint64)
    bits[g.permutation(32768)[:total]] = ref.to_bits(g.random(total).astype(np.float32))
    path, tier = _check(bits, total)
    assert tier == (span.TIER_SPAN if total == 20000 else span.TIER_DIGITS)
    assert path == ref.emulate(bits, total)[1]
