"""The bracket path of the one-workgroup quantile select (gdn_score.hip, select_onewg_kernel), restated in numpy
(tests/_select_bracket_ref.py: sample, brackets, one counting pass with bins, counting finish, fallback) against
np.median / np.percentile on the inputs of tests/test_gpu_select_bracket.py and on random rows."""
import numpy as np
import pytest

import _select_bracket_ref as ref


def _check(bits, total, c=ref.C):
    vals, path = ref.emulate(bits, total, c)
    real = bits[bits != ref.FILLER].view(np.float64)
    np.testing.assert_array_equal(ref.med_iqr_from(vals, total), ref.numpy_med_iqr(real))
    return path


@pytest.mark.parametrize("t", ref.T_CASES)
def test_restated_select_equals_numpy_on_the_gpu_tests_inputs(t):
    cases = ref.make_cases(t)
    for name, err in cases.items():
        path = _check(ref.to_bits(err), t)
        if t < 4 * ref.S or name in ("sample_all_equal", "all_equal"):
            assert path == 1, name
        if t >= 4 * ref.S and name in ref.GROUPS["iid"]:
            assert path == 0, name          # the seeds of the GPU test stay inside their brackets


def test_restated_select_equals_numpy_on_200_random_rows():
    g = np.random.default_rng(7)
    took = [0, 0]
    for seed in range(200):
        t = int(g.integers(4 * ref.S, 32769))
        kind = seed % 4
        err = (g.random(t), np.exp(g.standard_normal(t)), g.gamma(2.0, 0.6, t), np.round(g.random(t), 2))[kind]
        bits = ref.to_bits(err.astype(np.float32))
        took[_check(bits, t)] += 1
        # a margin far too small: ranks miss their brackets and must agree through the restated fallback
        took[_check(bits, t, c=0.02)] += 1
    assert took[0] >= 150 and took[1] >= 50, took


@pytest.mark.parametrize("total,path", [(20000, 0), (12000, 1)])
def test_restated_select_with_the_filler_scattered_over_the_slots(total, path):
    """total < pitch: the filler sorts last in the sample, the ranks scale by the real samples; fewer than S / 2
    real samples are a degenerate sample."""
    g = np.random.default_rng(total)
    bits = np.full(32768, ref.FILLER, dtype=np.uint64)
    bits[g.permutation(32768)[:total]] = ref.to_bits(g.random(total).astype(np.float32))
    assert _check(bits, total) == path
