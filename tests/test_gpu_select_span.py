"""The one-span tier in front of the three-interval tier of the one-workgroup quantile select (gdn_score.hip,
select_onewg_kernel) on the device: med_iqr bit for bit against np.median / np.percentile on the float64 keys, the
path per sensor against the numpy restatement of both tiers (tests/_select_span_ref.py, checked on the CPU by
tests/test_cpu_select_span_emulation.py), and the same bits and paths with GDN_SELECT_SPAN=0 (the three-interval
tier alone).  Launches carry at most five sensors; 4096 is the smallest row that enters the brackets, 32768 the largest
that the kernel takes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _select_bracket_ref as ref
import _select_span_ref as span

pytestmark = pytest.mark.gpu

T_SPAN = [4 * ref.S, 4 * ref.S + 1, 8191, 32768]
_ROWS, _WANT = {}, {}


def _rows(t):
    """[(name, float32 errors [t])]: every shared case, then the three extra rows."""
    if t not in _ROWS:
        cases = ref.make_cases(t)
        rows = [(k, cases[k]) for group in ref.GROUPS.values() for k in group]
        _ROWS[t] = rows + list(span.extra_rows(t).items())
    return _ROWS[t]


def _want(t):
    """(numpy's med_iqr [rows, 2], the restatement's path [rows]); computed once, shared, never changed."""
    if t not in _WANT:
        med, path = [], []
        for name, err in _rows(t):
            bits = ref.to_bits(err)
            med.append(ref.numpy_med_iqr(bits.view(np.float64)))
            path.append(span.emulate(bits, t)[1])
        _WANT[t] = (np.stack(med), np.array(path))
    return _WANT[t]


def _select_rows(t, dev="cuda:0"):
    """(med_iqr [rows, 2], path [rows]) of the device, five sensors per launch, keys from the keys kernel."""
    from gdn_amd import ops
    rows = _rows(t)
    med, path = [], []
    for i in range(0, len(rows), 5):
        errs = [e for _, e in rows[i:i + 5]]
        gt = torch.from_numpy(np.stack(errs, axis=1)).to(dev)            # pred = 0: |pred - gt| = gt exactly
        keys = ops.score_keys(torch.zeros_like(gt), gt, t)
        m, p = ops.score_select_paths(keys, 1, len(errs), t, t)
        med.append(m.cpu())
        path.append(p.cpu())
    return torch.cat(med), torch.cat(path)


def _all_tables(dev="cuda:0"):
    return {t: _select_rows(t, dev) for t in T_SPAN}


# ----------------------------------------------------------------------- 1. both tiers against numpy, path by path
@pytest.mark.parametrize("t", T_SPAN)
def test_span_select_equals_numpy_and_takes_the_restated_path(t, gpu_device):
    got, path = _select_rows(t, gpu_device)
    want, want_path = _want(t)
    for i, (name, _) in enumerate(_rows(t)):
        np.testing.assert_array_equal(got[i].numpy(), want[i], err_msg=f"{name} t={t}")
        assert int(path[i]) == int(want_path[i]), (name, t)
    names = [k for k, _ in _rows(t)]
    assert int(want_path[names.index("zeros_and_lognormal")]) == 1       # its ties go through the digit passes
    for k in ref.GROUPS["iid"] + ["abs_normal", "abs_uniform_difference"]:
        assert int(want_path[names.index(k)]) == 0, k                    # (not passing on the fallback alone)


# -------------------------------------------------------------- 2. GDN_SELECT_SPAN=0: the same bits, the same paths
def test_the_three_interval_tier_alone_gives_the_same_bits_and_paths(gpu_device, tmp_path):
    """The knob is read once per process: a fresh child runs every row under it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, torch; sys.path.insert(0, %r); sys.path.insert(0, %r + '/tests');"
            "import test_gpu_select_span as m; torch.save(m._all_tables(), sys.argv[1])")
    f = str(tmp_path / "tables.pt")
    subprocess.run([sys.executable, "-c", code % (root, root), f], check=True, timeout=300,
                   env=dict(os.environ, GDN_SELECT_SPAN="0"))
    child = torch.load(f, weights_only=True)
    for t in T_SPAN:
        got, path = _select_rows(t, gpu_device)
        assert torch.equal(child[t][0].view(torch.int64), got.view(torch.int64)), t
        assert torch.equal(child[t][1], path), t
        np.testing.assert_array_equal(child[t][0].numpy(), _want(t)[0])


# ------------------------------------------------------------------------ 3. per-sensor counts, the filler scattered
def test_span_select_with_per_sensor_counts_and_the_filler_in_random_slots(gpu_device):
    from gdn_amd import ops
    pitch, counts = 32768, [20000, 5000, 20000, 5000]
    g = np.random.default_rng(17)
    bits = np.full((len(counts), pitch), ref.FILLER, dtype=np.uint64)
    for i, c in enumerate(counts):
        err = (g.random(c) if i < 2 else np.exp(g.standard_normal(c))).astype(np.float32)
        bits[i, g.permutation(pitch)[:c]] = ref.to_bits(err)
    plane = torch.from_numpy(bits.view(np.int64)).to(gpu_device).view(torch.float64)
    cnt = torch.tensor(counts, dtype=torch.int32, device=gpu_device)
    path = torch.full((len(counts),), -1, dtype=torch.int32, device=gpu_device)
    got = ops.score_select_counts(plane, 1, len(counts), pitch, cnt, path=path).cpu().numpy()
    for i, c in enumerate(counts):
        real = bits[i][bits[i] != ref.FILLER].view(np.float64)
        assert real.size == c
        np.testing.assert_array_equal(got[i], ref.numpy_med_iqr(real), err_msg=f"sensor {i}, {c} keys")
        _, want_path, tier = span.emulate(bits[i], c)
        assert int(path[i]) == want_path, (i, c)
        assert tier == (span.TIER_SPAN if c == 20000 else span.TIER_DIGITS)    # 5000: too few real samples


# ----------------------------------------------------------------------- 4. a rank just past the span's last bin
def test_a_rank_just_past_the_last_bin_of_the_span_still_equals_numpy(gpu_device):
    from gdn_amd import ops
    err = span.rank_past_the_span()
    t = err.size
    bits = ref.to_bits(err)
    _, want_path, tier = span.emulate(bits, t)
    assert tier != span.TIER_SPAN                                        # the restatement falls through here
    gt = torch.from_numpy(np.stack([err, err[::-1].copy()], axis=1)).to(gpu_device)
    keys = ops.score_keys(torch.zeros_like(gt), gt, t)
    got, path = ops.score_select_paths(keys, 1, 2, t, t)
    want = ref.numpy_med_iqr(bits.view(np.float64))
    np.testing.assert_array_equal(got[0].cpu().numpy(), want)
    np.testing.assert_array_equal(got[1].cpu().numpy(), want)            # the same keys in reverse order
    assert int(path[0]) == want_path
