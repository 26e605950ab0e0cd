"""The one-workgroup quantile select's bracket path (gdn_score.hip, select_onewg_kernel) on the device: med_iqr bit
for bit against np.median / np.percentile on the float64 keys, and through gdn_score_select_paths which sensors the
brackets settled (0) and which fell back to the digit passes (1).  Inputs: tests/_select_bracket_ref.py, whose numpy
restatement tests/test_cpu_select_bracket_emulation.py checks on the CPU."""
import numpy as np
import pytest
import torch

import _select_bracket_ref as ref

pytestmark = pytest.mark.gpu


def _select(errs, t, dev):
    """errs: list of float32 rows [t] -> (med_iqr [n, 2], path [n]) of the device, keys from the keys kernel."""
    from gdn_amd import ops
    gt = torch.from_numpy(np.stack(errs, axis=1)).to(dev)            # pred = 0: |pred - gt| = gt exactly
    keys = ops.score_keys(torch.zeros_like(gt), gt, t)
    got, path = ops.score_select_paths(keys, 1, len(errs), t, t)
    assert torch.equal(got, ops.score_quantiles(torch.zeros_like(gt), gt))
    return got.cpu().numpy(), path.cpu().numpy()


@pytest.mark.parametrize("t", ref.T_CASES)
@pytest.mark.parametrize("group", list(ref.GROUPS))
def test_bracket_select_equals_numpy(group, t, gpu_device):
    cases = ref.make_cases(t)
    names = ref.GROUPS[group]
    got, path = _select([cases[k] for k in names], t, gpu_device)
    for i, name in enumerate(names):
        keys = np.abs(0.0 - cases[name].astype(np.float64))
        np.testing.assert_array_equal(got[i], ref.numpy_med_iqr(keys), err_msg=f"{name} t={t}")
        if t < 4 * ref.S or name in ("sample_all_equal", "all_equal"):
            assert path[i] == 1, (name, t)                           # below the threshold / a sample that says nothing
        elif group == "iid":
            assert path[i] == 0, (name, t)                           # (not passing on the fallback alone)


@pytest.mark.parametrize("total,want_path", [(20000, 0), (12000, 1)])
def test_bracket_select_with_the_filler_scattered_over_the_slots(total, want_path, gpu_device):
    """total < pitch with the filler in arbitrary slots (the rolling calibration's ring): the filler sorts last in
    the sample and the ranks scale by the real samples; fewer than half the sample real -> digit passes."""
    from gdn_amd import ops
    n, pitch = 3, 32768
    g = np.random.default_rng(total)
    bits = np.full((n, pitch), ref.FILLER, dtype=np.uint64)
    for i in range(n):
        bits[i, g.permutation(pitch)[:total]] = ref.to_bits(g.random(total).astype(np.float32))
    plane = torch.from_numpy(bits.view(np.int64)).to(gpu_device).view(torch.float64)
    got, path = ops.score_select_paths(plane, 1, n, pitch, total)
    for i in range(n):
        real = bits[i][bits[i] != ref.FILLER].view(np.float64)
        np.testing.assert_array_equal(got[i].cpu().numpy(), ref.numpy_med_iqr(real))
        assert int(path[i]) == want_path
        assert ref.emulate(bits[i], total)[1] == want_path
