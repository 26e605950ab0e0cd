"""CPU suite of the raw-readings front end: the yardstick of the GPU tests (tests/_prep_ref.py) against
what the reference's own scripts produced (tests/golden/prep_ref.npz, from scripts/process_swat.py's norm and
downsample), the sub-push arithmetic of a prep= detector, Prep's file format, the refusals by name, and the additive
entry points in header, bindings and library."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _prep_ref as ref
from conftest import GOLDEN, ROOT

GDN_ERR_ARG, GDN_ERR_UNSUPPORTED = -1, -3
FAKE = 4096          # a non-null, 16-byte aligned address that is never dereferenced on the host
NEW = {"gdn_prep_stats_workspace_bytes": "long long", "gdn_prep_stats": "int", "gdn_prep_series": "int",
       "gdn_prep_ticks": "int"}


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "prep_ref.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def test_the_restatement_equals_the_reference_bit_for_bit_on_the_finite_pair(gold):
    down = int(gold["down"])
    tab = ref.table(ref.stats(gold["train"]))
    assert np.array_equal(tab.view(np.int64), gold["ref_table"].view(np.int64))
    assert tab[3, 0] == 1.0 and tab[3, 1] == -7.25                   # the constant sensor: range 0 -> 1
    for name in ("train", "test"):
        got, lab, filled = ref.series(gold[name], tab, down, labels=gold[name + "_labels"])
        want = gold["ref_" + name].T
        assert got.shape == want.shape == (7, gold[name].shape[0] // down) and not filled.any()
        assert np.array_equal(ref.bits32(got), ref.bits32(want.astype(np.float32)))
        assert np.array_equal(lab, gold["ref_" + name + "_labels"])
    assert (ref.series(gold["train"], tab, down)[0][3] == 0.0).all()
    assert gold["ref_test"].max() > 1.0 or gold["ref_test"].min() < 0.0          # test leaves the training range
    assert 0.0 < gold["ref_test_labels"].mean() < 1.0


def test_the_restatement_follows_the_reference_on_the_nan_pair(gold):
    down = int(gold["down"])
    assert 0.02 < np.isnan(gold["train_nan"]).mean() < 0.04 and np.isnan(gold["test_nan"][:, 5]).all()
    tab = ref.table(ref.stats(gold["train_nan"]))
    assert np.array_equal(tab.view(np.int64), gold["ref_table_nan"].view(np.int64))
    for name in ("train", "test"):
        raw = gold[name + "_nan"]
        got, lab, filled = ref.series(raw, tab, down, fill=ref.stats(raw)[:, 2], labels=gold[name + "_labels"])
        assert filled.any() and not filled.all()
        ref.assert_filled_rule(got, gold["ref_" + name + "_nan"].T, filled)
        assert np.array_equal(lab, gold["ref_" + name + "_labels_nan"])
    # without a fill a missing reading leaves its group: the all-NaN sensor and the all-NaN group are NaN, only they
    got, _, _ = ref.series(gold["test_nan"], tab, down)
    want_nan = np.zeros_like(got, dtype=bool)
    want_nan[5, :] = True
    want_nan[2, 3] = True
    assert np.array_equal(np.isnan(got), want_nan)


def test_nan_median_of_every_count():
    v = np.array([5.0, 1.0, 4.0, 2.0, 3.0, 9.0])
    for c in range(1, 7):
        assert ref._median(v[:c]) == np.median(v[:c])
    assert np.isnan(ref._median(v[:0]))


@pytest.mark.parametrize("down", [1, 2, 10])
@pytest.mark.parametrize("chunk", [1, 4])
def test_raw_push_plan_equals_the_brute_force_simulation(down, chunk):
    from gdn_amd.harness import raw_push_plan
    for pending in range(down):
        for r in range(1, 46):
            plan = raw_push_plan(pending, r, down, chunk)
            assert plan == ref.raw_pushes(pending, r, down, chunk), (pending, r)
            at = pending
            for rows, groups, left, replayable in plan:
                assert rows >= 1 and groups <= chunk and groups * down + left == at + rows and 0 <= left < down
                assert replayable == (at == 0 and rows == chunk * down)
                at = left
            assert sum(p[0] for p in plan) == r and sum(p[1] for p in plan) == (pending + r) // down
            assert plan[-1][2] == (pending + r) % down
    assert raw_push_plan(0, 0, down, chunk) == []
    with pytest.raises(ValueError, match="pending"):
        raw_push_plan(down, 1, down, chunk)


def test_prep_save_load_round_trip(tmp_path, gold):
    from gdn_amd import Prep
    from gdn_amd.prep import table_from_stats
    st = torch.from_numpy(ref.stats(gold["train"]))
    tab = table_from_stats(st)
    assert np.array_equal(tab.numpy().view(np.int64), gold["ref_table"].view(np.int64))
    names = [f" S{i}".strip() for i in range(7)]
    p = Prep(tab, st, 10, names)
    path = str(tmp_path / "prep.npz")
    p.save(path)
    q = Prep.load(path, "cpu")
    assert q.down == 10 and q.n == 7 and q.names == names
    assert torch.equal(q.table, tab) and torch.equal(q.stats, st)
    assert q.table.dtype == torch.float64 and sorted(np.load(path).files) == ["down", "names", "stats", "table"]
    with pytest.raises(ValueError, match="7 sensors"):
        Prep(tab, st, 10, names[:3])


def test_refusals_by_name(gold):
    from gdn_amd import Prep, _lib as binding
    from gdn_amd import main as cli
    from gdn_amd.prep import table_from_stats
    st = torch.from_numpy(ref.stats(gold["train"]))
    for down in (0, 65):
        with pytest.raises(ValueError, match=f"down = {down}"):
            Prep(table_from_stats(st), st, down)
    p = Prep(table_from_stats(st), st, 10)
    with pytest.raises(ValueError, match=r"t_raw = 9 .* down = 10"):
        p.series(torch.zeros((9, 7), dtype=torch.float64))
    with pytest.raises(ValueError, match="fill = 'median'"):
        p.series(torch.zeros((20, 7), dtype=torch.float64), fill="median")
    with pytest.raises(ValueError, match="-stream_raw needs -prep"):
        cli.check_stream_raw(True, True, False)
    with pytest.raises(ValueError, match="-stream_raw needs -stream"):
        cli.check_stream_raw(True, False, True)
    with pytest.raises(ValueError, match="-stream_raw needs -prep"):
        cli.from_args(["-stream", "4", "-stream_raw", "raw.csv"])
    cli.check_stream_raw(False, False, False)
    # the library decides before any launch (no device is touched here)
    lib = binding.load()
    for down in (0, 65):
        assert lib.gdn_prep_series(FAKE, 100, 7, 0, FAKE, None, down, None, FAKE, None, None) == GDN_ERR_UNSUPPORTED
        assert lib.gdn_prep_ticks(FAKE, 5, 0, FAKE, 0, 2 * FAKE, 7, down, FAKE, FAKE, 4, None) == GDN_ERR_UNSUPPORTED
    for n in (0, 4097):
        assert lib.gdn_prep_stats(FAKE, 100, n, 1, FAKE, FAKE, None) == GDN_ERR_UNSUPPORTED
        assert lib.gdn_prep_series(FAKE, 100, n, 0, FAKE, None, 10, None, FAKE, None, None) == GDN_ERR_UNSUPPORTED
        assert lib.gdn_prep_stats_workspace_bytes(100, n) == 0
    assert lib.gdn_prep_series(FAKE, 9, 7, 0, FAKE, None, 10, None, FAKE, None, None) == GDN_ERR_ARG
    assert lib.gdn_prep_series(FAKE, 100, 7, 0, FAKE, None, 10, None, FAKE, FAKE, None) == GDN_ERR_ARG
    assert lib.gdn_prep_ticks(FAKE, 45, 0, FAKE, 0, 2 * FAKE, 7, 10, FAKE, FAKE, 3, None) == GDN_ERR_ARG   # 4 groups > c
    assert lib.gdn_prep_ticks(FAKE, 5, 0, FAKE, 10, 2 * FAKE, 7, 10, FAKE, FAKE, 4, None) == GDN_ERR_ARG   # pending
    assert lib.gdn_prep_ticks(FAKE, 5, 0, FAKE, 0, FAKE, 7, 10, FAKE, FAKE, 4, None) == GDN_ERR_ARG        # one plane
    assert lib.gdn_prep_stats_workspace_bytes(403, 7) > 0 and lib.gdn_prep_stats_workspace_bytes(403, 7) % 32 == 0


def test_the_symbols_are_declared_bound_and_exported_and_the_abi_stays():
    from gdn_amd import _lib as binding
    header = open(os.path.join(ROOT, "include", "gdn_hip.h")).read()
    declared = dict((name, ret) for ret, name in re.findall(r"^(int|long long)\s+(gdn_\w+)\s*\(", header, flags=re.M))
    lib = binding.load()
    for name, ret in NEW.items():
        assert declared.get(name) == ret and name in binding.SIGNATURES, name
        fn = getattr(lib, name)                      # AttributeError: the symbol is missing
        assert fn.argtypes == binding.SIGNATURES[name]
        assert fn.restype is (ctypes.c_longlong if ret == "long long" else ctypes.c_int)
        params = re.search(name + r"\s*\(([^)]*)\)\s*;", header).group(1)
        assert len(params.split(",")) == len(binding.SIGNATURES[name]), name
    assert "#define GDN_ABI_VERSION 23" in header and binding.ABI_VERSION == 23 and lib.gdn_abi_version() == 23
    from gdn_amd import ops
    assert all(callable(getattr(ops, f)) for f in ("prep_stats", "prep_series", "prep_ticks"))
