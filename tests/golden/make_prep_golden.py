"""Generates tests/golden/prep_ref.npz.  RUNS ONLY WHERE THE REFERENCE IS AT HAND (needs pandas and sklearn).

It imports `norm` and `downsample` from the reference's own, unmodified scripts/process_swat.py BY PATH and runs them
on seeded raw data; the file holds the raw inputs and what the reference's functions returned (float64), nothing of
the reference's text.  Two pairs of (train [403, 7], test [257, 7]) raw files:
  finite pair   sensors on different engineering-unit scales, sensor 3 constant in train, test values outside the
                training range; labels 0/1 with attack runs that straddle group boundaries.
  NaN pair      the same with about 3 % NaN, sensor 5 ALL NaN in test; it goes through the scripts'
                fillna(mean).fillna(0) (pandas) before norm / downsample, as process_swat.main does.
"""
import importlib.util
import os

import numpy as np
import pandas as pd

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
DOWN = 10


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _raw(rng, t, shift):
    scales = np.array([1.0, 250.0, 0.003, 1.0, 1e4, 37.5, 2.0])
    offsets = np.array([0.0, -40.0, 1.5, 7.25, 3e5, 0.0, -1.0])
    walk = np.cumsum(rng.standard_normal((t, 7)) * 0.05, axis=0) + rng.standard_normal((t, 7)) * 0.3
    x = (walk + shift) * scales + offsets
    x[:, 3] = 7.25 if shift == 0.0 else x[:, 3]                     # constant in train, moving in test
    return np.ascontiguousarray(x)


def _pipeline(ps, train, test, train_lab, test_lab):
    """process_swat.main from the fillna on, on arrays."""
    tr, te = pd.DataFrame(train), pd.DataFrame(test)
    tr = tr.fillna(tr.mean()).fillna(0)
    te = te.fillna(te.mean()).fillna(0)
    x_train, x_test = ps.norm(tr.values, te.values)
    d_train, l_train = ps.downsample(x_train, train_lab, DOWN)
    d_test, l_test = ps.downsample(x_test, test_lab, DOWN)
    from sklearn.preprocessing import MinMaxScaler
    sc = MinMaxScaler(feature_range=(0, 1)).fit(tr.values)
    return (np.array(d_train, dtype=np.float64), np.array(l_train, dtype=np.float64),
            np.array(d_test, dtype=np.float64), np.array(l_test, dtype=np.float64),
            np.stack([sc.scale_, sc.min_], axis=1).astype(np.float64))


def main():
    ps = _load(os.path.join(REF, "scripts", "process_swat.py"), "ref_process_swat")
    rng = np.random.default_rng(20240)
    train, test = _raw(rng, 403, 0.0), _raw(rng, 257, 0.6)
    train_lab = np.zeros(403)
    test_lab = np.zeros(257)
    for a, b in ((17, 43), (95, 96), (120, 131), (249, 257)):
        test_lab[a:b] = 1.0
    out = {"down": np.int64(DOWN), "train": train, "test": test, "train_labels": train_lab, "test_labels": test_lab}
    keys = ("ref_train", "ref_train_labels", "ref_test", "ref_test_labels", "ref_table")
    out.update(zip(keys, _pipeline(ps, train, test, train_lab, test_lab)))
    train_nan, test_nan = train.copy(), test.copy()
    train_nan[rng.random(train.shape) < 0.03] = np.nan
    test_nan[rng.random(test.shape) < 0.03] = np.nan
    test_nan[:, 5] = np.nan
    test_nan[30:40, 2] = np.nan                                     # one whole group of one sensor
    out.update(train_nan=train_nan, test_nan=test_nan)
    out.update(zip((k + "_nan" for k in keys), _pipeline(ps, train_nan, test_nan, train_lab, test_lab)))
    np.savez_compressed(os.path.join(HERE, "prep_ref.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
