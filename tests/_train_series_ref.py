"""Yardsticks of the train-series tests (tests/test_cpu_train_series.py pins them, tests/test_gpu_train_series.py
uses them): numpy restatements of gdn_mse_batch_means and of SeriesWindows.batch's indexing."""
import numpy as np


def mse_batch_means(pred, y, batch):
    """(batch_means float64 [ceil(rows / batch)], mean float64): per logical minibatch (the last one ragged) the mean
    of the squared fp32 differences, accumulated in float64; then the plain average of the means."""
    pred, y = np.asarray(pred, dtype=np.float32), np.asarray(y, dtype=np.float32)
    means = []
    for s in range(0, pred.shape[0], batch):
        diff = (pred[s:s + batch] - y[s:s + batch]).astype(np.float32)      # the difference is formed in fp32
        means.append(np.mean(diff.astype(np.float64) ** 2))
    means = np.asarray(means, dtype=np.float64)
    return means, float(means.sum() / len(means))


def windows(series, ticks, w):
    """(x [B, n, w], y [B, n]) of target ticks `ticks` of a series [n, T]: datasets/TimeDataset.py's windows."""
    series, ticks = np.asarray(series), np.asarray(ticks, dtype=np.int64)
    cols = ticks[:, None] + np.arange(-w, 0)[None, :]
    return np.ascontiguousarray(series[:, cols].transpose(1, 0, 2)), np.ascontiguousarray(series[:, ticks].T)
