"""What tests/test_gpu_fleet_prep.py, tests/test_gpu_fleet_checkpoint.py and tests/_fleet_checkpoint_worker.py share:
the small model (n = 70, w = 5, d = 16), a fleet of U = 3 units with tables, thresholds and histories of their own, a
Prep with down = 4, and the list of everything a fleet remembers.  The same seeds give the same model, tables and ticks
in every process."""
import copy
import functools

import torch

from test_gpu_forward_parity import random_params

SHAPE = (70, 5, 6, 16, 1, 32)            # n, w, k, d, out layers, inter
MSL = (27, 15, 20, 64, 1, 32)            # a shape the resident-series evaluator (from_calibration) has a kernel for
N, W = SHAPE[:2]
UNITS, CHUNK, DOWN, TOP_M, LOG = 3, 4, 4, 3, 6


def bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a.contiguous()), bits(b.contiguous()))


def gen(*seed):
    return torch.Generator().manual_seed(sum((j + 1) * 1009 * int(s) for j, s in enumerate(seed)) + 5)


@functools.lru_cache(maxsize=None)
def _cpu_model(shape):
    return random_params(*shape[:4], seed=shape[0] + shape[1], out_layer_num=shape[4], inter=shape[5])


def model_on(dev, shape=SHAPE):
    return copy.deepcopy(_cpu_model(shape)).to(dev).eval()


def tables(dev, g, units=UNITS, n=N):
    med = torch.rand((units, n), generator=g, dtype=torch.float64) * 0.1
    iqr = torch.rand((units, n), generator=g, dtype=torch.float64) * 0.2 + 0.05
    return torch.stack([med, iqr], dim=2).contiguous().to(dev)


def setup(dev, seed=1, shape=SHAPE):
    """(model, med_iqr [U, n, 2], threshold [U] host float64, history [U, n, w + 2]) of the fleet of every test."""
    g = gen(seed)
    n, w = shape[:2]
    history = torch.rand((UNITS, n, w + 2), generator=g).to(dev)
    return model_on(dev, shape), tables(dev, g, n=n), torch.tensor([0.5, 1.0, 1.5], dtype=torch.float64), history


def raw_ticks(g, r, dtype, dev, units=UNITS, n=N):
    """Raw ticks [U, r, n] in engineering units: sensor i reads 50 + 10 i .. 150 + 10 i."""
    base = 50.0 + 10.0 * torch.arange(n, dtype=torch.float64)
    return (torch.rand((units, r, n), generator=g, dtype=torch.float64) * 100.0 + base).to(dtype).to(dev)


def make_prep(dev, down=DOWN, n=N):
    """The min-max table of those ranges, stated directly (scale = 1 / 100, offset = -(50 + 10 i) / 100)."""
    from gdn_amd.prep import Prep
    lo = 50.0 + 10.0 * torch.arange(n, dtype=torch.float64)
    scale = torch.full((n,), 1.0 / 100.0, dtype=torch.float64)
    stats = torch.stack([lo, lo + 100.0, lo + 50.0, torch.full((n,), 1000.0, dtype=torch.float64)], dim=1)
    return Prep(torch.stack([scale, 0.0 - lo * scale], dim=1).to(dev), stats.to(dev), down)


def memory(fleet):
    """Everything a fleet remembers between pushes, by name: what a save must carry and a contract must equal."""
    from gdn_amd import ops
    out = {"state": fleet.state, "med_iqr": fleet.med_iqr, "threshold": fleet.threshold}
    for name in ("log_ticks", "log_sensors", "gaps", "ring_keys", "ring_keep", "recal_kept", "recal_counts", "events",
                 "clear", "calib_counts"):
        t = getattr(fleet, name, None)
        if t is not None:
            out[name] = t
    if getattr(fleet, "prep", None) is not None:
        ticks, pending = ops.fleet_prep_views(fleet.pend, fleet.units, fleet.n, fleet.prep.down)
        out["pending"] = pending
        # (rows of the open group only: the rest of a unit's plane is whatever an earlier group left)
        for u, p in enumerate(pending[:, 0].tolist()):
            out[f"pending_ticks{u}"] = ticks[u, :p]
    return {k: v.clone() for k, v in out.items()}


def assert_same_memory(a, b, skip=()):
    assert sorted(set(a) - set(skip)) == sorted(set(b) - set(skip))
    for k in a:
        if k not in skip:
            assert same(a[k], b[k]), k
