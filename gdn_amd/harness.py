"""Callers of the hot path, mirroring the reference's loops:

  test()            <- test.py:21-79   (eval loop: forward per batch, MSE, concatenated outputs)
  train()           <- train.py:27-112 (Adam lr 1e-3, MSE, per-epoch validation, best checkpoint,
                                        early stop after 15 epochs without improvement)
  SeriesEvaluator   the throughput form of test() + evaluate.get_full_err_scores for a series
                    that is already resident in HBM: forward launches write straight into one
                    [T, N] prediction buffer, scoring runs on device, the whole step can be
                    captured in a HIP graph and replayed.
  shard / DDP       one process per GPU: windows are independent, so a series is split into
                    contiguous shards (no collective in the forward); scoring needs per-sensor
                    order statistics over ALL ticks -> one all-to-all by sensor + one all-gather
                    of the [N,2] median/IQR table; training all-reduces one flat gradient bucket.
"""
from __future__ import annotations

import contextlib
import ctypes
import gc
import os
import warnings
from typing import NamedTuple

import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
# the checkpoint layer of StreamDetector and StreamFleet, under the names it always had here
from .checkpoint import (FLEET_CHECKPOINT_FORMAT, STREAM_CHECKPOINT_FORMAT,  # noqa: F401
                         _CKPT_CONFIG, _CKPT_INTS, _CKPT_STRS, _EVENTS_FIELDS, _FLEET_CKPT, _FLEET_CKPT_CONFIG,
                         _FLEET_CKPT_INTS, _FLEET_CKPT_STRS, _UNIT_CONFIG, _check_recal_threshold, _checkpoint_expect,
                         _ckpt_format, _ckpt_int, _ckpt_str, _fingerprint, _fleet_ckpt_format, _host_copies,
                         checkpoint_recal_threshold, events_bytes, fleet_checkpoint_check, fleet_checkpoint_config,
                         fleet_checkpoint_events, fleet_unit_to_stream, model_fingerprint, prep_units,
                         read_stream_checkpoint, stream_calib_bytes, stream_checkpoint_check,
                         stream_checkpoint_config, stream_checkpoint_events, stream_to_fleet_unit,
                         write_stream_checkpoint)


# --------------------------------------------------------------------------- eval loop

@contextlib.contextmanager
def capture(graph, pool=None):
    """`torch.cuda.graph(graph)` with the cyclic garbage collector out of the way.  torch 2.10 no longer collects
    on entry, and a collection that fires INSIDE the captured region can finalise an older `CUDAGraph` or free a
    cached block of a dead graph pool — HIP calls that are illegal while a stream is capturing; the error is
    raised from a destructor and ends the process (seen once in the GPU suite: `Fatal Python error: Aborted` under
    `Garbage-collecting`).  So: collect before, keep the collector disabled until the capture has ended."""
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph, pool=pool):
            yield
    finally:
        if was_enabled:
            gc.enable()


class _Replay:
    """One launch sequence, captured once in a HIP graph and replayed from then on: the ONE copy of that rule.

    `launch(*args())` issues it with static arguments only; `args` is asked once per capture, outside it, for the eager
    run and the captured one alike.  `key()` names what the captured pointers depend on (`model._constants().key`:
    asking builds the constants outside the capture); every holder remembers its own.  `on_stale()` runs when the key
    CHANGED since the last capture, never at the first.  `graph`: the `CUDAGraph`, None while nothing is captured.

    A call without `use_graph` (and with nothing captured) launches eagerly and touches no `torch.cuda`.  A live graph
    under a fresh key is replayed.  Otherwise the old graph is released FIRST (outside any capture; the holder has the
    only reference), the sequence is launched eagerly AND THAT LAUNCH IS THE RUN (a detector's state may move only
    once; it is also the warm-up: occupancy queries, lazy buffers), then synchronize and capture the same call, which
    executes nothing.  A call returns what `launch` returned: a replay, the value recorded at the capture."""

    def __init__(self, launch, use_graph: bool = True, key=lambda: None, on_stale=None, args=tuple):
        self.launch, self.use_graph, self.key, self.on_stale, self.args = launch, bool(use_graph), key, on_stale, args
        self.graph = self._key = self._value = None

    def drop(self):
        """Release the graph (outside any capture); the next call captures again."""
        self.graph = self._value = None

    def capture(self, args=None):
        """Capture now, with no eager run: for a caller whose eager run has happened and who knows that nothing else (a
        collective above all) is in flight.  Calls replay from here on, whatever `use_graph` says."""
        self.drop()
        args = self.args() if args is None else args
        graph = torch.cuda.CUDAGraph()
        with capture(graph):
            self._value = self.launch(*args)
        self.graph = graph

    def __call__(self):
        if self.graph is None and not self.use_graph:
            return self.launch(*self.args())
        key = self.key()
        if self.graph is not None and key == self._key:
            self.graph.replay()
            return self._value
        self.drop()
        if self.on_stale is not None and self._key not in (None, key):
            self.on_stale()
        self._key = key
        args = self.args()
        value = self.launch(*args)
        torch.cuda.synchronize()
        self.capture(args)
        return value


def test(model, dataloader, device=None, as_tensors: bool = False):
    """Mirror of the reference test() (test.py:21-79).  Returns (avg_loss, [predictions, ground
    truth, labels]) with the three results as python lists, exactly like the reference; per-batch
    losses stay on the device and are read once at the end (the reference syncs every batch).
    `as_tensors=True` keeps the three results as device tensors [T, N] (gdn_amd.evaluate accepts
    them directly): the `.tolist()` of the reference costs seconds at T = 10^5 windows."""
    device = device or next(model.parameters()).device
    model.eval()
    preds, gts, labs, losses = [], [], [], []
    for x, y, labels, edge_index in dataloader:
        x, y, labels = [item.to(device).float() for item in (x, y, labels)]
        with torch.no_grad():
            predicted = model(x, edge_index)
            losses.append(F.mse_loss(predicted, y, reduction="mean"))
            preds.append(predicted)
            gts.append(y)
            labs.append(labels.unsqueeze(1).repeat(1, predicted.shape[1]))
    avg_loss = float(torch.stack(losses).double().sum().item() / len(losses)) if losses else 0.0
    if not preds:
        return avg_loss, [[], [], []]
    out = [torch.cat(preds), torch.cat(gts), torch.cat(labs)]
    return avg_loss, (out if as_tensors else [t.tolist() for t in out])


def train(model=None, save_path="", config=None, train_dataloader=None, val_dataloader=None, use_graph=False,
          **_ignored):
    """Mirror of the reference train() (train.py:27-112): same optimizer, loss, checkpoint and
    early-stop rule.  Returns the list of per-step losses.

    `use_graph=True` (or config["hip_graph"]) runs every full-size minibatch as one replay of a
    `GraphedTrainStep` (captured at the first batch's size) and the ragged last batch of an epoch
    eagerly with the same optimizer; losses stay on the device until the epoch ends (the
    reference syncs with `.item()` every step)."""
    config = config or {}
    use_graph = use_graph or bool(config.get("hip_graph", False))
    device = next(model.parameters()).device
    graphed = None
    if not use_graph:
        optimizer = torch.optim.Adam(model.parameters(), lr=0.001, weight_decay=config.get("decay", 0))
    losses, best = [], _BestSoFar()
    # Range of the training inputs (include/gdn_hip.h "range guard"): decided ONCE — config["wide"] when the caller
    # knows (python -m gdn_amd.main looks at its resident series), else from the first batch — and pinned on the
    # model for every training step of the run: no per-step host check, and the captured step needs the answer before
    # the capture.  A range the caller has set is left alone; validation data gets its own range (eval guard)
    auto = getattr(model, "operand_range", "auto") == "auto"
    wide = config.get("wide", None)
    for _epoch in range(config.get("epoch", 1)):
        model.train()
        epoch_losses = []
        for x, labels, _attack, edge_index in train_dataloader:
            x, labels = x.float().to(device), labels.float().to(device)
            if wide is None and auto:
                wide = model.input_exceeds_limit(x, margin=16.0)      # (the weights move during training)
            with pinned_range(model, wide) if auto else contextlib.nullcontext():
                if use_graph and graphed is None:
                    graphed = GraphedTrainStep(model, x.shape[0], lr=0.001, weight_decay=config.get("decay", 0),
                                               wide=model.operand_range == "wide")
                    optimizer = graphed.optimizer
                if graphed is not None and x.shape[0] == graphed.x.shape[0]:
                    graphed.x.copy_(x)
                    graphed.y.copy_(labels)
                    epoch_losses.append(graphed.step().clone())
                else:
                    epoch_losses.append(_eager_step(model, optimizer, x, labels, edge_index))
        step_losses = torch.stack(epoch_losses).tolist() if epoch_losses else []
        losses.extend(step_losses)
        val_loss = test(model, val_dataloader, device)[0] if val_dataloader is not None else None
        if best.update(val_loss, float(sum(step_losses)), model, save_path):
            break
    return losses


@contextlib.contextmanager
def pinned_range(model, wide):
    """`model.operand_range` set to "wide" / "narrow" for the block — the caller has looked at its data, so nothing
    inside (a captured step above all) runs a host check — and back to what it was afterwards, exceptions included."""
    before = getattr(model, "operand_range", "auto")
    model.operand_range = "wide" if wide else "narrow"
    try:
        yield
    finally:
        model.operand_range = before


def _eager_step(model, optimizer, x, y, edge_index=None):
    """One optimisation step of the reference's train() (train.py:52-66) through autograd; returns the detached loss."""
    optimizer.zero_grad()
    loss = F.mse_loss(model(x, edge_index), y, reduction="mean")
    loss.backward()
    sync_gradients(model)
    optimizer.step()
    return loss.detach()


class _BestSoFar:
    """The reference's checkpoint and early-stop rule (train.py:89-108), one epoch per `update`.  With a validation
    loss: save on a strictly better one, stop after 15 epochs without.  Without: save on a better summed training
    loss, never stop."""

    def __init__(self):
        self.min_loss, self.stale = 1e8, 0

    def update(self, val_loss, summed_loss, model, save_path) -> bool:
        loss = summed_loss if val_loss is None else val_loss
        if loss < self.min_loss:
            if save_path:
                torch.save(model.state_dict(), save_path)
            self.min_loss, self.stale = loss, 0
        elif val_loss is not None:
            self.stale += 1
        return self.stale >= 15


# --------------------------------------------------------------------------- sharding / DDP
def world():
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def shard_range(total: int, rank: int, world_size: int):
    """Contiguous, balanced split of `total` windows: the first (total % world) ranks get one extra."""
    base, extra = divmod(total, world_size)
    start = rank * base + min(rank, extra)
    return start, start + base + (1 if rank < extra else 0)


def sensor_range(n: int, rank: int, world_size: int):
    return shard_range(n, rank, world_size)


def pack_gradients(model, flat: torch.Tensor | None = None) -> torch.Tensor:
    """All gradients in ONE flat fp32 bucket (9 729 values = 38 KiB at the SWaT shape), written into
    `flat` when given (a static buffer for HIP-graph capture)."""
    grads = [p.grad.reshape(-1) for p in model.parameters() if p.grad is not None]
    if flat is None:
        return torch.cat(grads)
    torch.cat(grads, out=flat)
    return flat


def unpack_gradients(model, flat: torch.Tensor, world_size: int) -> None:
    """Averaged bucket back into the parameters' gradients: one scale, one multi-tensor copy."""
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    if world_size > 1:
        flat.div_(world_size)
    views, off = [], 0
    for g in grads:
        views.append(flat[off:off + g.numel()].view_as(g))
        off += g.numel()
    torch._foreach_copy_(grads, views)


def sync_gradients(model, group=None) -> None:
    """Data-parallel gradient averaging: pack, one all-reduce (RCCL over xGMI on GPUs; latency bound
    at this size), unpack.  No-op in a single process."""
    _rank, size = world()
    if size == 1 or not any(p.grad is not None for p in model.parameters()):
        return
    flat = pack_gradients(model)
    dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
    unpack_gradients(model, flat, size)


def broadcast_parameters(model, src: int = 0) -> None:
    _rank, size = world()
    if size == 1:
        return
    for t in list(model.parameters()) + list(model.buffers()):
        dist.broadcast(t.data, src=src)


KEY_SLICE = 2048    # the select kernel's slice: exchanged key rows are padded to a multiple of it


class HipScoreBackend:
    """Per-rank compute of the distributed scoring; tests inject an oracle-backed stand-in to
    exercise the exchange logic on CPU (gloo)."""

    @staticmethod
    def keys(pred_tn, gt_tn, pitch, out=None):
        return ops.score_keys(pred_tn, gt_tn, pitch, out=out)

    @staticmethod
    def select(keys_flat, blocks, n, pitch, total, ws=None, out=None):
        return ops.score_select(keys_flat, blocks, n, pitch, total, ws=ws, out=out)

    @staticmethod
    def select_workspace(blocks, n, pitch, device):
        return ops.score_select_workspace(blocks, n, pitch, device)

    @staticmethod
    def smooth_max(pred_tn, gt_tn, med_iqr, first_tick, halo_pred, halo_gt, anomaly=None):
        return ops.score_smooth_max(pred_tn, gt_tn, med_iqr, want_scores=False, first_tick=first_tick,
                                    halo_pred=halo_pred, halo_gt=halo_gt, anomaly=anomaly)[1]


def distributed_anomaly(pred_local, gt_local, total_ticks: int, backend=HipScoreBackend, group=None,
                        rehearse: bool = False):
    """Anomaly score of a series whose ticks are sharded contiguously over the ranks.

    Step 1  every rank turns ITS ticks into radix keys |pred-gt| (float64), already transposed to
            [sensor, tick] and padded to a common pitch, so the rows of the sensors rank r owns are one
            contiguous chunk: `all_to_all_single` sends them with no packing, and rank r selects
            median / IQR of its sensors straight over the received [rank, sensor, pitch] blocks
            (padding is a filler the select ignores) — no unpacking either.
    Step 2  all-gather of the per-sensor [median, IQR] rows -> every rank has the [N,2] table.
    Step 3  each rank normalises / smooths / maxes its own ticks; the 3-tick halo before its first
            tick comes from its predecessors (all-gather of every rank's last <=3 rows).
    Returns anomaly[local ticks] (float64).  Single process: plain local scoring."""
    rank, size = world()
    t_local, n = pred_local.shape
    if size == 1 and not (rehearse and dist.is_initialized()):
        keys = backend.keys(pred_local, gt_local, t_local)
        med_iqr = backend.select(keys, 1, n, t_local, t_local)
        return backend.smooth_max(pred_local, gt_local, med_iqr, 0, None, None)
    # (rehearse: run the full exchange with a 1-rank process group — exercises the RCCL calls on a
    # one-GPU box)
    dev = pred_local.device
    bounds = [shard_range(total_ticks, r, size) for r in range(size)]
    sens = [sensor_range(n, r, size) for r in range(size)]
    s0, s1 = sens[rank]
    n_mine = s1 - s0
    # ---- step 1
    longest = max(e - s for s, e in bounds)
    pitch = max(KEY_SLICE, (longest + KEY_SLICE - 1) // KEY_SLICE * KEY_SLICE)
    if t_local > 0:
        send = backend.keys(pred_local, gt_local, pitch)                 # [n, pitch], rows grouped by owner
    else:
        send = torch.full((n, pitch), -1, dtype=torch.int64, device=dev).view(torch.float64)   # all filler
    in_sizes = [(b - a) * pitch for a, b in sens]
    out_sizes = [n_mine * pitch] * size
    recv = torch.empty((size * n_mine * pitch,), dtype=torch.float64, device=dev)
    dist.all_to_all_single(recv, send.reshape(-1), out_sizes, in_sizes, group=group)
    if n_mine:
        my_mi = backend.select(recv, size, n_mine, pitch, total_ticks).to(torch.float64)
    else:
        my_mi = torch.empty((0, 2), dtype=torch.float64, device=dev)
    # ---- steps 2+3 in ONE all-gather: every rank publishes [its median/IQR rows (padded to the
    # largest sensor share) | its last <=3 (pred, gt) rows, right-aligned, as float64 (lossless)].
    # The halo = the 3 ticks before my first one; a shard shorter than 3 ticks makes it span several
    # predecessors.
    cap = max(b - a for a, b in sens)
    pub = torch.zeros((cap * 2 + 6 * n,), dtype=torch.float64, device=dev)
    pub[: n_mine * 2] = my_mi.reshape(-1)
    take = min(3, t_local)
    if take:
        tail = pub[cap * 2:].view(2, 3, n)
        tail[0, 3 - take:] = pred_local[t_local - take:]
        tail[1, 3 - take:] = gt_local[t_local - take:]
    gathered = [torch.empty_like(pub) for _ in range(size)]
    dist.all_gather(gathered, pub, group=group)
    med_iqr = torch.cat([g[: (b - a) * 2].view(-1, 2) for g, (a, b) in zip(gathered, sens)]).contiguous()
    first_tick = bounds[rank][0]
    halo_p = halo_g = None
    if first_tick > 0:
        rows = [torch.zeros((2, 3, n), dtype=torch.float64, device=dev)]      # ticks "before 0": never read
        for r in range(rank):
            have = min(3, bounds[r][1] - bounds[r][0])
            if have:
                rows.append(gathered[r][cap * 2:].view(2, 3, n)[:, 3 - have:])
        prev = torch.cat(rows, dim=1)[:, -3:].to(pred_local.dtype)
        halo_p, halo_g = prev[0].contiguous(), prev[1].contiguous()
    if t_local == 0:
        return torch.empty((0,), dtype=torch.float64, device=dev)
    return backend.smooth_max(pred_local, gt_local, med_iqr, first_tick, halo_p, halo_g)


class ShardedEvaluator:
    """The multi-rank eval step with its one real exchange hidden behind the forward.

    Same arithmetic as `SeriesEvaluator.forward_only()` + `distributed_anomaly()`, reorganised for one
    process per GPU over xGMI:
      * the local shard runs in chunks of `chunk` ticks; as soon as a chunk's predictions exist its
        radix keys (already transposed to [sensor, tick], rows grouped by owning rank) leave in an
        ASYNC `all_to_all_single`, so the transfers (N*T*8 bytes per rank in total) overlap the
        forward of the following chunks; only the last chunk's transfer is exposed;
      * the receive side is one [chunk, rank, my sensors, pitch] buffer = `chunks*ranks` row blocks of
        the blocked radix select — no packing or unpacking on either side;
      * every buffer, and the index tables that pick the median/IQR rows and the 3-tick halo out of the
        ONE all-gather that follows, are built once: a step issues no allocation-heavy torch code.
    `forward(start, stop)` must fill `self.pred[start:stop]`; the default runs the fused HIP forward."""

    def __init__(self, model, x_local, y_local: torch.Tensor, total_ticks: int, chunk: int = 4096,
                 backend=HipScoreBackend, forward=None, group=None, use_graph: bool = False):
        self.rank, self.size = world()
        self.use_graph, self._warm = bool(use_graph), False
        self.group, self.backend, self.model = group, backend, model
        self.x, self.y, self.total = x_local, y_local, total_ticks
        self.t, self.n = y_local.shape
        dev = y_local.device
        size, n = self.size, self.n
        self.bounds = [shard_range(total_ticks, r, size) for r in range(size)]
        if self.bounds[self.rank][1] - self.bounds[self.rank][0] != self.t:
            raise ValueError("y_local does not have this rank's share of the ticks (harness.shard_range)")
        self.sens = [sensor_range(n, r, size) for r in range(size)]
        s0, s1 = self.sens[self.rank]
        self.n_mine = s1 - s0
        longest = max(e - s for s, e in self.bounds)
        # every rank must agree on chunk count and pitch: both follow from the LONGEST shard
        self.pitch = max(KEY_SLICE, (min(chunk, longest) + KEY_SLICE - 1) // KEY_SLICE * KEY_SLICE)
        self.nchunks = max(1, (longest + self.pitch - 1) // self.pitch)
        self.pred = torch.empty((self.t, n), dtype=torch.float32, device=dev)
        filler = torch.full((self.nchunks, n, self.pitch), -1, dtype=torch.int64, device=dev)
        self.send = filler.view(torch.float64)          # chunks this rank has no ticks for stay all filler
        self.recv = torch.empty((self.nchunks, size, self.n_mine, self.pitch), dtype=torch.float64, device=dev)
        self.in_sizes = [(b - a) * self.pitch for a, b in self.sens]
        self.out_sizes = [self.n_mine * self.pitch] * size
        # published row: [my median/IQR rows, padded to the largest share | last 3 (pred, y) rows, right aligned]
        self.cap = max(b - a for a, b in self.sens)
        self.row = self.cap * 2 + 6 * n
        self.pub = torch.zeros((self.row,), dtype=torch.float64, device=dev)
        self.take = min(3, self.t)
        if self.take:
            self.pub[self.cap * 2:].view(2, 3, n)[1, 3 - self.take:] = y_local[self.t - self.take:].double()
        self.gathered = torch.empty((size * self.row,), dtype=torch.float64, device=dev)
        mi_idx = [r * self.row + (s - a) * 2 + h for r, (a, b) in enumerate(self.sens) for s in range(a, b)
                  for h in (0, 1)]
        self.mi_idx = torch.tensor(mi_idx, dtype=torch.int64, device=dev)
        # the 3 ticks before my first one, newest last; a shard shorter than 3 ticks makes them span ranks
        self.first_tick = self.bounds[self.rank][0]
        src = []                                        # (rank, row in its right-aligned 3-row tail)
        for r in range(self.rank - 1, -1, -1):
            have = min(3, self.bounds[r][1] - self.bounds[r][0])
            src.extend((r, 2 - j) for j in range(have))
            if len(src) >= 3:
                break
        src = (src[:3] + [(0, 0)] * 3)[:3][::-1]        # ticks before tick 0 are never read: any valid index
        halo_idx = [[[r * self.row + self.cap * 2 + which * 3 * n + j * n + c for c in range(n)] for r, j in src]
                    for which in (0, 1)]
        self.halo_idx = torch.tensor(halo_idx, dtype=torch.int64, device=dev)
        self.forward = forward if forward is not None else self._hip_forward
        self._wide = None
        # per-step buffers of the scoring kernels, allocated once (backends without the hooks allocate per call)
        self._sel_ws = self._sel_out = self._anomaly = None
        if hasattr(backend, "select_workspace") and self.n_mine:
            self._sel_ws = backend.select_workspace(self.nchunks * size, self.n_mine, self.pitch, dev)
            self._sel_out = torch.empty((self.n_mine, 2), dtype=torch.float64, device=dev)
        if hasattr(backend, "select_workspace") and self.t:
            self._anomaly = torch.empty((self.t,), dtype=torch.float64, device=dev)
        self._med_iqr = torch.empty((n, 2), dtype=torch.float64, device=dev)
        self._halo64 = torch.empty((2, 3, n), dtype=torch.float64, device=dev)
        self._halo = torch.empty((2, 3, n), dtype=torch.float32, device=dev)
        # the compute segments of a step (below): eager until _capture_segments() has captured them
        self._segs = [_Replay(self._seg_forward, False, args=lambda c=c: (c,)) for c in range(self.nchunks)]
        self._segs += [_Replay(self._seg_select, False), _Replay(self._seg_finish, False)]

    _graphs = property(lambda self: [seg.graph for seg in self._segs] if self._segs[0].graph is not None else None,
                       doc="the segments' graphs; None unless they are captured")

    def _hip_forward(self, start, stop):
        if self._wide is None:      # range of the resident shard, looked at once
            self._wide = self.model.wide_for(self.x)
        self.model.forward_into(self.x[start:stop], self.pred[start:stop], wide=self._wide)

    # A step = nchunks x [forward + keys of the chunk | async all-to-all of its key rows] -> [select of my sensors'
    # median / IQR + my last 3 prediction rows into the published row] -> all-gather -> [median/IQR table, halo,
    # smoothing + max].  The bracketed COMPUTE segments are plain launch sequences with static arguments: with
    # `use_graph` each is captured once in a HIP graph and a step is nchunks + 2 replays and nchunks + 1
    # collectives issued from Python — against ~10 launches per chunk before (a 0.35 ms GPU step does not survive
    # ~100 us of Python per rank).  The collectives themselves stay eager: RCCL inside a captured graph is not
    # something this one-GPU box can vouch for.
    def _seg_forward(self, c):
        a, b = min(self.t, c * self.pitch), min(self.t, (c + 1) * self.pitch)
        if b > a:
            self.forward(a, b)
            self.backend.keys(self.pred[a:b], self.y[a:b], self.pitch, out=self.send[c])

    def _seg_select(self):
        if self.n_mine:
            if self._sel_ws is not None:        # the select writes straight into the row this rank publishes
                self.backend.select(self.recv.reshape(-1), self.nchunks * self.size, self.n_mine, self.pitch, self.total,
                                    ws=self._sel_ws, out=self.pub[: self.n_mine * 2].view(self.n_mine, 2))
            else:
                mi = self.backend.select(self.recv.reshape(-1), self.nchunks * self.size, self.n_mine, self.pitch,
                                         self.total)
                self.pub[: self.n_mine * 2] = mi.reshape(-1)
        if self.take:
            self.pub[self.cap * 2:].view(2, 3, self.n)[0, 3 - self.take:] = self.pred[self.t - self.take:]

    def _seg_finish(self):
        torch.index_select(self.gathered, 0, self.mi_idx, out=self._med_iqr.view(-1))
        halo_p = halo_g = None
        if self.first_tick > 0:
            torch.index_select(self.gathered, 0, self.halo_idx.view(-1), out=self._halo64.view(-1))
            self._halo.copy_(self._halo64)
            halo_p, halo_g = self._halo[0], self._halo[1]
        if self.t == 0:
            return torch.empty((0,), dtype=torch.float64, device=self.pred.device)
        extra = {"anomaly": self._anomaly} if self._anomaly is not None else {}
        return self.backend.smooth_max(self.pred, self.y, self._med_iqr, self.first_tick, halo_p, halo_g, **extra)

    def _capture_segments(self):
        """One eager step has run (plans, constants, RCCL channels are warm): capture the compute segments.  Returns
        False (and stays eager) when anything about the capture fails."""
        try:
            torch.cuda.synchronize()
            for seg in self._segs:
                seg.capture()
            return True
        except Exception as exc:     # noqa: BLE001 — a capture that fails must not take the evaluator down with it
            warnings.warn(f"ShardedEvaluator: HIP-graph capture of the compute segments failed ({exc!r}); running eagerly")
            for seg in self._segs:
                seg.drop()
            torch.cuda.synchronize()
            return False

    def step(self):
        if self.use_graph and self._graphs is None and self._warm:      # at the start of the second step: no
            self.use_graph = self._capture_segments()                   # collective is in flight here
        works = []
        for c in range(self.nchunks):
            self._segs[c]()
            works.append(dist.all_to_all_single(self.recv[c].reshape(-1), self.send[c].reshape(-1),
                                                self.out_sizes, self.in_sizes, group=self.group, async_op=True))
        for w in works:
            w.wait()
        self._segs[self.nchunks]()
        dist.all_gather_into_tensor(self.gathered, self.pub, group=self.group)
        self._warm = True
        return self._segs[self.nchunks + 1]()


# --------------------------------------------------------------------------- resident-series evaluator
def too_few_readings(counts, min_kept: int, t: int) -> str:
    """The refusal of calib="sensor" when a sensor has fewer than `min_kept` real readings: the first 8 such sensors
    and their counts (`counts` [n] on the host)."""
    short = torch.nonzero(counts < min_kept).flatten()[:8].tolist()
    return (f"min_kept = {min_kept}: sensors {short} have only {[int(counts[i]) for i in short]} real readings among "
            f"the {t} scored ticks; too few for their median / IQR rows")


# the checks and the read that SeriesEvaluator and StreamDetector (status_gaps: SeriesTrainer too) have in common
def _check_calib(calib):
    if calib not in ("tick", "sensor"):
        raise ValueError(f"calib = {calib!r}: 'tick' (complete ticks) or 'sensor' (each sensor's own readings)")


def _check_top_m(top_m, n: int):
    if not 1 <= int(top_m) <= min(8, n):
        raise ValueError(f"top_m = {top_m}: the score launch keeps 1 to 8 sensors per tick, at most all {n}")


def _status_gaps(counters, with_gaps: bool, who: str):
    if not with_gaps:
        raise ValueError(f"status_gaps(): the {who} was built with gaps=False and counts no missing readings")
    both = counters.cpu()
    return both[0], both[1]


class SeriesEvaluator:
    """Eval forward + anomaly score over a series of T windows resident in HBM.

    One `step()` = the reference's `test()` over the series in batches of `batch` windows
    (test.py:43-62) followed by `get_full_err_scores` + max over sensors (evaluate.py:6-68,
    :131-139), with nothing leaving the device.  With `use_graph=True` the launches of a step
    are captured once in a HIP graph and replayed."""

    def __init__(self, model, x_all: torch.Tensor | None, y_all: torch.Tensor | None, batch: int,
                 use_graph: bool = True, want_scores: bool = False, streams: int = 3, coalesce: int = 1,
                 series: torch.Tensor | None = None, top_m: int = 0, gaps: bool = False, min_kept: int = 64,
                 calib: str = "tick"):
        """`batch` = the logical minibatch of the reference's loader; `coalesce` consecutive batches
        (contiguous in the resident series) go out as ONE launch — eval results do not depend on the
        minibatch size, and launches of a few thousand windows amortise the per-workgroup prologue.
        `top_m` >= 1 (up to 8): the score launch is gdn_score_smooth_topm — `top_scores` [T, m] float64 and
        `top_sensors` [T, m] int32 hold every tick's m largest sensor scores and their sensors, `anomaly` is column 0
        of `top_scores` (see `localise`).  0: exactly the launches of a plain step.
        `gaps=True` (needs `series=` in fp32, x_all = y_all = None) gives the evaluator the streaming
        detector's notion of a missing reading: a value of the series that is not finite.  The constructor runs
        gdn_series_fill ONCE: `series` becomes the FILLED series (every missing reading held at its sensor's latest
        earlier real one; what the forward, `y` and `localise` read), `raw_series` keeps the caller's, `valid` [t, n] /
        `keep` [t] uint8 say which readings are real and which ticks are complete, `kept` counts the latter (the ONE
        host read gaps adds) and fewer than `min_kept` of them are refused.  A step is then forward ->
        gdn_score_keys_keep -> gdn_score_select over the kept ticks -> the `_gaps` smooth launch: the table is
        calibrated on complete ticks and a missing reading's normalised error is exactly 0.0.  series[:, :w] must be
        finite.  On a finite series the step writes the bits of gaps=False; gaps=False issues the launches it did.
        `calib="sensor"` (needs gaps=True) calibrates every sensor on ITS OWN real readings instead of
        on complete ticks: `counts` [n] int32 (t - missing_total, formed once from gdn_series_fill's counters) stays on
        the device, `kept` is the smallest of them (read with the head check: still ONE host read) and a sensor with
        fewer than `min_kept` real readings is refused.  A step is forward -> gdn_score_keys_valid ->
        gdn_score_select_counts -> the `_gaps` smooth launch.  `calib="tick"` (the default) is the path above."""
        _check_calib(calib)
        if calib == "sensor" and not gaps:
            raise ValueError("calib='sensor' calibrates around missing readings: it needs gaps=True")
        self.with_gaps = bool(gaps)
        self.calib = calib
        self.raw_series = self.valid = self.keep = self._gap_counters = self.counts = None
        self.kept = None
        if self.with_gaps:
            series, y_all = self._fill(model, x_all, y_all, series, int(min_kept))
        # `series` [N, T_raw] (datasets/TimeDataset.py:42 layout) replaces x_all: window t is
        # series[:, t : t+W], built inside the kernel — no [T, N, W] tensor
        assert (x_all is None) != (series is None), "give either the window tensor or the raw series"
        self.series = series
        self.model, self.x, self.y, self.batch = model.eval(), x_all, y_all, batch * max(1, coalesce)
        assert y_all.is_cuda and self.src.is_cuda
        # range of the resident data, looked at ONCE (include/gdn_hip.h "range guard"): beyond the 16-bit operand
        # range of the matrix-core kernels the whole evaluator runs on the fp32 row-gather kernels
        self.wide = model.wide_for(self.src)
        # gaps=True at a shape without a series kernel (the fp32 tile form below d = 32 reads windows only): the windows
        # of the filled series are cut ONCE, here, and the forward reads them — the streaming detector's route
        self._windows = None
        if self.with_gaps and not self._has_series_kernel():
            self._windows = self._cut_windows()
        self.logical_batch, self.coalesce = batch, max(1, coalesce)
        self.t, self.n = y_all.shape
        dev = y_all.device
        self.pred = torch.empty((self.t, self.n), dtype=torch.float32, device=dev)
        self.ws = ops.score_workspace(self.t, self.n, dev)
        self.med_iqr = torch.empty((self.n, 2), dtype=torch.float64, device=dev)
        self.anomaly = torch.empty((self.t,), dtype=torch.float64, device=dev)
        self.scores = torch.empty((self.n, self.t), dtype=torch.float64, device=dev) if want_scores else None
        self.top_m = int(top_m)
        self.top_scores = self.top_sensors = None
        if self.top_m:
            if want_scores:
                raise ValueError("top_m replaces the [N, T] score table: ask for one of want_scores and top_m")
            _check_top_m(top_m, self.n)
            self.top_scores = torch.empty((self.t, self.top_m), dtype=torch.float64, device=dev)
            self.top_sensors = torch.empty((self.t, self.top_m), dtype=torch.int32, device=dev)
            self.anomaly = self.top_scores[:, 0]
        self.use_graph = use_graph
        def look_again():                   # a parameter changed under a captured graph: the x limit follows it
            self.wide = model.wide_for(self.src)
        # captured graphs bake in the pointers of the model's folded constants: that is their key
        self._step, self._forward = (_Replay(fn, use_graph, lambda: model._constants().key, look_again)
                                     for fn in (self._launch_all, self._launch_forward))
        # GDN_FUSE_KEYS=1: the forward's epilogue writes the scoring keys itself (gdn_forward_fused_plan_keys) and
        # the gdn_score_keys launch disappears.  Measured SLOWER and therefore off by default: the 127 scattered
        # 8-byte stores per window (row pitch 256 KB) cost the forward ~40 us per 32768 windows, the transposing
        # keys kernel 14 us (step 0.379 vs 0.352 ms).
        self.fuse_keys = os.environ.get("GDN_FUSE_KEYS", "0") == "1" and not self.with_gaps   # (the keys need `keep`)
        # independent batches are launched round-robin on side streams (fork/join around the
        # forward), so consecutive launches overlap each other's ramp-up and tail.  Round 1, 4096-window launches:
        # two streams 0.634 ms/step vs 0.697 with one and 0.676 with four.  Round 3, 512-window launches of two
        # windows per workgroup (gdn_forward_dense.hip, fused_op): 72.2 M windows/s on two streams, 74.4 M on
        # three, 69.9 M on four — three is the default
        n_launch = (self.t + self.batch - 1) // self.batch
        self.side = [torch.cuda.Stream(device=dev) for _ in range(min(streams, n_launch))] if streams > 1 else []

    def _fill(self, model, x_all, y_all, series, min_kept: int):
        """gaps=True: refuse what has no meaning with missing readings, fill the series once, count the complete
        ticks.  Returns (the filled series, the derived gt [t, n]); everything here precedes any forward."""
        if x_all is not None or series is None:
            raise ValueError("gaps=True: missing readings are held in the resident series; give series= and no window "
                             "tensor")
        if y_all is not None:
            raise ValueError("gaps=True: y_all is derived from the filled series; pass y_all=None")
        if series.dtype != torch.float32:
            raise ValueError(f"gaps=True: the series must be fp32, got {series.dtype} (a bf16 series cannot be filled)")
        if min_kept < 1:
            raise ValueError(f"min_kept = {min_kept}: the calibration needs at least one complete tick")
        w = model.gnn_layers[0].gnn.lin.weight.shape[1]
        self.raw_series = ops._chk(series, name="series")
        filled, gt, self.valid, self.keep, self._gap_counters = ops.series_fill(self.raw_series, w)
        if self.calib == "sensor":          # every sensor's real readings among the scored ticks; stays on the device
            self.counts = (gt.shape[0] - self._gap_counters[0]).to(torch.int32)
        head_real, kept = torch.stack([torch.isfinite(self.raw_series[:, :w]).all().long(),
                                       self.keep.sum() if self.counts is None else self.counts.min().long()
                                       ]).tolist()                           # ONE host read
        if not head_real:
            raise ValueError(f"series: its first {w} ticks hold a value that is not finite; with gaps=True every "
                             "missing reading is held at an earlier real one, so the series must begin on real readings")
        self.kept = int(kept)
        if self.kept < min_kept and self.counts is not None:
            raise ValueError(too_few_readings(self.counts.cpu(), min_kept, gt.shape[0]))
        if self.kept < min_kept:
            raise ValueError(f"min_kept = {min_kept}: only kept = {self.kept} of the {gt.shape[0]} scored ticks have "
                             "all their readings; too few for a median / IQR table")
        return filled, gt

    def _has_series_kernel(self) -> bool:
        """Whether forward_series takes this model's shape: asked with ONE window (every refusal of the library is
        decided before its launch; an accepted window is the warm-up that builds the plan)."""
        try:
            self.model.forward_series(self.series, 0, 1, wide=self.wide)
        except _lib.GdnHipError:
            return False
        return True

    def _cut_windows(self) -> torch.Tensor:
        """[t, n, w] windows of the filled series, by gdn_windows_gather in launches of up to 4096 windows."""
        n, t_raw = self.series.shape
        t = self.y.shape[0]
        w = t_raw - t
        if t * n * w * 4 > 8 * _VALIDATE_CHUNK_BYTES:
            raise ValueError(f"gaps=True: the model has no series kernel at this shape and the window tensor "
                             f"[{t}, {n}, {w}] fp32 exceeds {8 * _VALIDATE_CHUNK_BYTES >> 20} MB; score a shorter series")
        dev = self.series.device
        starts = torch.arange(w, t_raw, dtype=torch.int64, device=dev)
        x = torch.empty((t, n, w), dtype=torch.float32, device=dev)
        y = torch.empty((min(t, 4096), n), dtype=torch.float32, device=dev)
        for s in range(0, t, 4096):
            ops.windows_gather(self.series, starts, min(4096, t - s), w, x[s:], y, first=s)
        return x

    @property
    def src(self) -> torch.Tensor:
        """The resident data: the raw series when there is one (gaps=True: the filled one), else the window tensor."""
        return self.series if self.series is not None else self.x

    def status_gaps(self):
        """(missing_total [n] int64, missing_run [n] int64) on the host, gaps=True only: every sensor's missing readings
        among the scored ticks and the run of them that ends at the last tick (StreamDetector.status_gaps' counters
        after the same ticks).  ONE read (a synchronisation)."""
        return _status_gaps(self._gap_counters, self.with_gaps, "evaluator")

    def _launch_forward(self, with_keys: bool = False):
        m = self.model
        # constants and the plan are built (when stale) HERE, on the caller's stream, before the fork: built
        # lazily inside the first side-stream launch, the launches on the other side streams would read them
        # unordered (first eager step after a parameter update: garbage in some windows)
        if m.out_layer_num == 1 and not m.training and not self.wide:
            m._plan(m._constants(), self.src.dtype == torch.bfloat16)
        elif m.out_layer_num > 1 and not m.training:     # the OutLayer MLP's plan, for the same reason
            m._mlp_tail(m._constants())
        spans = [(s, min(self.t, s + self.batch)) for s in range(0, self.t, self.batch)]
        # scoring hand-off: the forward's epilogue writes the float64 radix keys |pred - y| of its windows into
        # their columns of the [n, t] key block at the head of the scoring workspace (no gdn_score_keys launch)
        def keys(s, e):
            return (self.y[s:e], self.ws.data_ptr() + 8 * s, self.t) if with_keys else None
        if self.series is not None and self._windows is None:
            def launch(s, e):
                m.forward_series(self.series, s, e - s, out=self.pred[s:e], keys=keys(s, e), wide=self.wide)
        else:
            x = self.x if self._windows is None else self._windows

            def launch(s, e):
                m.forward_into(x[s:e], self.pred[s:e], keys=keys(s, e), wide=self.wide)
        if len(self.side) < 2:
            for s, e in spans:
                launch(s, e)
            return
        main = torch.cuda.current_stream()
        fork = torch.cuda.Event()
        fork.record(main)
        for st in self.side:
            st.wait_event(fork)
        for i, (s, e) in enumerate(spans):
            with torch.cuda.stream(self.side[i % len(self.side)]):
                launch(s, e)
        for st in self.side:
            join = torch.cuda.Event()
            join.record(st)
            main.wait_event(join)

    def _launch_score(self, have_keys: bool = False):
        """The table, then the sweep.  Under gaps=True the table is the select over `kept` (a host constant of the data:
        the step stays capturable) of the keys of complete ticks, the filler elsewhere, and the sweep takes the validity
        plane."""
        st = torch.cuda.current_stream().cuda_stream
        pred, y, med, keys, t, n = (self.pred.data_ptr(), self.y.data_ptr(), self.med_iqr.data_ptr(), self.ws.data_ptr(),
                                    self.t, self.n)
        if have_keys:       # keys [n, t] already sit at the head of the workspace (same layout gdn_score_quantiles uses)
            _lib.call("gdn_score_select", keys, 1, n, t, t, keys + 8 * t * n, med, st)
        elif self.counts is not None:     # calib="sensor": the counts are device data fixed at construction
            _lib.call("gdn_score_keys_valid", pred, y, self.valid.data_ptr(), t, n, t, keys, st)
            _lib.call("gdn_score_select_counts", keys, 1, n, t, self.counts.data_ptr(), 1, keys + 8 * t * n, med, None,
                      st)
        elif self.with_gaps:
            _lib.call("gdn_score_keys_keep", pred, y, self.keep.data_ptr(), t, n, t, keys, st)
            _lib.call("gdn_score_select", keys, 1, n, t, self.kept, keys + 8 * t * n, med, st)
        else:
            _lib.call("gdn_score_quantiles", pred, y, t, n, keys, med, st)
        if self.top_m:
            name, out = "gdn_score_smooth_topm", (self.top_m, self.top_scores.data_ptr(), self.top_sensors.data_ptr())
        else:
            name = "gdn_score_smooth_max"
            out = (None if self.scores is None else self.scores.data_ptr(), self.anomaly.data_ptr())
        gaps = (self.valid.data_ptr(), None) if self.with_gaps else ()
        _lib.call(name + "_gaps" if self.with_gaps else name, pred, y, med, t, n, 0, None, None, *out, *gaps, st)

    def _launch_all(self):
        fuse = self.fuse_keys and not self.wide and self.model.fused_keys_supported(self.src.dtype == torch.bfloat16)
        self._launch_forward(with_keys=fuse)
        self._launch_score(have_keys=fuse)

    graph = property(lambda self: self._step.graph, doc="the captured step, None before its first graphed call")
    fgraph = property(lambda self: self._forward.graph, doc="... of forward_only()")

    def forward_only(self):
        """Forward launches only (multi-GPU: scoring then goes through distributed_anomaly)."""
        self._forward()
        return self.pred

    def step(self):
        self._step()
        return self.anomaly


# --------------------------------------------------------------------------- fleet archive evaluator
class UnitSeries(NamedTuple):
    """One unit of a FleetEvaluator as `localise` and `episodes(evaluator, hi, ...)` read an evaluator: views of the
    fleet's tensors, nothing copied."""
    model: object
    src: torch.Tensor            # [n, T_raw]: the unit's (filled) series
    pred: torch.Tensor           # [t, n]
    y: torch.Tensor              # [t, n]
    t: int
    top_m: int
    top_scores: torch.Tensor | None      # [t, m] float64
    top_sensors: torch.Tensor | None     # [t, m] int32


class FleetEvaluator:
    """The archive side of a fleet: eval forward + median / IQR table + smoothed anomaly scores of U
    units of ONE model, every unit's series resident in HBM, in one captured step.

    `series` [U, n, T_raw] fp32 on the device; unit u contributes t = T_raw - w scored ticks and is scored as
    SeriesEvaluator(model, None, y, batch, series=series[u], ...) scores it, bit for bit: `pred`, `y` [U, t, n],
    `med_iqr` [U, n, 2], `anomaly` [U, t], with `top_m` `top_scores` / `top_sensors` [U, t, m] (anomaly is their column
    0), with `want_scores` `scores` [U, n, t].  A step is U * ceil(t / batch) forward_series launches round-robin over
    the side streams, ONE keys launch for all units, the select over U * n rows in spans of at most 65535, ONE smooth
    launch; with `use_graph` one replay.  The route (`wide`) is decided once for the whole block, as a fleet shares its
    route.  A model whose shape forward_series refuses is refused here (no window-tensor fallback), so is bf16.

    `gaps=True`: SeriesEvaluator's gaps=True per unit.  The constructor runs gdn_series_fill once per unit and holds
    `raw_series`, `series` (filled), `valid` [U, t, n], `keep` [U, t], `kept` [U] (int64, host) and with
    `calib="sensor"` `counts` [U, n] int32 (device) after ONE host read for all units; a unit whose first w ticks are
    not finite or that has fewer than `min_kept` complete ticks (real readings of a sensor) is refused by number.

    `unit(u)` is what `localise` / `episodes` take; `fleet(chunk, ...)` deploys the last step as a StreamFleet."""

    def __init__(self, model, series: torch.Tensor, batch: int, use_graph: bool = True, want_scores: bool = False,
                 top_m: int = 0, gaps: bool = False, min_kept: int = 64, calib: str = "tick", streams: int = 3):
        _check_calib(calib)
        if calib == "sensor" and not gaps:
            raise ValueError("calib='sensor' calibrates around missing readings: it needs gaps=True")
        w = model.gnn_layers[0].gnn.lin.weight.shape[1]
        if not isinstance(series, torch.Tensor) or series.dim() != 3:
            raise ValueError("FleetEvaluator needs a series [U, n, T_raw], got "
                             f"{tuple(series.shape) if isinstance(series, torch.Tensor) else type(series)}")
        units, n, t_raw = series.shape
        if t_raw <= w:
            raise ValueError(f"series [U, n, T_raw]: T_raw = {t_raw} leaves no tick to score behind a window of {w}")
        if series.dtype == torch.bfloat16:
            raise _lib.GdnHipError("series is bfloat16: FleetEvaluator runs on fp32 storage only (a bf16 series is not "
                                   "supported by the fleet-series launches)")
        if series.dtype != torch.float32:
            raise TypeError(f"series: expected {torch.float32}, got {series.dtype}")
        if top_m and want_scores:
            raise ValueError("top_m replaces the [U, n, t] score table: ask for one of want_scores and top_m")
        if top_m:
            _check_top_m(top_m, n)
        if int(batch) < 1 or int(min_kept) < 1:
            raise ValueError(f"batch = {batch}, min_kept = {min_kept}: both at least 1")
        t = t_raw - w
        ops.fleet_series_check(units, t, n)          # (the 2 GiB cap of the key block among the limits)
        if n != model.embedding.weight.shape[0]:
            raise ValueError(f"series [U, n, T_raw]: n = {n}, the model has {model.embedding.weight.shape[0]} sensors")
        series = ops._chk(series, name="series")     # on the device, contiguous
        dev = series.device
        self.model, self.batch, self.units, self.n, self.t, self.w = model.eval(), int(batch), units, n, t, w
        self.with_gaps, self.calib, self.top_m, self.use_graph = bool(gaps), calib, int(top_m), use_graph
        self.raw_series = self.valid = self.keep = self._gap_counters = self.counts = self.kept = None
        if self.with_gaps:
            self._fill(series, int(min_kept))
        else:
            self.series = series
            self.y = series[:, :, w:].transpose(1, 2).contiguous()
            self._sel_counts = torch.full((units, n), t, dtype=torch.int32, device=dev)
        self.wide = model.wide_for(self.series)      # ONE route for the whole block
        try:                                         # every refusal of the library precedes its launch; an accepted
            model.forward_series(self.series[0], 0, 1, wide=self.wide)       # window is the warm-up that builds the plan
        except _lib.GdnHipError as exc:
            raise _lib.GdnHipError(f"FleetEvaluator: forward_series has no kernel for this model's shape ({exc}); the "
                                   "window-tensor route is SeriesEvaluator's") from exc
        self.pred = torch.empty((units, t, n), dtype=torch.float32, device=dev)
        self.keys = torch.empty((units, n, t), dtype=torch.float64, device=dev)
        self._ws = ops.fleet_select_workspace(units, n, t, dev)
        self.med_iqr = torch.empty((units, n, 2), dtype=torch.float64, device=dev)
        self.scores = torch.empty((units, n, t), dtype=torch.float64, device=dev) if want_scores else None
        self.top_scores = self.top_sensors = None
        if self.top_m:
            self.top_scores = torch.empty((units, t, self.top_m), dtype=torch.float64, device=dev)
            self.top_sensors = torch.empty((units, t, self.top_m), dtype=torch.int32, device=dev)
            self.anomaly = self.top_scores[:, :, 0]
        else:
            self.anomaly = torch.empty((units, t), dtype=torch.float64, device=dev)
        self.spans = [(u, s, min(t, s + self.batch)) for u in range(units) for s in range(0, t, self.batch)]
        self.side = [torch.cuda.Stream(device=dev) for _ in range(min(streams, len(self.spans)))] if streams > 1 else []

        def look_again():                   # a parameter changed under a captured graph: the x limit follows it
            self.wide = model.wide_for(self.series)
        self._step = _Replay(self._launch_all, use_graph, lambda: model._constants().key, look_again)

    def _fill(self, raw, min_kept: int):
        """gaps=True: gdn_series_fill per unit into the stacked planes, the counts on the device, ONE host read."""
        units, n, t, w = self.units, self.n, self.t, self.w
        dev = raw.device
        self.raw_series = raw
        self.series = torch.empty_like(raw)
        self.y = torch.empty((units, t, n), dtype=torch.float32, device=dev)
        self.valid = torch.empty((units, t, n), dtype=torch.uint8, device=dev)
        self.keep = torch.empty((units, t), dtype=torch.uint8, device=dev)
        self._gap_counters = torch.empty((units, 2, n), dtype=torch.int64, device=dev)
        ws = torch.empty((_lib.load().gdn_series_fill_workspace_bytes(n, t + w) // 8,), dtype=torch.int64, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        for u in range(units):              # construction is not the step: the existing kernel, once per unit
            _lib.call("gdn_series_fill", raw[u].data_ptr(), n, t + w, w, self.series[u].data_ptr(), self.y[u].data_ptr(),
                      self.valid[u].data_ptr(), self.keep[u].data_ptr(), self._gap_counters[u].data_ptr(),
                      ws.data_ptr(), st)
        if self.calib == "sensor":          # every sensor's real readings among the scored ticks
            self.counts = (t - self._gap_counters[:, 0]).to(torch.int32)
            self._sel_counts, least = self.counts, self.counts.amin(dim=1).long()
        else:                               # the complete ticks of unit u, for every sensor of unit u
            least = self.keep.sum(dim=1)
            self._sel_counts = least.to(torch.int32).view(units, 1).expand(units, n).contiguous()
        head = torch.isfinite(raw[:, :, :w]).all(dim=2).all(dim=1).long()
        both = torch.stack([head, least]).cpu()                              # ONE host read for all units
        bad = torch.nonzero(both[0] == 0).flatten()[:8].tolist()
        if bad:
            raise ValueError(f"series: the first {w} ticks of units {bad} hold a value that is not finite; with gaps=True "
                             "every missing reading is held at an earlier real one, so every unit's series must begin "
                             "on real readings")
        self.kept = both[1].clone()
        short = torch.nonzero(self.kept < min_kept).flatten()[:8].tolist()
        if short:
            what = "real readings of their scarcest sensor" if self.calib == "sensor" else "complete ticks"
            raise ValueError(f"min_kept = {min_kept}: units {short} have only {[int(self.kept[u]) for u in short]} {what} "
                             f"among the {t} scored ticks; too few for their median / IQR tables")

    def status_gaps(self):
        """(missing_total [U, n] int64, missing_run [U, n] int64) on the host, gaps=True only: SeriesEvaluator.status_gaps
        per unit.  ONE read (a synchronisation)."""
        if not self.with_gaps:
            raise ValueError("status_gaps(): the fleet evaluator was built with gaps=False and counts no missing readings")
        both = self._gap_counters.cpu()
        return both[:, 0], both[:, 1]

    def _launch_forward(self):
        m = self.model
        # constants and the plan are built (when stale) HERE, on the caller's stream, before the fork: the side streams
        # would read them unordered otherwise (SeriesEvaluator._launch_forward)
        if m.out_layer_num == 1 and not self.wide:
            m._plan(m._constants(), False)
        elif m.out_layer_num > 1:
            m._mlp_tail(m._constants())

        def launch(u, s, e):
            m.forward_series(self.series[u], s, e - s, out=self.pred[u, s:e], wide=self.wide)
        if len(self.side) < 2:
            for span in self.spans:
                launch(*span)
            return
        main = torch.cuda.current_stream()
        fork = torch.cuda.Event()
        fork.record(main)
        for st in self.side:
            st.wait_event(fork)
        for i, span in enumerate(self.spans):
            with torch.cuda.stream(self.side[i % len(self.side)]):
                launch(*span)
        for st in self.side:
            join = torch.cuda.Event()
            join.record(st)
            main.wait_event(join)

    def _launch_all(self):
        """forward -> ONE keys launch -> the select spans -> ONE smooth launch."""
        self._launch_forward()
        tick = self.with_gaps and self.counts is None
        ops.fleet_series_keys(self.pred, self.y, self.t, out=self.keys, keep=self.keep if tick else None,
                              valid=self.valid if self.counts is not None else None)
        ops.fleet_select_counts(self.keys, self._sel_counts, 1, self._ws, self.med_iqr)
        if self.top_m:
            ops.fleet_series_smooth_topm(self.pred, self.y, self.med_iqr, self.top_m, self.top_scores, self.top_sensors,
                                         valid=self.valid)
        else:
            ops.fleet_series_smooth_max(self.pred, self.y, self.med_iqr, want_scores=False, anomaly=self.anomaly,
                                        scores=self.scores, valid=self.valid)

    graph = property(lambda self: self._step.graph, doc="the captured step, None before its first graphed call")

    def step(self):
        self._step()
        return self.anomaly

    def thresholds(self) -> torch.Tensor:
        """[U] float64 on the device: every unit's largest anomaly score of the last step."""
        return self.anomaly.amax(dim=1)

    def unit(self, u: int) -> UnitSeries:
        """Unit u as `localise(evaluator, ticks)` and `episodes(evaluator, hi, ...)` read an evaluator (views)."""
        if not 0 <= int(u) < self.units:
            raise ValueError(f"unit {u} outside [0, {self.units})")
        top = (None, None) if not self.top_m else (self.top_scores[u], self.top_sensors[u])
        return UnitSeries(self.model, self.series[u], self.pred[u], self.y[u], self.t, self.top_m, *top)

    def fleet(self, chunk: int, **kw):
        """A StreamFleet from the last step (step() first), as StreamFleet.from_calibration(model, series, chunk,
        calib_gaps=<gaps>, calib=<calib>, **kw) builds it, without its loop: the tables, `thresholds()`, every unit's
        last w (filled) ticks as the history, `calib_kept` / `calib_counts`, and with `recal=R` every unit's ring seeded
        by the rule of `_seed_ring` from ONE keys launch.  `gaps=` and `calib=` default to the evaluator's."""
        units, n, t, w = self.units, self.n, self.t, self.w
        kw.setdefault("gaps", self.with_gaps)
        if kw.setdefault("calib", self.calib) != self.calib:
            raise ValueError(f"calib = {kw['calib']!r}: the evaluator calibrated with calib = {self.calib!r}")
        _check_calib_period(self.series, self.with_gaps, kw["gaps"], "fleet")
        fleet_check_shape(units, chunk, n, w)
        R = int(kw.get("recal", 0))
        if self.calib == "sensor" and not R:
            kw["calib"] = "tick"            # no ring: the fleet never calibrates anything itself
        history = kw.pop("history", None)
        fleet = StreamFleet(self.model, self.med_iqr, self.thresholds(),
                            self.series[:, :, -w:].contiguous() if history is None else history, chunk, **kw)
        if self.with_gaps:
            fleet.calib_kept = self.kept.clone()
        if self.calib == "sensor":
            fleet.calib_counts = self.counts.clone()
        if R:                               # _seed_ring per unit: the last s rows, oldest first, into slots R - s .. R - 1
            s = min(R, t)
            sensor = self.calib == "sensor"
            keep = None if sensor or self.keep is None else self.keep[:, -s:].contiguous()
            keys = ops.fleet_series_keys(self.pred[:, -s:].contiguous(), self.y[:, -s:].contiguous(), s, keep=keep,
                                         valid=self.valid[:, -s:].contiguous() if sensor else None)
            fleet.ring_keys[:, :, R - s:].copy_(keys)
            if keep is None:
                fleet.ring_keep[:, R - s:].fill_(1)
            else:
                fleet.ring_keep[:, R - s:].copy_(keep)
        return fleet


# --------------------------------------------------------------------------- localisation
class Localisation(NamedTuple):
    """What `localise` returns, one row per tick: the m most deviating sensors, their smoothed scores, predicted
    and observed values, and for each of them the sensors it was reading (-1 = padding) with their attention."""
    ticks: torch.Tensor          # [Q] int64
    sensors: torch.Tensor        # [Q, m] int64
    scores: torch.Tensor         # [Q, m] float64
    predicted: torch.Tensor      # [Q, m] fp32
    observed: torch.Tensor       # [Q, m] fp32
    neighbours: torch.Tensor     # [Q, m, K+1] int64
    attention: torch.Tensor      # [Q, m, K+1] fp32

    def numpy(self) -> dict:
        return {name: getattr(self, name).cpu().numpy() for name in self._fields}


def _row_indices(rows, device, limit: int, error: str) -> torch.Tensor:
    rows = torch.as_tensor(rows, device=device).to(torch.int64).reshape(-1)
    if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= limit):
        raise ValueError(error)
    return rows


def _localisation(model, src, ticks, rows, sensors, top_scores, pred, observed) -> Localisation:
    """The Localisation of `ticks` [Q] from row `rows` [Q] of the tables pred / observed [T, n] and of the windows in
    `src`, for the sensors [Q, m] int64 with the scores top_scores [Q, m]: ONE model.attention_at."""
    m = sensors.shape[1]
    at = rows.view(-1, 1).expand(-1, m)
    nb = model.attention_neighbours()
    att = model.attention_at(src, at.reshape(-1), sensors.reshape(-1))
    return Localisation(ticks, sensors, top_scores, pred[at, sensors], observed[at, sensors], nb[sensors],
                        att.reshape(rows.numel(), m, nb.shape[1]))


def localise(evaluator: SeriesEvaluator, ticks, m: int | None = None) -> Localisation:
    """Which sensors deviate at `ticks` (rows of the evaluator's prediction table) and which neighbours they were
    reading: the top-m table of the evaluator's last step (SeriesEvaluator(top_m >= 1) or FleetEvaluator.unit(u),
    step() first) plus one gdn_attention_at launch on its resident data.  `m` defaults to the evaluator's top_m."""
    ev = evaluator
    if not ev.top_m:
        raise ValueError("localise needs an evaluator built with top_m >= 1")
    m = ev.top_m if m is None else int(m)
    if not 1 <= m <= ev.top_m:
        raise ValueError(f"m = {m}: the evaluator keeps {ev.top_m} sensors per tick")
    ticks = _row_indices(ticks, ev.pred.device, ev.t, f"ticks outside [0, {ev.t})")
    return _localisation(ev.model, ev.src, ticks, ticks, ev.top_sensors[ticks, :m].long(), ev.top_scores[ticks, :m],
                         ev.pred, ev.y)


# --------------------------------------------------------------------------- alarm episodes
class Episodes(NamedTuple):
    """An episode table, device tensors of `cap` rows of which the first min(count, cap) are written:
    one row per incident — first tick, first tick of the clearing run (exclusive; -1 while the episode is open), the
    largest score, the first tick that holds it and the top sensors of that tick.  Ticks are global."""
    start: torch.Tensor          # [cap] int64
    end: torch.Tensor            # [cap] int64
    peak: torch.Tensor           # [cap] float64
    peak_tick: torch.Tensor      # [cap] int64
    sensors: torch.Tensor        # [cap, m] int32
    count: torch.Tensor          # [1] int64: episodes raised, beyond cap too

    def numpy(self) -> dict:
        """The written rows on the host (ONE synchronisation); `count` as a Python int."""
        count = int(self.count.item())
        rows = min(count, self.start.shape[0])
        out = {name: getattr(self, name)[:rows].cpu().numpy() for name in self._fields[:-1]}
        out["count"] = count
        return out


def episodes(scores, top_sensors=None, hi=None, lo=None, on: int = 1, off: int = 1, cap: int = 4096,
             first_tick: int = 0) -> Episodes:
    """The alarm episodes of a scored series: `scores` [T] float64 and `top_sensors` [T, m] int32 on
    the device, raised after `on` ticks above `hi`, cleared after `off` ticks at or below `lo` (None: hi).  Or
    `episodes(evaluator, hi, ...)` for a SeriesEvaluator (or a FleetEvaluator.unit(u)) built with top_m= whose step()
    has run: its top_scores[:, 0] and top_sensors; the peak ticks go straight into `localise(evaluator, ticks)`.  One
    gdn_episodes_scan (five launches, parallel over T), no synchronisation."""
    if not isinstance(scores, torch.Tensor) and hasattr(scores, "top_m"):
        ev = scores                                         # a SeriesEvaluator, or FleetEvaluator.unit(u)
        if isinstance(top_sensors, torch.Tensor) and top_sensors.dim() > 0:
            raise ValueError("episodes(evaluator, hi, ...): the evaluator brings its own top_sensors")
        if top_sensors is not None:                         # episodes(evaluator, hi[, lo]): the levels move up one place;
            if hi is not None and lo is not None:           # what follows them goes by keyword
                raise ValueError("episodes(evaluator, hi, lo, on=, off=, cap=, first_tick=)")
            top_sensors, hi, lo = None, top_sensors, (hi if lo is None else lo)
        if not ev.top_m:
            raise ValueError("episodes needs an evaluator built with top_m >= 1")
        scores, top_sensors = ev.top_scores[:, 0].contiguous(), ev.top_sensors
    if hi is None or top_sensors is None:
        raise ValueError("episodes(scores, top_sensors, hi, ...): the raise level hi and top_sensors are needed")
    hi, lo, on, off, cap = ops.episodes_check(hi, lo, on, off, cap)
    if int(first_tick) < 0:
        raise ValueError(f"first_tick = {first_tick} is negative")
    start, end, peak_tick, peak, sensors, count = ops.episodes_scan(scores, top_sensors, hi, lo, on, off, cap, first_tick)
    return Episodes(start, end, peak, peak_tick, sensors, count)


# --------------------------------------------------------------------------- alarm tuning
class AlarmSweep(NamedTuple):
    """The counters of P alarm settings against labelled incidents, device tensors.  Row p of `counts`
    holds ops.ALARM_SWEEP_COUNTERS for (hi[p], lo[p], on[p], off[p]); -1 in all eight marks a row that is not a
    setting (lo > hi, a NaN level, on / off outside 1 .. 4096)."""
    hi: torch.Tensor             # [P] float64
    lo: torch.Tensor             # [P] float64: the level used (hi * lo_frac already multiplied out)
    on: torch.Tensor             # [P] int32
    off: torch.Tensor            # [P] int32
    counts: torch.Tensor         # [P, 8] int64
    incidents: torch.Tensor      # [1] int64: I, the maximal runs of labelled ticks
    label_ticks: torch.Tensor    # [1] int64
    ticks: torch.Tensor          # [1] int64: T

    def numpy(self) -> dict:
        """Everything on the host (ONE synchronisation: one packed copy); the three totals as Python ints."""
        P = self.hi.shape[0]
        flat = torch.cat([self.hi.view(torch.int64), self.lo.view(torch.int64), self.on.long(), self.off.long(),
                          self.counts.reshape(-1), self.incidents, self.label_ticks, self.ticks]).cpu().numpy()
        out = {"hi": flat[:P].view(np.float64), "lo": flat[P:2 * P].view(np.float64),
               "on": flat[2 * P:3 * P].astype(np.int32), "off": flat[3 * P:4 * P].astype(np.int32),
               "counts": flat[4 * P:12 * P].reshape(P, 8)}
        out["incidents"], out["label_ticks"], out["ticks"] = (int(v) for v in flat[12 * P:])
        return out

    def f1(self) -> torch.Tensor:
        """[P] float64: the event F1 of every row, 2 * true_episodes * incidents_hit / (true_episodes * I + incidents_hit
        * episodes); 0 where that denominator is 0 and in rows that are not settings."""
        ep, te, ih = (self.counts[:, j].double() for j in range(3))
        den = te * self.incidents.double() + ih * ep
        return torch.where((den > 0) & (self.counts[:, 0] >= 0), 2.0 * te * ih / den.clamp(min=1.0), torch.zeros_like(den))

    def best(self, min_recall: float = 0.0, max_delay=None) -> dict:
        """The setting to deploy, chosen on the device: among the valid rows with incidents_hit / I >= min_recall (and a
        mean delay delay_sum / incidents_hit <= max_delay) the largest event F1; ties go to the smaller delay_sum, then
        the smaller alarm_ticks, then the lower row.  Returns dict(hi=, lo=, on=, off=) plus the row's counters, `row`
        and `f1`: `StreamDetector(threshold=hi, events=dict(on=, off=, lo=))`.  No row qualifies: ValueError."""
        c = self.counts
        P = c.shape[0]
        ih = c[:, 2].double()
        ok = (c[:, 0] >= 0) & (ih >= float(min_recall) * self.incidents.double())
        if max_delay is not None:
            ok = ok & (c[:, 3].double() <= float(max_delay) * ih)
        f1 = self.f1()
        big = torch.iinfo(torch.int64).max
        ok = ok & (f1 == torch.where(ok, f1, torch.full_like(f1, -1.0)).max())
        for j in (3, 5):
            ok = ok & (c[:, j] == torch.where(ok, c[:, j], torch.full_like(c[:, j], big)).min())
        rows = torch.arange(P, device=c.device)
        row = torch.where(ok, rows, torch.full_like(rows, P)).min()
        at = row.clamp(max=P - 1)
        packed = torch.cat([row.reshape(1), self.hi[at].view(torch.int64).reshape(1), self.lo[at].view(torch.int64).reshape(1),
                            self.on[at].long().reshape(1), self.off[at].long().reshape(1), c[at],
                            f1[at].view(torch.int64).reshape(1)]).cpu().numpy()
        if int(packed[0]) >= P:
            raise ValueError(f"alarm sweep: none of the {P} settings is valid and reaches min_recall = {min_recall}"
                             + ("" if max_delay is None else f" within max_delay = {max_delay}"))
        out = {"hi": float(packed[1:2].view(np.float64)[0]), "lo": float(packed[2:3].view(np.float64)[0]),
               "on": int(packed[3]), "off": int(packed[4])}
        out.update({name: int(v) for name, v in zip(ops.ALARM_SWEEP_COUNTERS, packed[5:13])})
        out["row"], out["f1"] = int(packed[0]), float(packed[13:14].view(np.float64)[0])
        return out


def alarm_sweep_table(hi, lo=None, on=1, off=1, product: bool = True, lo_frac=None) -> tuple:
    """The settings of a sweep as host tensors (hi, lo float64 [P]; on, off int32 [P]).  `product=True`: the grid of the
    four sequences, hi slowest and off fastest; `product=False`: P explicit rows (scalars are broadcast).  The clear
    level is `lo` (None: hi) or, through `lo_frac`, hi * lo_frac — a float64 multiply in torch whose product is the
    level used.  Explicit rows are checked whole (ops.alarm_sweep_check); in a grid every value is, and a row of it
    whose lo lies above its hi is left to the device, which marks it with -1."""
    if lo is not None and lo_frac is not None:
        raise ValueError("lo and lo_frac: give the clear level one way")

    def seq(value, dtype):                                  # (Python floats are float64, a tensor keeps its values)
        exact = isinstance(value, (torch.Tensor, np.ndarray))
        return (torch.as_tensor(value) if exact else torch.as_tensor(value, dtype=dtype)).detach().cpu().to(dtype).reshape(-1)
    if not product:
        if lo_frac is not None:
            h, f = seq(hi, torch.float64), seq(lo_frac, torch.float64)
            if f.numel() not in (1, h.numel()) and h.numel() != 1:
                raise ValueError(f"lo_frac: {f.numel()} values, hi has {h.numel()}")
            lo = h * f
        return ops.alarm_sweep_check(hi, hi if lo is None else lo, on, off)
    # every sequence checked on its own (the row in a message is the place in that sequence), then the grid
    h = ops.alarm_sweep_check(hi, hi, 1, 1)[0]
    n_on, n_off = ops.alarm_sweep_check(0.0, 0.0, on, 1)[2], ops.alarm_sweep_check(0.0, 0.0, 1, off)[3]
    second = seq(1.0 if (lo is None and lo_frac is None) else (lo if lo_frac is None else lo_frac), torch.float64)
    if bool((second != second).any()):
        raise ValueError(f"{'lo' if lo_frac is None else 'lo_frac'}[{int(torch.nonzero(second != second)[0])}] = nan: "
                         "the level must be a number")
    i, j, k, m = (g.reshape(-1) for g in torch.meshgrid(*(torch.arange(c.numel()) for c in (h, second, n_on, n_off)),
                                                       indexing="ij"))
    glo = second[j] if lo is not None else h[i] * second[j]
    return ops.alarm_sweep_check(h[i], glo, n_on[k].long(), n_off[m].long(), ordered=False)


def _labels_u8(labels, device) -> torch.Tensor:
    labels = torch.as_tensor(labels).to(device)
    if labels.dim() != 1:
        raise ValueError(f"labels: expected [T], got {tuple(labels.shape)}")
    return (labels > 0).to(torch.uint8)


def _incident_edges(lab: torch.Tensor) -> tuple:
    """(first tick, end (exclusive)) of every maximal run of labelled ticks of lab [T] uint8, int64 on lab's device."""
    pad = torch.zeros((1,), dtype=lab.dtype, device=lab.device)
    step = torch.diff(torch.cat([pad, lab, pad]).to(torch.int8))
    return torch.nonzero(step == 1)[:, 0], torch.nonzero(step == -1)[:, 0]


def alarm_sweep(scores, labels, hi, lo=None, on=1, off=1, product: bool = True, lo_frac=None) -> AlarmSweep:
    """Sweep alarm settings against labelled incidents: `scores` [T] float64 on the device — or a
    SeriesEvaluator built with top_m >= 1 whose step() has run: its top_scores[:, 0] — and `labels` [T] of any numeric
    or bool dtype (> 0: the tick lies inside an incident).  The settings: alarm_sweep_table(hi, lo, on, off, product,
    lo_frac).  One gdn_alarm_sweep launch for the counters; I and the labelled ticks by torch ops; no synchronisation."""
    if isinstance(scores, SeriesEvaluator):
        if not scores.top_m:
            raise ValueError("alarm_sweep needs an evaluator built with top_m >= 1")
        scores = scores.top_scores[:, 0].contiguous()
    t_hi, t_lo, t_on, t_off = alarm_sweep_table(hi, lo, on, off, product, lo_frac)
    if not isinstance(scores, torch.Tensor) or not scores.is_cuda:
        raise _lib.GdnHipError("scores: a float64 tensor on a HIP device is needed (no CPU fallback)")
    dev = scores.device
    lab = _labels_u8(labels, dev)
    if lab.shape != scores.shape:
        raise ValueError(f"labels: {tuple(lab.shape)}, scores {tuple(scores.shape)}")
    t_hi, t_lo, t_on, t_off = (t.to(dev) for t in (t_hi, t_lo, t_on, t_off))
    counts = ops.alarm_sweep(scores, lab, t_hi, t_lo, t_on, t_off)
    step = torch.diff(lab.to(torch.int8), prepend=torch.zeros((1,), dtype=torch.int8, device=dev))
    return AlarmSweep(t_hi, t_lo, t_on, t_off, counts, (step == 1).sum().reshape(1), lab.sum(dtype=torch.int64).reshape(1),
                      torch.full((1,), scores.shape[0], dtype=torch.int64, device=dev))


class EpisodeReport(NamedTuple):
    """One setting's episodes against the labelled incidents, row by row (device tensors).  Per incident: `begin`, `end`
    (exclusive), `hit`, `episode` (the row of the first episode that overlaps it, -1: none), `delay` = max(0, that
    episode's raise tick - begin), 0 where not hit.  Per episode: `label_ticks` inside its span, `true` = it holds one;
    `spans` [rows, 2]: (start, end) with an open episode ending at T."""
    begin: torch.Tensor
    end: torch.Tensor
    hit: torch.Tensor
    episode: torch.Tensor
    delay: torch.Tensor
    label_ticks: torch.Tensor
    true: torch.Tensor
    spans: torch.Tensor
    open: torch.Tensor           # [1] int64

    def counters(self) -> torch.Tensor:
        """[8] int64: the aggregates in the order of ops.ALARM_SWEEP_COUNTERS — by construction the sweep's row."""
        z = torch.zeros((1,), dtype=torch.int64, device=self.begin.device)
        delay = torch.cat([self.delay, z])
        return torch.stack([z[0] + self.spans.shape[0], self.true.sum(), self.hit.sum(), delay.sum(), delay.max(),
                            (self.spans[:, 1] - self.spans[:, 0]).sum(), self.label_ticks.sum(), self.open[0]])


def episode_report(episodes: Episodes, labels, on: int) -> EpisodeReport:
    """Per-incident and per-episode tables for ONE setting: `episodes` from `harness.episodes(...)` (first_tick 0) with
    on-delay `on`, `labels` [T] as in alarm_sweep.  Torch ops on the device (searchsorted over the episodes' ends, a
    prefix sum of the labels) and one host read of the count: this is reporting.  A table that holds fewer rows than
    were raised (count > cap) is refused."""
    on = ops.episodes_check(None, None, on, 1, 0)[2]
    cap, count = episodes.start.shape[0], int(episodes.count.item())
    if count > cap:
        raise ValueError(f"episode_report: {count} episodes were raised, the table keeps cap = {cap}: scan with a larger cap")
    dev = episodes.start.device
    lab = _labels_u8(labels, dev)
    T = lab.shape[0]
    start = episodes.start[:count]
    end = torch.where(episodes.end[:count] < 0, torch.full_like(start, T), episodes.end[:count])
    upto = torch.cat([torch.zeros((1,), dtype=torch.int64, device=dev), torch.cumsum(lab, 0, dtype=torch.int64)])
    label_ticks = upto[end] - upto[start.clamp(min=0)]
    begin, stop = _incident_edges(lab)
    k = torch.searchsorted(end, begin, right=True)          # the first episode that ends after the incident begins
    far = torch.full((1,), T + 1, dtype=torch.int64, device=dev)
    hit = torch.cat([start, far])[k] < stop
    delay = torch.where(hit, (torch.cat([start, far])[k] + (on - 1) - begin).clamp(min=0), torch.zeros_like(begin))
    is_open = (episodes.end[count - 1:count] < 0).long() if count else torch.zeros((1,), dtype=torch.int64, device=dev)
    return EpisodeReport(begin, stop, hit, torch.where(hit, k, torch.full_like(k, -1)), delay, label_ticks,
                         label_ticks > 0, torch.stack([start, end], dim=1), is_open)


# --------------------------------------------------------------------------- graphed train step
class _CapturedStep:
    """One optimisation step of the reference's train() (train.py:52-79) issued as two halves: `_first` (the caller's
    `pre` hook, then forward, loss and backward) and `_second` (the optimizer, then the `post` hook).  With more than
    one rank (or `split=True`, the rehearsal of it) ONE eager op sits between the halves, the all-reduce of a flat
    gradient bucket.

    At the reference's batch sizes a step is a few dozen launches of a few microseconds each, so issuing them from
    Python costs more than running them.  With `use_graph` the halves are captured once — one HIP graph, or two around
    the all-reduce — and a step is one or two replays.  `_capture`: snapshot `_saved()`; `WARMUP` eager steps (lazy
    attribute / occupancy queries, allocations); restore the snapshot, then `_after_restore()` — capturing must not
    train the model; capture (which executes nothing) through `capture()` into one shared pool.

    `x` / `y` are the static input buffers: copy each minibatch into them, call `step()`, read `loss` (a device scalar)
    whenever convenient.

    `pre` / `post`: optional callables that issue launches on the current stream immediately before the step's first
    launch and immediately after the optimizer's — in eager mode, in the warm-up steps of the capture and INSIDE the
    captured graph (with two graphs: `pre` in the first, `post` in the second).  harness.SeriesTrainer hangs the
    window gather and the cursor / loss bookkeeping of an epoch there.  None: exactly the launches of a plain step.

    A subclass sets `model`, `x`, `y`, `loss` and `optimizer` and provides `_forward_backward()`, `_update()`,
    `_all_reduce()`, `_saved()` (the tensors whose values the warm-up must not change) and `_after_restore()`."""

    WARMUP = 2

    def __init__(self, use_graph: bool, split: bool | None, pre, post):
        self.pre, self.post = pre, post
        self.use_graph, self._graphs = use_graph, None
        # two graphs around the (eager) gradient all-reduce; forced on by `split=True` for rehearsal
        self._split = world()[1] > 1 if split is None else bool(split)

    def _own_validity(self, gaps: bool, batch: int, n: int, dev):
        """`gaps=True`: the step owns static `valid` [batch, n] uint8 and `row_valid` [batch] int32 beside
        `x` / `y` — which targets were observed and how many per window, all of them until a gather says otherwise —
        and its loss is the masked launch.  One rank only: per-rank masked means are not the global masked mean."""
        self.gaps = bool(gaps)
        self.valid = self.row_valid = None
        if not self.gaps:
            return
        if world()[1] > 1:
            raise _lib.GdnHipError("gaps=True runs in one process: every rank would divide by its own number of observed "
                                   "targets, and the average of per-rank masked means is not the global masked mean")
        self.valid = torch.ones((batch, n), dtype=torch.uint8, device=dev)
        self.row_valid = torch.full((batch,), n, dtype=torch.int32, device=dev)

    def _first(self):
        if self.pre is not None:
            self.pre()
        self._forward_backward()

    def _second(self):
        self._update()
        if self.post is not None:
            self.post()

    def _warm_up(self):
        for _ in range(self.WARMUP):
            self._first()
            self._all_reduce()
            self._second()

    def _capture(self):
        saved = [(t, t.detach().clone()) for t in self._saved()]
        self._warm_up()
        torch.cuda.synchronize()
        with torch.no_grad():
            for t, s in saved:
                t.copy_(s)
            self._after_restore()
        torch.cuda.synchronize()
        pool = torch.cuda.graph_pool_handle()
        graphs = []
        for half in ((self._first,), (self._second,)) if self._split else ((self._first, self._second),):
            g = torch.cuda.CUDAGraph()
            with capture(g, pool=pool):
                for fn in half:
                    fn()
            graphs.append(g)
        self._graphs = graphs

    def prepare(self):
        """Capture now (the first `step()` otherwise does): a caller whose hooks keep state of their own
        (harness.SeriesTrainer's cursor) resets it after the warm-up steps of the capture have moved it."""
        if self.use_graph and self._graphs is None:
            self._capture()

    def step(self):
        if self.use_graph:
            self.prepare()
            self._graphs[0].replay()
            if self._split:
                self._all_reduce()                       # the only eager op of a multi-rank step
                self._graphs[1].replay()
        else:
            self._first()
            if self._split:
                self._all_reduce()
            self._second()
        # a replay writes parameters and BatchNorm statistics through raw pointers: no Python forward runs and no
        # version counter moves, so the model's cached eval constants (sensor graph, attention terms, BatchNorm
        # folds) must be dropped here or eval after training serves stale ones
        self.model.invalidate_constants()
        return self.loss


class AutogradTrainStep(_CapturedStep):
    """The step through torch autograd and torch.optim.Adam(fused=True, capturable=True): used when `NativeTrainStep`
    does not apply (a custom `model.dp` module, an injected graph, an OutLayer or a shape the training kernels do not
    take).  The halves hold the per-step rebuild of the sensor graph and the folded attention terms, the HIP
    forward/backward of the graph layer and of the train-mode head, the fused MSE loss + gradient kernel, torch's
    dropout draw and the fused Adam.  Split: packing the gradient bucket is the tail of the first half, averaging +
    unpacking the head of the second.  The warm-up runs on a side stream, as torch asks of autograd work that precedes
    a capture."""

    WARMUP = 3

    def __init__(self, model, batch: int, lr: float = 1e-3, weight_decay: float = 0.0, use_graph: bool = True,
                 split: bool | None = None, wide: bool = False, pre=None, post=None, gaps: bool = False):
        super().__init__(use_graph, split, pre, post)
        self.wide = bool(wide)
        p0 = next(model.parameters())
        if not p0.is_cuda:
            raise RuntimeError("GraphedTrainStep needs the model on a HIP device")
        dev = p0.device
        n, w = model.embedding.weight.shape[0], model.gnn_layers[0].gnn.lin.weight.shape[1]
        self.model = model.train()
        self.x = torch.zeros((batch, n, w), dtype=torch.float32, device=dev)
        self.y = torch.zeros((batch, n), dtype=torch.float32, device=dev)
        self.loss = torch.zeros((), dtype=torch.float32, device=dev)
        self._d_out = torch.empty((batch, n), dtype=torch.float32, device=dev)
        self._mse_ws = ops.mse_workspace(dev)
        # fused: one multi-tensor launch for all 13 parameters instead of ~40 small ones
        self.optimizer = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=weight_decay, capturable=True,
                                          fused=True)
        self._flat = None                                # static gradient bucket (split mode)
        self._own_validity(gaps, batch, n, dev)
        self._torch_mse = bool(os.environ.get("GDN_TORCH_MSE")) and not self.gaps     # (torch's loss knows no mask)
        self._dbg = None                                 # diagnostic snapshot buffers (tools/probe_mse_replay.py)

    # `loss` is written in place so it survives replays
    def _forward_backward(self):
        self.optimizer.zero_grad(set_to_none=True)      # backward then writes fresh gradients: no fill, no add
        with pinned_range(self.model, self.wide):       # no host check inside a captured step
            out = self.model(self.x, None)
        if self._torch_mse:     # diagnostic (tools/probe_mse_replay.py): the round-1 form with torch's reduction
            loss = F.mse_loss(out, self.y, reduction="mean")
            loss.backward()
            self.loss.copy_(loss.detach())
            if self._dbg is not None:
                self._dbg["out"].copy_(out.detach())
                self._dbg["loss_raw"].copy_(loss.detach())
        else:
            # loss + its gradient in one launch (train.py:20-23, :72); autograd starts from d_out
            ops.mse_loss_grad(out.detach(), self.y, self._mse_ws, loss=self.loss, d_out=self._d_out, valid=self.valid,
                              row_valid=self.row_valid)
            out.backward(self._d_out)
        if self._dbg is not None:
            for name, prm in self.model.named_parameters():
                self._dbg["g/" + name].copy_(prm.grad)
        if self._split:                                  # the bucket is part of the first graph
            if self._flat is None:
                self._flat = pack_gradients(self.model)
            else:
                pack_gradients(self.model, self._flat)

    def _update(self):
        if self._split:                                  # ... and its unpacking part of the second
            unpack_gradients(self.model, self._flat, world()[1])
        self.optimizer.step()

    def _all_reduce(self):
        if world()[1] > 1:
            dist.all_reduce(self._flat, op=dist.ReduceOp.SUM)

    def _saved(self):
        return list(self.model.parameters()) + list(self.model.buffers())

    def _after_restore(self):
        for state in self.optimizer.state.values():
            for v in state.values():
                if torch.is_tensor(v):
                    v.zero_()

    def _warm_up(self):
        side = torch.cuda.Stream(device=self.x.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            super()._warm_up()
        torch.cuda.current_stream().wait_stream(side)


def flat_layout(params):
    """Slots of the flat parameter / gradient / optimizer-state buffers: [(offset, count)] per parameter, every
    slot on a 16-byte boundary (the kernels read rows as float4), and the padded total."""
    slices, total = [], 0
    for p in params:
        slices.append((total, p.numel()))
        total += (p.numel() + 3) & ~3
    return slices, total


def all_reduce_flat(flat_g, group=None):
    """The one collective of a data-parallel training step: the flat gradient buffer is summed over the ranks
    as it stands (the 1/ranks is applied by gdn_adam_step's grad_scale).  No-op in a single process."""
    if world()[1] > 1:
        dist.all_reduce(flat_g, op=dist.ReduceOp.SUM, group=group)
    return 1.0 / max(1, world()[1])


class _FlatAdam:
    """What `train()` needs from an optimizer for the batches that do not go through the captured step (the
    ragged last batch of an epoch): zero_grad() / step() over the SAME flat Adam state as the native step."""

    def __init__(self, owner):
        self.owner = owner

    def zero_grad(self, set_to_none: bool = True):
        for p in self.owner.params:
            p.grad = None

    def step(self, grad_scale: float = 1.0):
        """`p.grad` -> the flat gradient buffer -> gdn_adam_step.  The gradients are taken AS THEY ARE: train()
        has already averaged them over the ranks (sync_gradients), so the 1/ranks the captured step folds into
        the optimizer kernel must not be applied a second time here."""
        o = self.owner
        with torch.no_grad():
            for p, (off, cnt) in zip(o.params, o.slices):
                if p.grad is not None:
                    o.flat_g[off:off + cnt].copy_(p.grad.reshape(-1))
                else:
                    o.flat_g[off:off + cnt].zero_()
        o._adam(grad_scale)
        o.model.invalidate_constants()


def _ptr_array(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def _float_array(values):
    return (ctypes.c_float * len(values))(*values)


class NativeTrainStep(_CapturedStep):
    """the step with nothing but this library's kernels between the input batch and the updated
    parameters — no autograd graph, no torch optimizer, no mask tensor.

      * every parameter is a VIEW into one flat fp32 buffer; gradients, Adam's exp_avg / exp_avg_sq are flat
        buffers of the same layout;
      * forward: sensor graph + folded attention terms (they depend on the parameters of this step) ->
        projection -> attention/aggregate (keeps alpha) -> train-mode head with the dropout mask DRAWN in the
        kernels from (seed, step) -> fused MSE loss + its gradient;
      * backward: every kernel writes its parameter gradients straight into their slots of the flat gradient
        buffer (the two shares of the embedding gradient meet in one slot: gdn_terms_bwd_acc), so there is
        no zero_grad, no packing and no unpacking;
      * with several ranks the flat gradient buffer IS the bucket of the one all-reduce (sum; the 1/ranks is
        folded into the optimizer kernel);
      * gdn_adam_step: one launch over the flat buffers, torch.optim.Adam's update.

    Every address a launch takes — workspace, parameter and gradient slots — is fixed in the constructor and looked up
    there once; a launch reads only VALUES (dropout rate, BatchNorm momentum / eps / running statistics, the current
    stream) when it is issued.  BatchNorm uses per-rank batch statistics (standard DDP)."""

    BETAS, EPS = (0.9, 0.999), 1e-8

    @staticmethod
    def applicable(model) -> bool:
        if not (type(model.dp) is nn.Dropout and model._hip_train_head_ok() and model.injected_graph is None
                and next(model.parameters()).is_cuda):
            return False
        n, d = model.embedding.weight.shape
        w = model.gnn_layers[0].gnn.lin.weight.shape[1]
        if not _lib.load().gdn_train_supported(n, w, d, model.topk):     # shape outside the training kernels
            return False
        # out_layer_num > 1: the OutLayer MLP must be one gdn_mlp_train_fwd takes (any row count > 1)
        return model.out_layer_num == 1 or ops.mlp_train_supported(model.out_layer, model.embedding.weight.shape[1], 2)

    def __init__(self, model, batch: int, lr: float = 1e-3, weight_decay: float = 0.0, use_graph: bool = True,
                 split: bool | None = None, seed: int | None = None, wide: bool = False, pre=None, post=None,
                 gaps: bool = False):
        super().__init__(use_graph, split, pre, post)
        self._lib = _lib
        # inputs beyond the 16-bit operand range of the matrix-core kernels: the `_wide` (fp32 row-gather) entry
        # points throughout, decided by the caller from its data (harness.train: first batch / config["wide"])
        self.wide = bool(wide)
        self._sfx = "_wide" if self.wide else ""
        self.model = model.train()
        dev = next(model.parameters()).device
        self.lr, self.wd = float(lr), float(weight_decay)
        self.params = list(model.parameters())
        # flat parameter buffer; every slot starts on a 16-byte boundary (the kernels read rows as float4)
        self.slices, total = flat_layout(self.params)
        self.count = total
        self.flat_p = torch.zeros((total,), dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, (off, cnt) in zip(self.params, self.slices):
                self.flat_p[off:off + cnt].copy_(p.detach().reshape(-1))
                p.data = self.flat_p[off:off + cnt].view(p.shape)
        model.invalidate_constants()
        model._key_tensors = None
        self.flat_g = torch.zeros_like(self.flat_p)
        self.exp_avg = torch.zeros_like(self.flat_p)
        self.exp_avg_sq = torch.zeros_like(self.flat_p)
        if seed is None:
            # derived from torch's seed WITHOUT drawing from the global generator: the loaders' shuffle stream stays
            # the reference's (main.py:221-228 seeds, main.py:128-148 draws)
            seed = (int(torch.initial_seed()) * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & (2 ** 62 - 1)
        self.state = torch.tensor([seed, 0], dtype=torch.int64, device=dev)     # {dropout seed, steps taken}
        self.optimizer = _FlatAdam(self)

        n, d = model.embedding.weight.shape
        w, k = model.gnn_layers[0].gnn.lin.weight.shape[1], model.topk
        self.n, self.d, self.w, self.k, self.batch = n, d, w, k, batch
        lib = _lib.load()
        pitch = ops.nbr_pitch(k)
        f32 = dict(dtype=torch.float32, device=dev)
        self.x = torch.zeros((batch, n, w), **f32)
        self.y = torch.zeros((batch, n), **f32)
        self.loss = torch.zeros((), **f32)
        bn_rows = batch * n
        self.ws = dict(
            topk=torch.empty((n, k), dtype=torch.int64, device=dev),
            nbr=torch.empty((n, pitch), dtype=torch.uint16, device=dev),
            deg=torch.empty((n,), dtype=torch.int32, device=dev),
            rent=torch.empty((n, (n + 15) & ~15), dtype=torch.int32, device=dev),
            rlen=torch.empty((n,), dtype=torch.int32, device=dev),
            terms=torch.empty((128 + 2 * n,), **f32),
            xlin=torch.empty((bn_rows, d), **f32), s_i=torch.empty((bn_rows,), **f32), s_j=torch.empty((bn_rows,), **f32),
            z=torch.empty((bn_rows, d), **f32), alpha=torch.empty((bn_rows, pitch), **f32),
            out=torch.empty((batch, n), **f32), d_out=torch.empty((batch, n), **f32),
            # zero-filled ONCE: the head kernels are told so (buffers_zeroed = 1) and leave them zeroed after every backward
            stats=torch.zeros((lib.gdn_head_train_stats_bytes(d) // 8,), dtype=torch.float64, device=dev),
            head_ws=torch.zeros((lib.gdn_head_train_workspace_bytes(n, d) // 8,), dtype=torch.float64, device=dev),
            d_z=torch.empty((bn_rows, d), **f32), d_xlin=torch.empty((bn_rows, d), **f32),
            d_si=torch.empty((bn_rows,), **f32), d_sj=torch.empty((bn_rows,), **f32),
            proj_ws=torch.empty((lib.gdn_project_bwd_workspace_bytes(n, w, d) // 4,), **f32),
            # [ticket (zero, left zero by every call) | d_bias rows | d_pi tables of shapes beyond LDS, e.g. 512 sensors]
            bwd_ws=torch.zeros((lib.gdn_attn_aggregate_bwd_workspace_bytes(batch, n, d, k) // 4,), **f32),
            d_a=torch.empty((128,), **f32), d_c=torch.empty((2 * n,), **f32),
            mse_ws=ops.mse_workspace(dev),
            head_mse_ws=torch.zeros((lib.gdn_head_mse_workspace_bytes() // 8,), dtype=torch.float64, device=dev),
        )
        self._mlp = None
        if model.out_layer_num > 1:
            hidden, _last = ops.mlp_train_layers(model.out_layer)
            h, layers = hidden[0][0].out_features, len(hidden) + 1
            self._mlp = (h, layers, [bn for _lin, bn in hidden])
            self.ws.update(
                act=torch.empty((bn_rows, d), **f32), d_act=torch.empty((bn_rows, d), **f32),
                mlp_saved=torch.empty((lib.gdn_mlp_train_saved_bytes(bn_rows, d, h, layers),), dtype=torch.uint8, device=dev),
                mlp_ws=torch.empty((lib.gdn_mlp_train_workspace_bytes(bn_rows, d, h, layers),), dtype=torch.uint8, device=dev))
        self._need_reverse = self.wide or bool(lib.gdn_attn_aggregate_bwd_uses_reverse(n, d, k))
        self._side = (torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev))
        self._fork = os.environ.get("GDN_TRAIN_FORK", "0") == "1"
        # GDN_FUSE_MSE=1: loss + d_out from the head's last forward pass (gdn_head_train_fwd_rng_mse) instead of
        # the gdn_mse_loss_grad launch — measured SLOWER (0.198 vs 0.193 ms: 512 workgroups each pay the block
        # reductions and the ticket), so off by default
        self._own_validity(gaps, batch, n, dev)
        self._fuse_mse = os.environ.get("GDN_FUSE_MSE", "0") == "1" and not self.gaps    # (the head's loss knows no mask)

        # the address tables of the launches: workspace and static buffers by name, parameter (P) and gradient (G)
        # slots by parameter name, and the groups the launches take together
        self._pt = {key: t.data_ptr() for key, t in self.ws.items()}
        self._pt.update(x=self.x.data_ptr(), y=self.y.data_ptr(), loss=self.loss.data_ptr(), rng=self.state.data_ptr())
        if self.gaps:
            self._pt.update(valid=self.valid.data_ptr(), row_valid=self.row_valid.data_ptr())
        name_of = {id(p): name for name, p in model.named_parameters()}
        names = [name_of[id(p)] for p in self.params]
        P = self._P = {name: self.flat_p.data_ptr() + 4 * off for name, (off, _c) in zip(names, self.slices)}
        G = self._G = {name: self.flat_g.data_ptr() + 4 * off for name, (off, _c) in zip(names, self.slices)}
        att = ["gnn_layers.0.gnn." + leaf for leaf in ("lin.weight", "att_i", "att_j", "att_em_i", "att_em_j")]
        bn = ["gnn_layers.0.bn.weight", "gnn_layers.0.bn.bias", "bn_outlayer_in.weight", "bn_outlayer_in.bias"]
        last = 0 if self._mlp is None else 3 * (self._mlp[1] - 1)      # the OutLayer's closing Linear
        last = [f"out_layer.mlp.{last}.weight", f"out_layer.mlp.{last}.bias"]
        self._att_p, self._att_g = [P[nm] for nm in att], [G[nm] for nm in att]
        self._bn_p, self._bn_g = [P[nm] for nm in bn], [G[nm] for nm in bn]
        self._last_p, self._last_g = [P[nm] for nm in last], [G[nm] for nm in last]
        if self._mlp is not None:       # the hidden layers' {Linear weight, bias, BatchNorm weight, bias}, as the kernels take them
            hidden = [f"out_layer.mlp.{3 * l + j}.{kind}" for l in range(self._mlp[1] - 1) for j, kind in
                      ((0, "weight"), (0, "bias"), (1, "weight"), (1, "bias"))]
            self._mlp_p, self._mlp_g = _ptr_array([P[nm] for nm in hidden]), _ptr_array([G[nm] for nm in hidden])

    def _bn_run(self, bn):
        if not bn.track_running_stats or bn.running_mean is None:
            return 0.0, None, None, None
        return float(bn.momentum), bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.num_batches_tracked.data_ptr()

    # the first half of a step, stage by stage ------------------------------------------------------------------
    def _forward_backward(self):
        m = self.model
        main = torch.cuda.current_stream()
        st = main.cuda_stream
        p_drop = float(m.dp.p) if m.dp.training else 0.0
        bn1, bn2 = m.gnn_layers[0].bn, m.bn_outlayer_in
        m1, rm1, rv1, nb1 = self._bn_run(bn1)
        m2, rm2, rv2, nb2 = self._bn_run(bn2)
        eps = (float(bn1.eps), float(bn2.eps))
        run = (m1, m2, rm1, rv1, nb1, rm2, rv2, nb2)
        reverse_on = self._graph_terms_project(main, st)
        self._aggregate(st)
        self._head_forward(p_drop, eps, run, st)
        if self._mlp is not None or not self._fuse_mse:
            self._loss(st)
        # backward: gradients land in their slots of flat_g
        self._head_backward(p_drop, eps, st)
        main.wait_stream(reverse_on)                 # reverse lists
        self._aggregate_backward(st)
        self._project_backward_finish(st)
        self._terms_backward(st)

    def _graph_terms_project(self, main, st):
        """Graph + folded attention terms of THIS step's parameters (models/GDN.py:145-165, graph_layer.py:94-104),
        then the projection.  Returns the stream the reverse lists are written on."""
        call, pt, emb = self._lib.call, self._pt, self._P["embedding.weight"]
        n, d, w, k, b = self.n, self.d, self.w, self.k, self.batch
        if not self._fork:
            # graph rows and folded terms in one launch (independent work, one launch less on the critical path)
            call("gdn_topk_graph_terms", emb, n, d, k, pt["topk"], pt["nbr"], pt["deg"], *self._att_p, w, pt["terms"], st)
            if self._need_reverse:       # only the row-gather backward reads the reverse lists
                call("gdn_graph_reverse", pt["nbr"], pt["deg"], n, k, pt["rent"], pt["rlen"], st)
            call("gdn_project_fwd" + self._sfx, pt["x"], self._att_p[0], pt["terms"], b, n, w, d, pt["xlin"],
                 pt["s_i"], pt["s_j"], st)
            return main
        # GDN_TRAIN_FORK=1: three independent chains forked onto side streams (parallel branches of the captured
        # graph): [top-k graph] | [folded terms -> projection] | [reverse lists, needed by the backward only] —
        # measured SLOWER than the serial chain inside a HIP graph (0.235 vs 0.218 ms), so off by default
        side, side2 = self._side
        side.wait_stream(main)
        s2 = side.cuda_stream
        call("gdn_node_terms", *self._att_p, emb, n, d, w, pt["terms"], s2)
        call("gdn_project_fwd" + self._sfx, pt["x"], self._att_p[0], pt["terms"], b, n, w, d, pt["xlin"],
             pt["s_i"], pt["s_j"], s2)
        call("gdn_topk_graph", emb, n, d, k, pt["topk"], pt["nbr"], pt["deg"], None, st)
        side2.wait_stream(main)
        call("gdn_graph_reverse", pt["nbr"], pt["deg"], n, k, pt["rent"], pt["rlen"], side2.cuda_stream)
        main.wait_stream(side)
        return side2

    def _aggregate(self, st):
        pt = self._pt
        self._lib.call("gdn_attn_aggregate_fwd" + self._sfx, pt["xlin"], pt["s_i"], pt["s_j"], pt["nbr"], pt["deg"],
                       self._P["gnn_layers.0.gnn.bias"], self.batch, self.n, self.d, self.k, pt["z"], pt["alpha"], st)

    def _head_forward(self, p_drop, eps, run, st):
        call, pt, emb = self._lib.call, self._pt, self._P["embedding.weight"]
        b, n, d = self.batch, self.n, self.d
        if self._mlp is None and self._fuse_mse:     # the loss and its gradient come out of the head's last forward pass
            call("gdn_head_train_fwd_rng_mse", pt["z"], emb, *self._bn_p, *self._last_p, pt["rng"], p_drop, b, n, d,
                 *eps, *run, pt["stats"], pt["out"], pt["y"], pt["head_mse_ws"], pt["loss"], pt["d_out"], 1, st)
        elif self._mlp is None:
            call("gdn_head_train_fwd_rng", pt["z"], emb, *self._bn_p, *self._last_p, pt["rng"], p_drop, b, n, d,
                 *eps, *run, pt["stats"], pt["out"], 1, st)
        else:
            # out_layer_num > 1: head passes up to the dropped-out activation, then the MLP on the matrix cores
            h, layers, bns = self._mlp
            runs = [self._bn_run(bn) for bn in bns]
            call("gdn_head_train_fwd_act", pt["z"], emb, *self._bn_p, None, None, 1.0, pt["rng"], p_drop, b, n, d,
                 *eps, *run, pt["stats"], pt["act"], 1, st)
            call("gdn_mlp_train_fwd", pt["act"], self._mlp_p, _ptr_array([q for r in runs for q in (r[1], r[2])]),
                 _ptr_array([r[3] for r in runs]), _float_array([float(bn.eps) for bn in bns]),
                 _float_array([r[0] for r in runs]), *self._last_p, b * n, d, h, layers,
                 pt["mlp_saved"], pt["mlp_ws"], pt["out"], st)

    def _loss(self, st):
        pt = self._pt
        if self.gaps:
            self._lib.call("gdn_mse_loss_grad_masked", pt["out"], pt["y"], pt["valid"], pt["row_valid"], self.batch,
                           self.n, pt["mse_ws"], pt["loss"], pt["d_out"], None, st)
            return
        self._lib.call("gdn_mse_loss_grad", pt["out"], pt["y"], self.batch * self.n, pt["mse_ws"], pt["loss"],
                       pt["d_out"], st)

    def _head_backward(self, p_drop, eps, st):
        call, pt, emb, d_emb = self._lib.call, self._pt, self._P["embedding.weight"], self._G["embedding.weight"]
        b, n, d = self.batch, self.n, self.d
        if self._mlp is None:
            # (buffers_zeroed | 2: the head's small finishing reduction runs in the combined tail launch below)
            call("gdn_head_train_bwd_rng", pt["d_out"], pt["z"], emb, *self._bn_p, self._last_p[0], pt["rng"], p_drop,
                 pt["stats"], b, n, d, *eps, pt["head_ws"], pt["d_z"], d_emb, *self._bn_g, *self._last_g, 3, st)
        else:
            h, layers, _bns = self._mlp
            call("gdn_mlp_train_bwd", pt["d_out"], pt["act"], self._mlp_p, self._last_p[0], b * n, d, h, layers,
                 pt["mlp_saved"], pt["mlp_ws"], self._mlp_g, *self._last_g, pt["d_act"], st)
            call("gdn_head_train_bwd_act", pt["d_act"], pt["z"], emb, *self._bn_p, None, None, 1.0, pt["rng"],
                 p_drop, pt["stats"], b, n, d, *eps, pt["head_ws"], pt["d_z"], d_emb, *self._bn_g, 1, st)

    def _aggregate_backward(self, st):
        pt = self._pt
        self._lib.call("gdn_attn_aggregate_bwd" + self._sfx, pt["d_z"], pt["xlin"], pt["alpha"], pt["s_i"], pt["s_j"],
                       pt["nbr"], pt["rent"], pt["rlen"], self.batch, self.n, self.d, self.k, pt["d_xlin"], pt["d_si"],
                       pt["d_sj"], self._G["gnn_layers.0.gnn.bias"], pt["bwd_ws"], st)

    def _project_backward_finish(self, st):
        call, pt, d_lin = self._lib.call, self._pt, self._att_g[0]
        b, n, w, d = self.batch, self.n, self.w, self.d
        if self._mlp is None:
            # partial rows only; their reduction and the head's finishing reduction share ONE launch
            rows = ctypes.c_int(0)
            call("gdn_project_bwd_partials", pt["x"], pt["d_xlin"], pt["d_si"], pt["d_sj"], b, n, w, d,
                 pt["proj_ws"], ctypes.byref(rows), st)
            call("gdn_train_finish", pt["head_ws"], pt["stats"], 1, b, n, d, self._G["embedding.weight"], *self._bn_g,
                 *self._last_g, pt["proj_ws"], rows.value, w, d_lin, pt["d_a"], pt["d_c"], st)
        else:
            call("gdn_project_bwd", pt["x"], pt["d_xlin"], pt["d_si"], pt["d_sj"], b, n, w, d, pt["proj_ws"],
                 d_lin, pt["d_a"], pt["d_c"], st)

    def _terms_backward(self, st):
        pt = self._pt
        self._lib.call("gdn_terms_bwd_acc", *self._att_p, self._P["embedding.weight"], pt["d_a"], pt["d_c"], self.n,
                       self.d, self.w, *self._att_g, self._G["embedding.weight"], 1, st)

    # the second half, and what the scaffold asks ---------------------------------------------------------------
    def _all_reduce(self):
        all_reduce_flat(self.flat_g)

    def _adam(self, grad_scale: float | None = None):
        """gdn_adam_step over the flat buffers; `grad_scale` None = 1/ranks (flat_g holds the all-reduced SUM)."""
        if grad_scale is None:
            grad_scale = 1.0 / max(1, world()[1])
        self._lib.call("gdn_adam_step", self.flat_p.data_ptr(), self.flat_g.data_ptr(), self.exp_avg.data_ptr(),
                       self.exp_avg_sq.data_ptr(), self.state.data_ptr() + 8, self.count, self.lr, self.BETAS[0],
                       self.BETAS[1], self.EPS, self.wd, float(grad_scale), 0, 0,
                       torch.cuda.current_stream().cuda_stream)

    def _update(self):
        self._adam()

    def _saved(self):
        return [self.flat_p, self.exp_avg, self.exp_avg_sq, self.state] + list(self.model.buffers())

    def _after_restore(self):
        self.flat_g.zero_()


def GraphedTrainStep(model, batch: int, lr: float = 1e-3, weight_decay: float = 0.0, use_graph: bool = True,
                     split: bool | None = None, native: bool | None = None, wide: bool | None = None, pre=None,
                     post=None, gaps: bool = False):
    """The captured training step: `NativeTrainStep` when the model and its shape allow it (plain nn.Dropout, an
    OutLayer and a sensor count the training kernels take), else `AutogradTrainStep`.  `native=False` forces the
    autograd form.  `wide`: the inputs exceed the 16-bit operand range (None: model.operand_range == "wide").
    `pre` / `post`: launches issued (and captured) right before and right after the step, see _CapturedStep.
    `gaps=True`: the step also owns `valid` [batch, n] uint8 / `row_valid` [batch] int32 and its loss is
    the mean over the observed targets (gdn_mse_loss_grad_masked; GDN_FUSE_MSE / GDN_TORCH_MSE are ignored); one rank
    only.  False: exactly the launches of a plain step."""
    if native is None:
        native = NativeTrainStep.applicable(model)
    if wide is None:
        wide = getattr(model, "operand_range", "auto") == "wide"
    cls = NativeTrainStep if native else AutogradTrainStep
    extra = {"gaps": True} if gaps else {}
    return cls(model, batch, lr=lr, weight_decay=weight_decay, use_graph=use_graph, split=split, wide=wide, pre=pre,
               post=post, **extra)


# --------------------------------------------------------------------------- epochs from the resident series
def epoch_order(loader) -> torch.Tensor:
    """The dataset positions one epoch of `loader` (a torch DataLoader, num_workers = 0) would yield, as ONE int64
    tensor, drawing from torch's generators exactly what iterating the loader draws: the iterator's base seed
    (torch/utils/data/dataloader.py, _BaseDataLoaderIter.__init__) and then whatever the batch sampler draws (a
    RandomSampler: the seed of its permutation) — so a run that asks for the order sees the same shuffles, and leaves
    the generator in the same state, as a run that iterates.  Milliseconds per epoch instead of per batch: no
    collate of `batch` zero-dimensional tensors."""
    torch.empty((), dtype=torch.int64).random_(generator=loader.generator)
    order = [i for b in loader.batch_sampler for i in b]
    return torch.tensor(order, dtype=torch.int64)


def _window_ticks(source):
    """(target ticks int64 [T], DataLoader or None) of what `train_series` / `Main` hand over: an index loader
    (`main.IndexLoader`: `.loader` over a TensorDataset of window indices, `.windows.starts` their ticks) or a plain
    tensor / sequence of target ticks (trained or scored in the given order, nothing drawn)."""
    if source is None:
        return None, None
    if hasattr(source, "loader") and hasattr(source, "windows"):
        idx = source.loader.dataset.tensors[0]
        starts = source.windows.starts
        return starts[idx.to(starts.device)], source.loader
    return torch.as_tensor(source).to(torch.int64).reshape(-1), None


_VALIDATE_CHUNK_BYTES = 256 << 20       # window buffer of validate_series: a few thousand windows at the usual shapes
_validate_x: dict = {}                  # (device, floats) -> gathered-window buffer, reused across calls


class SeriesFill(NamedTuple):
    """A series with missing readings, held once (`fill_series`): what training and validation share."""
    series: torch.Tensor        # [n, T] fp32, every missing reading at its sensor's latest earlier real one
    raw: torch.Tensor           # [n, T] fp32, the caller's
    valid: torch.Tensor         # [T - w, n] uint8, time-major: row t - w says which readings of tick t are real
    counters: torch.Tensor      # [2, n] int64: missing_total, missing_run over ticks w .. T - 1


def fill_series(raw, w: int) -> SeriesFill:
    """gdn_series_fill ONCE for a training series, after ONE host read: raw[:, :w] must be finite, since
    a missing reading is held at an earlier real one."""
    if raw.dim() != 2 or raw.dtype != torch.float32:
        raise ValueError(f"gaps=True: expected the series [n, T] in fp32, got {tuple(raw.shape)} {raw.dtype}")
    if not bool(torch.isfinite(raw[:, :w]).all()):
        raise ValueError(f"series: its first {w} ticks hold a value that is not finite; with gaps=True every missing "
                         "reading is held at an earlier real one, so the series must begin on real readings")
    raw = ops._chk(raw, name="series")
    filled, _gt, valid, _keep, counters = ops.series_fill(raw, w)
    return SeriesFill(filled, raw, valid, counters)


def masked_share(valid, starts, w: int) -> float:
    """The share of the targets of the windows `starts` (target ticks) that are missing: ONE host read."""
    starts = torch.as_tensor(starts).to(torch.int64).reshape(-1).to(valid.device)
    if starts.numel() == 0:
        return 0.0
    return 1.0 - float(valid[starts - w].float().mean())


def validate_series(model, series, starts, batch: int, wide=None, valid=None):
    """harness.test's loss and outputs for the windows of target ticks `starts` of a series [n, T] resident on the
    device, with nothing but launches per chunk: (val_loss, pred [Tv, n], gt [Tv, n]).

    A chunk (a multiple of `batch`, a few thousand windows — eval results do not depend on the minibatch) is cut by
    ONE gdn_windows_gather into a cached buffer, its targets straight into their rows of `gt`, and goes through
    `model.forward_into` into its rows of `pred`; ONE gdn_mse_batch_means then forms F.mse_loss of every logical
    minibatch and test.py's sum(losses) / len(losses), and one float64 comes back to the host.  An OutLayer the fast
    path refuses (GDN.mlp_fast_path_supported) goes through `model(x)` on the gathered chunk.

    `valid`: the validity plane [T - w, n] uint8 of `series`, which is then the FILLED series
    (`fill_series`).  Each chunk's gather also cuts its validity rows and gdn_mse_batch_means_masked closes the pass:
    a minibatch's loss is the mean over its observed targets, a minibatch without one is left out of the average, and
    the result is 0.0 when none has one.  `pred` / `gt` are what the call without `valid` returns."""
    model.eval()
    series = ops._chk(series, name="series")
    n, series_len = series.shape
    w = model.gnn_layers[0].gnn.lin.weight.shape[1]
    dev = series.device
    starts = ops.check_window_table(starts, w, series_len).to(dev).contiguous()
    tv = int(starts.numel())
    pred = torch.empty((tv, n), dtype=torch.float32, device=dev)
    gt = torch.empty((tv, n), dtype=torch.float32, device=dev)
    if tv == 0:
        return 0.0, pred, gt
    if wide is None:
        wide = model.wide_for(series)
    fast = model.out_layer_num == 1 or model.mlp_fast_path_supported()
    per_window = n * w * 4
    chunk = max(1, min(4096, _VALIDATE_CHUNK_BYTES // per_window) // batch) * batch
    chunk = min(chunk, (tv + batch - 1) // batch * batch)
    key = (dev, chunk * n * w)
    xbuf = _validate_x.get(key)
    if xbuf is None:
        xbuf = _validate_x[key] = torch.empty((chunk * n * w,), dtype=torch.float32, device=dev)
    if valid is not None:
        vrows = torch.empty((tv, n), dtype=torch.uint8, device=dev)
        row_valid = torch.empty((chunk,), dtype=torch.int32, device=dev)
    for s in range(0, tv, chunk):
        rows = min(chunk, tv - s)
        x = xbuf[: rows * n * w].view(rows, n, w)
        if valid is None:
            ops.windows_gather(series, starts, rows, w, x, gt[s:s + rows], first=s)
        else:
            ops.windows_gather(series, starts, rows, w, x, gt[s:s + rows], first=s, valid=valid,
                               valid_out=vrows[s:s + rows], row_valid=row_valid)
        if fast:
            model.forward_into(x, pred[s:s + rows], wide=wide)
        else:
            with pinned_range(model, wide), torch.no_grad():
                pred[s:s + rows].copy_(model(x, None))
    if valid is not None:
        mean = ops.mse_batch_means(pred, gt, batch, valid=vrows)[1]
    else:
        _means, mean = ops.mse_batch_means(pred, gt, batch)
    return float(mean.item()), pred, gt


class SeriesTrainer:
    """An epoch of harness.train as `len(order) // batch` graph replays with no host work between them.

    Owns a `GraphedTrainStep` whose `pre` hook is ONE gdn_windows_gather launch — it reads the cursor and cuts the
    step's windows from the resident series straight into the step's static `x` / `y` — and whose `post` hook is
    gdn_epoch_advance (the step's loss into its row of the loss table, the cursor on); the device copy of the epoch's
    table of target ticks (capacity fixed here, so the pointers a captured graph holds stay valid); the cursor; the
    loss table.  `train_starts`: the target tick of every training window (SeriesWindows.starts[train indices]).

    `gaps=True`: `series` is the RAW series and may hold missing readings (values that are not finite)
    after its first `w` ticks.  The constructor holds them once (`fill_series`; `fill=` hands over a fill already
    done): `.series` is the filled series every window and target is cut from, `.raw_series` the caller's, `.valid`
    the validity plane, `.status_gaps()` the counters.  The gather hook also cuts the validity bytes of the step's
    targets into the step's `valid` / `row_valid`, and the step's loss is the mean over the observed targets.  On a
    finite series an epoch writes the bits of gaps=False; gaps=False issues the launches it did."""

    def __init__(self, model, series, w: int, train_starts, batch: int, lr: float = 1e-3, weight_decay: float = 0.0,
                 wide: bool = False, use_graph: bool = True, native: bool | None = None, gaps: bool = False,
                 fill: SeriesFill | None = None):
        self.gaps = bool(gaps)
        self.raw_series = self.valid = self._gap_counters = None
        if self.gaps:
            fill = fill_series(series, int(w)) if fill is None else fill
            series, self.raw_series, self.valid, self._gap_counters = fill
        elif fill is not None:
            raise ValueError("fill= is the held series of gaps=True")
        self.series = ops._chk(series, name="series")
        dev = self.series.device
        self.model, self.w, self.batch, self.wide = model, int(w), int(batch), bool(wide)
        self.train_starts = ops.check_window_table(train_starts, self.w, self.series.shape[1]).to(dev)
        cap = int(self.train_starts.numel())
        self.full_steps = cap // self.batch
        self.table = torch.zeros((max(1, cap),), dtype=torch.int64, device=dev)
        self.cursor = torch.zeros((1,), dtype=torch.int64, device=dev)
        self.loss_table = torch.zeros((self.full_steps + 1,), dtype=torch.float32, device=dev)
        self._tail = None                                # (x, y) of the ragged last batch, by its size
        self.step = GraphedTrainStep(model, self.batch, lr=lr, weight_decay=weight_decay, use_graph=use_graph,
                                     native=native, wide=self.wide, pre=self._gather, post=self._advance, gaps=self.gaps)
        self.optimizer = self.step.optimizer
        self._mse_ws = ops.mse_workspace(dev) if self.gaps else None     # the ragged tail's masked launch

    # the hooks: static arguments only (they are captured with the step)
    def _gather(self):
        # (count = the table's capacity: a captured launch cannot learn an epoch's length, and epoch() replays exactly
        # len(order) // batch times, so no replay reaches an entry beyond the epoch)
        if self.gaps:
            ops.windows_gather(self.series, self.table, self.batch, self.w, self.step.x, self.step.y, cursor=self.cursor,
                               valid=self.valid, valid_out=self.step.valid, row_valid=self.step.row_valid)
            return
        ops.windows_gather(self.series, self.table, self.batch, self.w, self.step.x, self.step.y, cursor=self.cursor)

    def _advance(self):
        ops.epoch_advance(self.step.loss, self.cursor, self.loss_table)

    def status_gaps(self):
        """(missing_total [n] int64, missing_run [n] int64) on the host, gaps=True only: every sensor's missing readings
        among ticks w .. T - 1 of the series and the run of them that ends at the last tick.  ONE read."""
        return _status_gaps(self._gap_counters, self.gaps, "trainer")

    def _masked_tail_step(self, x, y, valid, row_valid):
        """The ragged last batch under gaps=True: `_eager_step` with the masked launch in F.mse_loss's place — autograd
        starts from d_out — and the same sync_gradients / optimizer calls.  Returns the loss (a device scalar)."""
        self.optimizer.zero_grad()
        out = self.model(x, None)
        loss, d_out = ops.mse_loss_grad(out.detach(), y, self._mse_ws, valid=valid, row_valid=row_valid)
        out.backward(d_out)
        sync_gradients(self.model)
        self.optimizer.step()
        return loss

    def epoch(self, order) -> list:
        """Train on windows train_starts[order] in that order; returns the step losses (ONE device-to-host read)."""
        order = torch.as_tensor(order).to(torch.int64).reshape(-1)
        total = int(order.numel())
        if total > self.table.numel():
            raise ValueError(f"an epoch of {total} windows on a trainer built for {self.table.numel()}")
        if total and (int(order.min()) < 0 or int(order.max()) >= self.train_starts.numel()):
            raise ValueError(f"window positions outside [0, {self.train_starts.numel()})")
        dev = self.series.device
        self.table[:total].copy_(self.train_starts[order.to(dev)])
        full, rest = divmod(total, self.batch)
        self.model.train()
        # the warm-up steps of the capture run on this epoch's first windows and move the cursor: capture first, then
        # put the cursor at the epoch's start
        if full:
            self.step.prepare()
        self.cursor.zero_()
        for _ in range(full):
            self.step.step()
        steps = full
        if rest:
            # the ragged last batch: today's eager branch of harness.train on windows the same kernel gathered
            if self._tail is None or self._tail[0].shape[0] != rest:
                n = self.series.shape[0]
                self._tail = (torch.empty((rest, n, self.w), dtype=torch.float32, device=dev),
                              torch.empty((rest, n), dtype=torch.float32, device=dev))
                if self.gaps:
                    self._tail += (torch.empty((rest, n), dtype=torch.uint8, device=dev),
                                   torch.empty((rest,), dtype=torch.int32, device=dev))
            x, y = self._tail[:2]
            if self.gaps:
                ops.windows_gather(self.series, self.table, rest, self.w, x, y, first=full * self.batch, count=total,
                                   valid=self.valid, valid_out=self._tail[2], row_valid=self._tail[3])
                with pinned_range(self.model, self.wide):
                    self.loss_table[full].copy_(self._masked_tail_step(*self._tail))
            else:
                ops.windows_gather(self.series, self.table, rest, self.w, x, y, first=full * self.batch, count=total)
                with pinned_range(self.model, self.wide):
                    self.loss_table[full].copy_(_eager_step(self.model, self.optimizer, x, y))
            steps += 1
        return self.loss_table[:steps].tolist() if steps else []


def train_series(model=None, save_path="", config=None, series=None, w: int | None = None, train_loader_or_indices=None,
                 val_starts=None, use_graph: bool | None = None, gaps: bool | None = None,
                 fill: SeriesFill | None = None):
    """harness.train's loop (same optimizer, loss, `wide` decision, checkpoint rule, 15-epoch early stop, returned
    list of step losses) for a series [n, T] resident on the device: every epoch is one upload of the window table and
    a run of graph replays (SeriesTrainer), every validation pass `validate_series`.

    `train_loader_or_indices` / `val_starts`: an index loader (`main.IndexLoader`) — its DataLoader is asked for the
    epoch's order (`epoch_order`: the shuffles and the generator's state are those of a run that iterates it, the
    validation loader's per-epoch draw included) — or a tensor of target ticks, taken in the given order.
    `use_graph` None: config["hip_graph"], default True.  One process only.

    `gaps` (None: config["train_gaps"], default False): `series` may hold missing readings (values that
    are not finite) after its first `w` ticks.  They are held ONCE (`fill_series`, or the `fill=` of a caller that has
    done it); the `wide` decision looks at the filled series; the trainer and every validation pass cut windows,
    targets and validity bytes from that one fill, and every loss is the mean over the observed targets."""
    if world()[1] > 1:
        raise _lib.GdnHipError("train_series runs in one process: sharding an epoch of the resident series across ranks is "
                          "not implemented (harness.train with per-rank loaders does data-parallel training)")
    config = config or {}
    if use_graph is None:
        use_graph = bool(config.get("hip_graph", True))
    w = int(w if w is not None else model.gnn_layers[0].gnn.lin.weight.shape[1])
    if gaps is None:
        gaps = bool(config.get("train_gaps", False))
    raw, plane = series, None
    if gaps:
        fill = fill_series(raw, w) if fill is None else fill
        series, plane = fill.series, fill.valid
    elif fill is not None:
        raise ValueError("fill= is the held series of gaps=True")
    train_starts, train_loader = _window_ticks(train_loader_or_indices)
    val_ticks, val_loader = _window_ticks(val_starts)
    batch = int(train_loader.batch_size if train_loader is not None else config.get("batch", 128))
    val_batch = int(val_loader.batch_size if val_loader is not None else batch)
    range_before = getattr(model, "operand_range", "auto")
    wide = config.get("wide", None)
    if range_before != "auto":
        wide = range_before == "wide"
    elif wide is None:
        # the resident series is there to be looked at: all of it, not the first batch (the weights move: margin)
        wide = model.train().input_exceeds_limit(series, margin=16.0)
    trainer = None
    losses, best = [], _BestSoFar()
    for _epoch in range(config.get("epoch", 1)):
        order = epoch_order(train_loader) if train_loader is not None else torch.arange(train_starts.numel())
        if trainer is None:
            extra = {"gaps": True, "fill": fill} if gaps else {}
            trainer = SeriesTrainer(model, raw, w, train_starts, min(batch, max(1, int(train_starts.numel()))),
                                    lr=0.001, weight_decay=config.get("decay", 0), wide=wide, use_graph=use_graph, **extra)
        step_losses = trainer.epoch(order)
        losses.extend(step_losses)
        val_loss = None
        if val_ticks is not None:
            if val_loader is not None:
                epoch_order(val_loader)                  # what iterating the validation loader draws
            val_loss = (validate_series(model, series, val_ticks, val_batch, valid=plane)[0] if gaps else
                        validate_series(model, series, val_ticks, val_batch)[0])
        if best.update(val_loss, float(sum(step_losses)), model, save_path):
            break
    return losses


# --------------------------------------------------------------------------- streaming detector
_STREAM_MAX_CHUNK = 4096                # ticks per push: validate_series' cap on windows per launch


def raw_push_plan(pending: int, r: int, down: int, chunk: int) -> list:
    """The sub-pushes of `r` raw ticks handed to a prep= detector that holds `pending` < down raw ticks of an open
    group: a list of (raw_rows, groups, new_pending, replayable).  A sub-push carries at most chunk * down - pending
    raw ticks, so it completes at most `chunk` model ticks and a long push reaches a group boundary with its first
    sub-push; groups = (pending + raw_rows) // down model ticks are scored, new_pending raw ticks stay open.
    replayable: the sub-push starts on a group boundary and carries exactly chunk * down raw ticks (the captured
    graph's shape).  Pure host arithmetic."""
    if down < 1 or chunk < 1 or r < 0 or not 0 <= pending < down:
        raise ValueError(f"raw_push_plan: pending = {pending}, r = {r}, down = {down}, chunk = {chunk}")
    plan = []
    while r > 0:
        rows = min(r, chunk * down - pending)
        groups, left = divmod(pending + rows, down)
        plan.append((rows, groups, left, pending == 0 and rows == chunk * down))
        pending, r = left, r - rows
    return plan


def events_config(events, m: int) -> dict:
    """StreamDetector's events=dict(on=, off=, lo=, cap=) checked on the host and completed: {"on", "off", "cap", "m",
    "lo"} with on = off = 1, cap = 4096 and lo = None (the raise level) by default; an unknown key is refused by name."""
    unknown = sorted(set(events) - {"on", "off", "lo", "cap"})
    if unknown:
        raise ValueError(f"events: unknown key {unknown[0]!r} (on, off, lo, cap)")
    _, lo, on, off, cap = ops.episodes_check(None, events.get("lo"), events.get("on", 1), events.get("off", 1),
                                             events.get("cap", 4096))
    return {"on": on, "off": off, "cap": cap, "m": int(m), "lo": lo}


def _check_stream_head(model):
    """The refusal StreamDetector and StreamFleet share: an OutLayer that forward_into has no kernel for."""
    if model.out_layer_num > 1 and not ops.mlp_fast_tail_supported(model.out_layer, model.embedding.weight.shape[1]):
        raise model._refusal("refuse_outlayer")            # (GDN.mlp_fast_path_supported's answer, from host facts)


def _seed_ring(ring_keys, ring_keep, pred, gt, keep=None, valid=None):
    """Seed the ring (ring_keys [n, R], ring_keep [R]) of a stream or of one unit of a fleet: the keys of the last
    s = min(R, t) rows of a period normal by declaration, oldest first, into slots R - s .. R - 1 with keep = 1 (no
    alarm is excluded): the stream starts at slot 0, so it overwrites the empty slots first and the oldest seeded tick
    last.  `keep` [t] uint8 (a calibration with missing readings): a tick that is not complete gets the filler and
    keep = 0, as gdn_stream_calib_write_gaps would have left it.  `valid` [t, n] uint8 (calib="sensor") takes keep's
    place: every tick is kept and the filler sits in the keys of its missing readings, as
    gdn_stream_calib_write_sensor would have left it."""
    R = ring_keep.shape[0]
    s = min(R, pred.shape[0])
    if valid is not None:
        keys, keep = ops.score_keys(pred[-s:], gt[-s:], s, valid=valid[-s:]), None
    else:
        keys = ops.score_keys(pred[-s:], gt[-s:], s, keep=None if keep is None else keep[-s:])
    if keep is None:
        ring_keep[R - s:].fill_(1)
    else:
        ring_keep[R - s:].copy_(keep[-s:])
    ring_keys[:, R - s:].copy_(keys)


def _episodes(events, m: int, cap: int) -> Episodes:
    """The episode table of one events allocation (a stream's, or one unit's block of a fleet's), as views."""
    carry, start, end, peak_tick, peak, sensors = ops.stream_events_views(events, m, cap)
    return Episodes(start, end, peak, peak_tick, sensors, carry[:1])


def _check_calib_gaps(calib, calib_gaps):
    if calib == "sensor" and not calib_gaps:
        raise ValueError("calib='sensor' calibrates every sensor on its own real readings: pass calib_gaps=True "
                         "(and gaps=True) too")


def _check_calib_period(series, calib_gaps, gaps, who: str):
    """What the two from_calibration refuse about gaps= / calib_gaps= and the period, by name (`who`: what is built)."""
    if calib_gaps and not gaps:
        raise ValueError(f"calib_gaps=True calibrates under the rules of a gaps=True {who}: pass gaps=True too")
    if gaps and not calib_gaps and isinstance(series, torch.Tensor) and not bool(torch.isfinite(series).all()):
        raise ValueError("series: the calibration period holds a value that is not finite; gaps=True fills the "
                         "stream, not the calibration (fill or cut the period first)")


def _calibrate_period(model, series, w: int, batch: int, calib_gaps: bool, min_kept: int, calib: str, seed: bool):
    """ONE SeriesEvaluator step over a period `series` [n, T > w] known to be normal: (med_iqr, threshold = the period's
    largest anomaly score, the period's — with calib_gaps: the FILLED period's — last w ticks, kept, counts, and with
    `seed` the rows a ring is seeded from: (pred, y, keep, valid under calib="sensor"), else None).  Views of the
    evaluator's tensors."""
    if calib_gaps:
        ev = SeriesEvaluator(model, None, None, batch=batch, use_graph=False, series=series, gaps=True,
                             min_kept=min_kept, calib=calib)
    else:
        ev = SeriesEvaluator(model, None, series[:, w:].t().contiguous(), batch=batch, use_graph=False, series=series)
    threshold = ev.step().max()
    rows = (ev.pred, ev.y, ev.keep, ev.valid if calib == "sensor" else None) if seed else None
    return ev.med_iqr, threshold, ev.series[:, -w:], ev.kept, ev.counts, rows


class _StreamCore:
    """What StreamDetector and StreamFleet state once on the host: the rules of the options they share, the static
    buffers of a push under a leading shape (() for a stream, (units,) for a fleet), the question whether the forward
    is the guarded launch, and recal_every's clock.  The wording that differs between the two comes from the caller."""

    def _set_calib(self, calib, gaps, recal):
        _check_calib(calib)
        if calib == "sensor" and not (gaps and int(recal) > 0):
            raise ValueError("calib='sensor' recalibrates every sensor on its own real readings: it needs gaps=True and "
                             "a calibration ring (recal=R)")
        self.calib = calib

    def _check_lists(self, top_m, log, entries: str):
        _check_top_m(top_m, self.n)
        if int(log) < 0:
            raise ValueError(f"log = {log}: the alarm log holds 0 or more {entries}")

    def _set_recal(self, recal, exclude_alarms, recal_every, recal_min, ring_bytes, no_ring: str):
        """recal, exclude_alarms, recal_every and recal_min (default max(64, R // 4)): host facts only.  `ring_bytes()`
        asks the library for the size of the ring(s), 0: none for this shape, refused with `no_ring`."""
        self.recal, self.exclude_alarms, self.recal_every = int(recal), bool(exclude_alarms), int(recal_every)
        self.recal_min = 0
        if self.recal_every < 0 or (self.recal_every and not self.recal):
            raise ValueError(f"recal_every = {recal_every}: recalibrating every so many ticks needs a calibration ring "
                             "(recal=R) and a positive number of ticks")
        if self.recal:
            if self.recal < self.chunk:
                raise ValueError(f"recal = {recal}: the calibration ring must hold at least one push of chunk = "
                                 f"{self.chunk} ticks (no two rows of a push may share a slot)")
            if ring_bytes() <= 0:
                raise ValueError(f"recal = {recal}: {no_ring}")
            self.recal_min = max(64, self.recal // 4) if recal_min is None else int(recal_min)
            if not 1 <= self.recal_min <= self.recal:
                raise ValueError(f"recal_min = {recal_min}: between 1 and recal = {self.recal} kept ticks")
        elif recal_min is not None:
            raise ValueError(f"recal_min = {recal_min}: there is no calibration ring (recal = 0)")

    def _set_recal_threshold(self, recal_threshold):
        """recal_threshold (None: off, else the margin on the ring's largest score): host facts only."""
        self.recal_threshold = None
        self.ring_peak = self.ring_eligible = self.ring_peak_slot = self.clear_frac = self._thr_ws = None
        if recal_threshold is not None:
            if not self.recal:
                raise ValueError(f"recal_threshold = {recal_threshold!r}: re-deriving the threshold needs a calibration "
                                 "ring (recal=R)")
            self.recal_threshold = ops.check_ring_margin(recal_threshold, "recal_threshold")

    def _margin(self, threshold):
        """recalibrate()'s `threshold` as a margin or None (the table only): None is the constructor's setting, False
        the table only, a number a one-off margin (refused by name when it is not finite or <= 0)."""
        if threshold is None:
            return getattr(self, "recal_threshold", None)   # (an object put together without the constructor: off)
        if threshold is False:
            return None
        return ops.check_ring_margin(threshold, "threshold")

    def _ring_buffers(self):
        """The outputs and the workspace of the threshold step, allocated at its first use (a detector that never asks
        for it allocates and launches nothing): `ring_peak`, `ring_eligible`, `ring_peak_slot` per unit, and with
        episodes `clear_frac` = lo / threshold as they stand (1 where that is not a number or exceeds 1, so that the
        clear level never rises above the threshold)."""
        units, dev = getattr(self, "units", 1), self.state.device
        if self.ring_peak is None:
            self.ring_peak = torch.full((units,), float("-inf"), dtype=torch.float64, device=dev)
            self.ring_eligible = torch.zeros((units,), dtype=torch.int32, device=dev)
            self.ring_peak_slot = torch.full((units,), -1, dtype=torch.int32, device=dev)
            self._thr_ws = ops.fleet_ring_threshold_workspace(units, self.recal, dev)
        if self.clear_frac is None and self.events is not None:
            frac = self.clear.view(-1) / self.threshold.view(-1)
            self.clear_frac = torch.where(torch.isfinite(frac) & (frac <= 1.0), frac, torch.ones_like(frac))

    def _ring_threshold(self, margin: float, select=None):
        """The threshold step after a table rewrite: two launches, no host read (ops.fleet_ring_threshold); a single
        stream is the fleet of one unit.  min_eligible is recal_min."""
        if not isinstance(self.threshold, torch.Tensor):
            raise ValueError("threshold: the device scalar the captured graph reads was replaced by a plain number; "
                             "write into it (det.threshold[0] = value) and it can be re-derived in place")
        self._ring_buffers()
        n, R = self.n, self.recal
        ops.fleet_ring_threshold(self.state, self.ring_keys.view(-1, n, R), self.ring_keep.view(-1, R),
                                 self.med_iqr.view(-1, n, 2), self.w, margin, self.recal_min, self._thr_ws,
                                 self.threshold.view(-1), self.ring_peak, self.ring_eligible, self.ring_peak_slot,
                                 select=select, clear_frac=self.clear_frac,
                                 clear=None if self.clear_frac is None else self.clear.view(-1),
                                 by_sensor=self.calib == "sensor")

    def _alloc_push(self, lead: tuple, log, dev):
        """The static buffers of a push, zeros: per stream under `lead` = (), per unit under (units,)."""
        c, n, w, m = self.chunk, self.n, self.w, self.top_m

        def zeros(shape, dtype):
            return torch.zeros(lead + shape, dtype=dtype, device=dev)
        self.chunk_buf = zeros((c, n), torch.float32)
        self.x = zeros((c, n, w), torch.float32)
        self.pred = zeros((c, n), torch.float32)
        self.top_scores = zeros((c, m), torch.float64)
        self.top_sensors = zeros((c, m), torch.int32)
        self.alarm = zeros((c,), torch.int32)
        self.log_ticks = zeros((int(log),), torch.int64) if log else None
        self.log_sensors = zeros((int(log), m), torch.int32) if log else None
        self.raw_buf = self.valid = self.gap_chunk = self.gaps = None
        if self.with_gaps:
            self.raw_buf = zeros((c, n), torch.float32)
            self.valid = zeros((c, n), torch.uint8)
            self.gap_chunk = zeros((2, n), torch.int32)
            self.gaps = zeros((2, n), torch.int64)                   # missing_total, missing_run

    # the launches of a push take static arguments only (they are captured)
    def _guarded(self) -> bool:
        m = self.model
        if self.wide or m.operand_range != "auto" or m.out_layer_num != 1:
            return False
        c = m._constants()
        return not c.large and m._plan(c, False) is not None

    def _hand(self, ticks: int):
        """recal_every's clock: `ticks` more model ticks were handed over; recalibrate when they cross a multiple of it."""
        before, self._handed = self._handed, self._handed + ticks
        if self.recal_every and self._handed // self.recal_every > before // self.recal_every:
            self.recalibrate()

    # save and resume: what the two classes share around their `_ckpt_tensors()` — checkpoint key -> the
    # device tensor (a view) that holds it, for the options the object was built with
    def _config(self) -> dict:
        cfg = {"units": self.units} if hasattr(self, "units") else {}
        cfg.update({"n": self.n, "w": self.w, "chunk": self.chunk, "top_m": self.top_m,
                    "log": 0 if self.log_ticks is None else self.log_ticks.shape[-1], "with_gaps": int(self.with_gaps),
                    "recal": self.recal, "exclude_alarms": int(self.exclude_alarms), "recal_every": self.recal_every,
                    "recal_min": self.recal_min, "calib": self.calib, "wide": int(self.wide),
                    "prep": int(self.prep is not None), "prep_down": 0 if self.prep is None else self.prep.down})
        return cfg

    def _ckpt_read(self, dev: dict) -> tuple:
        """({key: numpy array} of the device tensors `dev`, the model's fingerprint): ONE batch of non-blocking copies on
        the current stream, the model's tensors included, and ONE synchronisation."""
        weights = self.model.state_dict()
        names = sorted(weights)
        host = _host_copies(list(dev.values()) + [weights[k] for k in names])
        torch.cuda.current_stream().synchronize()
        return {k: t.numpy() for k, t in zip(dev, host)}, _fingerprint(names, host[len(dev):])

    def _ckpt_finish(self, sd: dict, ints: dict, keys: tuple, cfg: dict, fingerprint: str) -> dict:
        """`sd` completed by what lives on the host: the empty log of log=0, the shared optional keys, the 0-d ints
        `keys` (from `ints` and the configuration `cfg`) and the two strings."""
        if self.log_ticks is None:
            lead = (cfg["units"],) if "units" in cfg else ()
            sd["log_ticks"] = np.zeros(lead + (0,), np.int64)
            sd["log_sensors"] = np.zeros(lead + (0, self.top_m), np.int32)
        if self.recal_threshold is not None:
            sd["recal_threshold"] = np.array(self.recal_threshold, dtype=np.float64)
        if self.events is not None:
            sd["events_cfg"] = np.array([self.events_cfg[k] for k in _EVENTS_FIELDS], dtype=np.int64)
        ints = dict(ints, **{k: v for k, v in cfg.items() if k != "calib"})
        sd.update({k: np.array(int(ints[k]), dtype=np.int64) for k in keys})
        sd["calib"], sd["model_sha256"] = np.array(self.calib), np.array(fingerprint)
        return sd

    def _ckpt_same_config(self, cfg: dict, who: str, noun: str) -> None:
        """The file's configuration `cfg` against this object's own, field by field: refused before any device work."""
        for k, mine in self._config().items():
            if cfg[k] != mine:
                raise ValueError(f"{who}: {k} = {cfg[k]!r}, this {noun} was built with {k} = {mine!r}")

    def _ckpt_fill(self, sd):
        """The body of load_state_dict after the checks: the captured graphs dropped, every array of `_ckpt_tensors()`
        copied INTO the allocation that holds it.  `clear_frac` and `calib_counts` come into being from the file: the
        fractions behind the clear levels are the file's, else (at their next use) those of the levels just loaded.
        Returns the reader of `sd`'s arrays."""
        for full in (self._full, *self._prep_full.values()):
            full.drop()

        def host(key):
            return torch.from_numpy(np.array(sd[key]))      # (a copy: numpy.load may hand out read-only arrays)
        self.clear_frac = self.calib_counts = None
        for k, t in self._ckpt_tensors().items():
            t.copy_(host(k))
        self.clear_frac = host("clear_frac").to(self.state.device) if "clear_frac" in sd else None
        self.calib_counts = host("calib_counts").to(self.state.device) if "calib_counts" in sd else None
        self._last = 0
        return host


class StreamDetector(_StreamCore):
    """Scores ticks as they arrive against a frozen calibration, with nothing but launches per push.

    The stream's state lives on the device (include/gdn_hip.h "streaming detector"): the last w ticks of every sensor,
    the float64 smoothing carry, the tick / alarm counters and the alarm log.  A push of `chunk` ticks is ONE copy
    into the static chunk buffer and ONE replay of a graph captured once: gdn_stream_windows (the chunk's windows cut
    from history + chunk) -> model.forward_into -> gdn_stream_score (gdn_score_smooth_topm's arithmetic at the
    stream's position, flags against the threshold) -> gdn_stream_advance (the only writer of the state).  A shorter
    push issues the same launches eagerly with count = its ticks; a longer one is split.  No host synchronisation.

    The stream equals harness.SeriesEvaluator(top_m=...) with this `med_iqr` on [history[:, -w:] | stream]: the same
    windows, the same forward, the same float64 scoring bit for bit.

    `med_iqr` [n, 2] float64 and `threshold` (a number or a device float64 scalar) come from a period known to be
    normal (`from_calibration`); `history` [n, h >= w] fp32 holds the ticks before the stream (a cold start is
    refused).  `top_m` sensors per tick are kept (1 .. 8); `log` alarm entries are kept (0: no log).  `wide`: None asks
    model.wide_for(history) once, True / False is the caller's word; under operand_range == "auto" on the planned
    matrix-core route the forward is the guarded launch, which redoes an out-of-range push in fp32 on the device.

    `gaps=True` gives the detector a notion of a missing reading: a pushed value that is not finite
    (NaN, +inf, -inf).  The push lands in `raw_buf` and gdn_stream_fill leads the launches: it holds every missing
    reading at its sensor's latest real one (`chunk_buf` is then the FILLED chunk, which windows, forward, score, hist
    and localise() read) and writes the validity plane `valid` [chunk, n] uint8 (`valid[:r]` describes the last
    push).  The score and advance launches are their `_gaps` variants: the normalised error of a missing reading is
    exactly 0.0, so a dropped reading neither raises nor blinds the four ticks its error would sit in.
    `status_gaps()` reads the per-sensor counters.  `history[:, -w:]` must be finite.  With no missing reading the
    detector writes the bits a gaps=False detector writes; gaps=False issues exactly the launches it always did.

    `recal=R` gives the detector a calibration ring on the device: `ring_keys` [n, R] float64 holds the
    scoring keys |pred - gt| of the last R stream ticks (tick t in slot t mod R), `ring_keep` [R] uint8 which of them
    count.  gdn_stream_calib_write sits between the score and the advance launch (captured with them): a tick is kept
    unless it alarmed (`exclude_alarms`, default True) or — gaps=True — a reading of it was missing.  `recalibrate()`
    overwrites `med_iqr` IN PLACE with the median / IQR of the kept ticks (one gdn_score_select straight from the
    ring; the captured graph reads the table through the same pointer and stays) once `recal_min` ticks are kept
    (default max(64, R // 4)); `threshold` (IQR-normalised units) and the carry are not touched.  `recal_every=E`:
    `push` calls `recalibrate()` after every sub-push that crosses a multiple of E handed ticks.  `from_calibration`
    seeds the ring with the last min(R, T - w) calibration ticks.  The ring writer only reads the stream: a recal=R
    detector that never recalibrates writes the bits of a recal=0 one; recal=0 issues exactly the launches it did.

    `calib="sensor"` (needs gaps=True and recal=R) keeps a tick with missing readings in the ring: the
    ring write is gdn_stream_calib_write_sensor, which puts the filler into the keys of the missing readings only.
    `recalibrate()` then counts every sensor's real keys on the device and rewrites the row of every sensor that has
    at least `recal_min` of them; a dead sensor keeps its row and no longer stops the others.  The default "tick" is
    the rule above, launch for launch.

    `recal_threshold=margin` (needs recal=R; None: off) makes a recalibration whole: whenever
    `recalibrate()` has rewritten the table it also rewrites `threshold` IN PLACE — a number in units of that table —
    as margin times the largest smoothed score the ring supports under the new table (the rule of `from_calibration`,
    over the ticks whose four-tick window the ring holds whole, if at least `recal_min` are), and with events= the
    clear level as the new threshold times `clear_frac` (lo / threshold at construction).  Two more launches, no
    host read, no recapture.  `recalibrate(threshold=...)` overrides it once.  With exclude_alarms=True the ring holds
    no tick that alarmed, so only a change of table or a margin above 1 raises the threshold.

    `prep=Prep` puts the raw-readings front end on the device: `push()` then takes RAW ticks [r, n], fp32
    or float64, in engineering units at the raw rate, and gdn_prep_ticks leads the launches: it normalises every
    reading with the Prep's min-max table and writes the median of each completed group of `prep.down` raw ticks as
    one model tick into `raw_buf` (gaps=True; a group with no finite reading is a missing reading) or `chunk_buf`.
    The raw ticks of an open group wait in two float64 planes on the device that alternate (`raw_pending` counts
    them on the host).  `chunk`, `recal_every`, `history`, the counters and the log stay in model ticks; a sub-push
    carries up to chunk * down raw ticks (`raw_push_plan`); one that completes no group issues that one launch and
    scores nothing; one that starts on a group boundary with exactly chunk * down raw ticks is ONE copy and ONE replay
    of a graph captured with the front end in it.  A prep= detector pushed raw ticks writes the bits a plain one
    writes when pushed prep.series(raw).t(); prep=None issues exactly the launches it always did.

    `save(path)` / `StreamDetector.load(path, model, prep=)` (`state_dict()` / `load_state_dict(sd)` through
    a dict of numpy arrays) carry a running detector across a process boundary: the state, the table in force, the
    threshold, the log, the gap counters, the ring, the open group's raw ticks, the host counters and the configuration
    go into one .npz; the static buffers of a push, the workspaces and the graphs do not.  A stream cut by a save and a
    load writes the bits of the uninterrupted stream; a push before a save and after a load issues the launches it
    always did.

    `events=dict(on=, off=, lo=, cap=)` turns the flag per tick into an event list: an episode is raised
    after `on` ticks above `threshold` (read on the device through the pointer the score launch reads) and cleared after
    `off` ticks at or below the clear level `lo` (a float64 scalar on the device, `clear`; None: the threshold at
    construction).  gdn_stream_events sits between the score and the advance launch (captured with them) and writes only
    its own allocation, `events`: the carried state and a table of `cap` rows (default 4096) that `episodes()` returns;
    `status()` then ends with (episodes, episode_open).  The table equals harness.episodes on the evaluator's scores of
    [history[:, -w:] | stream], bit for bit, however the stream is cut into pushes or by save / load.  The default
    events=None constructs, pushes, saves and loads exactly as it always did."""

    def __init__(self, model, med_iqr, threshold, history, chunk: int, top_m: int = 1, log: int = 4096,
                 use_graph: bool = True, wide: bool | None = None, gaps: bool = False, recal: int = 0,
                 exclude_alarms: bool = True, recal_every: int = 0, recal_min: int | None = None,
                 calib: str = "tick", prep=None, events=None, recal_threshold=None):
        self._build(model, med_iqr, threshold, history, chunk, top_m, log, use_graph, wide, gaps, recal,
                    exclude_alarms, recal_every, recal_min, calib, prep, events=events, recal_threshold=recal_threshold)

    def _build(self, model, med_iqr, threshold, history, chunk, top_m, log, use_graph, wide, gaps, recal,
               exclude_alarms, recal_every, recal_min, calib, prep, device=None, events=None, recal_threshold=None):
        """The constructor's body.  `history=None` is load()'s private path: nothing is seeded — the state is
        gdn_stream_state_bytes(n, w) of zeros, the table zeros, the threshold inf, all on `device`, `wide` the
        caller's word — and load_state_dict fills the allocations."""
        self._set_calib(calib, gaps, recal)
        self.model = model.eval()
        w = model.gnn_layers[0].gnn.lin.weight.shape[1]
        n = model.embedding.weight.shape[0]
        self.n, self.w, self.chunk, self.top_m, self.use_graph = n, w, int(chunk), int(top_m), bool(use_graph)
        if not 1 <= self.chunk <= _STREAM_MAX_CHUNK:
            raise ValueError(f"chunk = {chunk}: a push scores 1 to {_STREAM_MAX_CHUNK} ticks (longer pushes are split)")
        if self.chunk * n * w * 4 > _VALIDATE_CHUNK_BYTES:
            raise ValueError(f"chunk = {chunk}: the window buffer [{chunk}, {n}, {w}] fp32 exceeds "
                             f"{_VALIDATE_CHUNK_BYTES >> 20} MB; use a smaller chunk")
        self._check_lists(top_m, log, "entries")
        self.events_cfg = None if events is None else events_config(events, self.top_m)     # host facts only
        self._set_recal(recal, exclude_alarms, recal_every, recal_min,                      # ... before any device work
                        lambda: _lib.load().gdn_stream_calib_bytes(n, self.recal),
                        f"no calibration ring for n = {n}, R = {recal} (1 <= n <= 4096, 64 <= R <= 2^20, "
                        "8 n R <= 2 GiB)")
        self._set_recal_threshold(recal_threshold)
        _check_stream_head(model)
        self.with_gaps = bool(gaps)
        if history is None:
            dev = torch.empty((0,), device=device).device           # ("cuda" -> the current device, with its index)
            self.med_iqr = torch.zeros((n, 2), dtype=torch.float64, device=dev)
            self.threshold = torch.full((1,), float("inf"), dtype=torch.float64, device=dev)
            self.state = ops.stream_state_empty(n, w, dev)
            self.wide = bool(wide)
        else:
            history = ops._chk(history, name="history")
            if history.dim() != 2 or history.shape[0] != n:
                raise ValueError(f"expected a history of shape [{n}, h], got {tuple(history.shape)}")
            dev = history.device
            med_iqr = ops._chk(med_iqr, torch.float64, name="med_iqr")
            if med_iqr.shape != (n, 2):
                raise ValueError(f"expected med_iqr of shape [{n}, 2], got {tuple(med_iqr.shape)}")
            self.med_iqr = med_iqr.clone()
            self.threshold = torch.as_tensor(threshold, dtype=torch.float64).reshape(1).to(dev).clone()
            if self.with_gaps and history.shape[1] >= w and not bool(torch.isfinite(history[:, -w:]).all()):
                raise ValueError(f"history: its last {w} ticks hold a value that is not finite; with gaps=True every "
                                 "missing reading is held at an earlier real one, so the stream must begin on real "
                                 "readings")
            self.state = ops.stream_state(history, w)
            self.wide = model.wide_for(history[:, -w:]) if wide is None else bool(wide)
        m = self.top_m
        self._alloc_push((), log, dev)
        self.events = self.clear = None
        if self.events_cfg is not None:
            # the clear level: a float64 scalar on the device (None: the raise level at construction); load() fills it
            lo = self.events_cfg.pop("lo")
            if history is not None:
                hi = float(self.threshold.item())
                lo = hi if lo is None else lo
                if lo > hi:
                    raise ValueError(f"events: lo = {lo} lies above the raise level (threshold = {hi})")
            self.clear = torch.full((1,), 0.0 if lo is None else lo, dtype=torch.float64, device=dev)
            self.events = ops.stream_events_alloc(m, self.events_cfg["cap"], dev)
        self.ring_keys = self.ring_keep = self._recal_ws = None
        if self.recal:
            self.ring_keys, self.ring_keep = ops.stream_calib_ring(n, self.recal, dev)
            self._recal_ws = ops.score_select_workspace(1, n, self.recal, dev)
        if self.recal_threshold is not None:
            self._ring_buffers()
        self._recal_counts = torch.zeros((n,), dtype=torch.int32, device=dev) if calib == "sensor" else None
        self.recal_counts = None            # calib="sensor": every sensor's real keys at the last recalibrate() (host)
        self.recals = 0                     # tables written by recalibrate()
        self.recal_kept = 0                 # ... and the kept ticks behind the last one
        self._handed = 0                    # ticks handed to push(): recal_every's clock
        # the full push (its key: the graph bakes in the folded constants' pointers); `_guarded()` is asked once a capture
        self._full = _Replay(lambda *a: self._launch(*a), use_graph, lambda: model._constants().key,    # (looked up late)
                             args=lambda: (self.chunk, self._guarded()))
        self._prep_full = {}                # prep=: raw dtype -> the full raw push, the front end reading `_raw_stage`'s
        self._last = 0                      # ticks of the last (sub-)push: what the static buffers hold
        self.calib_kept = None              # from_calibration(calib_gaps=True): the complete ticks behind the table
        self.calib_counts = None            # ... calib="sensor": every sensor's real readings behind it (device int32)
        self.prep = prep
        self.raw_pending = 0                # prep=: raw ticks of the open group, held in _pend[_pend_at]
        if prep is not None:
            if prep.n != n:
                raise ValueError(f"prep: fitted on {prep.n} sensors, the model has {n}")
            if prep.table.device != dev:
                raise ValueError(f"prep: its table is on {prep.table.device}, the detector on {dev}")
            rows = max(1, prep.down - 1)
            self._pend = [torch.zeros((rows, n), dtype=torch.float64, device=dev) for _ in range(2)]
            self._pend_at = 0
            self._raw_stage = {}            # raw dtype -> the static staging buffer [chunk * down, n] of its pushes

    @classmethod
    def from_calibration(cls, model, series, chunk: int, batch: int = 8192, calib_gaps: bool = False,
                         min_kept: int = 64, **kw):
        """A detector calibrated on `series` [n, T] fp32 on the device, a period known to be normal: ONE
        SeriesEvaluator step over it gives `med_iqr`; threshold = the largest anomaly score of that period (the rule
        of `-report val`); history = its last w ticks unless `history=` names the ticks the stream really follows.
        `gaps=True` passes through; the calibration itself knows no missing reading, so a series that is not finite
        is then refused — unless `calib_gaps=True` (needs gaps=True): the period is then scored by
        SeriesEvaluator(gaps=True, min_kept=...), i.e. under the detector's own rules — missing readings held, the
        table from the complete ticks, a missing reading's error neutral — the default history is the FILLED period's
        last w ticks, and the ring is seeded with the period's own keep flags.  `calib_kept` is the number of complete
        ticks behind the table (None without calib_gaps).  The stream's own counters start at zero.
        `calib="sensor"` (needs calib_gaps=True) goes to the evaluator and the detector alike: the table
        comes from every sensor's own real readings, the ring is seeded through the period's validity plane, and
        `calib_kept` is the smallest per-sensor count, `calib_counts` [n] int32 (device) all of them.  Without a ring
        (recal = 0) only the calibration follows it: the detector has nothing to recalibrate."""
        calib = kw.get("calib", "tick")
        _check_calib_gaps(calib, calib_gaps)
        series = ops._chk(series, name="series")
        _check_calib_period(series, calib_gaps, kw.get("gaps"), "detector")
        w = model.gnn_layers[0].gnn.lin.weight.shape[1]
        if series.dim() != 2 or series.shape[1] <= w:
            raise ValueError(f"calibration needs a series [n, T] with T > {w}, got {tuple(series.shape)}")
        R = int(kw.get("recal", 0))
        table, threshold, tail, kept, counts, rows = _calibrate_period(model, series, w, batch, calib_gaps, min_kept,
                                                                       calib, bool(R))
        history = kw.pop("history", tail)
        if calib == "sensor" and not R:
            kw["calib"] = "tick"            # no ring: the detector never calibrates anything itself
        det = cls(model, table, threshold, history, chunk, **kw)
        det.calib_kept = kept
        det.calib_counts = counts
        if det.recal:
            _seed_ring(det.ring_keys, det.ring_keep, *rows)
        return det

    def _launch(self, count: int, guard: bool):
        if self.with_gaps:
            ops.stream_fill(self.state, self.raw_buf, self.w, self.chunk_buf, self.valid, self.gap_chunk, count=count)
        ops.stream_windows(self.state, self.chunk_buf, self.w, self.x, count=count)
        x = self.x if count == self.chunk else self.x[:count]
        self.model.forward_into(x, self.pred[:count], wide=self.wide, guard=guard)
        # valid, gap_chunk and gaps are None on a plain detector: the wrappers then call the plain symbols
        ops.stream_score(self.state, self.pred, self.chunk_buf, self.med_iqr, self.threshold, self.top_m,
                         self.top_scores, self.top_sensors, self.alarm, count=count, valid=self.valid)
        if self.events is not None:
            ops.stream_events(self.state, self.top_scores, self.top_sensors, self.threshold, self.clear,
                              self.events_cfg["on"], self.events_cfg["off"], self.events_cfg["cap"], self.events,
                              count=count)
        if self.recal:
            ops.stream_calib_write(self.state, self.pred, self.chunk_buf, self.alarm, self.ring_keys, self.ring_keep,
                                   self.exclude_alarms, count=count, valid=self.valid,
                                   by_sensor=self.calib == "sensor")
        ops.stream_advance(self.state, self.chunk_buf, self.pred, self.med_iqr, self.alarm, self.top_sensors, self.w,
                           self.top_m, self.log_ticks, self.log_sensors, count=count, valid=self.valid,
                           gap_chunk=self.gap_chunk, gaps=self.gaps)

    graph = property(lambda self: self._full.graph, doc="the captured full push, None before the first one")
    _prep_graphs = property(lambda self: {dt: full.graph for dt, full in self._prep_full.items() if full.graph is not None},
                            doc="raw dtype -> the graph captured with the front end reading that dtype's staging buffer")

    def _push(self, ticks):
        r = ticks.shape[0]
        (self.raw_buf if self.with_gaps else self.chunk_buf)[:r].copy_(ticks)
        self._last = r
        if r == self.chunk:
            self._full()
        else:
            self._launch(r, self._guarded())

    def _launch_prep(self, stage, rows: int, groups: int, guard: bool):
        """gdn_prep_ticks over stage[:rows] and the pending plane, then the launches of a push of `groups` ticks."""
        ops.prep_ticks(stage, self._pend[self._pend_at], self.raw_pending, self._pend[self._pend_at ^ 1],
                       self.prep.down, self.prep.table, self.raw_buf if self.with_gaps else self.chunk_buf, rows=rows)
        if groups:
            self._launch(groups, guard)

    def _push_raw(self, ticks, groups: int, left: int, replayable: bool):
        rows = ticks.shape[0]
        stage = self._raw_stage.get(ticks.dtype)
        if stage is None:
            stage = self._raw_stage[ticks.dtype] = torch.zeros((self.chunk * self.prep.down, self.n), dtype=ticks.dtype,
                                                               device=self.state.device)
            # (a replayable sub-push opens and leaves no group: the graph neither reads nor writes a pending plane)
            self._prep_full[ticks.dtype] = _Replay(
                self._launch_prep, self.use_graph, self._full.key,
                args=lambda: (stage, self.chunk * self.prep.down, self.chunk, self._guarded()))
        stage[:rows].copy_(ticks)
        self._last = groups
        if replayable:
            self._prep_full[ticks.dtype]()
        else:
            self._launch_prep(stage, rows, groups, self._guarded() if groups else False)
        self._pend_at ^= 1
        self.raw_pending = left

    def _push_prep(self, ticks):
        if ticks.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"ticks: expected raw {torch.float32} or {torch.float64}, got {ticks.dtype}")
        if ticks.shape[0] < 1:
            raise ValueError("a push needs at least one raw tick")
        at = 0
        for rows, groups, left, replayable in raw_push_plan(self.raw_pending, ticks.shape[0], self.prep.down, self.chunk):
            self._push_raw(ticks[at:at + rows], groups, left, replayable)
            at += rows
            self._hand(groups)
        r = self._last
        return self.top_scores[:r], self.top_sensors[:r], self.alarm[:r]

    def push(self, ticks):
        """Score `ticks` [r, n] fp32 (device or host), oldest first.  Returns views (top_scores [r', m] float64,
        top_sensors [r', m] int32, alarm [r'] int32) of the static buffers, valid until the next push; r' = r when
        r <= chunk, else the ticks of the last of the pushes it was split into (the counters and the log hold all).
        prep=: `ticks` are RAW ticks, fp32 or float64; the views cover the model ticks the last sub-push completed
        (possibly none)."""
        if ticks.dim() != 2 or ticks.shape[1] != self.n:
            raise ValueError(f"expected ticks of shape [r, {self.n}], got {tuple(ticks.shape)}")
        if self.prep is not None:
            return self._push_prep(ticks)
        if ticks.dtype != torch.float32:
            raise TypeError(f"ticks: expected {torch.float32}, got {ticks.dtype}")
        if ticks.shape[0] < 1:
            raise ValueError("a push needs at least one tick")
        for s in range(0, ticks.shape[0], self.chunk):
            self._push(ticks[s:s + self.chunk])
            self._hand(self._last)
        r = self._last
        return self.top_scores[:r], self.top_sensors[:r], self.alarm[:r]

    def recalibrate(self, threshold=None) -> int:
        """`threshold`: None — the constructor's `recal_threshold`; a number — a one-off margin; False —
        the table only.  With a margin, and only when the table was rewritten, two more launches re-derive `threshold`
        (and with events= the clear level) in place from the ring under the new table: margin times the largest
        smoothed score among the ring's eligible ticks, if at least `recal_min` are eligible; `ring_peak`,
        `ring_eligible` and `ring_peak_slot` (device tensors of one element) say what was found.  No further host read.
        Overwrite `med_iqr` in place with the median / IQR per sensor of the kept ticks in the calibration ring
        (np.median and numpy's 'linear' 25th / 75th percentiles: gdn_score_quantiles' arithmetic, ONE gdn_score_select
        straight from the ring) and return how many ticks that was; with fewer than `recal_min` kept, write nothing
        and return 0.  Eager, ONE host read (a synchronisation).  `threshold`, the carry and the captured graph stay:
        the three normalised errors before the switch keep the table they were computed with.
        calib="sensor": gdn_score_key_counts over the ring, then gdn_score_select_counts(min_count = recal_min) into
        `med_iqr` in place: the row of every sensor with at least `recal_min` real keys is rewritten, the others stay.
        The ONE host read is of the counts: `recal_counts` [n] int64 (host), `recal_kept` = the smallest count among
        the rewritten sensors (0 if none); returns the NUMBER OF SENSORS whose row was rewritten."""
        if not self.recal:
            raise ValueError("recalibrate(): the detector was built with recal=0 and keeps no calibration ring")
        margin = self._margin(threshold)
        if self.calib == "sensor":
            ops.score_key_counts(self.ring_keys, 1, self.n, self.recal, out=self._recal_counts)
            ops.score_select_counts(self.ring_keys, 1, self.n, self.recal, self._recal_counts, self.recal_min,
                                    self._recal_ws, out=self.med_iqr)
            self.recal_counts = self._recal_counts.cpu().to(torch.int64)
            done = self.recal_counts[self.recal_counts >= self.recal_min]
            self.recal_kept = int(done.min()) if done.numel() else 0
            self.recals += 1 if done.numel() else 0
            if margin is not None and done.numel():
                self._ring_threshold(margin)
            return int(done.numel())
        total = int(self.ring_keep.sum())
        if total < self.recal_min:
            return 0
        ops.score_select(self.ring_keys, 1, self.n, self.recal, total, self._recal_ws, out=self.med_iqr)
        if margin is not None:
            self._ring_threshold(margin)
        self.recals += 1
        self.recal_kept = total
        return total

    def calibration(self):
        """(a copy of the table in force [n, 2] float64, the kept ticks the last recalibrate() computed it from: 0 while
        it is still the constructor's table)."""
        return self.med_iqr.clone(), self.recal_kept

    def status(self):
        """(ticks, alarms, log_ticks[:logged], log_sensors[:logged]): ONE read of the counters (a synchronisation).
        A prep= detector appends `raw_pending`, the raw ticks of the open group (a host value)."""
        ticks, alarms, logged = (int(v) for v in self.state[:3].tolist())
        tail = () if self.prep is None else (self.raw_pending,)
        if self.events is not None:                         # events on: `episodes` raised so far and `episode_open`
            raised, is_open = self.events[:2].tolist()
            tail += (int(raised), bool(is_open))
        if self.log_ticks is None:
            dev = self.state.device
            return (ticks, alarms, torch.empty((0,), dtype=torch.int64, device=dev),
                    torch.empty((0, self.top_m), dtype=torch.int32, device=dev)) + tail
        return (ticks, alarms, self.log_ticks[:logged], self.log_sensors[:logged]) + tail

    def status_gaps(self):
        """(missing_total [n] int64, missing_run [n] int64) on the host, gaps=True only: the missing readings of every
        sensor since the stream began, and the run of missing readings that ends at the last scored tick (0 after a
        real reading; >= w: the sensor's whole window is held values).  ONE read (a synchronisation)."""
        return _status_gaps(self.gaps, self.with_gaps, "detector")

    def episodes(self) -> Episodes:
        """The stream's episode table (events= only): views of the events allocation, so a later push
        moves them.  The open episode's row holds its peak so far and end = -1."""
        if self.events is None:
            raise ValueError("episodes(): the detector was built with events=None and keeps no episode table")
        return _episodes(self.events, self.top_m, self.events_cfg["cap"])

    def localise(self, rows=None) -> Localisation:
        """harness.localise for the last push: which sensors deviate at its alarm rows (`rows=None`; or the given
        rows of the push) and which neighbours they were reading — ONE model.attention_at on the static window
        buffer.  `ticks` are global stream ticks; the other fields mean what they mean for `localise`; under gaps=True
        `observed` is the FILLED reading (the held value where the reading was missing: see `valid`)."""
        r = self._last
        if rows is None:
            rows = torch.nonzero(self.alarm[:r]).view(-1)
        rows = _row_indices(rows, self.state.device, r, f"rows outside [0, {r}) of the last push")
        first = self.state[0] - r                       # (advance has run: ticks counts the push already)
        return _localisation(self.model, self.x, first + rows, rows, self.top_sensors[rows].long(), self.top_scores[rows],
                             self.pred, self.chunk_buf)

    # save and resume: a stream cut by a save and a load writes the bits of the uninterrupted stream
    def _expect(self, check_model: bool = True) -> dict:
        """stream_checkpoint_check's `expect` for this detector: its model's shape and fingerprint, its prep, and the
        loaded library's ABI version and byte sizes."""
        expect = _checkpoint_expect(self.model, self.prep, self.recal, check_model)
        expect["events"], expect["recal_threshold"] = self.events_cfg, self.recal_threshold
        return expect

    def _ckpt_tensors(self) -> dict:
        """Checkpoint key -> the device tensor (a view) that holds it; an option that is off has no tensor and no key.
        The raw ticks of the open group are not in it: they alternate between two planes (state_dict, load_state_dict)."""
        held = {"state": self.state.view(torch.uint8), "med_iqr": self.med_iqr,
                "threshold": torch.as_tensor(self.threshold, dtype=torch.float64).reshape(1),
                "log_ticks": self.log_ticks, "log_sensors": self.log_sensors, "gaps": self.gaps,
                "ring_keys": self.ring_keys, "ring_keep": self.ring_keep, "calib_counts": self.calib_counts,
                "events": None if self.events is None else self.events.view(torch.uint8), "events_lo": self.clear,
                "clear_frac": None if self.recal_threshold is None else self.clear_frac}
        return {k: t for k, t in held.items() if t is not None}

    def state_dict(self) -> dict:
        """Everything a continuation of this stream depends on, as a flat dict of numpy arrays (no Python objects:
        numpy.savez writes it, numpy.load(allow_pickle=False) reads it): the device state as raw bytes, the table in
        force, the threshold, the alarm log, the gap counters, the calibration ring, the raw ticks of the open
        downsample group; the host counters; the configuration; and the identity of what wrote it (format, ABI version,
        byte sizes, the model's fingerprint).  The static buffers of a push, the workspaces and the captured graphs are
        outputs or scratch and stay behind.  Read-only: ONE batch of device-to-host copies on the current stream and
        ONE synchronisation; the pushes after it write the bits they would have written."""
        lib = _lib.load()
        dev = self._ckpt_tensors()
        if self.prep is not None:
            dev["pending"] = self._pend[self._pend_at][:self.raw_pending]
        sd, fingerprint = self._ckpt_read(dev)
        if self.recal_counts is not None:
            sd["recal_counts"] = self.recal_counts.to(torch.int64).numpy().copy()
        ints = {"format": STREAM_CHECKPOINT_FORMAT, "abi": lib.gdn_abi_version(),
                "state_bytes": lib.gdn_stream_state_bytes(self.n, self.w),
                "calib_bytes": lib.gdn_stream_calib_bytes(self.n, self.recal) if self.recal else 0,
                "handed": self._handed, "recals": self.recals, "recal_kept": self.recal_kept,
                "calib_kept": -1 if self.calib_kept is None else int(self.calib_kept), "raw_pending": self.raw_pending}
        return self._ckpt_finish(sd, ints, _CKPT_INTS, self._config(), fingerprint)

    def load_state_dict(self, sd, check_model: bool = True) -> None:
        """Take the stream of `sd` (state_dict()'s dict, or a file's) up where it was saved.  `sd` is checked first
        (stream_checkpoint_check, and its configuration against this detector's own, field by field: a ValueError that
        names the field, before any device work); the captured graphs are dropped; then every array is copied INTO the
        allocations this detector already has, so the pointers a later capture records are the ones it always had.
        Afterwards the last push is empty (`valid[:0]`, `localise()` with no rows) and the first full push captures
        the graph again."""
        stream_checkpoint_check(sd, self._expect(check_model))
        self._ckpt_same_config(stream_checkpoint_config(sd), "stream checkpoint", "detector")
        if not isinstance(self.threshold, torch.Tensor):    # (a caller's plain number: back to the device scalar)
            self.threshold = torch.zeros((1,), dtype=torch.float64, device=self.state.device)
        host = self._ckpt_fill(sd)
        self.raw_pending = _ckpt_int(sd, "raw_pending")
        if self.prep is not None:
            self._pend_at = 0
            self._pend[0][:self.raw_pending].copy_(host("pending"))
        self.recal_counts = host("recal_counts") if "recal_counts" in sd else None
        kept = _ckpt_int(sd, "calib_kept")
        self.calib_kept = None if kept < 0 else kept
        self._handed, self.recals = _ckpt_int(sd, "handed"), _ckpt_int(sd, "recals")
        self.recal_kept = _ckpt_int(sd, "recal_kept")

    def save(self, path: str) -> None:
        """state_dict() as one .npz at exactly `path` (write_stream_checkpoint: a temporary file beside it, then
        os.replace — a save that dies half-way leaves the previous checkpoint loadable)."""
        write_stream_checkpoint(path, self.state_dict())

    @classmethod
    def load(cls, path: str, model, prep=None, device="cuda", check_model: bool = True, use_graph: bool = True):
        """A detector that continues the stream saved at `path`: built from the file's configuration, the caller's
        `model` and — when the file says one was used — `prep` (on `device`), with no history (nothing is seeded),
        then load_state_dict.  Refused with a ValueError that names the field, before any device work: an unknown
        format, another ABI version or byte size, another n or w, a prep against the file's word or with another down,
        other weights (unless check_model=False), a missing key or an array of the wrong shape or dtype."""
        sd = read_stream_checkpoint(path)
        _ckpt_format(sd)                                    # (an unknown format first: its other fields may differ)
        R = _ckpt_int(sd, "recal")
        if R < 0:
            raise ValueError(f"stream checkpoint: recal = {R} is negative")
        stream_checkpoint_check(sd, _checkpoint_expect(model, prep, R, check_model))
        cfg = stream_checkpoint_config(sd)
        events = stream_checkpoint_events(sd)               # (None: the file has no episode table, nor has the detector)
        if events is not None:
            events = {k: events[k] for k in ("on", "off", "cap", "lo")}
        det = cls.__new__(cls)
        det._build(model, None, None, None, cfg["chunk"], cfg["top_m"], cfg["log"], use_graph, bool(cfg["wide"]),
                   bool(cfg["with_gaps"]), cfg["recal"], bool(cfg["exclude_alarms"]), cfg["recal_every"],
                   cfg["recal_min"] if cfg["recal"] else None, cfg["calib"], prep, device=device,
                   events=events, recal_threshold=checkpoint_recal_threshold(sd))
        det.load_state_dict(sd, check_model=False)          # (the weights were compared above, once)
        return det


# --------------------------------------------------------------------------- streaming fleet
def fleet_check_shape(units: int, chunk: int, n: int, w: int) -> None:
    """The host facts a fleet's buffers depend on, refused by name before any device work: 1 <= units, 1 <= chunk,
    units * chunk <= 4096 windows per launch, and a window buffer [units, chunk, n, w] fp32 within the evaluators' cap."""
    if int(units) < 1:
        raise ValueError(f"units = {units}: a fleet has at least one unit")
    if int(chunk) < 1 or int(units) * int(chunk) > _STREAM_MAX_CHUNK:
        raise ValueError(f"units * chunk = {units} * {chunk}: a push scores 1 to {_STREAM_MAX_CHUNK} windows in one "
                         "launch (longer pushes are split in time; more units: more fleets)")
    if int(units) * int(chunk) * n * w * 4 > _VALIDATE_CHUNK_BYTES:
        raise ValueError(f"units * chunk = {units} * {chunk}: the window buffer [{units}, {chunk}, {n}, {w}] fp32 exceeds "
                         f"{_VALIDATE_CHUNK_BYTES >> 20} MB; use a smaller chunk")


def fleet_check_push(ticks, counts, units: int, n: int, raw: bool = False):
    """The host checks of StreamFleet.push, before any device work: `ticks` [units, r >= 1, n] fp32 (`raw`: the raw
    ticks of a prep= fleet, fp32 or float64); `counts` None, a host sequence / tensor of `units` integers in 0 .. r
    (returned as a host int64 tensor), or a device int32 tensor [units] (returned as it is: the kernels clamp it)."""
    if ticks.dim() != 3 or ticks.shape[0] != units or ticks.shape[2] != n:
        raise ValueError(f"expected ticks of shape [{units}, r, {n}], got {tuple(ticks.shape)}")
    if raw and ticks.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"ticks: expected raw {torch.float32} or {torch.float64}, got {ticks.dtype}")
    if not raw and ticks.dtype != torch.float32:
        raise TypeError(f"ticks: expected {torch.float32}, got {ticks.dtype}")
    r = ticks.shape[1]
    if r < 1:
        raise ValueError("a push needs at least one tick")
    if counts is None:
        return None
    if isinstance(counts, torch.Tensor) and counts.is_cuda:
        if counts.dtype != torch.int32 or counts.shape != (units,):
            raise ValueError(f"counts: a device tensor must be {torch.int32} of shape [{units}], got {counts.dtype} "
                             f"{tuple(counts.shape)}")
        return counts
    host = torch.as_tensor(counts)
    if host.dim() != 1 or host.shape[0] != units or host.dtype.is_floating_point or host.dtype == torch.bool:
        raise ValueError(f"counts: expected {units} integers (one per unit), got {host.dtype} {tuple(host.shape)}")
    host = host.to(torch.int64)
    if bool(((host < 0) | (host > r)).any()):
        raise ValueError(f"counts = {host.tolist()}: every unit contributes 0 to r = {r} of the pushed ticks")
    return host


def fleet_clear_levels(lo, threshold, units: int) -> torch.Tensor:
    """The clear levels of a fleet's events= as a host float64 tensor [units]: `lo` None (each unit's raise level), one
    number or `units` of them, against `threshold` (one number or [units]).  Refused by name: another shape, a NaN
    level, a lo[u] above threshold[u]."""
    hi = torch.as_tensor(threshold, dtype=torch.float64).detach().cpu().reshape(-1).expand(units)
    if lo is None:
        return hi.clone()
    lo = torch.as_tensor(lo, dtype=torch.float64).detach().cpu()
    if lo.dim() > 1 or lo.numel() not in (1, units):
        raise ValueError(f"events: lo is one number, None or [{units}] of them, got {tuple(lo.shape)}")
    lo = lo.reshape(-1).expand(units).clone()
    if bool(torch.isnan(lo).any()):
        raise ValueError("events: lo holds a NaN; the clear level must be a number")
    bad = torch.nonzero(lo > hi).flatten()
    if bad.numel():
        u = int(bad[0])
        raise ValueError(f"events: lo[{u}] = {float(lo[u])} lies above the raise level of unit {u} (threshold[{u}] = "
                         f"{float(hi[u])})")
    return lo


def fleet_check_prep(prep, units: int, chunk: int, n: int, itemsize: int = 4) -> None:
    """The host facts of a fleet's prep=, refused by name before any device work: a Prep fitted on another sensor count,
    a PrepUnits (per-unit tables) of another number of units, and a staging buffer [units, chunk * down,
    n] of `itemsize` bytes per reading beyond the evaluators' cap."""
    if prep.n != n:
        raise ValueError(f"prep: fitted on {prep.n} sensors, the model has {n}")
    if getattr(prep, "tables", None) is not None and prep.units != int(units):
        raise ValueError(f"prep: per-unit tables of {prep.units} units, the fleet has units = {int(units)}")
    if int(units) * int(chunk) * prep.down * n * int(itemsize) > _VALIDATE_CHUNK_BYTES:
        raise ValueError(f"prep: the raw staging buffer [{units}, {chunk} * {prep.down}, {n}] of {itemsize}-byte readings "
                         f"exceeds {_VALIDATE_CHUNK_BYTES >> 20} MB; use a smaller chunk")


def fleet_raw_cuts(r: int, down: int, chunk: int) -> list:
    """The sub-pushes of `r` raw ticks of the time axis handed to a prep= fleet: a list of (first raw row, raw rows,
    rows of the returned views).  A sub-push carries at most chunk * down raw rows, whatever any unit holds: with
    p < down pending raw ticks it completes (p + rows) // down <= chunk model ticks, so no plan depends on the pending
    state (unlike raw_push_plan).  The views cover min(chunk, (down - 1 + rows) // down) rows: the most model ticks a
    unit can have completed.  Pure host arithmetic."""
    if down < 1 or chunk < 1 or r < 0:
        raise ValueError(f"fleet_raw_cuts: r = {r}, down = {down}, chunk = {chunk}")
    span = chunk * down
    return [(s, min(span, r - s), min(chunk, (down - 1 + min(span, r - s)) // down)) for s in range(0, r, span)]


def fleet_raw_hand(raw_handed: int, rows: int, down: int) -> int:
    """recal_every's clock of a prep= fleet: the model ticks that `rows` more raw rows of the time axis hand over when
    `raw_handed` were handed before — model ticks handed = raw rows handed // down.  Pure host arithmetic."""
    return (raw_handed + rows) // down - raw_handed // down


class StreamFleet(_StreamCore):
    """Scores the ticks of U units of ONE model with one push: a rack of identical servers, a line of identical pumps —
    the same sensor list and the same trained model, but a median / IQR table, a threshold, a history, counters and an
    alarm log per unit (include/gdn_hip.h "streaming fleet").

    A push issues ONE copy of `ticks` into the static [U, chunk, n] buffer, ONE small write of the static counts buffer
    and ONE replay of a graph captured at the first push: fleet_windows -> model.forward_into on the [U * chunk, n, w]
    view -> fleet_score -> fleet_advance (the only writer of the states).  How many rows a unit contributes is DATA on
    the device, not a launch argument: the same graph serves a full push, a short one and one in which some units are
    silent, so there is no eager variant for short pushes.  A push of r > chunk ticks is split in time.

    `med_iqr` [U, n, 2] float64, `threshold` a number or [U], `history` [U, n, h >= w] fp32 on the device; `chunk` ticks
    per unit and push with U * chunk <= 4096; `top_m`, `log` (entries per unit; 0: no log) and `use_graph` as
    StreamDetector's.

    The contract: for every unit u the fleet writes the bits of StreamDetector(model, med_iqr[u], threshold[u],
    history[u], chunk, top_m, log, wide=<the same word>) pushed that unit's real rows in the same cuts, a push with
    counts[u] == 0 skipped: top_scores, top_sensors and alarm on the real rows, the whole state block (`unit_state(u)`,
    the layout ops.stream_state_views reads), the log and the counters.  A window's forward does not depend on what else
    is in its batch.  What IS per launch is the route: `wide=None` asks model.wide_for over ALL units' histories once,
    and under operand_range == "auto" a guarded forward that meets ONE out-of-range reading redoes the push of all
    units in fp32; each route is still the evaluator's on that route.  Rows of a push that are not real are cut as zero
    windows, so a route decision never outlives the push that caused it.

    `gaps=True` is StreamDetector's gaps=True per unit: a pushed value that is not finite is a missing
    reading.  The push lands in `raw_buf` [U, chunk, n] and fleet_fill leads the launches; `chunk_buf` is then the FILLED
    chunk, `valid` [U, chunk, n] uint8 the last push's plane (rows at or beyond counts[u] unspecified), and the score and
    advance launches are their gaps forms.  `status_gaps()` reads the per-unit, per-sensor counters.  Only a unit's real
    rows are looked at: a non-finite value in a row at or beyond counts[u] is not a missing reading.  The last w ticks
    of every unit's history must be finite.

    `events=dict(on=, off=, lo=, cap=)` is StreamDetector's events= per unit: fleet_events sits between the score and
    the advance launch and folds every unit's real rows into that unit's block of `events` [U, words] (a single
    stream's events allocation per row); `clear` [U] float64 on the device holds the clear levels (`lo`: one number,
    None = each unit's threshold at construction, or [U]); `episodes(u)` returns unit u's table.  A silent unit's block
    is not touched, whatever episode is open in it.

    Both are off by default, and then a push issues exactly the launches it always did.  With them the contract above
    reads StreamDetector(..., gaps=True / events=...) for every unit, `status_gaps()` and `episodes()` included; it is
    still ONE copy of the ticks, one counts write and ONE replay per push, one graph for full, short and silent units.

    `recal=R` is StreamDetector's recal=R per unit: `ring_keys` [U, n, R] float64 and `ring_keep` [U, R]
    uint8 in one allocation, unit u's slices a single stream's ring.  fleet_calib_write sits between the score (events)
    and the advance launch, captured with them: ONE more launch in the same replay, and a silent unit's ring is not
    touched.  `exclude_alarms`, `recal_min` (default max(64, R // 4)) and `calib="sensor"` (needs gaps=True) mean what
    they mean to a detector.  `recalibrate(units=None)` rewrites `med_iqr` IN PLACE for every unit (or those named) with
    at least `recal_min` kept ticks — per sensor under calib="sensor" — in a fixed number of launches with NO host read:
    the keep sums (or the per-sensor key counts) become per-row counts on the device and gdn_score_select_counts reads
    the rings as U * n sensors.  `recal_kept` [U] / `recal_counts` [U, n] int32 stay on the device; `calibration()`
    reads them.  The graph reads the table through the same pointer and stays; thresholds, carries, logs and episode
    tables are not touched.  `recal_every=E`: `push` calls `recalibrate()` after every sub-push in which the ticks
    handed per unit (r, the time axis of `ticks`, whatever `counts` says) cross a multiple of E.  When every unit
    contributes every tick that equals U detectors with recal_every=E; otherwise all units are recalibrated on the
    fleet's clock, each from whatever its own ring holds.  The contract above then reads StreamDetector(recal=R, ...)
    for every unit: ring, keep flags and the table after recalibrate().  recal=0 issues exactly the launches it did.
    `recal_threshold=margin` is StreamDetector's per unit: `recalibrate()` then re-derives `threshold` [U]
    (and `clear` [U] under events=) in place from the rings under the tables just written, two more launches after the
    select and still no host read; a unit left out, silent or with fewer than `recal_min` eligible ticks keeps its own.

    `prep=Prep` is StreamDetector's prep= per unit with ONE table for all units: `push()` then takes RAW
    ticks [U, r, n], fp32 or float64, and `counts` are RAW counts.  gdn_fleet_prep_ticks leads the captured launches (in
    front of fleet_fill under gaps=True): per unit it completes the groups of `prep.down` raw ticks its open group and
    its real raw rows make up, writes their medians as model ticks into `raw_buf` (gaps=True) or `chunk_buf`, writes
    `counts` [U] — on the device, the model ticks each unit completed in the last sub-push — and keeps the open group in
    `pend` (ops.fleet_prep_views), in place.  Pending counts are data on the device like everything else: one graph per
    raw dtype serves every mix of open groups, counts and silent units.  A sub-push carries up to chunk * down raw rows
    of the time axis: ONE copy into the static staging buffer of that dtype, one write of `raw_counts`, ONE replay.
    `chunk`, `recal`, `log` and `history` stay in model ticks; recal_every's clock counts raw rows of the time axis
    handed // down.  A prep= fleet pushed raw ticks writes, for every unit, the bits of this fleet without prep pushed
    that unit's completed medians with counts = groups, hence those of StreamDetector(prep=prep, ...) pushed that unit's
    real raw rows; a silent unit keeps its open group byte for byte.  prep=None issues exactly the launches it did.

    `save(path)` / `StreamFleet.load(path, model, prep=)` (`state_dict()` / `load_state_dict(sd)`) carry a
    running fleet across a process boundary under StreamDetector's rules (§3.8e): states, tables in force, thresholds,
    logs, gap counters, rings, episode tables and clear levels, open groups, the counters and the configuration go into
    one .npz with a format number of its own; the static buffers of a push, the workspaces and the graphs do not.  A
    fleet stream cut by a save and a load writes the bits of the uninterrupted one.

    `prep=PrepUnits` gives every unit a min-max table of its own — pumps of one model with duty points,
    hence raw ranges, of their own: the same copy, counts write and replay, the leading launch
    gdn_fleet_prep_ticks_units (the same kernel body, reading tables[u]).  The contract per unit reads
    StreamDetector(prep=prep.unit(u), ...).  A checkpoint keeps the tables' fingerprint (`prep_units_sha256`, an optional
    key) and `load(path, model, prep=)` refuses a shared Prep for such a file, per-unit tables for a shared one, and other
    tables, by that name.

    Unit hand-over: `unit_state_dict(u)` is the dict StreamDetector.load_state_dict / load accepts (the
    unit leaves the fleet and goes on alone, bit for bit); `load_unit(u, sd)` takes a detector's state dict into unit u
    in place, through the pointers the captured graph reads (no recapture; every other unit's memory stays byte for
    byte); `reset_unit(u, med_iqr, threshold, history)` re-seeds one unit as the constructor seeds it.
    `localise(u, rows=None)` is StreamDetector.localise for unit u's real rows of the last sub-push.

    Out of scope: a command-line flag, more than one process."""

    def __init__(self, model, med_iqr, threshold, history, chunk: int, top_m: int = 1, log: int = 4096,
                 use_graph: bool = True, wide: bool | None = None, gaps: bool = False, events=None, recal: int = 0,
                 exclude_alarms: bool = True, recal_every: int = 0, recal_min: int | None = None,
                 calib: str = "tick", prep=None, recal_threshold=None):
        self._build(model, med_iqr, threshold, history, chunk, top_m, log, use_graph, wide, gaps, events, recal,
                    exclude_alarms, recal_every, recal_min, calib, prep, recal_threshold=recal_threshold)

    def _build(self, model, med_iqr, threshold, history, chunk, top_m, log, use_graph, wide, gaps, events, recal,
               exclude_alarms, recal_every, recal_min, calib, prep, units=None, device=None, recal_threshold=None):
        """The constructor's body.  `history=None` is load()'s private path: nothing is seeded — `units` states of
        zeros, the tables zeros, the thresholds inf and the clear levels 0, all on `device`, `wide` the caller's word —
        and load_state_dict fills the allocations."""
        self._set_calib(calib, gaps, recal)
        self.model = model.eval()
        w = model.gnn_layers[0].gnn.lin.weight.shape[1]
        n = model.embedding.weight.shape[0]
        seeded = history is not None
        if seeded:
            if not isinstance(history, torch.Tensor) or history.dim() != 3 or history.shape[1] != n:
                raise ValueError(f"expected a history of shape [U, {n}, h], got "
                                 f"{tuple(history.shape) if isinstance(history, torch.Tensor) else type(history)}")
            units = history.shape[0]
        units = int(units)
        fleet_check_shape(units, chunk, n, w)
        self.units, self.n, self.w, self.chunk, self.top_m = units, n, w, int(chunk), int(top_m)
        self.use_graph = bool(use_graph)
        self._check_lists(top_m, log, "entries per unit")
        if prep is not None:
            fleet_check_prep(prep, units, self.chunk, n)
        if seeded:
            if not isinstance(med_iqr, torch.Tensor) or med_iqr.shape != (units, n, 2):
                raise ValueError(f"expected med_iqr of shape [{units}, {n}, 2], got "
                                 f"{tuple(med_iqr.shape) if isinstance(med_iqr, torch.Tensor) else type(med_iqr)}")
            threshold = torch.as_tensor(threshold, dtype=torch.float64)
            if threshold.numel() not in (1, units) or threshold.dim() > 1:
                raise ValueError(f"threshold: one number or [{units}] of them, got {tuple(threshold.shape)}")
        # the options: host facts only, before any device work
        self._set_recal(recal, exclude_alarms, recal_every, recal_min,
                        lambda: _lib.load().gdn_fleet_calib_bytes(units, n, self.recal),
                        f"no calibration rings for units = {units}, n = {n}, R = {recal} (1 <= units <= 4096, "
                        "1 <= n <= 4096, 64 <= R <= 2^20, 8 units n R <= 2 GiB)")
        self._set_recal_threshold(recal_threshold)
        self.with_gaps = bool(gaps)
        self.events_cfg = None if events is None else events_config({**events, "lo": None}, self.top_m)
        if seeded:
            clear = None if events is None else fleet_clear_levels(events.get("lo"), threshold, units)
            if self.with_gaps and history.shape[2] >= w and not bool(torch.isfinite(history[:, :, -w:]).all()):
                raise ValueError(f"history: the last {w} ticks of a unit hold a value that is not finite; with "
                                 "gaps=True every missing reading is held at an earlier real one, so every unit's "
                                 "stream must begin on real readings")
        _check_stream_head(model)
        if seeded:
            history = ops._chk(history, name="history")
            dev = history.device
            self.med_iqr = ops._chk(med_iqr, torch.float64, name="med_iqr").clone()
            self.threshold = threshold.reshape(-1).expand(units).to(dev).clone()
            self.state = ops.fleet_state(history, w)
            self.wide = model.wide_for(history[:, :, -w:]) if wide is None else bool(wide)
        else:
            dev = torch.empty((0,), device=device).device           # ("cuda" -> the current device, with its index)
            clear = torch.zeros((units,), dtype=torch.float64)
            self.med_iqr = torch.zeros((units, n, 2), dtype=torch.float64, device=dev)
            self.threshold = torch.full((units,), float("inf"), dtype=torch.float64, device=dev)
            self.state = ops.fleet_state_empty(units, n, w, dev)
            self.wide = bool(wide)
        m = self.top_m
        self.counts = torch.zeros((units,), dtype=torch.int32, device=dev)
        self._alloc_push((units,), log, dev)
        self.events = self.clear = None
        if self.events_cfg is not None:
            self.events_cfg.pop("lo")
            self.clear = clear.to(dev)
            self.events = ops.fleet_events_alloc(units, m, self.events_cfg["cap"], dev)
        self.ring_keys = self.ring_keep = self._recal_ws = self.recal_kept = self.recal_counts = None
        if self.recal:
            self.ring_keys, self.ring_keep = ops.fleet_calib_ring(units, n, self.recal, dev)
            self._recal_ws = ops.fleet_select_workspace(units, n, self.recal, dev)
            # what the last recalibrate() counted, on the device: the kept ticks per unit (tick calibration) and the
            # count handed to the select per (unit, sensor); a unit left out through `units=` shows counts 0
            self.recal_kept = torch.zeros((units,), dtype=torch.int32, device=dev) if calib == "tick" else None
            self.recal_counts = torch.zeros((units, n), dtype=torch.int32, device=dev)
        if self.recal_threshold is not None:
            self._ring_buffers()
        self.recals = 0                     # calls of recalibrate()
        self._handed = 0                    # ticks per unit handed to push(): recal_every's clock
        self.calib_kept = None              # from_calibration(calib_gaps=True): per unit, the ticks behind the table
        self.calib_counts = None            # ... calib="sensor": every sensor's real readings behind it [U, n]
        self._full = _Replay(lambda *a: self._launch(*a), use_graph, lambda: model._constants().key,
                             args=lambda: (self._guarded(),))
        self._last = 0                      # ticks per unit of the last (sub-)push: what the static buffers hold
        self.prep = prep
        self._raw_handed = 0                # prep=: raw rows of the time axis handed to push()
        self._prep_full = {}                # prep=: raw dtype -> the push with the front end reading `_raw_stage`'s
        if prep is not None:
            if prep.table.device != dev:
                raise ValueError(f"prep: its table is on {prep.table.device}, the fleet on {dev}")
            self.pend = ops.fleet_prep_state(units, n, prep.down, dev)       # open groups and their lengths, per unit
            self.raw_counts = torch.zeros((units,), dtype=torch.int32, device=dev)
            self._raw_stage = {}            # raw dtype -> the static staging buffer [U, chunk * down, n] of its pushes

    @classmethod
    def from_calibration(cls, model, series, chunk: int, batch: int = 8192, calib_gaps: bool = False,
                         min_kept: int = 64, **kw):
        """A fleet calibrated on `series` [U, n, T] fp32 on the device, each unit's own period known to be normal: ONE
        SeriesEvaluator step per unit at construction (not a hot path) under the rules of
        StreamDetector.from_calibration — the table is that step's med_iqr, the threshold the largest anomaly score of
        the unit's period, the history its last w ticks.  `gaps=` and `events=` pass through; without `calib_gaps` the
        calibration itself knows no missing reading, so with gaps=True a series that is not finite is refused.
        `calib_gaps=True` (needs gaps=True), `min_kept=`, `calib="sensor"` (needs calib_gaps=True) and `recal=R` mean
        per unit what they mean to StreamDetector.from_calibration: the period is scored under the detector's own rules,
        the default history is the FILLED period's last w ticks, and unit u's ring is seeded as a detector's
        is (_seed_ring) — with the period's keep flags under calib_gaps, through its validity plane under
        calib="sensor".  `calib_kept` [U] int64 (host; None without calib_gaps) and `calib_counts` [U, n] int32 (device;
        calib="sensor") are the detectors' per unit."""
        calib = kw.get("calib", "tick")
        _check_calib(calib)
        _check_calib_gaps(calib, calib_gaps)
        _check_calib_period(series, calib_gaps, kw.get("gaps"), "fleet")
        series = ops._chk(series, name="series")
        w = model.gnn_layers[0].gnn.lin.weight.shape[1]
        if series.dim() != 3 or series.shape[2] <= w:
            raise ValueError(f"calibration needs a series [U, n, T] with T > {w}, got {tuple(series.shape)}")
        fleet_check_shape(series.shape[0], chunk, series.shape[1], w)
        R = int(kw.get("recal", 0))
        if calib == "sensor" and not R:
            kw["calib"] = "tick"            # no ring: the fleet never calibrates anything itself
        tables, thresholds, histories, seeds, kept, counts = [], [], [], [], [], []
        for unit in series:
            table, threshold, tail, k, cnt, rows = _calibrate_period(model, unit, w, batch, calib_gaps, min_kept, calib,
                                                                     bool(R))
            thresholds.append(threshold)
            tables.append(table.clone())
            histories.append(tail.clone())
            kept.append(k)
            counts.append(cnt)
            if R:                            # the rows _seed_ring would read: the period's last min(R, T - w)
                s = min(R, rows[0].shape[0])
                seeds.append(tuple(None if t is None else t[-s:].clone() for t in rows))
        history = kw.pop("history", None)
        fleet = cls(model, torch.stack(tables), torch.stack(thresholds),
                    torch.stack(histories) if history is None else history, chunk, **kw)
        if calib_gaps:
            fleet.calib_kept = torch.as_tensor([int(k) for k in kept], dtype=torch.int64)
        if calib == "sensor":
            fleet.calib_counts = torch.stack(counts)
        for u, rows in enumerate(seeds):
            _seed_ring(fleet.ring_keys[u], fleet.ring_keep[u], *rows)
        return fleet

    def _launch(self, guard: bool):
        rows = self.units * self.chunk
        if self.with_gaps:
            ops.fleet_fill(self.state, self.raw_buf, self.counts, self.w, self.chunk_buf, self.valid, self.gap_chunk)
        ops.fleet_windows(self.state, self.chunk_buf, self.counts, self.w, self.x)
        self.model.forward_into(self.x.view(rows, self.n, self.w), self.pred.view(rows, self.n), wide=self.wide,
                                guard=guard)
        # valid, gap_chunk and gaps are None on a plain fleet: the wrappers then call the plain symbols
        ops.fleet_score(self.state, self.pred, self.chunk_buf, self.med_iqr, self.threshold, self.counts, self.w,
                        self.top_m, self.top_scores, self.top_sensors, self.alarm, valid=self.valid)
        if self.events is not None:
            ops.fleet_events(self.state, self.top_scores, self.top_sensors, self.threshold, self.clear, self.counts,
                             self.n, self.w, self.events_cfg["on"], self.events_cfg["off"], self.events_cfg["cap"],
                             self.events)
        if self.recal:
            ops.fleet_calib_write(self.state, self.pred, self.chunk_buf, self.alarm, self.counts, self.w,
                                  self.ring_keys, self.ring_keep, self.exclude_alarms, valid=self.valid,
                                  by_sensor=self.calib == "sensor")
        ops.fleet_advance(self.state, self.chunk_buf, self.pred, self.med_iqr, self.alarm, self.top_sensors,
                          self.counts, self.w, self.top_m, self.log_ticks, self.log_sensors, valid=self.valid,
                          gap_chunk=self.gap_chunk, gaps=self.gaps)

    graph = property(lambda self: self._full.graph, doc="the captured push, None before the first one")
    _prep_graphs = property(lambda self: {dt: full.graph for dt, full in self._prep_full.items() if full.graph is not None},
                            doc="raw dtype -> the graph captured with the front end reading that dtype's staging buffer")

    def _launch_prep(self, stage, guard: bool):
        """gdn_fleet_prep_ticks over the staging buffer and the pending state (it writes `counts`), then the push."""
        ops.fleet_prep_ticks(stage, self.raw_counts, self.pend, self.prep.down, self.prep.table,
                             self.raw_buf if self.with_gaps else self.chunk_buf, self.counts)
        self._launch(guard)

    def _prep_stage(self, dtype):
        stage = self._raw_stage.get(dtype)
        if stage is None:
            fleet_check_prep(self.prep, self.units, self.chunk, self.n, torch.empty((), dtype=dtype).element_size())
            stage = self._raw_stage[dtype] = torch.zeros((self.units, self.chunk * self.prep.down, self.n), dtype=dtype,
                                                         device=self.state.device)
            self._prep_full[dtype] = _Replay(self._launch_prep, self.use_graph, self._full.key,
                                             args=lambda: (stage, self._guarded()))
        return stage, self._prep_full[dtype]

    def _write_counts(self, into, counts, s: int, r: int):
        """Sub-push from row `s` of the time axis, `r` rows long: every unit's clamp(counts[u] - s, 0, r) into `into`."""
        if counts is None:
            into.fill_(r)
        elif counts.is_cuda:
            torch.clamp(counts - s if s else counts, 0, r, out=into)
        else:
            into.copy_((counts - s).clamp_(0, r).to(torch.int32))

    def _push_prep(self, ticks, counts):
        down = self.prep.down
        stage, full = self._prep_stage(ticks.dtype)
        for s, rows, views in fleet_raw_cuts(ticks.shape[1], down, self.chunk):
            stage[:, :rows].copy_(ticks[:, s:s + rows])
            self._write_counts(self.raw_counts, counts, s, rows)
            self._last = views
            full()
            self._hand(fleet_raw_hand(self._raw_handed, rows, down))
            self._raw_handed += rows
        r = self._last
        return self.top_scores[:, :r], self.top_sensors[:, :r], self.alarm[:, :r]

    def push(self, ticks, counts=None):
        """Score `ticks` [U, r, n] fp32 (device or host), oldest first, r ticks per unit.  `counts`: None — every unit
        contributes all r ticks; a host sequence or tensor of U integers, checked here to lie in 0 .. r (ValueError
        before any device work); or a device int32 tensor [U], which the kernels clamp.  A unit's real rows are its
        FIRST counts[u] rows of `ticks`.  Returns views (top_scores [U, r', m] float64, top_sensors [U, r', m] int32,
        alarm [U, r'] int32) of the static buffers, valid until the next push; r' = r when r <= chunk, else the ticks of
        the last of the pushes it was split into.  Rows of the views at or beyond counts[u] are UNSPECIFIED (whatever an
        earlier push left there).
        prep=: `ticks` are RAW ticks, fp32 or float64, and `counts` RAW counts under the same three forms; a sub-push
        carries up to chunk * down raw rows and gives unit u clamp(counts[u] - its first row, 0, its rows).  `counts`
        (the fleet's buffer, on the device) then holds the model ticks each unit completed in the last sub-push, and the
        views cover min(chunk, (down - 1 + rows) // down) rows of it; rows at or beyond counts[u] are UNSPECIFIED."""
        counts = fleet_check_push(ticks, counts, self.units, self.n, raw=self.prep is not None)
        if self.prep is not None:
            return self._push_prep(ticks, counts)
        for s in range(0, ticks.shape[1], self.chunk):
            part = ticks[:, s:s + self.chunk]
            r = part.shape[1]
            (self.raw_buf if self.with_gaps else self.chunk_buf)[:, :r].copy_(part)
            self._write_counts(self.counts, counts, s, r)
            self._last = r
            self._full()
            self._hand(r)
        r = self._last
        return self.top_scores[:, :r], self.top_sensors[:, :r], self.alarm[:, :r]

    def _unit_mask(self, units):
        """recalibrate()'s `units`: None, a device uint8 / bool [U] mask (taken as it is) or a host sequence of unit
        indices (one small copy to the device)."""
        if units is None:
            return None
        if isinstance(units, torch.Tensor) and units.is_cuda:
            if units.dtype not in (torch.uint8, torch.bool) or units.shape != (self.units,):
                raise ValueError(f"units: a device mask must be uint8 or bool of shape [{self.units}], got {units.dtype} "
                                 f"{tuple(units.shape)}")
            return units.contiguous()
        idx = torch.as_tensor(units, dtype=torch.int64).reshape(-1)
        if idx.numel() and bool(((idx < 0) | (idx >= self.units)).any()):
            raise ValueError(f"units = {idx.tolist()}: the fleet has units 0 .. {self.units - 1}")
        mask = torch.zeros((self.units,), dtype=torch.uint8)
        mask[idx] = 1
        return mask.to(self.state.device)

    def recalibrate(self, units=None, threshold=None) -> None:
        """`threshold`: None — the constructor's `recal_threshold`; a number — a one-off margin; False —
        the tables only.  With a margin, two more launches after the select and still no host read: every unit that is
        selected and whose ring holds at least `recal_min` eligible ticks gets threshold[u] = margin times the largest
        smoothed score among them under its table in force (and with events= clear[u] = threshold[u] * clear_frac[u]);
        the others keep theirs.  `ring_peak`, `ring_eligible`, `ring_peak_slot` [U] on the device say what was found.
        Overwrite `med_iqr` [U, n, 2] in place from the calibration rings, per unit what
        StreamDetector.recalibrate() writes: tick calibration rewrites the table of every unit whose ring holds at
        least `recal_min` kept ticks, calib="sensor" the row of every (unit, sensor) with that many real keys; the other
        rows stay bit for bit.  `units`: None (all), a host sequence of unit indices or a device uint8 / bool [U] mask;
        a unit left out keeps its table.  A fixed number of launches and NO host read: gdn_fleet_ring_counts (sensor:
        gdn_score_key_counts, then the mask), then gdn_score_select_counts(min_count = recal_min) straight from the
        rings, one call per 65535 rows.  The counts stay on the device: `recal_kept` [U] int32 (tick calibration; a
        unit left out keeps its entry) and `recal_counts` [U, n] int32 (what the select was handed: 0 for a unit left
        out); `calibration()` reads them.  Thresholds, carries, logs, episode tables and the captured graph stay."""
        if not self.recal:
            raise ValueError("recalibrate(): the fleet was built with recal=0 and keeps no calibration rings")
        margin = self._margin(threshold)
        select = self._unit_mask(units)
        ops.fleet_ring_counts(self.ring_keys, self.ring_keep, self.recal_counts, self.recal_kept, select,
                              by_sensor=self.calib == "sensor")
        ops.fleet_select_counts(self.ring_keys, self.recal_counts, self.recal_min, self._recal_ws, self.med_iqr)
        if margin is not None:
            self._ring_threshold(margin, select)
        self.recals += 1

    def calibration(self):
        """(a copy of the tables in force [U, n, 2] float64 on the device, the counts of the last recalibrate() on the
        host: `recal_kept` [U] under tick calibration, `recal_counts` [U, n] under calib="sensor"; zeros before the
        first one).  ONE read (a synchronisation)."""
        if not self.recal:
            raise ValueError("calibration(): the fleet was built with recal=0 and keeps no calibration rings")
        return self.med_iqr.clone(), (self.recal_kept if self.calib == "tick" else self.recal_counts).cpu()

    def status(self):
        """Per unit (ticks [U], alarms [U], logged [U]) as host int64 tensors: ONE read of the counters (a
        synchronisation).  Unit u's log is log_ticks[u, :logged[u]] / log_sensors[u, :logged[u]]."""
        head = ops.fleet_state_views(self.state, self.units, self.n, self.w)[0].cpu()
        return head[:, 0].clone(), head[:, 1].clone(), head[:, 2].clone()

    def unit_state(self, u: int) -> torch.Tensor:
        """Unit u's slice of the state (a view): a single stream's state, the layout ops.stream_state_views reads."""
        return self.state[u]

    def status_gaps(self):
        """(missing_total [U, n] int64, missing_run [U, n] int64) on the host, gaps=True only: per unit what
        StreamDetector.status_gaps() returns.  ONE read (a synchronisation)."""
        if not self.with_gaps:
            raise ValueError("status_gaps(): the fleet was built with gaps=False and counts no missing readings")
        both = self.gaps.cpu()
        return both[:, 0], both[:, 1]

    def episodes(self, u: int) -> Episodes:
        """Unit u's episode table (events= only): views of the unit's block of the events allocation, read exactly as
        StreamDetector.episodes() reads a single stream's; a later push moves them."""
        if self.events is None:
            raise ValueError("episodes(): the fleet was built with events=None and keeps no episode tables")
        if not 0 <= int(u) < self.units:
            raise ValueError(f"episodes({u}): the fleet has units 0 .. {self.units - 1}")
        return _episodes(self.events[int(u)], self.top_m, self.events_cfg["cap"])

    # save and resume: a fleet stream cut by a save and a load writes the bits of the uninterrupted one
    def _expect(self, check_model: bool = True) -> dict:
        """fleet_checkpoint_check's `expect` for this fleet: its model's shape and fingerprint, its units, prep and
        events, and the loaded library's ABI version and byte sizes."""
        expect = _checkpoint_expect(self.model, self.prep, self.recal, check_model, units=self.units)
        expect["units"], expect["events"] = self.units, self.events_cfg
        expect["recal_threshold"] = self.recal_threshold
        return expect

    def _pend_views(self) -> tuple:
        """(the open groups [U, down, n] float64, their lengths [U, tiles] int32: one word per sensor tile of a unit)."""
        return ops.fleet_prep_views(self.pend, self.units, self.n, self.prep.down)

    def _ckpt_tensors(self) -> dict:
        """Checkpoint key -> the device tensor (a view) that holds it, unit axis first; an option that is off has no
        tensor and no key.  The lengths of the open groups are not in it: a file holds one per unit, the device one per
        sensor tile (_state_dict, load_state_dict, load_unit)."""
        held = {"state": self.state.view(torch.uint8).view(self.units, -1), "med_iqr": self.med_iqr,
                "threshold": self.threshold, "log_ticks": self.log_ticks, "log_sensors": self.log_sensors,
                "gaps": self.gaps, "ring_keys": self.ring_keys, "ring_keep": self.ring_keep,
                "recal_counts": self.recal_counts, "recal_kept": self.recal_kept, "events": self.events,
                "clear": self.clear, "clear_frac": None if self.recal_threshold is None else self.clear_frac,
                "calib_counts": self.calib_counts,
                "pending_ticks": None if self.prep is None else self._pend_views()[0]}
        return {k: t for k, t in held.items() if t is not None}

    def state_dict(self) -> dict:
        """Everything a continuation of this fleet depends on, as a flat dict of numpy arrays (numpy.savez writes it,
        numpy.load(allow_pickle=False) reads it), StreamDetector.state_dict's keys with a leading unit axis: `state`
        uint8 [U, state_bytes], `med_iqr`, `threshold`, the logs, `gaps`, the rings with `recal_kept` / `recal_counts`,
        `events` / `clear` / `events_cfg`, `calib_kept` / `calib_counts` where present, with prep= the open groups
        (`pending_ticks` [U, down, n] float64, `pending` [U] int32: tile 0's count, all tiles of a unit agree) and the
        raw rows handed; the host counters, the configuration, and the identity of what wrote it.  The staging, chunk,
        window, prediction and output buffers, gap_chunk, counts, the workspaces and the graphs stay behind.
        Read-only: ONE batch of device-to-host copies on the current stream and ONE synchronisation.
        prep=PrepUnits adds the optional `prep_units_sha256` (the tables' fingerprint)."""
        sd = self._state_dict(slice(None))
        if prep_units(self.prep) is not None:
            sd["prep_units_sha256"] = np.array(prep_units(self.prep))
        return sd

    def _state_dict(self, sel: slice) -> dict:
        """state_dict() of the units `sel` as a fleet of that many units (all of them: the fleet's own; one: what
        unit_state_dict converts), the host counters and the configuration the fleet's."""
        lib = _lib.load()
        U = len(range(*sel.indices(self.units)))
        dev = {k: t[sel] for k, t in self._ckpt_tensors().items()}
        if self.prep is not None:
            dev["pending"] = self._pend_views()[1][sel]
        sd, fingerprint = self._ckpt_read(dev)
        if self.calib_kept is not None:
            sd["calib_kept"] = torch.as_tensor(self.calib_kept, dtype=torch.int64).reshape(self.units)[sel].numpy().copy()
        if self.prep is not None:
            tiles = sd["pending"]
            assert (tiles == tiles[:, :1]).all(), "the pending counts of a unit's sensor tiles disagree"
            sd["pending"] = np.ascontiguousarray(tiles[:, 0])
        ints = {"format": FLEET_CHECKPOINT_FORMAT, "abi": lib.gdn_abi_version(),
                "state_bytes": lib.gdn_stream_state_bytes(self.n, self.w),
                "calib_bytes": lib.gdn_fleet_calib_bytes(U, self.n, self.recal) if self.recal else 0,
                "handed": self._handed, "raw_handed": self._raw_handed, "recals": self.recals}
        return self._ckpt_finish(sd, ints, _FLEET_CKPT_INTS, dict(self._config(), units=U), fingerprint)

    def load_state_dict(self, sd, check_model: bool = True) -> None:
        """Take the fleet stream of `sd` (state_dict()'s dict, or a file's) up where it was saved.  `sd` is checked first
        (fleet_checkpoint_check, and its configuration against this fleet's own, field by field: a ValueError that names
        the field, before any device work); the captured graphs are dropped; then every array is copied INTO the
        allocations this fleet already has, so the pointers a later capture records are the ones it always had.  A
        unit's pending count goes to every sensor tile's word.  Afterwards the last push is empty."""
        fleet_checkpoint_check(sd, self._expect(check_model))
        self._ckpt_same_config(fleet_checkpoint_config(sd), _FLEET_CKPT, "fleet")
        host = self._ckpt_fill(sd)
        if self.prep is not None:
            words = self._pend_views()[1]
            words.copy_(host("pending").view(-1, 1).expand(-1, words.shape[1]))
        self.calib_kept = host("calib_kept") if "calib_kept" in sd else None
        self._handed, self.recals = _ckpt_int(sd, "handed", _FLEET_CKPT), _ckpt_int(sd, "recals", _FLEET_CKPT)
        self._raw_handed = _ckpt_int(sd, "raw_handed", _FLEET_CKPT)

    def save(self, path: str) -> None:
        """state_dict() as one .npz at exactly `path` (write_stream_checkpoint: a temporary file beside it, then
        os.replace — a save that dies half-way leaves the previous checkpoint loadable)."""
        write_stream_checkpoint(path, self.state_dict())

    @classmethod
    def load(cls, path: str, model, prep=None, device="cuda", check_model: bool = True, use_graph: bool = True):
        """A fleet that continues the streams saved at `path`: built from the file's configuration, the caller's `model`
        and — when the file says one was used — `prep` (on `device`), with no history (nothing is seeded), then
        load_state_dict.  Refused with a ValueError that names the field, before any device work: an unknown format, a
        single detector's file, another ABI version or byte size, another n or w, a prep against the file's word or with
        another down, other weights (unless check_model=False), a missing key or an array of the wrong shape or dtype."""
        sd = read_stream_checkpoint(path)
        _fleet_ckpt_format(sd)                              # (an unknown format first: its other fields may differ)
        units, R = _ckpt_int(sd, "units", _FLEET_CKPT), _ckpt_int(sd, "recal", _FLEET_CKPT)
        if units < 1 or R < 0:
            raise ValueError(f"{_FLEET_CKPT}: units = {units}, recal = {R}: at least one unit, no negative ring")
        fleet_checkpoint_check(sd, _checkpoint_expect(model, prep, R, check_model, units=units))
        cfg = fleet_checkpoint_config(sd)
        events = fleet_checkpoint_events(sd)                # (None: the file has no episode tables, nor has the fleet)
        if events is not None:
            events = {k: events[k] for k in ("on", "off", "cap")}
        fleet = cls.__new__(cls)
        fleet._build(model, None, None, None, cfg["chunk"], cfg["top_m"], cfg["log"], use_graph, bool(cfg["wide"]),
                     bool(cfg["with_gaps"]), events, cfg["recal"], bool(cfg["exclude_alarms"]), cfg["recal_every"],
                     cfg["recal_min"] if cfg["recal"] else None, cfg["calib"], prep, units=units, device=device,
                     recal_threshold=checkpoint_recal_threshold(sd, _FLEET_CKPT))
        fleet.load_state_dict(sd, check_model=False)        # (the weights were compared above, once)
        return fleet

    # unit hand-over: unit u's block of every allocation is a single stream's byte for byte
    def _unit(self, u, what: str) -> int:
        if not 0 <= int(u) < self.units:
            raise ValueError(f"{what}({u}): the fleet has units 0 .. {self.units - 1}")
        return int(u)

    def unit_prep(self, u: int):
        """The prep a detector of unit `u` takes: prep.unit(u) under per-unit tables, else the fleet's own (or None)."""
        return self.prep.unit(u) if getattr(self.prep, "tables", None) is not None else self.prep

    def unit_state_dict(self, u: int) -> dict:
        """Unit `u` as the state dict of a single detector (fleet_unit_to_stream of that unit's slice of state_dict()):
        StreamDetector.load_state_dict / load accept it — with the fleet's model and `unit_prep(u)` — and the detector,
        pushed the unit's later ticks in the same cuts, writes the bits unit u writes in the fleet that went on; its
        recal_every clock starts from the fleet's.  Read-only: ONE batch of copies of that unit's blocks alone and ONE
        synchronisation."""
        u = self._unit(u, "unit_state_dict")
        return fleet_unit_to_stream(self._state_dict(slice(u, u + 1)), 0)

    def _config_dict(self, model_sha256: str) -> dict:
        """What stream_to_fleet_unit reads of a fleet's state dict, from host facts alone (no device read)."""
        lib = _lib.load()
        sd = {k: np.array(int(v), dtype=np.int64) for k, v in self._config().items() if k != "calib"}
        sd.update(format=np.array(FLEET_CHECKPOINT_FORMAT, dtype=np.int64), calib=np.array(self.calib),
                  abi=np.array(lib.gdn_abi_version(), dtype=np.int64), model_sha256=np.array(model_sha256),
                  state_bytes=np.array(lib.gdn_stream_state_bytes(self.n, self.w), dtype=np.int64))
        if self.events is not None:
            sd["events_cfg"] = np.array([self.events_cfg[k] for k in _EVENTS_FIELDS], dtype=np.int64)
        if self.recal_threshold is not None:
            sd["recal_threshold"] = np.array(self.recal_threshold, dtype=np.float64)
        return sd

    def _clear_frac_unit(self, u: int, frac=None):
        """clear_frac[u] under recal_threshold= and events=: `frac`, else lo / threshold of the unit's levels as they
        stand (_ring_buffers' rule); the other units' fractions come into being as they would have at their next use."""
        if self.recal_threshold is None or self.events is None:
            return
        self._ring_buffers()
        if frac is None:
            frac = self.clear[u] / self.threshold[u]
            frac = torch.where(torch.isfinite(frac) & (frac <= 1.0), frac, torch.ones_like(frac))
        self.clear_frac[u].copy_(frac)

    def load_unit(self, u: int, sd, check_model: bool = True) -> None:
        """Take the stream of a detector's state dict `sd` (StreamDetector.state_dict(), or a file's) into unit `u`, IN
        PLACE: every array goes into unit u's block of the allocations the captured graph reads, so nothing is
        recaptured and every other unit's memory stays byte for byte.  Checked first, before any device write
        (stream_to_fleet_unit, then stream_checkpoint_check against unit_prep(u)): n, w, top_m, log, gaps, recal and its
        flags, calib, wide (the route is per launch), prep / down, events, recal_threshold, the model's fingerprint
        (unless check_model=False) and the ABI version must be the fleet's — a ValueError names the field.  chunk and
        recal_every are the fleet's: unit u goes on as the detector would have alone, on the fleet's clock.  Afterwards
        unit u has no rows in the static buffers of the last push (counts[u] = 0: localise(u) is empty)."""
        u = self._unit(u, "load_unit")
        expect = _checkpoint_expect(self.model, self.unit_prep(u), self.recal, check_model)
        expect["events"], expect["recal_threshold"] = self.events_cfg, self.recal_threshold
        sha = expect["model"] if check_model else _ckpt_str(sd, "model_sha256")
        unit = stream_to_fleet_unit(sd, self._config_dict(sha))
        stream_checkpoint_check(sd, expect)

        def host(key):
            return torch.from_numpy(np.array(unit[key]))             # (a copy: numpy.load may hand out read-only arrays)
        held = self._ckpt_tensors()
        held.pop("clear_frac", None)                                 # (it may not exist yet: _clear_frac_unit below)
        if self.prep is not None:
            p = int(unit["pending"])
            held.pop("pending_ticks")[u, :p].copy_(host("pending_ticks"))    # the rows of the open group only
            self._pend_views()[1][u].fill_(p)
        for k, t in held.items():
            if k in unit:                                            # (calib_counts: only a detector that has them)
                t[u].copy_(host(k))
        self._clear_frac_unit(u, host("clear_frac").to(self.state.device) if "clear_frac" in unit else None)
        if self.calib_kept is not None and "calib_kept" in unit:
            self.calib_kept[u] = int(unit["calib_kept"])
        self.counts[u] = 0

    def reset_unit(self, u: int, med_iqr, threshold, history, lo=None, seed=None) -> None:
        """Re-seed unit `u` as the constructor seeds a unit — a pump repaired or replaced: `med_iqr` [n, 2] float64,
        `threshold` one number, `history` [n, h >= w] fp32 on the device (the state starts after its last w ticks, counters
        and carry zero).  The unit's log and gap counters are emptied, its ring is emptied or — `seed` = (pred, gt, keep,
        valid), the rows from_calibration seeds a ring from (_seed_ring) — seeded, its episode table is emptied with the
        clear level `lo` (None: the threshold) and no raw group stays open.  Afterwards unit u equals a fresh
        StreamDetector(model, med_iqr, threshold, history, ...) of the fleet's options; the other units, the fleet's
        `wide` word, its clocks and the captured graph are untouched.  Refused before any write to the fleet: another
        shape, gaps=True with a non-finite tail of `history` (as the constructor refuses it), a `lo` above the threshold
        or without events=, a `seed` without a ring."""
        u = self._unit(u, "reset_unit")
        n, w = self.n, self.w
        history = ops._chk(history, name="history")
        if history.dim() != 2 or history.shape[0] != n:
            raise ValueError(f"expected a history of shape [{n}, h], got {tuple(history.shape)}")
        med_iqr = ops._chk(med_iqr, torch.float64, name="med_iqr")
        if med_iqr.shape != (n, 2):
            raise ValueError(f"expected med_iqr of shape [{n}, 2], got {tuple(med_iqr.shape)}")
        threshold = torch.as_tensor(threshold, dtype=torch.float64)
        if threshold.numel() != 1:
            raise ValueError(f"threshold: one number for one unit, got {tuple(threshold.shape)}")
        if self.events is None and lo is not None:
            raise ValueError(f"lo = {lo!r}: the fleet was built with events=None and keeps no clear level")
        if seed is not None and not self.recal:
            raise ValueError("seed: the fleet was built with recal=0 and keeps no calibration rings")
        clear = None if self.events is None else fleet_clear_levels(lo, threshold, 1)
        if self.with_gaps and history.shape[1] >= w and not bool(torch.isfinite(history[:, -w:]).all()):
            raise ValueError(f"history: its last {w} ticks hold a value that is not finite; with gaps=True every missing "
                             "reading is held at an earlier real one, so the unit's stream must begin on real readings")
        state = ops.stream_state(history, w)                          # (a history shorter than w is refused here)
        self.state[u].copy_(state)
        self.med_iqr[u].copy_(med_iqr)
        self.threshold[u].copy_(threshold.reshape(()))
        if self.log_ticks is not None:
            self.log_ticks[u].zero_()
            self.log_sensors[u].zero_()
        if self.with_gaps:
            self.gaps[u].zero_()
        if self.recal:
            self.ring_keys[u].view(torch.int64).fill_(-1)            # all ones: the filler (ops.stream_calib_ring)
            self.ring_keep[u].zero_()
            self.recal_counts[u].zero_()
            if self.recal_kept is not None:
                self.recal_kept[u].zero_()
            if seed is not None:
                _seed_ring(self.ring_keys[u], self.ring_keep[u], *seed)
        if self.events is not None:
            self.events[u].zero_()
            self.clear[u].copy_(clear[0])
            self._clear_frac_unit(u)
        if self.prep is not None:
            ops.fleet_prep_views(self.pend, self.units, n, self.prep.down)[1][u].zero_()
        self.counts[u] = 0

    def localise(self, u: int, rows=None) -> Localisation:
        """StreamDetector.localise for unit `u`'s real rows of the last sub-push: which sensors deviate at its alarm rows
        (`rows=None`; or the given rows, refused at or beyond counts[u]) and which neighbours they were reading — ONE
        model.attention_at on the fleet's static window buffer.  The fields are a detector's of that unit (`ticks`: the
        unit's own stream ticks; under gaps=True `observed` is the FILLED reading).  A silent unit returns an empty
        result.  ONE read of counts[u] (a synchronisation)."""
        u = self._unit(u, "localise")
        r = min(max(int(self.counts[u]), 0), self._last)
        if rows is None:
            rows = torch.nonzero(self.alarm[u, :r]).view(-1)
        rows = _row_indices(rows, self.state.device, r, f"rows outside [0, {r}): unit {u} has counts[{u}] = {r} real "
                            "rows in the last push")
        first = self.state[u, 0] - r                        # (advance has run: ticks counts the push already)
        c, n = self.chunk, self.n
        flat = self.units * c
        return _localisation(self.model, self.x.view(flat, n, self.w), first + rows, u * c + rows,
                             self.top_sensors[u, rows].long(), self.top_scores[u, rows], self.pred.view(flat, n),
                             self.chunk_buf.view(flat, n))
