"""The checkpoint of a running StreamDetector or StreamFleet: a flat dict of numpy arrays, one .npz, no
Python objects.  Host code only.

A checkpoint is described ONCE: two `Kind` records (a detector's file, a fleet's file) and the table `ENTRIES` of the
arrays a file holds — under which key per kind, of which dtype, of which shape, under which options.  A fleet's file is
the detector's rules with a leading unit axis; every real difference between the two is a row of the table or a field
of a record.  The checkers, the configuration and events readers and the unit hand-over converters all walk it; the two
classes of harness.py map the same keys to their device tensors (`_ckpt_tensors`).  A new option's key is added here."""
from __future__ import annotations

import contextlib
import hashlib
import os
from typing import Callable, NamedTuple

import numpy as np
import torch

STREAM_CHECKPOINT_FORMAT = 1
# a fleet's file has a format number of its own; a detector's file has no "units", a fleet's file holds
# keys a detector's checker calls foreign
FLEET_CHECKPOINT_FORMAT = 1
# 0-d int64: identity, the configuration, the host counters (calib_kept: -1 for None; prep_down: 0 without a prep)
_CKPT_INTS = ("format", "abi", "state_bytes", "calib_bytes", "n", "w", "chunk", "top_m", "log", "with_gaps", "recal",
              "exclude_alarms", "recal_every", "recal_min", "wide", "prep", "prep_down", "handed", "recals",
              "recal_kept", "calib_kept", "raw_pending")
_CKPT_STRS = ("calib", "model_sha256")
_CKPT_CONFIG = ("n", "w", "chunk", "top_m", "log", "with_gaps", "recal", "exclude_alarms", "recal_every", "recal_min",
                "calib", "wide", "prep", "prep_down")
_FLEET_CKPT = "fleet checkpoint"
_FLEET_CKPT_INTS = ("format", "units", "abi", "state_bytes", "calib_bytes", "n", "w", "chunk", "top_m", "log",
                    "with_gaps", "recal", "exclude_alarms", "recal_every", "recal_min", "wide", "prep", "prep_down",
                    "handed", "raw_handed", "recals")
_FLEET_CKPT_STRS = ("calib", "model_sha256")
_FLEET_CKPT_CONFIG = ("units", "n", "w", "chunk", "top_m", "log", "with_gaps", "recal", "exclude_alarms", "recal_every",
                      "recal_min", "calib", "wide", "prep", "prep_down")
_EVENTS_FIELDS = ("on", "off", "cap", "m")


class Kind(NamedTuple):
    """One kind of checkpoint: how it is called, its format number, its 0-d keys, and the words its refusals use."""
    who: str
    format: int
    ints: tuple                 # 0-d int64 keys
    strs: tuple                 # 0-d string keys
    config: tuple               # the keys of the configuration it was saved under
    units: bool                 # the leading shape of every per-unit array: False — (), True — (units,)
    optional_strs: tuple        # 0-d string keys a file may hold
    counters: tuple             # the ints refused when negative (the fleet's list is the longer one: an open drift)
    noun: str
    tables: str                 # ... its refusals about events speak of (the wording differs: an open drift)
    resumed: tuple


DETECTOR = Kind("stream checkpoint", STREAM_CHECKPOINT_FORMAT, _CKPT_INTS, _CKPT_STRS, _CKPT_CONFIG, False, (),
                ("handed", "recals", "recal_kept", "log", "recal", "recal_every", "recal_min"),
                "detector", "an episode table", ("with one", "without one"))
FLEET = Kind(_FLEET_CKPT, FLEET_CHECKPOINT_FORMAT, _FLEET_CKPT_INTS, _FLEET_CKPT_STRS, _FLEET_CKPT_CONFIG, True,
             ("prep_units_sha256",),
             ("handed", "raw_handed", "recals", "log", "recal", "recal_every", "recal_min", "chunk", "top_m"),
             "fleet", "episode tables", ("with them", "without them"))


def events_bytes(m: int, cap: int) -> int:
    """gdn_stream_events_bytes(m, cap) by host arithmetic: the carry, four 8-byte columns and the sensors."""
    return (160 + 32 * cap + 4 * cap * m + 7) & ~7


def stream_calib_bytes(n: int, R: int) -> int:
    """gdn_stream_calib_bytes(n, R) by host arithmetic (0 without a ring): the keys, the keep flags, 8-byte padding."""
    return (8 * n * R + R + 7) & ~7 if R else 0


def always(p) -> bool:
    return True


def never(p) -> bool:
    return False


class Entry(NamedTuple):
    """One array of a checkpoint.  `det` / `fleet`: its key in a detector's / a fleet's file (None: that kind has none).
    `dtype`: one, or (detector's, fleet's).  `shape(i, lead)`: its shape from the file's ints `i` (plus `open_rows` and
    `events_cap`) under the leading shape `lead`.  `required(p)` / `allowed(p)`: whether the options `p` of the file
    (`present`) demand it / admit it.  `per_unit`: it has the unit axis; `scalar`: one number per unit, which a
    detector's file keeps as (1,); `raw`: bytes that the two kinds read as different words."""
    det: str | None
    fleet: str | None
    dtype: object
    shape: Callable
    required: Callable
    allowed: Callable | None = None         # None: only when required
    per_unit: bool = True
    scalar: bool = False
    raw: bool = False

    def key(self, kind: Kind):
        return self.fleet if kind.units else self.det

    def np_dtype(self, kind: Kind):
        return np.dtype(self.dtype[kind.units] if isinstance(self.dtype, tuple) else self.dtype)

    def admits(self, p) -> bool:
        return self.required(p) or (self.allowed is not None and self.allowed(p))


def _one(i, lead):
    return lead or (1,)


def _ring(p) -> bool:
    return bool(p["recal"])


_EVENTS = Entry("events", "events", (np.uint8, np.int64),
                lambda i, lead: lead + (events_bytes(i["top_m"], i["events_cap"]) // (8 if lead else 1),),
                lambda p: p["events"], raw=True)
_CLEAR = Entry("events_lo", "clear", np.float64, _one, lambda p: p["events"], scalar=True)
_EVENTS_CFG = Entry("events_cfg", "events_cfg", np.int64, lambda i, lead: (len(_EVENTS_FIELDS),), lambda p: p["events"],
                    per_unit=False)
_PENDING_TICKS = Entry("pending", "pending_ticks", np.float64, lambda i, lead: lead + (i["open_rows"], i["n"]),
                       lambda p: p["prep"])
_PENDING = Entry(None, "pending", np.int32, lambda i, lead: lead, lambda p: p["prep"])
_RECAL_KEPT = Entry(None, "recal_kept", np.int32, lambda i, lead: lead, lambda p: _ring(p) and p["tick"])
_CALIB_KEPT = Entry(None, "calib_kept", np.int64, lambda i, lead: lead, never, always)
# the order of the rows is the order in which a missing or misshapen key is named: the required ones, then the others
ENTRIES = (
    Entry("state", "state", np.uint8, lambda i, lead: lead + (i["state_bytes"],), always),
    Entry("med_iqr", "med_iqr", np.float64, lambda i, lead: lead + (i["n"], 2), always),
    Entry("threshold", "threshold", np.float64, _one, always, scalar=True),
    Entry("log_ticks", "log_ticks", np.int64, lambda i, lead: lead + (i["log"],), always),
    Entry("log_sensors", "log_sensors", np.int32, lambda i, lead: lead + (i["log"], i["top_m"]), always),
    Entry("gaps", "gaps", np.int64, lambda i, lead: lead + (2, i["n"]), lambda p: p["with_gaps"]),
    Entry("ring_keys", "ring_keys", np.float64, lambda i, lead: lead + (i["n"], i["recal"]), _ring),
    Entry("ring_keep", "ring_keep", np.uint8, lambda i, lead: lead + (i["recal"],), _ring),
    # a fleet keeps the counts of its last recalibrate() on the device under both calibrations and `recal_kept` per unit;
    # a detector keeps `recal_kept` as an int and the counts (calib="sensor", after a recalibrate()) as a host array
    Entry(None, "recal_counts", np.int32, lambda i, lead: lead + (i["n"],), _ring),
    _RECAL_KEPT,
    _PENDING_TICKS,             # the raw ticks of the open group: a detector's rows are raw_pending, a unit's prep_down
    _PENDING,                   # ... whose number a detector keeps as the int raw_pending
    _EVENTS,
    _CLEAR,
    _EVENTS_CFG,
    _CALIB_KEPT,                # (a detector keeps it as an int, -1: none)
    Entry("calib_counts", "calib_counts", np.int32, lambda i, lead: lead + (i["n"],), never, always),
    Entry("recal_counts", None, np.int64, lambda i, lead: (i["n"],), never, always),
    Entry("recal_threshold", "recal_threshold", np.float64, lambda i, lead: (), never, always, per_unit=False),
    Entry("clear_frac", "clear_frac", np.float64, _one, never, always, scalar=True),
)


def present(kind: Kind, sd, ints, calib: str, events=...) -> dict:
    """The options of a file that decide which entries it holds."""
    if events is ...:
        events = _events(kind, sd)
    return {"with_gaps": bool(ints["with_gaps"]), "recal": ints["recal"], "tick": calib == "tick",
            "prep": bool(ints["prep"]), "events": events is not None}


# --------------------------------------------------------------------------- the model's fingerprint
def _host_copies(tensors) -> list:
    """Host copies of `tensors`, issued and not waited for: a device tensor goes into pinned memory with a
    non-blocking copy on the current stream (the caller synchronises ONCE before reading any), a host tensor is
    taken as it is."""
    out = []
    for t in tensors:
        t = t.detach()
        if t.is_cuda:
            out.append(torch.empty(t.shape, dtype=t.dtype, pin_memory=True).copy_(t, non_blocking=True))
        else:
            out.append(t)
    return out


def _fingerprint(names, host) -> str:
    h = hashlib.sha256()
    for name, t in zip(names, host):
        h.update(f"{name}|{t.dtype}|{tuple(t.shape)}|".encode())
        h.update(t.contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def model_fingerprint(model) -> str:
    """SHA-256 (hex) over the model's state_dict: every tensor in key order as its name, dtype, shape and bytes.  Equal
    for equal weights on any device; one changed bit of a parameter or of a BatchNorm running statistic changes it.
    Device tensors are read in one batch of copies and ONE synchronisation."""
    sd = model.state_dict()
    names = sorted(sd)
    host = _host_copies([sd[k] for k in names])
    if any(sd[k].is_cuda for k in names):
        torch.cuda.current_stream().synchronize()
    return _fingerprint(names, host)


def prep_units(prep):
    """The fingerprint of a per-unit prep's tables (PrepUnits.fingerprint), None for a shared Prep or no prep at all:
    what tells the two forms apart on the host."""
    return prep.fingerprint() if getattr(prep, "tables", None) is not None else None


# --------------------------------------------------------------------------- reading the 0-d keys
def _ckpt_int(sd, key: str, who: str = "stream checkpoint") -> int:
    if key not in sd:
        raise ValueError(f"{who}: key {key!r} is missing (a truncated or foreign file)")
    a = np.asarray(sd[key])
    if a.dtype != np.int64 or a.shape != ():
        raise ValueError(f"{who}: {key!r} must be one int64, got {a.dtype} {a.shape}")
    return int(a)


def _ckpt_str(sd, key: str, who: str = "stream checkpoint") -> str:
    if key not in sd:
        raise ValueError(f"{who}: key {key!r} is missing (a truncated or foreign file)")
    a = np.asarray(sd[key])
    if a.dtype.kind != "U" or a.shape != ():
        raise ValueError(f"{who}: {key!r} must be one string, got {a.dtype} {a.shape}")
    return str(a)


def checkpoint_recal_threshold(sd, who: str = "stream checkpoint"):
    """The margin a checkpoint (a detector's or a fleet's) was saved with under recal_threshold=, None
    for a file saved without it — every file written before the option existed.  Host data only."""
    if "recal_threshold" not in sd:
        return None
    a = np.asarray(sd["recal_threshold"])
    if a.dtype != np.float64 or a.shape != () or not (np.isfinite(a) and a > 0):
        raise ValueError(f"{who}: 'recal_threshold' must be one finite float64 > 0, got {a.dtype} {a.shape} {a!r}")
    return float(a)


def _check_recal_threshold(sd, expect, recal: int, events, who: str):
    """What the checker refuses about the optional keys of recal_threshold=: `recal_threshold` without a ring,
    `clear_frac` without it or without episode tables, and — against a detector or fleet that exists already — a
    margin on one side only, or another one.  The shapes are checked with the other optional keys."""
    margin = checkpoint_recal_threshold(sd, who)
    if margin is not None and not recal:
        raise ValueError(f"{who}: recal_threshold = {margin} without a calibration ring (recal = 0)")
    if "clear_frac" in sd and (margin is None or events is None):
        raise ValueError(f"{who}: key 'clear_frac' without recal_threshold and events (a truncated or foreign file)")
    if "recal_threshold" in expect:                         # (load() builds from the file: nothing to compare)
        mine = expect["recal_threshold"]
        if margin != mine:
            raise ValueError(f"{who}: recal_threshold = {margin}, this one was built with recal_threshold = {mine} "
                             "(the threshold in the file was, or was not, re-derived from the ring)")


def _format(kind: Kind, sd) -> None:
    fmt = _ckpt_int(sd, "format", kind.who)
    if fmt != kind.format:
        raise ValueError(f"{kind.who}: format = {fmt} is not known to this version (it reads format {kind.format})")
    if kind.units and "units" not in sd:
        raise ValueError(f"{kind.who}: key 'units' is missing: this is a single detector's checkpoint "
                         "(StreamDetector.load reads it)")


def _config(kind: Kind, sd) -> dict:
    cfg = {k: _ckpt_str(sd, k, kind.who) if k in kind.strs else _ckpt_int(sd, k, kind.who) for k in kind.config}
    if cfg["calib"] not in ("tick", "sensor"):
        raise ValueError(f"{kind.who}: calib = {cfg['calib']!r}: 'tick' or 'sensor'")
    return cfg


def _events(kind: Kind, sd):
    who = kind.who
    names = [e.key(kind) for e in (_EVENTS, _EVENTS_CFG, _CLEAR)]
    keys = [k for k in names if k in sd]
    if not keys:
        return None
    if len(keys) != 3:
        raise ValueError(f"{who}: key {keys[0]!r} without the rest of {', '.join(names)} (a truncated or foreign file)")
    cfg = np.asarray(sd[names[1]])
    if cfg.dtype != np.int64 or cfg.shape != (len(_EVENTS_FIELDS),):
        raise ValueError(f"{who}: 'events_cfg' must be int64 ({len(_EVENTS_FIELDS)},), got {cfg.dtype} {cfg.shape}")
    if not kind.units:                                      # (one clear level: a part of the detector's events=)
        lo = np.asarray(sd[names[2]])
        if lo.dtype != np.float64 or lo.shape != (1,):
            raise ValueError(f"{who}: 'events_lo' must be float64 (1,), got {lo.dtype} {lo.shape}")
    out = {k: int(v) for k, v in zip(_EVENTS_FIELDS, cfg)}
    if not (1 <= out["on"] <= 4096 and 1 <= out["off"] <= 4096 and 0 <= out["cap"] <= 1 << 20 and 1 <= out["m"] <= 8):
        raise ValueError(f"{who}: events_cfg = {out} outside 1 <= on, off <= 4096, 0 <= cap <= 2^20, 1 <= m <= 8")
    if not kind.units:
        out["lo"] = float(lo[0])
    return out


def _ckpt_format(sd) -> None:
    _format(DETECTOR, sd)


def _fleet_ckpt_format(sd) -> None:
    _format(FLEET, sd)


def stream_checkpoint_config(sd) -> dict:
    """The configuration a checkpoint was saved under (`_CKPT_CONFIG`) as Python values; a missing or mistyped field
    is refused by name.  Host data only."""
    return _config(DETECTOR, sd)


def fleet_checkpoint_config(sd) -> dict:
    """The configuration a fleet checkpoint was saved under (`_FLEET_CKPT_CONFIG`) as Python values; a missing or
    mistyped field is refused by name.  Host data only."""
    return _config(FLEET, sd)


def stream_checkpoint_events(sd):
    """The events configuration of a checkpoint ({"on", "off", "cap", "m", "lo"}), None for a file saved without an
    episode table; the three optional keys come together or not at all.  Host data only."""
    return _events(DETECTOR, sd)


def fleet_checkpoint_events(sd):
    """The events configuration of a fleet checkpoint ({"on", "off", "cap", "m"}), None for a file saved without episode
    tables; `events`, `events_cfg` and `clear` come together or not at all.  Host data only."""
    return _events(FLEET, sd)


# --------------------------------------------------------------------------- the checker
def _check(kind: Kind, sd, expect) -> None:
    """The one body of stream_checkpoint_check and fleet_checkpoint_check.  The order of the checks decides which field
    a doubly wrong file is refused for."""
    who = kind.who
    _format(kind, sd)
    ints = {k: _ckpt_int(sd, k, who) for k in kind.ints}
    strs = {k: _ckpt_str(sd, k, who) for k in kind.strs}
    cfg = _config(kind, sd)
    lead = ()
    if kind.units:
        lead = (ints["units"],)
        if lead[0] < 1:
            raise ValueError(f"{who}: units = {lead[0]}: a fleet has at least one unit")
        if expect.get("units") is not None and lead[0] != int(expect["units"]):
            raise ValueError(f"{who}: units = {lead[0]}, this fleet has units = {int(expect['units'])}")
    for k in ("n", "w"):                                    # (first: the byte sizes below are those of the model's n, w)
        if ints[k] != int(expect[k]):
            raise ValueError(f"{who}: {k} = {ints[k]}, the model has {k} = {int(expect[k])}")
    for k in ("abi", "state_bytes", "calib_bytes"):
        if ints[k] != int(expect[k]):
            raise ValueError(f"{who}: {k} = {ints[k]} was saved by another build of the library (this one has {k} = "
                             f"{int(expect[k])}); the state's layout is not known to agree")
    down = expect.get("prep_down")
    if bool(ints["prep"]) != (down is not None):
        raise ValueError(f"{who}: prep: the {kind.noun} was saved " + ("with" if ints["prep"] else "without")
                         + " a raw-readings front end and is resumed " + ("without one (pass prep=)" if ints["prep"]
                                                                          else "with one (pass prep=None)"))
    if down is not None:
        if ints["prep_down"] != int(down):
            raise ValueError(f"{who}: prep_down = {ints['prep_down']}, the prep given has down = {int(down)}")
        if int(expect.get("prep_n", ints["n"])) != ints["n"]:
            raise ValueError(f"{who}: prep: fitted on {int(expect['prep_n'])} sensors, n = {ints['n']}")
    elif ints["prep_down"] != 0:
        raise ValueError(f"{who}: prep_down = {ints['prep_down']} without a prep")
    if kind.units:                                          # per-unit prep tables: a fleet's alone
        tables = _ckpt_str(sd, "prep_units_sha256", who) if "prep_units_sha256" in sd else None
        if tables is not None and not ints["prep"]:
            raise ValueError(f"{who}: key 'prep_units_sha256' without a prep (a truncated or foreign file)")
        if down is not None and tables != expect.get("prep_units"):
            if tables is None or expect.get("prep_units") is None:
                raise ValueError(f"{who}: prep_units_sha256: the fleet was saved with " + (
                    "one shared prep table and is resumed with per-unit tables (pass the Prep)" if tables is None else
                    "per-unit prep tables and is resumed with one shared Prep (pass the PrepUnits)"))
            raise ValueError(f"{who}: prep_units_sha256 differs from the per-unit tables given: the open groups and the "
                             "scores behind the state were normalised with other tables")
    if expect.get("model") is not None and strs["model_sha256"] != expect["model"]:
        raise ValueError(f"{who}: model_sha256 differs from the model given: the scores are the model's, so resuming "
                         "under other weights changes the alarm rate (check_model=False resumes all the same)")
    if not kind.units and not 0 <= ints["raw_pending"] < max(1, ints["prep_down"]):
        raise ValueError(f"{who}: raw_pending = {ints['raw_pending']} outside an open group of prep_down = "
                         f"{ints['prep_down']} raw ticks")
    for k in kind.counters:
        if ints[k] < 0:
            raise ValueError(f"{who}: {k} = {ints[k]} is negative")
    if not kind.units and ints["calib_kept"] < -1:
        raise ValueError(f"{who}: calib_kept = {ints['calib_kept']} (-1: none)")
    if kind.units and not cfg["prep"] and ints["raw_handed"] != 0:
        raise ValueError(f"{who}: raw_handed = {ints['raw_handed']} without a prep")
    events = _events(kind, sd)
    if "events" in expect:                                  # (load() builds the object from the file: nothing to compare)
        mine = expect["events"]
        if (events is None) != (mine is None):
            raise ValueError(f"{who}: events: the {kind.noun} was saved " + ("without" if events is None else "with")
                             + f" {kind.tables} and is resumed "
                             + (f"{kind.resumed[0]} (pass events=None)" if events is None
                                else f"{kind.resumed[1]} (pass events=)"))
        for k in _EVENTS_FIELDS if events is not None else ():
            if events[k] != int(mine[k]):
                raise ValueError(f"{who}: events.{k} = {events[k]}, this {kind.noun} was built with events.{k} = "
                                 f"{int(mine[k])}")
    if events is not None and events["m"] != ints["top_m"]:
        raise ValueError(f"{who}: events.m = {events['m']}, top_m = {ints['top_m']}")
    _check_recal_threshold(sd, expect, ints["recal"], events, who)
    p = present(kind, sd, ints, cfg["calib"], events)
    i = dict(ints, open_rows=ints["prep_down"] if kind.units else ints["raw_pending"],
             events_cap=events["cap"] if events is not None else 0)
    table = [e for e in ENTRIES if e.key(kind) is not None]
    known = {e.key(kind) for e in table if e.admits(p)} | set(kind.ints) | set(kind.strs) | set(kind.optional_strs)
    for k in sd:
        if k not in known:
            raise ValueError(f"{who}: key {k!r} does not belong to this configuration (a foreign file)")
    for e in [e for e in table if e.required(p)] + [e for e in table if not e.required(p) and e.key(kind) in sd]:
        k, dtype, shape = e.key(kind), e.np_dtype(kind), e.shape(i, lead)
        if k not in sd:
            raise ValueError(f"{who}: key {k!r} is missing (a truncated or foreign file)")
        a = np.asarray(sd[k])
        if a.dtype != dtype or a.shape != shape:
            raise ValueError(f"{who}: {k!r} must be {dtype} {shape} under this configuration, got {a.dtype} {a.shape}")
    if kind.units:                                          # (a detector keeps these as ints, checked above)
        if cfg["prep"]:
            pending = np.asarray(sd["pending"])
            if ((pending < 0) | (pending >= ints["prep_down"])).any():
                raise ValueError(f"{who}: pending = {pending.tolist()} outside an open group of prep_down = "
                                 f"{ints['prep_down']} raw ticks (0 .. {ints['prep_down'] - 1})")
        for k in ("recal_kept", "recal_counts", "calib_counts", "calib_kept"):
            if k in sd and (np.asarray(sd[k]) < 0).any():
                raise ValueError(f"{who}: {k} holds a negative count")


def stream_checkpoint_check(sd, expect) -> None:
    """Refuse a checkpoint dict `sd` (StreamDetector.state_dict() or a loaded file) that the loader cannot continue,
    with a ValueError that names the field.  `expect` holds the loader's own facts: "n", "w" (the model's), "abi"
    (the loaded library's ABI version), "state_bytes" = gdn_stream_state_bytes(n, w) and "calib_bytes" =
    gdn_stream_calib_bytes(n, R) for the file's R (0 without a ring) as the loaded library reports them, "model" (its
    model_fingerprint, or None: do not compare), "prep_down" (the caller's Prep.down, or None: no prep) and "prep_n";
    a detector that exists already adds "events" (its events configuration or None) and "recal_threshold".
    Host data only: no device work, no library call."""
    _check(DETECTOR, sd, expect)


def fleet_checkpoint_check(sd, expect) -> None:
    """stream_checkpoint_check for a fleet checkpoint dict (StreamFleet.state_dict() or a loaded file).  `expect` as
    there, with "state_bytes" PER UNIT, "calib_bytes" = gdn_fleet_calib_bytes(units, n, R) for the file's units and R,
    and — a fleet that exists already — "units".  "prep_units": PrepUnits.fingerprint() of the caller's per-unit tables,
    None (or absent) for a shared Prep; the file's optional `prep_units_sha256` must say the same."""
    _check(FLEET, sd, expect)


def _checkpoint_expect(model, prep, recal: int, check_model: bool = True, units=None) -> dict:
    """The loader's own facts for the checker (`units=None`: a detector's): host arithmetic and host library calls, plus
    ONE batch read of the model's tensors for its fingerprint when `check_model`."""
    from . import _lib
    lib = _lib.load()
    w = model.gnn_layers[0].gnn.lin.weight.shape[1]
    n = model.embedding.weight.shape[0]
    ring = lib.gdn_stream_calib_bytes(n, recal) if units is None else lib.gdn_fleet_calib_bytes(units, n, recal)
    expect = {"n": n, "w": w, "abi": lib.gdn_abi_version(), "state_bytes": lib.gdn_stream_state_bytes(n, w),
              "calib_bytes": ring if recal else 0}
    if units is not None and prep is not None and getattr(prep, "tables", None) is not None and prep.units != int(units):
        raise ValueError(f"{_FLEET_CKPT}: prep: per-unit tables of {prep.units} units, units = {int(units)}")
    expect.update({"model": model_fingerprint(model) if check_model else None,
                   "prep_down": None if prep is None else prep.down, "prep_n": None if prep is None else prep.n})
    if units is not None:
        expect["prep_units"] = prep_units(prep)
    return expect


# --------------------------------------------------------------------------- the file
def write_stream_checkpoint(path: str, sd) -> None:
    """`sd` as ONE .npz at exactly `path` (numpy.savez; no suffix is appended): written to path + ".tmp" beside it, made
    durable, then moved over `path` with os.replace, so a process that dies in the middle of a save leaves the
    previous checkpoint as it was."""
    tmp = path + ".tmp"
    try:
        with open(tmp, "wb") as f:
            np.savez(f, **sd)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        with contextlib.suppress(OSError):
            os.unlink(tmp)
        raise


def read_stream_checkpoint(path: str) -> dict:
    """The arrays of a checkpoint file (allow_pickle=False: it holds no Python objects)."""
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


# --------------------------------------------------------------------------- unit hand-over
# (DESIGN §3.8m): unit u's block of every fleet array is a single stream's byte for byte, so a unit moves between a
# fleet's dict and a detector's by slicing and renaming along ENTRIES; what is left is the configuration, checked by name
_UNIT_CONFIG = ("n", "w", "top_m", "log", "with_gaps", "recal", "exclude_alarms", "recal_min", "calib", "wide", "prep",
                "prep_down")
_BY_HAND = (_PENDING_TICKS,)                                # a pair of keys the converters do not simply rename


def _pairs():
    return [e for e in ENTRIES if e.det is not None and e.fleet is not None and e not in _BY_HAND]


def fleet_unit_to_stream(sd_fleet, u: int) -> dict:
    """Unit `u` of a fleet's state dict as the state dict of a single detector (StreamDetector.load_state_dict's input):
    the unit's slice of every per-unit array under the detector's key, the open group cut to its length, the fleet's
    configuration, chunk and clocks (`handed`: recal_every goes on from the fleet's clock; `recals`: the fleet's calls).
    `recal_counts` travels under every calibration (the fleet keeps it under both); under calib="sensor" `recal_kept` is
    the smallest count that reached recal_min, as a detector states it.  The fingerprint of per-unit prep tables stays
    behind: the detector takes prep.unit(u).  Host data only."""
    who = _FLEET_CKPT
    _format(FLEET, sd_fleet)
    cfg = _config(FLEET, sd_fleet)
    ints = {k: _ckpt_int(sd_fleet, k, who) for k in _FLEET_CKPT_INTS}
    U, n, R = cfg["units"], cfg["n"], cfg["recal"]
    u = int(u)
    if not 0 <= u < U:
        raise ValueError(f"{who}: unit {u}: the file holds units 0 .. {U - 1}")

    def unit(key):
        if key not in sd_fleet:
            raise ValueError(f"{who}: key {key!r} is missing (a truncated or foreign file)")
        return np.array(np.asarray(sd_fleet[key])[u])       # (a contiguous copy; one number stays 0-d)
    p = present(FLEET, sd_fleet, ints, cfg["calib"], None)
    sd = {}
    recal_kept = pending = 0
    for e in ENTRIES:
        if e is _EVENTS:
            p["events"] = _events(FLEET, sd_fleet) is not None
        if e is _RECAL_KEPT and R:
            # a detector states the counts of its last recalibrate() as int64 and, under calib="sensor", `recal_kept` as
            # the smallest of them that reached recal_min
            counts = sd["recal_counts"] = unit("recal_counts").astype(np.int64)
            done = counts[counts >= cfg["recal_min"]]
            recal_kept = int(unit(e.fleet)) if p["tick"] else int(done.min()) if done.size else 0
        elif e is _PENDING_TICKS and p["prep"]:
            pending = int(unit(_PENDING.fleet))
            if not 0 <= pending < cfg["prep_down"]:
                raise ValueError(f"{who}: pending[{u}] = {pending} outside an open group of prep_down = {cfg['prep_down']}")
            sd[e.det] = np.ascontiguousarray(unit(e.fleet)[:pending])       # the open group only
        elif e in _pairs() and (e.required(p) or e.fleet in sd_fleet):
            a = unit(e.fleet) if e.per_unit else np.array(sd_fleet[e.fleet])
            sd[e.det] = a.view(e.np_dtype(DETECTOR)) if e.raw else a.reshape(1) if e.scalar else a
    out = dict(ints, format=STREAM_CHECKPOINT_FORMAT, calib_bytes=stream_calib_bytes(n, R), recal_kept=recal_kept,
               calib_kept=int(unit(_CALIB_KEPT.fleet)) if _CALIB_KEPT.fleet in sd_fleet else -1, raw_pending=pending)
    sd.update({k: np.array(int(out[k]), dtype=np.int64) for k in _CKPT_INTS})
    sd["calib"], sd["model_sha256"] = np.array(cfg["calib"]), np.array(_ckpt_str(sd_fleet, "model_sha256", who))
    return sd


def stream_to_fleet_unit(sd_stream, sd_fleet_config) -> dict:
    """A detector's state dict as ONE unit of the fleet whose state dict (or any dict that holds its configuration keys,
    `abi`, `state_bytes`, `model_sha256` and the optional events_cfg / recal_threshold) is `sd_fleet_config`: the unit's
    block of every per-unit array under the fleet's key, without the unit axis (`pending_ticks`: the rows of the open
    group only, `pending` their number; `recal_counts` int32, from the detector's or — tick calibration — its
    `recal_kept` for every sensor).  Refused with a ValueError that names the field: any of n, w, top_m, log, with_gaps,
    recal, exclude_alarms, recal_min, calib, wide, prep, prep_down, events (and on, off, cap, m), recal_threshold,
    model_sha256, abi or state_bytes that differs.  chunk, recal_every and the clocks are the fleet's.  Host data only."""
    who = "unit hand-over"
    _format(DETECTOR, sd_stream)
    mine, theirs = _config(DETECTOR, sd_stream), _config(FLEET, sd_fleet_config)
    for k in _UNIT_CONFIG:
        if mine[k] != theirs[k]:
            raise ValueError(f"{who}: {k} = {mine[k]!r}, the fleet was built with {k} = {theirs[k]!r}"
                             + (" (the route is per launch: all units of a push share it)" if k == "wide" else ""))
    for k in ("abi", "state_bytes"):
        a, b = _ckpt_int(sd_stream, k), _ckpt_int(sd_fleet_config, k, _FLEET_CKPT)
        if a != b:
            raise ValueError(f"{who}: {k} = {a}, the fleet has {k} = {b} (another build of the library)")
    if _ckpt_str(sd_stream, "model_sha256") != _ckpt_str(sd_fleet_config, "model_sha256", _FLEET_CKPT):
        raise ValueError(f"{who}: model_sha256 differs from the fleet's model: a fleet scores all units with one model")
    ev, fev = _events(DETECTOR, sd_stream), None
    if _EVENTS_CFG.fleet in sd_fleet_config:                # (the configuration alone: the tables need not be there)
        fev = _events(FLEET, {_EVENTS.fleet: None, _CLEAR.fleet: None, _EVENTS_CFG.fleet: sd_fleet_config[_EVENTS_CFG.fleet]})
    if (ev is None) != (fev is None):
        raise ValueError(f"{who}: events: the detector keeps " + ("no" if ev is None else "an") + " episode table, the "
                         "fleet " + ("does" if ev is None else "does not"))
    for k in _EVENTS_FIELDS if ev is not None else ():
        if ev[k] != fev[k]:
            raise ValueError(f"{who}: events.{k} = {ev[k]}, the fleet was built with events.{k} = {fev[k]}")
    margin, theirs_margin = checkpoint_recal_threshold(sd_stream), checkpoint_recal_threshold(sd_fleet_config, _FLEET_CKPT)
    if margin != theirs_margin:
        raise ValueError(f"{who}: recal_threshold = {margin}, the fleet was built with recal_threshold = {theirs_margin}")
    n, R = mine["n"], mine["recal"]
    p = present(DETECTOR, sd_stream, mine, mine["calib"], ev)

    def arr(key):
        if key not in sd_stream:
            raise ValueError(f"{who}: key {key!r} is missing (a truncated or foreign file)")
        return np.ascontiguousarray(np.asarray(sd_stream[key]))
    out = {}
    for e in ENTRIES:
        if e is _RECAL_KEPT and R:
            # a fleet keeps `recal_kept` per unit under tick calibration only, and int32 counts under both: the
            # detector's, or — tick calibration, which keeps none — its `recal_kept` for every sensor
            kept = _ckpt_int(sd_stream, "recal_kept")
            if p["tick"]:
                out[e.fleet] = np.array(kept, dtype=np.int32)
            out["recal_counts"] = (arr("recal_counts") if "recal_counts" in sd_stream else
                                   np.full((n,), kept if p["tick"] else 0)).astype(np.int32)
        elif e is _PENDING_TICKS and p["prep"]:
            out[e.fleet] = arr(e.det)
            out[_PENDING.fleet] = np.array(_ckpt_int(sd_stream, "raw_pending"), dtype=np.int32)
        elif e is _CALIB_KEPT and _ckpt_int(sd_stream, "calib_kept") >= 0:
            out[e.fleet] = np.array(_ckpt_int(sd_stream, "calib_kept"), dtype=np.int64)
        elif e in _pairs() and e.per_unit and (e.required(p) or e.det in sd_stream):
            a = arr(e.det)
            out[e.fleet] = a.view(e.np_dtype(FLEET)) if e.raw else a.reshape(()) if e.scalar else a
    return out
