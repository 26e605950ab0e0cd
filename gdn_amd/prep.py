"""Raw readings in: the reference's scripts/process_swat.py / process_wadi.py on the device.

    prep = Prep.fit(raw_train, down=10)                  # min-max table from the training file's own readings
    series, labels = prep.series(raw, fill="mean", labels=attack, skip=2160)
    harness.StreamDetector(..., prep=prep).push(raw_ticks)

A raw block is tick-major [t_raw, n], fp32 or float64, on the device; the prepared series is sensor-major [n, T] fp32,
the layout of `series=` everywhere.  Every reading is normalised as x * scale + offset in float64 (sklearn's
MinMaxScaler(0, 1).transform bit for bit) and a prepared tick is np.median over `down` raw ticks, rounded to fp32.  A
reading that is not finite is missing: filled with the file's own mean (`fill="mean"`, the scripts'
fillna(mean).fillna(0)) or left out of its group's median (an empty group is NaN, a missing reading downstream).

    python -m gdn_amd.prep -train RAW.csv -test RAW.csv -out DIR [-down 10] [-skip 2160] [-label attack]
                           [-drop_cols K] [-fill mean]

writes DIR/train.csv, test.csv, list.txt (what `python -m gdn_amd.main -data_root` reads) and DIR/prep.npz."""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from . import ops

_EPS10 = 10.0 * float(np.finfo(np.float64).eps)          # sklearn's _handle_zeros_in_scale: a range below it is 1.0


def table_from_stats(stats: torch.Tensor) -> torch.Tensor:
    """[n, 2] float64 (scale, offset) of MinMaxScaler(0, 1) from stats [n, 4] (min, max, mean, count): scale =
    1 / range, offset = 0 - min * scale, range = 1.0 where max - min < 10 eps (a constant sensor maps to 0.0)."""
    lo, hi = stats[:, 0], stats[:, 1]
    rng = hi - lo
    rng = torch.where(rng < _EPS10, torch.ones_like(rng), rng)
    scale = 1.0 / rng
    return torch.stack([scale, 0.0 - lo * scale], dim=1).contiguous()


class Prep:
    """A fitted front end: `table` [n, 2] float64 (scale, offset) and `stats` [n, 4] float64 (the training file's
    min, max, mean, count per sensor) on one device, `down` raw ticks per prepared tick, the sensor `names`."""

    def __init__(self, table: torch.Tensor, stats: torch.Tensor, down: int, names=None):
        self.down = ops._prep_down(down)
        if table.dtype != torch.float64 or table.dim() != 2 or table.shape[1] != 2:
            raise ValueError(f"expected a float64 table [n, 2] (scale, offset), got {table.dtype} {tuple(table.shape)}")
        n = table.shape[0]
        if stats.dtype != torch.float64 or stats.shape != (n, 4):
            raise ValueError(f"expected float64 stats [{n}, 4] (min, max, mean, count), got {stats.dtype} "
                             f"{tuple(stats.shape)}")
        self.table, self.stats, self.n = table.contiguous(), stats.contiguous(), n
        self.names = [str(s) for s in names] if names is not None else [str(i) for i in range(n)]
        if len(self.names) != n:
            raise ValueError(f"{len(self.names)} sensor names for {n} sensors")

    @classmethod
    def fit(cls, raw_train: torch.Tensor, down: int = 10, names=None) -> "Prep":
        """The min-max table of `raw_train` [t_raw, n] (device; fp32 or float64): ONE gdn_prep_stats over its finite
        readings, then a handful of float64 torch ops on [n] vectors.  A sensor with no finite reading gets (1, 0)."""
        down = ops._prep_down(down)
        stats = ops.prep_stats(raw_train)
        return cls(table_from_stats(stats), stats, down, names)

    def series(self, raw: torch.Tensor, fill: str | None = None, labels: torch.Tensor | None = None, skip: int = 0):
        """(series [n, T - skip] fp32, labels [T - skip] float64 or None) of `raw` [t_raw, n], T = t_raw // down.
        fill="mean": a missing reading is replaced by the mean of ITS OWN file's finite readings (0 for a sensor with
        none) before the normalisation — one gdn_prep_stats on `raw` itself; fill=None leaves it missing.  `labels`
        [t_raw] float64 on the device: rint(max) per group.  `skip` drops leading prepared ticks (the scripts'
        iloc[2160:] of the training file)."""
        if fill not in (None, "mean"):
            raise ValueError(f"fill = {fill!r}: None (a missing reading stays missing) or 'mean' (the file's own mean)")
        if raw.dim() == 2 and raw.shape[0] < self.down:
            raise ValueError(f"t_raw = {raw.shape[0]} raw ticks are fewer than down = {self.down}: not one prepared tick")
        if raw.dim() != 2 or raw.shape[1] != self.n:
            raise ValueError(f"expected raw of shape [t_raw, {self.n}], got {tuple(raw.shape)}")
        T = raw.shape[0] // self.down
        if not 0 <= int(skip) < T:
            raise ValueError(f"skip = {skip}: between 0 and the {T} prepared ticks, exclusive")
        fill_v = ops.prep_stats(raw)[:, 2].contiguous() if fill == "mean" else None
        series, lab = ops.prep_series(raw, self.table, self.down, fill=fill_v, labels=labels)
        if skip:
            series = series[:, skip:].contiguous()
            lab = None if lab is None else lab[skip:].contiguous()
        return series, lab

    def save(self, path: str) -> None:
        np.savez(path, table=self.table.cpu().numpy(), stats=self.stats.cpu().numpy(), down=np.int64(self.down),
                 names=np.array(self.names, dtype=str))

    @classmethod
    def load(cls, path: str, device="cuda") -> "Prep":
        with np.load(path, allow_pickle=False) as z:
            return cls(torch.from_numpy(z["table"]).to(device), torch.from_numpy(z["stats"]).to(device), int(z["down"]),
                       [str(s) for s in z["names"]])


class PrepUnits:
    """A fitted front end per unit of a fleet: `tables` [U, n, 2] float64 and `stats` [U, n, 4] float64 on
    one device — unit u's are a Prep's, fitted on that unit's own raw readings — with ONE `down` and ONE list of sensor
    `names` for all units (one model).  harness.StreamFleet(prep=PrepUnits) normalises unit u with tables[u]
    (gdn_fleet_prep_ticks_units); `unit(u)` is the plain Prep of that unit, views of the same memory."""

    def __init__(self, tables: torch.Tensor, stats: torch.Tensor, down: int, names=None):
        self.down = ops._prep_down(down)
        if tables.dtype != torch.float64 or tables.dim() != 3 or tables.shape[0] < 1 or tables.shape[2] != 2:
            raise ValueError(f"expected float64 tables [U >= 1, n, 2] (scale, offset per unit), got {tables.dtype} "
                             f"{tuple(tables.shape)}")
        units, n = tables.shape[:2]
        if stats.dtype != torch.float64 or stats.shape != (units, n, 4):
            raise ValueError(f"expected float64 stats [{units}, {n}, 4] (min, max, mean, count per unit), got "
                             f"{stats.dtype} {tuple(stats.shape)}")
        if stats.device != tables.device:
            raise ValueError(f"tables are on {tables.device}, stats on {stats.device}")
        self.tables, self.stats, self.units, self.n = tables.contiguous(), stats.contiguous(), units, n
        self.table = self.tables                                     # (what ops.fleet_prep_ticks is handed, either form)
        self.names = [str(s) for s in names] if names is not None else [str(i) for i in range(n)]
        if len(self.names) != n:
            raise ValueError(f"{len(self.names)} sensor names for {n} sensors")
        self._sha256 = None

    @classmethod
    def fit(cls, raw_train: torch.Tensor, down: int = 10, names=None) -> "PrepUnits":
        """Every unit's min-max table from its own `raw_train[u]` [t_raw, n] (device; fp32 or float64): Prep.fit per
        unit, U launches of gdn_prep_stats at fit time."""
        if raw_train.dim() != 3 or raw_train.shape[0] < 1:
            raise ValueError(f"expected raw_train of shape [U, t_raw, n], got {tuple(raw_train.shape)}")
        return cls.from_preps([Prep.fit(unit, down, names) for unit in raw_train])

    @classmethod
    def from_preps(cls, preps) -> "PrepUnits":
        """The fitted Preps of U units, stacked; `down` and `n` must agree (refused by name), the names are the first's."""
        preps = list(preps)
        if not preps:
            raise ValueError("from_preps: at least one Prep")
        for u, p in enumerate(preps):
            if p.down != preps[0].down:
                raise ValueError(f"down: unit {u} has down = {p.down}, unit 0 has down = {preps[0].down}")
            if p.n != preps[0].n:
                raise ValueError(f"n: unit {u} was fitted on {p.n} sensors, unit 0 on {preps[0].n}")
        return cls(torch.stack([p.table for p in preps]), torch.stack([p.stats for p in preps]), preps[0].down,
                   preps[0].names)

    def unit(self, u: int) -> Prep:
        if not 0 <= int(u) < self.units:
            raise ValueError(f"unit({u}): the tables cover units 0 .. {self.units - 1}")
        return Prep(self.tables[int(u)], self.stats[int(u)], self.down, self.names)

    def series(self, raw: torch.Tensor, fill: str | None = None, labels: torch.Tensor | None = None, skip: int = 0):
        """(series [U, n, T - skip] fp32, labels [T - skip] or None) of `raw` [U, t_raw, n]: Prep.series per unit (one
        gdn_prep_series each); `labels` [t_raw] belong to the time axis all units share."""
        if raw.dim() != 3 or raw.shape[0] != self.units:
            raise ValueError(f"expected raw of shape [{self.units}, t_raw, {self.n}], got {tuple(raw.shape)}")
        done = [self.unit(u).series(raw[u], fill=fill, labels=labels, skip=skip) for u in range(self.units)]
        return torch.stack([s for s, _ in done]), done[0][1]

    def fingerprint(self) -> str:
        """SHA-256 (hex) over down, the shape and the bytes of `tables`: what a fleet checkpoint keeps of them.  ONE
        device read at its first use."""
        if self._sha256 is None:
            host = self.tables.detach().cpu().contiguous().numpy()
            self._sha256 = tables_fingerprint(host, self.down)
        return self._sha256

    def save(self, path: str) -> None:
        np.savez(path, tables=self.tables.cpu().numpy(), stats=self.stats.cpu().numpy(), down=np.int64(self.down),
                 names=np.array(self.names, dtype=str))

    @classmethod
    def load(cls, path: str, device="cuda") -> "PrepUnits":
        with np.load(path, allow_pickle=False) as z:
            return cls(torch.from_numpy(z["tables"]).to(device), torch.from_numpy(z["stats"]).to(device), int(z["down"]),
                       [str(s) for s in z["names"]])


def tables_fingerprint(tables: np.ndarray, down: int) -> str:
    """PrepUnits.fingerprint's arithmetic on a host array [U, n, 2] float64."""
    import hashlib
    tables = np.ascontiguousarray(tables, dtype=np.float64)
    h = hashlib.sha256(f"prep_units|{int(down)}|{tables.shape}|".encode())
    h.update(tables.tobytes())
    return h.hexdigest()


# --------------------------------------------------------------------------- command line
def read_raw_csv(path: str, label: str = "attack", drop_cols: int = 0, names=None):
    """(raw [t_raw, n] float64, labels [t_raw] float64, sensor names) of a raw CSV read as the scripts read it: the
    first column is the index, `drop_cols` further leading columns go, column names are stripped, the `label` column
    (zeros when the file has none) is taken out.  `names`: keep these sensors, in this order."""
    import pandas as pd
    df = pd.read_csv(path, index_col=0).iloc[:, drop_cols:]
    df = df.rename(columns=lambda x: x.strip())
    labels = df[label].to_numpy(dtype=np.float64) if label in df.columns else np.zeros(len(df))
    if label in df.columns:
        df = df.drop(columns=[label])
    if names is not None:
        df = df[list(names)]
    return np.ascontiguousarray(df.to_numpy(dtype=np.float64)), labels, list(df.columns)


def write_prepared_csv(path: str, series: torch.Tensor, labels, names, label: str, first: int = 0) -> None:
    """train.csv / test.csv as the scripts write them: the index, one column per sensor, the label column.  An fp32
    value is written as the float64 equal to it, so reading the file and casting to fp32 gives the bits back."""
    import pandas as pd
    df = pd.DataFrame(series.t().double().cpu().numpy(), columns=list(names))
    df[label] = labels.cpu().numpy()
    df.index = df.index + first
    df.to_csv(path)


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m gdn_amd.prep")
    parser.add_argument("-train", help="raw training CSV (first column: index)", type=str, required=True)
    parser.add_argument("-test", help="raw test CSV", type=str, required=True)
    parser.add_argument("-out", help="directory for train.csv, test.csv, list.txt, prep.npz", type=str, required=True)
    parser.add_argument("-down", help="raw ticks per prepared tick (median)", type=int, default=10)
    parser.add_argument("-skip", help="leading prepared ticks of train dropped", type=int, default=2160)
    parser.add_argument("-label", help="name of the label column", type=str, default="attack")
    parser.add_argument("-drop_cols", help="leading columns dropped after the index", type=int, default=0)
    parser.add_argument("-fill", help="'mean': fill missing readings with the file's own mean; 'none': leave them "
                        "missing (NaN where a whole group is)", type=str, default="mean", choices=["mean", "none"])
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    ops._prep_down(args.down)
    dev = torch.device("cuda", 0)
    fill = None if args.fill == "none" else "mean"
    train_np, train_lab, names = read_raw_csv(args.train, args.label, args.drop_cols)
    test_np, test_lab, _ = read_raw_csv(args.test, args.label, args.drop_cols, names=names)
    prep = Prep.fit(torch.from_numpy(train_np).to(dev), down=args.down, names=names)
    os.makedirs(args.out, exist_ok=True)
    for name, raw, lab, skip in (("train", train_np, train_lab, args.skip), ("test", test_np, test_lab, 0)):
        series, labels = prep.series(torch.from_numpy(raw).to(dev), fill=fill, labels=torch.from_numpy(lab).to(dev),
                                     skip=skip)
        write_prepared_csv(os.path.join(args.out, name + ".csv"), series, labels, names, args.label, first=skip)
        print(f"{name}: {raw.shape[0]} raw ticks of {raw.shape[1]} sensors -> {series.shape[1]} prepared ticks "
              f"(down {args.down}, skip {skip})")
    with open(os.path.join(args.out, "list.txt"), "w") as f:
        f.writelines(col + "\n" for col in names)
    prep.save(os.path.join(args.out, "prep.npz"))
    return prep


if __name__ == "__main__":
    main()
