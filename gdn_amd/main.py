"""Command line of the reference (main.py:199-256, run.sh:4-58), same flags and printed report:

    python -m gdn_amd.main -dataset msl -device cuda -slide_win 15 -topk 20 -batch 128 -epoch 30 ...
    bash run.sh 0 msl            (the reference's `bash run.sh <gpu_n> <dataset>`)

Reads ./data/<dataset>/{train.csv,test.csv,list.txt} exactly like main.py:44-53 (`-data_root` moves the
directory), builds the model with the reference's seeds and constructor (same initial weights), trains
with the reference's loop (harness.train: Adam 1e-3, best-validation checkpoint, early stop), evaluates
and prints `F1 score / precision / recall`.

What is different is WHERE the data lives: the two series stay in HBM as [N, T]
tensors and every window is cut from them on the device —
  * training batches: the DataLoader of main.py:128-148 is kept for what it decides (the random
    contiguous validation block, the shuffled order: same RNG draws as the reference), but it is only
    asked for an epoch's ORDER (harness.epoch_order); the [batch, N, W] block of every step is cut
    from the resident series (stride `slide_stride`, datasets/TimeDataset.py:44-58) by a kernel
    inside the captured step (harness.train_series), and the validation loss is formed on the device;
  * evaluation: `GDN.forward_series` builds the stride-1 windows inside the kernel; predictions, the
    anomaly scores and the threshold sweep never leave the device (gdn_amd/evaluate.py).
The reference's `TimeDataset` would materialise a W-fold copy of both series on the host."""
from __future__ import annotations

import argparse
import os
import random
from datetime import datetime
from pathlib import Path

import numpy as np
import torch
from torch.utils.data import DataLoader, Subset, TensorDataset

from . import evaluate, harness
from .model import GDN


def get_feature_map(dataset, data_root="./data"):
    """util/net_struct.py:4-10."""
    with open(os.path.join(data_root, dataset, "list.txt")) as f:
        return [ft.strip() for ft in f]


def get_fc_graph_struc(dataset, data_root="./data"):
    """util/net_struct.py:12-28: every feature's children = all the others."""
    feats = get_feature_map(dataset, data_root)
    return {ft: [o for o in feats if o is not ft] for ft in feats}


def build_loc_net(struc, all_features, feature_map):
    """util/preprocess.py:85-116: [2, E] (child index, parent index) of the prior graph.  The model ignores it
    (models/GDN.py:122) — built for API parity (`GDN(edge_index_sets, ...)`)."""
    src, dst = [], []
    for node, children in struc.items():
        if node not in all_features:
            continue
        if node not in feature_map:
            feature_map.append(node)
        p = feature_map.index(node)
        for child in children:
            if child in all_features and child in feature_map:
                src.append(feature_map.index(child))
                dst.append(p)
    return [src, dst]


def read_series(path, feature_map, want_labels):
    """main.py:44-64 + util/preprocess.py:67-83: columns in feature-map order -> [N, T] float64, labels [T]."""
    import pandas as pd
    df = pd.read_csv(path, sep=",", index_col=0)
    labels = df["attack"].to_numpy(dtype=np.float64) if want_labels and "attack" in df.columns else np.zeros(len(df))
    cols = [ft for ft in feature_map if ft in df.columns]
    return np.ascontiguousarray(df[cols].to_numpy(dtype=np.float64).T), labels


class SeriesWindows:
    """datasets/TimeDataset.py for a series resident on the device: window i covers columns
    [starts[i] - W, starts[i]) and predicts column starts[i]; `batch(idx)` gathers x[B,N,W], y[B,N], labels[B]."""

    def __init__(self, series_nt: torch.Tensor, labels_t: torch.Tensor, slide_win: int, slide_stride: int, mode: str):
        self.series, self.labels, self.w = series_nt, labels_t, slide_win
        t_len = series_nt.shape[1]
        rng = range(slide_win, t_len, slide_stride) if mode == "train" else range(slide_win, t_len)
        self.starts = torch.tensor(list(rng), dtype=torch.int64, device=series_nt.device)
        self._offs = torch.arange(-slide_win, 0, device=series_nt.device)

    def __len__(self):
        return int(self.starts.numel())

    def batch(self, idx: torch.Tensor):
        at = self.starts[idx.to(self.starts.device)]
        cols = at.view(-1, 1) + self._offs.view(1, -1)                       # [B, W]
        x = self.series[:, cols].permute(1, 0, 2).contiguous()               # [B, N, W]
        return x, self.series[:, at].t().contiguous(), self.labels[at]


class IndexLoader:
    """A torch DataLoader over window indices (so that shuffling draws what the reference's loader draws),
    yielding (x, y, labels, edge_index) device batches like the reference's loaders."""

    def __init__(self, windows: SeriesWindows, indices: torch.Tensor, batch: int, shuffle: bool, edge_index):
        self.windows, self.edge_index = windows, edge_index
        self.loader = DataLoader(TensorDataset(indices), batch_size=batch, shuffle=shuffle, num_workers=0)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for (idx,) in self.loader:
            x, y, lab = self.windows.batch(idx)
            yield x, y, lab, self.edge_index


class Main:
    """main.py:36-195."""

    def __init__(self, train_config, env_config, debug=False):
        self.train_config, self.env_config, self.datestr = train_config, env_config, None
        dataset, root = env_config["dataset"], env_config.get("data_root", "./data")
        if env_config["device"] == "cpu":
            raise SystemExit("gdn_amd has no CPU path (the reference's `-device cpu` runs the reference)")
        self.device = torch.device("cuda", 0)                               # util/env.py: `cuda` + CUDA_VISIBLE_DEVICES
        feature_map = get_feature_map(dataset, root)
        fc_struc = get_fc_graph_struc(dataset, root)
        if env_config.get("tune_alarm"):
            check_attack_column(os.path.join(root, dataset, "test.csv"))
        train_np, _ = read_series(os.path.join(root, dataset, "train.csv"), feature_map, want_labels=False)
        test_np, test_labels = read_series(os.path.join(root, dataset, "test.csv"), feature_map, want_labels=True)
        self.feature_map = feature_map
        fc_edge_index = torch.tensor(build_loc_net(fc_struc, list(feature_map), feature_map=feature_map), dtype=torch.long)
        dev = self.device
        # TimeDataset holds float64 and the loops cast to float32 (train.py:66, test.py:44)
        self.train_series = torch.from_numpy(train_np).to(dev).float()
        self.test_series = torch.from_numpy(test_np).to(dev).float()
        self.test_labels = torch.from_numpy(test_labels).to(dev)
        cfg = dict(slide_win=train_config["slide_win"], slide_stride=train_config["slide_stride"])
        self.train_dataset = SeriesWindows(self.train_series, torch.zeros(train_np.shape[1], device=dev, dtype=torch.float64),
                                           cfg["slide_win"], cfg["slide_stride"], "train")
        self.test_dataset = SeriesWindows(self.test_series, self.test_labels, cfg["slide_win"], cfg["slide_stride"], "test")
        self.train_dataloader, self.val_dataloader = self.get_loaders(
            self.train_dataset, train_config["seed"], train_config["batch"], val_ratio=train_config["val_ratio"],
            edge_index=fc_edge_index)
        self.model = GDN([fc_edge_index], len(feature_map), dim=train_config["dim"], input_dim=train_config["slide_win"],
                         out_layer_num=train_config["out_layer_num"],
                         out_layer_inter_dim=train_config["out_layer_inter_dim"], topk=train_config["topk"]).to(dev)

    def get_loaders(self, train_dataset, seed, batch, val_ratio=0.1, edge_index=None):
        """main.py:128-148: a random contiguous validation block, shuffled training order."""
        dataset_len = int(len(train_dataset))
        train_use_len = int(dataset_len * (1 - val_ratio))
        val_use_len = int(dataset_len * val_ratio)
        val_start_index = random.randrange(train_use_len)
        indices = torch.arange(dataset_len)
        train_idx = torch.cat([indices[:val_start_index], indices[val_start_index + val_use_len:]])
        val_idx = indices[val_start_index:val_start_index + val_use_len]
        return (IndexLoader(train_dataset, train_idx, batch, True, edge_index),
                IndexLoader(train_dataset, val_idx, batch, False, edge_index))

    # ------------------------------------------------------------------------------------------------
    def run(self):
        # -train_gaps: train.csv may hold missing readings (NaN / inf).  They are held once, here; training, every
        # validation pass and the validation block of the report cut windows, targets and validity bytes from this fill
        train_gaps = bool(self.train_config.get("train_gaps"))
        check_train_gaps(train_gaps, bool(self.train_config.get("hip_graph", True)))
        fill = harness.fill_series(self.train_series, self.train_config["slide_win"]) if train_gaps else None
        looked_at = fill.series if train_gaps else self.train_series
        if len(self.env_config["load_model_path"]) > 0:
            model_save_path = self.env_config["load_model_path"]
        else:
            model_save_path = self.get_save_path()[0]
            # raw engineering units (the reference's main.py normalises nothing; scripts/process_*.py do, offline):
            # the resident training series is looked at once and the step runs on the fp32 row-gather kernels when
            # it exceeds the 16-bit operand range of the matrix-core ones (include/gdn_hip.h "range guard")
            self.train_config.setdefault("wide", self.model.train().input_exceeds_limit(looked_at, margin=16.0))
            if train_gaps:
                w = self.train_config["slide_win"]
                ticks = self.train_dataset.starts
                share = [harness.masked_share(fill.valid, ticks[ld.loader.dataset.tensors[0].to(ticks.device)], w)
                         for ld in (self.train_dataloader, self.val_dataloader)]
                print(f"train_gaps: {100 * share[0]:.3f} % of the training targets and {100 * share[1]:.3f} % of the "
                      "validation targets are missing and left out of the losses")
                self.train_log = harness.train_series(self.model, model_save_path, config=self.train_config,
                                                      series=self.train_series, w=w,
                                                      train_loader_or_indices=self.train_dataloader,
                                                      val_starts=self.val_dataloader, gaps=True, fill=fill)
            elif self.train_config.get("hip_graph", True):
                # epochs on the device (harness.train_series): the loaders decide the order (same draws), the windows
                # are cut inside the captured step, the validation loss is formed on the device
                self.train_log = harness.train_series(self.model, model_save_path, config=self.train_config,
                                                      series=self.train_series, w=self.train_config["slide_win"],
                                                      train_loader_or_indices=self.train_dataloader,
                                                      val_starts=self.val_dataloader)
            else:       # -no_hip_graph: the eager loop over the loaders, as before
                self.train_log = harness.train(self.model, model_save_path, config=self.train_config,
                                               train_dataloader=self.train_dataloader,
                                               val_dataloader=self.val_dataloader, use_graph=False)
        self.model.load_state_dict(torch.load(model_save_path, weights_only=True))
        best_model = self.model.to(self.device).eval()
        # test.py's loop with the windows built in the kernel from the resident series (stride 1)
        w = self.train_config["slide_win"]
        n_test = self.test_series.shape[1] - w
        if best_model.out_layer_num == 1:
            pred = best_model.forward_series(self.test_series, 0, n_test,
                                             wide=best_model.input_exceeds_limit(self.test_series))
        else:
            pred = self.predict_mlp_head(best_model, n_test)
        gt = self.test_series[:, w:].t().contiguous()
        labels = self.test_labels[w:]
        self.test_result = [pred, gt, labels.view(-1, 1).expand(-1, pred.shape[1])]
        val_ticks = self.train_dataset.starts[self.val_dataloader.loader.dataset.tensors[0].to(self.device)]
        harness.epoch_order(self.val_dataloader.loader)     # (the draw of iterating the loader, as test() did)
        if train_gaps:
            _, val_pred, val_gt = harness.validate_series(best_model, fill.series, val_ticks, self.train_config["batch"],
                                                          valid=fill.valid)
        else:
            _, val_pred, val_gt = harness.validate_series(best_model, self.train_series, val_ticks,
                                                          self.train_config["batch"])
        self.val_result = [val_pred, val_gt, self.train_dataset.labels[val_ticks].view(-1, 1).expand(-1, val_pred.shape[1])]
        info = self.get_score(self.test_result, self.val_result)
        if self.env_config.get("localise"):
            self.save_localisation(best_model, gt, float(info[4]), self.env_config["localise"])
        if self.env_config.get("stream"):
            self.stream_test_series(best_model, val_ticks, int(self.env_config["stream"]),
                                    gaps=bool(self.env_config.get("stream_gaps")),
                                    calib_gaps=bool(self.env_config.get("stream_calib_gaps")),
                                    recal=int(self.env_config.get("stream_recal") or 0),
                                    recal_every=int(self.env_config.get("stream_recal_every") or 0),
                                    recal_threshold=self.env_config.get("stream_recal_threshold"),
                                    by_sensor=bool(self.env_config.get("calib_by_sensor")),
                                    raw_path=self.env_config.get("stream_raw") or "",
                                    prep_path=self.env_config.get("prep") or "",
                                    save_path=self.env_config.get("stream_save") or "",
                                    resume_path=self.env_config.get("stream_resume") or "",
                                    events=stream_events_config(self.env_config.get("stream_on"),
                                                                self.env_config.get("stream_off"),
                                                                self.env_config.get("stream_clear"),
                                                                self.env_config.get("stream_events") or ""),
                                    events_path=self.env_config.get("stream_events") or "")
        if self.env_config.get("tune_alarm"):
            self.tune_alarm(best_model, gt, labels, self.env_config["tune_alarm"],
                            hi_steps=int(self.env_config.get("tune_hi_steps") or 32),
                            on=self.env_config.get("tune_on") or TUNE_ON, off=self.env_config.get("tune_off") or TUNE_OFF)
        return info

    def tune_alarm(self, model, gt, labels, path: str, hi_steps: int = 32, on="1,2,3,5,10", off="1,5,10,30"):
        """-tune_alarm OUT.npz: which (threshold, clear level, on-delay, off-delay) to deploy.  The test
        ticks are scored once (s_t = the evaluator's top_scores[:, 0]), a grid of settings — `hi_steps` raise levels
        taken evenly from the thresholds of the report's 400-step sweep, clear levels hi * TUNE_LO_FRAC, the on / off
        delays of -tune_on / -tune_off — is swept against the labelled incidents in one launch, the best row by event
        F1 is printed, and the whole sweep plus the choice is saved (numpy appends the suffix when OUT lacks it)."""
        ev = harness.SeriesEvaluator(model, None, gt, batch=8192, use_graph=False, series=self.test_series, top_m=1)
        ev.step()
        scores = ev.top_scores[:, 0].contiguous()
        _f, ths, _o = evaluate._sweep(scores, labels.reshape(-1) > 0, evaluate.TH_STEPS)
        hi, ticks_on, ticks_off = tune_alarm_grid(ths, hi_steps, on, off)
        sweep = harness.alarm_sweep(scores, labels, hi, lo_frac=TUNE_LO_FRAC, on=ticks_on, off=ticks_off)
        best = sweep.best()
        self.tune_result = dict(sweep.numpy(), **{"best_" + k: v for k, v in best.items()})
        np.savez(path, **self.tune_result)
        print(f"tune_alarm: {sweep.hi.shape[0]} settings over {self.tune_result['ticks']} ticks with "
              f"{self.tune_result['incidents']} labelled incidents; best event F1 {best['f1']:.4f}: threshold "
              f"{best['hi']:.6g}, clear {best['lo']:.6g}, on {best['on']}, off {best['off']} -> {best['episodes']} episodes "
              f"({best['true_episodes']} true), {best['incidents_hit']} incidents hit, mean delay "
              f"{best['delay_sum'] / max(1, best['incidents_hit']):.1f} ticks (max {best['delay_max']}), "
              f"{best['alarm_ticks']} alarm ticks")
        return self.tune_result

    def stream_test_series(self, model, val_ticks, chunk: int, show: int = 10, gaps: bool = False, recal: int = 0,
                           recal_every: int = 0, calib_gaps: bool = False, by_sensor: bool = False,
                           raw_path: str = "", prep_path: str = "", save_path: str = "", resume_path: str = "",
                           events=None, events_path: str = "", recal_threshold=None):
        """-stream C: the deployment form of the run.  A harness.StreamDetector is calibrated on the validation block
        of the training series (median / IQR per sensor and the largest anomaly score of that block: `-report val`'s
        threshold rule), then the test series after its first window is replayed through it in pushes of C ticks; the
        counters and the alarm log are read ONCE at the end and kept as `stream_result`.  -stream_gaps: the detector
        holds missing (non-finite) readings of the replayed ticks and keeps them out of the scores; the number of
        sensors that had any and the missing readings in all join the printed line and `stream_result`.
        -stream_recal R: the detector keeps a calibration ring of the last R ticks (seeded from the validation block)
        and, with -stream_recal_every E, rewrites its median / IQR table from it every E replayed ticks; the number
        of recalibrations and the ticks kept at the last one join the line and `stream_result`.
        -stream_recal_threshold MARGIN (with -stream_recal): every recalibration also re-derives the
        threshold from the ring under the new table, as MARGIN times the ring's largest smoothed score; the threshold
        in force is the line's, and the eligible ticks behind the last one join it and `stream_result`
        ("recal_threshold", "recal_eligible").
        -stream_calib_gaps (with -stream_gaps): the validation block may hold missing readings too; it is scored under
        the detector's rules (from_calibration(calib_gaps=True)) and the complete ticks the table was computed from
        join the line and `stream_result` ("calib_kept").
        -calib_by_sensor (with -stream_gaps -stream_calib_gaps): every sensor's table row comes from its own real
        readings (calib="sensor"); the smallest and largest per-sensor count join the line and `stream_result`
        ("calib_count_min", "calib_count_max"), and with -stream_recal the ring recalibrates per sensor as well.
        -stream_raw RAW.csv -prep prep.npz: the replayed ticks are the RAW file's (engineering units at the raw rate,
        columns as list.txt names them) from raw tick slide_win * down on, pushed C * down at a time through a prep=
        detector (gdn_amd.prep.Prep: min-max table and median downsample on the device); the calibration and the
        history are the prepared series' as before.  "raw_ticks" (pushed) and "raw_pending" (left in an open group)
        join the line and `stream_result`.
        -stream_save PATH: the detector is saved (StreamDetector.save) when the replay ends.
        -stream_resume PATH: the detector is StreamDetector.load(PATH) and not a fresh calibration: its configuration
        (gaps, ring, calibration rule, chunk) is the file's, -stream C only sizes the pushes, and the replay goes on at
        the tick the file's counters say has been consumed (of a -stream_raw file: model ticks * down + raw_pending);
        that tick joins the line and `stream_result` ("resumed_from").
        -stream_on A -stream_off B -stream_clear LO -stream_events OUT.npz (any of them): the detector
        keeps an episode table (events=dict(on=A, off=B, lo=LO)): one line per episode is printed — test ticks of its
        start and end, its peak and the sensors at the peak — the table joins `stream_result` ("episodes") and, with
        -stream_events, is saved to OUT.npz.  A resumed detector keeps the file's own events configuration."""
        check_calib_by_sensor(by_sensor, bool(chunk), gaps, calib_gaps)
        check_stream_raw(bool(raw_path), bool(chunk), bool(prep_path))
        check_stream_checkpoint(bool(save_path), bool(resume_path), bool(chunk))
        w = self.train_config["slide_win"]
        lo, hi = int(val_ticks.min()), int(val_ticks.max())
        normal = self.train_series[:, lo - w:hi + 1].contiguous()
        if recal_every and not recal:
            raise ValueError("-stream_recal_every needs -stream_recal R (the calibration ring it recalibrates from)")
        if recal_threshold is not None and not recal:
            raise ValueError("-stream_recal_threshold needs -stream_recal R (the ring the threshold is re-derived from)")
        rolling = {"recal": recal, "recal_every": recal_every} if recal else {}
        if recal_threshold is not None:
            rolling["recal_threshold"] = float(recal_threshold)
        if calib_gaps:
            if not gaps:
                raise ValueError("-stream_calib_gaps needs -stream_gaps (the detector whose rules the calibration follows)")
            rolling["calib_gaps"] = True
        if by_sensor:
            rolling["calib"] = "sensor"
        if events is not None:
            rolling["events"] = events
        step = chunk
        if raw_path:
            from .prep import Prep, read_raw_csv
            rolling["prep"] = Prep.load(prep_path, self.device)
            step = chunk * rolling["prep"].down
            raw_np, _labels, _names = read_raw_csv(raw_path, names=self.feature_map)
            ticks = torch.from_numpy(raw_np[w * rolling["prep"].down:]).to(self.device)
        else:
            ticks = self.test_series[:, w:].t().contiguous()
        resumed = None
        if resume_path:
            det = harness.StreamDetector.load(resume_path, model, prep=rolling.get("prep"), device=self.device)
            resumed = det.status()[0]
            gaps, recal = det.with_gaps, det.recal          # the file's configuration, whatever the other flags say
            calib_gaps, by_sensor = det.calib_kept is not None, det.calib_counts is not None
            at = resumed * det.prep.down + det.raw_pending if raw_path else resumed
            if at > ticks.shape[0]:
                raise ValueError(f"-stream_resume {resume_path}: the checkpoint has consumed {at} ticks, the replayed "
                                 f"file holds {ticks.shape[0]}")
            ticks = ticks[at:]
        else:
            det = harness.StreamDetector.from_calibration(model, normal, chunk, history=self.test_series[:, :w],
                                                          top_m=min(3, normal.shape[0]), gaps=gaps, **rolling)
        for s in range(0, ticks.shape[0], step):
            det.push(ticks[s:s + step])
        if save_path:
            det.save(save_path)
        scored, alarms, log_ticks, log_sensors = det.status()[:4]
        self.stream_result = {"chunk": chunk, "threshold": float(det.threshold.item()), "ticks": scored,
                              "alarms": alarms, "log_ticks": log_ticks.cpu().numpy(),
                              "log_sensors": log_sensors.cpu().numpy()}
        held = ""
        if resumed is not None:
            self.stream_result["resumed_from"] = resumed
            held = f"; resumed at tick {resumed} of the stream"
        if raw_path:
            self.stream_result["raw_ticks"], self.stream_result["raw_pending"] = int(ticks.shape[0]), det.raw_pending
            held += (f"; from {ticks.shape[0]} raw ticks, {rolling['prep'].down} to a tick, {det.raw_pending} left in "
                     "an open group")
        if gaps:
            missing_total, _run = det.status_gaps()
            self.stream_result["gap_sensors"] = int((missing_total > 0).sum())
            self.stream_result["missing"] = int(missing_total.sum())
            held += (f"; {self.stream_result['missing']} missing readings held on "
                     f"{self.stream_result['gap_sensors']} sensors")
        if by_sensor:
            lo_c, hi_c = torch.stack([det.calib_counts.min(), det.calib_counts.max()]).tolist()
            self.stream_result["calib_kept"] = det.calib_kept
            self.stream_result["calib_count_min"], self.stream_result["calib_count_max"] = int(lo_c), int(hi_c)
            held += f"; calibrated per sensor on {int(lo_c)} to {int(hi_c)} real validation readings"
        elif calib_gaps:
            self.stream_result["calib_kept"] = det.calib_kept
            held += f"; calibrated on {det.calib_kept} complete validation ticks"
        if recal:
            self.stream_result["recal"] = recal
            self.stream_result["recalibrations"] = det.recals
            self.stream_result["recal_kept"] = det.recal_kept
            held += (f"; {det.recals} recalibrations from a ring of {recal} ticks"
                     + (f", the last from {det.recal_kept} kept ticks" if det.recals and not by_sensor else "")
                     + (f", the last from at least {det.recal_kept} real readings per sensor"
                        if det.recal_kept and by_sensor else ""))
            if det.recal_threshold is not None:
                eligible = int(det.ring_eligible.item()) if det.recals else 0
                self.stream_result["recal_threshold"] = det.recal_threshold
                self.stream_result["recal_eligible"] = eligible
                held += (f", the threshold re-derived with margin {det.recal_threshold:g} from {eligible} eligible ticks "
                         "at the last one")
        lines = ""
        if det.events is not None:
            table = det.episodes().numpy()
            self.stream_result["episodes"] = table
            held += (f"; {table['count']} episodes (on {det.events_cfg['on']}, off {det.events_cfg['off']}, clear "
                     f"{float(det.clear.item()):.6g})")
            for j in range(table["start"].shape[0]):
                ends = "still open" if table["end"][j] < 0 else f"to {int(table['end'][j]) + w}"
                lines += (f"episode {j}: test ticks {int(table['start'][j]) + w} {ends}, peak {table['peak'][j]:.6g} at "
                          f"{int(table['peak_tick'][j]) + w}, sensors {table['sensors'][j].tolist()}\n")
            if events_path:
                np.savez(events_path, **table)
        first = ", ".join(str(int(t) + w) for t in self.stream_result["log_ticks"][:show])
        origin = f"from {normal.shape[1] - w} validation ticks" if resumed is None else f"from {resume_path}"
        print(f"stream: {scored} ticks in pushes of {chunk}, threshold {self.stream_result['threshold']:.6g} "
              f"{origin}: {alarms} alarm ticks" + held
              + (f"; first at test ticks {first}" if alarms else "") + "\n" + lines)
        return self.stream_result

    def save_localisation(self, model, gt, threshold: float, path: str, m: int = 3):
        """-localise PATH: for every test tick whose anomaly score exceeds the report's threshold, the m most
        deviating sensors with their scores, predicted / observed values, the sensors they were reading and the
        attention on them (harness.localise), saved as one .npz (numpy appends the suffix when PATH lacks it)."""
        ev = harness.SeriesEvaluator(model, None, gt, batch=8192, use_graph=False, series=self.test_series,
                                     top_m=min(m, gt.shape[1]))
        anomaly = ev.step()
        self.localisation = harness.localise(ev, torch.nonzero(anomaly > threshold).view(-1))
        np.savez(path, threshold=np.float64(threshold), **self.localisation.numpy())

    def predict_mlp_head(self, model, n_test: int, span: int = 8192):
        """Test predictions of an out_layer_num > 1 model: forward_series on the resident series, `span` windows per
        call (the staged route keeps xlin and z of one call in HBM).  An OutLayer forward_series refuses (hidden
        layers wider than 512 or of unequal widths) goes through the reference's loop: minibatches of materialised
        windows through model(x)."""
        if model.mlp_fast_path_supported():
            pred = torch.empty((n_test, self.test_series.shape[0]), dtype=torch.float32, device=self.device)
            wide = model.input_exceeds_limit(self.test_series)
            for s in range(0, n_test, span):
                e = min(n_test, s + span)
                model.forward_series(self.test_series, s, e - s, out=pred[s:e], wide=wide)
            return pred
        return torch.cat([model(x, None) for x, _y, _l, _e in IndexLoader(
            self.test_dataset, torch.arange(n_test), self.train_config["batch"], False, None)])

    def get_score(self, test_result, val_result):
        """main.py:150-174."""
        test_labels = test_result[2][:, 0]
        test_scores, _, _ = evaluate.anomaly_scores(test_result[0], test_result[1], device=self.device)
        if self.env_config["report"] == "best":
            info = evaluate.get_best_performance_data(test_scores, test_labels, topk=1, device=self.device)
        else:
            normal_scores, _, _ = evaluate.anomaly_scores(val_result[0], val_result[1], device=self.device)
            info = evaluate.get_val_performance_data(test_scores, normal_scores, test_labels, topk=1, device=self.device)
        print("=========================** Result **============================\n")
        print(f"F1 score: {info[0]}")
        print(f"precision: {info[1]}")
        print(f"recall: {info[2]}\n")
        return info

    def get_save_path(self, feature_name=""):
        """main.py:177-195."""
        dir_path = self.env_config["save_path"]
        if self.datestr is None:
            self.datestr = datetime.now().strftime("%m|%d-%H:%M:%S")
        paths = [f"./pretrained/{dir_path}/best_{self.datestr}.pt", f"./results/{dir_path}/{self.datestr}.csv"]
        for path in paths:
            Path(os.path.dirname(path)).mkdir(parents=True, exist_ok=True)
        return paths


def build_parser():
    """main.py:199-217 (single-dash long flags and defaults as in the reference) + -data_root / -no_hip_graph /
    -train_gaps / -localise / -stream / -stream_gaps / -stream_calib_gaps / -stream_recal / -stream_recal_every /
    -stream_recal_threshold /
    -stream_raw / -prep / -stream_save / -stream_resume / -stream_on / -stream_off / -stream_clear / -stream_events."""
    parser = argparse.ArgumentParser()
    parser.add_argument("-batch", help="batch size", type=int, default=128)
    parser.add_argument("-epoch", help="train epoch", type=int, default=100)
    parser.add_argument("-slide_win", help="slide_win", type=int, default=15)
    parser.add_argument("-dim", help="dimension", type=int, default=64)
    parser.add_argument("-slide_stride", help="slide_stride", type=int, default=5)
    parser.add_argument("-save_path_pattern", help="save path pattern", type=str, default="")
    parser.add_argument("-dataset", help="wadi / swat", type=str, default="wadi")
    parser.add_argument("-device", help="cuda / cpu", type=str, default="cuda")
    parser.add_argument("-random_seed", help="random seed", type=int, default=0)
    parser.add_argument("-comment", help="experiment comment", type=str, default="")
    parser.add_argument("-out_layer_num", help="outlayer num", type=int, default=1)
    parser.add_argument("-out_layer_inter_dim", help="out_layer_inter_dim", type=int, default=256)
    parser.add_argument("-decay", help="decay", type=float, default=0)
    parser.add_argument("-val_ratio", help="val ratio", type=float, default=0.1)
    parser.add_argument("-topk", help="topk num", type=int, default=20)
    parser.add_argument("-report", help="best / val", type=str, default="best")
    parser.add_argument("-load_model_path", help="trained model path", type=str, default="")
    parser.add_argument("-data_root", help="directory holding <dataset>/train.csv, test.csv, list.txt", type=str, default="./data")
    parser.add_argument("-no_hip_graph", help="launch every training step eagerly", action="store_true")
    parser.add_argument("-train_gaps", help="train.csv may hold missing (non-finite) readings after its first slide_win "
                        "ticks: hold them at the sensor's last real value and leave them out of the training and "
                        "validation losses (not with -no_hip_graph)", action="store_true")
    parser.add_argument("-localise", help="save the deviating sensors and their attention at the ticks above the "
                        "report's threshold to this .npz", type=str, default="")
    parser.add_argument("-stream", help="after the report, replay the test series through a streaming detector in "
                        "pushes of this many ticks (calibrated on the validation block)", type=int, default=0)
    parser.add_argument("-stream_gaps", help="with -stream: hold missing (non-finite) readings at the sensor's last "
                        "real one and keep them out of the scores", action="store_true")
    parser.add_argument("-stream_calib_gaps", help="with -stream -stream_gaps: calibrate on a validation block that has "
                        "missing readings itself, under the detector's rules", action="store_true")
    parser.add_argument("-stream_recal", help="with -stream: keep the scoring keys of the last R ticks in a calibration "
                        "ring on the device (R >= 64 and >= the push size; seeded from the validation block)", type=int,
                        default=0)
    parser.add_argument("-stream_recal_every", help="with -stream_recal: rewrite the median / IQR table from the ring "
                        "every E replayed ticks (alarm ticks excluded)", type=int, default=0)
    parser.add_argument("-stream_recal_threshold", help="with -stream_recal: every recalibration also re-derives the "
                        "threshold from the ring under the new table, as MARGIN times the ring's largest smoothed score",
                        type=float, default=None, metavar="MARGIN")
    parser.add_argument("-calib_by_sensor", help="with -stream -stream_gaps -stream_calib_gaps: calibrate (and, with "
                        "-stream_recal, recalibrate) every sensor on its own real readings, not on complete ticks only",
                        action="store_true")
    parser.add_argument("-stream_raw", help="with -stream and -prep: replay this RAW csv (engineering units, raw tick "
                        "rate) through the detector's on-device front end instead of the prepared test series",
                        type=str, default="")
    parser.add_argument("-prep", help="the prep.npz `python -m gdn_amd.prep` wrote (min-max table, down, sensor names)",
                        type=str, default="")
    parser.add_argument("-stream_save", help="with -stream: save the running detector to this .npz when the replay ends "
                        "(the file is written exactly here; no suffix is appended)", type=str, default="")
    parser.add_argument("-stream_resume", help="with -stream: start from this saved detector instead of a calibration on "
                        "the validation block, and go on at the tick it had consumed", type=str, default="")
    parser.add_argument("-stream_on", help="with -stream: raise an episode after this many ticks above the threshold",
                        type=int, default=None)
    parser.add_argument("-stream_off", help="with -stream: clear an episode after this many ticks at or below the clear "
                        "level", type=int, default=None)
    parser.add_argument("-stream_clear", help="with -stream: the clear level of an episode (default: the threshold)",
                        type=float, default=None)
    parser.add_argument("-stream_events", help="with -stream: save the episode table to this .npz", type=str, default="")
    parser.add_argument("-tune_alarm", help="after the report, sweep alarm settings (threshold, clear level, on / off "
                        "delay) against the labelled incidents of the test series, print the best one and save the "
                        "sweep to this .npz (test.csv needs an `attack` column)", type=str, default="")
    parser.add_argument("-tune_hi_steps", help="with -tune_alarm: raise levels, taken evenly from the report's "
                        "400-step threshold sweep", type=int, default=None)
    parser.add_argument("-tune_on", help="with -tune_alarm: on-delays in ticks, comma separated", type=str, default=None)
    parser.add_argument("-tune_off", help="with -tune_alarm: off-delays in ticks, comma separated", type=str, default=None)
    return parser


TUNE_ON, TUNE_OFF, TUNE_LO_FRAC = "1,2,3,5,10", "1,5,10,30", (1.0, 0.9, 0.75, 0.5)


def check_tune_alarm(tune_alarm: bool, hi_steps, on, off) -> None:
    """-tune_hi_steps, -tune_on and -tune_off shape the grid of -tune_alarm OUT.npz: refused by name without it, and
    when they do not hold what a grid needs."""
    for given, flag in ((hi_steps is not None, "-tune_hi_steps"), (on is not None, "-tune_on"), (off is not None, "-tune_off")):
        if given and not tune_alarm:
            raise ValueError(f"{flag} needs -tune_alarm OUT.npz: it shapes the grid of the alarm sweep")
    if hi_steps is not None and not 1 <= int(hi_steps) <= evaluate.TH_STEPS:
        raise ValueError(f"-tune_hi_steps {hi_steps}: 1 to {evaluate.TH_STEPS} raise levels")
    for text, flag in ((on, "-tune_on"), (off, "-tune_off")):
        if text is not None:
            tune_ticks(text, flag)


def tune_ticks(text: str, flag: str) -> list:
    """'1,2,3,5,10' -> [1, 2, 3, 5, 10]; anything but whole numbers from 1 to 4096 is refused by the flag's name."""
    try:
        ticks = [int(part) for part in str(text).split(",")]
    except ValueError:
        raise ValueError(f"{flag} {text!r}: whole numbers of ticks, comma separated") from None
    if not ticks or any(not 1 <= v <= 4096 for v in ticks):
        raise ValueError(f"{flag} {text!r}: every delay is 1 to 4096 ticks")
    return ticks


def tune_alarm_grid(thresholds, hi_steps: int, on: str, off: str) -> tuple:
    """(hi, on, off) of -tune_alarm's grid: `hi_steps` of the sweep's thresholds at evenly spaced places, duplicates
    dropped (a float64 tensor on the thresholds' device), and the two lists of delays."""
    thresholds = torch.as_tensor(thresholds, dtype=torch.float64).reshape(-1)
    at = torch.linspace(0, thresholds.numel() - 1, int(hi_steps), dtype=torch.float64).round().long()
    return torch.unique(thresholds[at.to(thresholds.device)]), tune_ticks(on, "-tune_on"), tune_ticks(off, "-tune_off")


def check_attack_column(path: str) -> None:
    """-tune_alarm matches episodes against labelled incidents: a test file without an `attack` column is refused by
    name (the report itself reads such a file as all normal)."""
    import pandas as pd
    if "attack" not in pd.read_csv(path, sep=",", index_col=0, nrows=0).columns:
        raise ValueError(f"-tune_alarm needs labels: {path} has no `attack` column")


def check_stream_events(stream_on: bool, stream_off: bool, stream_clear: bool, stream_events: bool, stream: bool) -> None:
    """-stream_on, -stream_off, -stream_clear and -stream_events configure the episode table of a streaming detector:
    they mean something only with -stream C (the detector).  Refused by name otherwise."""
    for given, flag in ((stream_on, "-stream_on"), (stream_off, "-stream_off"), (stream_clear, "-stream_clear"),
                        (stream_events, "-stream_events")):
        if given and not stream:
            raise ValueError(f"{flag} needs -stream C: the episode table is the streaming detector's")


def stream_events_config(stream_on, stream_off, stream_clear, stream_events: str):
    """StreamDetector's events= for the four flags: None when none of them is given (no episode table)."""
    if stream_on is None and stream_off is None and stream_clear is None and not stream_events:
        return None
    return {"on": 1 if stream_on is None else int(stream_on), "off": 1 if stream_off is None else int(stream_off),
            "lo": None if stream_clear is None else float(stream_clear)}


def check_stream_checkpoint(stream_save: bool, stream_resume: bool, stream: bool) -> None:
    """-stream_save and -stream_resume name the file a streaming detector is saved to or resumed from: they mean
    something only with -stream C (the detector).  Refused by name otherwise."""
    if stream_save and not stream:
        raise ValueError("-stream_save needs -stream C: the file holds the streaming detector the replay leaves behind")
    if stream_resume and not stream:
        raise ValueError("-stream_resume needs -stream C: the file holds a streaming detector, which the replay continues")


def check_stream_raw(stream_raw: bool, stream: bool, prep: bool) -> None:
    """-stream_raw names the raw file a streaming detector replays through its front end: it means something only
    with -stream C (the detector) and -prep prep.npz (the fitted table).  Refused by name otherwise."""
    if stream_raw and not stream:
        raise ValueError("-stream_raw needs -stream C: the raw file is replayed through the streaming detector")
    if stream_raw and not prep:
        raise ValueError("-stream_raw needs -prep prep.npz: raw readings are normalised with the table fitted on the "
                         "training file (python -m gdn_amd.prep)")


def check_calib_by_sensor(by_sensor: bool, stream: bool, stream_gaps: bool, stream_calib_gaps: bool) -> None:
    """-calib_by_sensor chooses how the streaming detector's calibration treats missing readings, so it has a meaning
    only where that calibration sees them: with -stream C -stream_gaps -stream_calib_gaps.  Refused by name otherwise."""
    if by_sensor and not (stream and stream_gaps and stream_calib_gaps):
        raise ValueError("-calib_by_sensor needs -stream C -stream_gaps -stream_calib_gaps: it calibrates every sensor "
                         "on its own real readings of a validation block that has missing ones")


def check_train_gaps(train_gaps: bool, hip_graph: bool) -> None:
    """-train_gaps trains through harness.train_series (the windows and their validity bytes are cut on the device);
    the eager loop over the loaders (-no_hip_graph) has no masked loss, so the pair is refused by name."""
    if train_gaps and not hip_graph:
        raise ValueError("-train_gaps needs the device-epoch path (harness.train_series): it cannot be combined with "
                         "-no_hip_graph, whose eager loop over the loaders has no masked loss")


def from_args(argv=None) -> Main:
    """The Main of a command line: flags checked, seeds set, data read, model built; `.run()` does the rest."""
    args = build_parser().parse_args(argv)
    check_train_gaps(args.train_gaps, not args.no_hip_graph)
    check_calib_by_sensor(args.calib_by_sensor, bool(args.stream), args.stream_gaps, args.stream_calib_gaps)
    check_stream_raw(bool(args.stream_raw), bool(args.stream), bool(args.prep))
    check_stream_checkpoint(bool(args.stream_save), bool(args.stream_resume), bool(args.stream))
    check_stream_events(args.stream_on is not None, args.stream_off is not None, args.stream_clear is not None,
                        bool(args.stream_events), bool(args.stream))
    check_tune_alarm(bool(args.tune_alarm), args.tune_hi_steps, args.tune_on, args.tune_off)
    random.seed(args.random_seed)                      # main.py:221-228
    np.random.seed(args.random_seed)
    torch.manual_seed(args.random_seed)
    torch.cuda.manual_seed(args.random_seed)
    torch.cuda.manual_seed_all(args.random_seed)
    os.environ["PYTHONHASHSEED"] = str(args.random_seed)
    train_config = {"batch": args.batch, "epoch": args.epoch, "slide_win": args.slide_win, "dim": args.dim,
                    "slide_stride": args.slide_stride, "comment": args.comment, "seed": args.random_seed,
                    "out_layer_num": args.out_layer_num, "out_layer_inter_dim": args.out_layer_inter_dim,
                    "decay": args.decay, "val_ratio": args.val_ratio, "topk": args.topk,
                    "hip_graph": not args.no_hip_graph, "train_gaps": args.train_gaps}
    env_config = {"save_path": args.save_path_pattern, "dataset": args.dataset, "report": args.report,
                  "device": args.device, "load_model_path": args.load_model_path, "data_root": args.data_root,
                  "localise": args.localise, "stream": args.stream,
                  "stream_gaps": args.stream_gaps, "stream_calib_gaps": args.stream_calib_gaps, "stream_recal": args.stream_recal,
                  "stream_recal_every": args.stream_recal_every, "calib_by_sensor": args.calib_by_sensor,
                  "stream_recal_threshold": args.stream_recal_threshold,
                  "stream_raw": args.stream_raw, "prep": args.prep, "stream_save": args.stream_save,
                  "stream_resume": args.stream_resume, "stream_on": args.stream_on, "stream_off": args.stream_off,
                  "stream_clear": args.stream_clear, "stream_events": args.stream_events,
                  "tune_alarm": args.tune_alarm, "tune_hi_steps": args.tune_hi_steps, "tune_on": args.tune_on,
                  "tune_off": args.tune_off}
    return Main(train_config, env_config, debug=False)


def main(argv=None):
    return from_args(argv).run()


if __name__ == "__main__":
    main()
