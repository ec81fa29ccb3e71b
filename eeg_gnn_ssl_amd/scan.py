"""Whole recordings through a trained detector, on the device: when are the seizures?

`DeviceEvaluator` stops at the clip: one probability per row of a clip table.  A `Scanner` (`TrainStep.scanner`) is the layer above
it.  It builds the table of the sliding windows of every recording (`clip_table_scan`), drives the evaluator's own pass over it --
the step's data chain without augmentation, the `save=False` forward, one captured HIP graph per step, the all-reduce of disjoint
slots -- and turns the clip probabilities into
    a per-second probability timeline per recording (`ops.scan_timeline`: overlap mean or max),
    seizure events (`ops.scan_events`: smoothing, hysteresis, gap merge, minimum duration) and, against annotated intervals,
    event- and bin-level scores (`ops.event_scores`: sensitivity, false alarms per 24 h, bin precision / recall / F1)
with three kernels on the stream behind the pass and ONE device-to-host copy of a ten-word integer record.  The semantics are those
of include/eeg_dcrnn.h; DESIGN.md §4.3 states them and §8 the limits."""
from __future__ import annotations

from collections import OrderedDict
from typing import Optional

import torch
import torch.distributed as dist

from . import ops
from .device_data import RecordingDataset, clip_table_scan, layout_recordings
from .evaluation import DeviceEvaluator

_W = {name: i for i, name in enumerate(ops.SCAN_RECORD)}


def _div(a, b):
    return float(a) / float(b) if b else float("nan")


def scores_from_scan_record(record, window: int, freq: int = 200):
    """The event- and bin-level scores from the int64 record of `ops.event_scores`, in float64 on the host: sensitivity = ref_hit /
    n_ref, false_alarms_per_24h = (n_hyp - hyp_hit) / (covered_bins * window / freq / 86400), bin precision, recall and F1 over the
    covered bins.  A ratio without support (no reference event, no covered bin, no predicted bin) is NaN; nothing raises."""
    rec = [int(v) for v in (record.cpu().tolist() if torch.is_tensor(record) else record)]
    tp, fp, fn = rec[_W["tp"]], rec[_W["fp"]], rec[_W["fn"]]
    days = rec[_W["covered_bins"]] * float(window) / float(freq) / 86400.0
    return OrderedDict([
        ("sensitivity", _div(rec[_W["ref_hit"]], rec[_W["n_ref"]])),
        ("false_alarms_per_24h", _div(rec[_W["n_hyp"]] - rec[_W["hyp_hit"]], days)),
        ("n_ref", rec[_W["n_ref"]]), ("n_hyp", rec[_W["n_hyp"]]),
        ("bin_precision", _div(tp, tp + fp)), ("bin_recall", _div(tp, tp + fn)), ("bin_F1", _div(2 * tp, 2 * tp + fp + fn))])


class ScanResult:
    """What `Scanner.run` / `Scanner.postprocess` return.  On the device: clip_probs (P,), clip_off (R+1,), bin_off (R+1,), timeline,
    smoothed (total_bins,) float32, cover (total_bins,) int32, events (R, E_max, 2) int32 (onset, offset exclusive, in bins),
    event_count (R,) int32, rec_records (R, words) int64.  On the host: record (the words of ops.SCAN_RECORD) and, when annotations
    were given, scores (OrderedDict: sensitivity, false_alarms_per_24h, n_ref, n_hyp, bin_precision, bin_recall, bin_F1); else None."""

    def __init__(self, clip_probs, clip_off, buffers, window: int, freq: int, annotated: bool):
        self.clip_probs, self.clip_off = clip_probs, clip_off
        self.bin_off, self.timeline, self.cover, self.smoothed = buffers.bin_off, buffers.timeline, buffers.cover, buffers.smoothed
        self.events, self.event_count, self.rec_records = buffers.events, buffers.event_count, buffers.rec_records
        self.window, self.freq = int(window), int(freq)
        self.record = buffers.record.cpu()                               # the post-processing's one device-to-host copy
        if int(self.record[_W["overflowed"]]):
            counts = self.event_count.cpu().tolist()
            e_max = int(self.events.shape[1])
            r = next(i for i, c in enumerate(counts) if c > e_max)
            raise ValueError(f"Scanner: recording {r} has {counts[r]} events, max_events={e_max} rows are kept ({int(self.record[_W['overflowed']])} "
                             f"recording(s) overflow): raise max_events, or min_bins / merge_gap / the thresholds")
        self.scores = scores_from_scan_record(self.record, self.window, self.freq) if annotated else None
        self._host = None

    def _offsets(self):
        if self._host is None:
            self._host = (self.clip_off.cpu().tolist(), self.bin_off.cpu().tolist(), self.event_count.cpu().tolist())
        return self._host

    def per_recording(self, r: int):
        """views of recording r: its clip probabilities, timeline, cover, smoothed timeline and events (n, 2)"""
        clip_off, bin_off, counts = self._offsets()
        c, b = slice(clip_off[r], clip_off[r + 1]), slice(bin_off[r], bin_off[r + 1])
        return OrderedDict([("clip_probs", self.clip_probs[c]), ("timeline", self.timeline[b]), ("cover", self.cover[b]),
                            ("smoothed", self.smoothed[b]), ("events", self.events[r, :counts[r]])])

    def bootstrap(self, n_boot: int = 2000, seed: int = 0, groups=None):
        """Bootstrap replicates of the scan's scores -> `BootstrapResult` (bootstrap.py): the R recordings are resampled with
        replacement -- or patients, through groups (R,) integer ids 0..G-1 --, a replicate's record is the weighted sum of
        `rec_records` (`ops.boot_records`) and its scores are `scores_from_scan_record` of that sum.  Needs annotations."""
        from .bootstrap import bootstrap_scan
        return bootstrap_scan(self, n_boot=n_boot, seed=seed, groups=groups)

    def events_seconds(self):
        """the detected events as a host list of (rec, onset_s, offset_s)"""
        _, _, counts = self._offsets()
        ev = self.events.cpu().tolist()
        sec = float(self.window) / float(self.freq)
        return [(r, ev[r][k][0] * sec, ev[r][k][1] * sec) for r in range(len(counts)) for k in range(counts[r])]


class Scanner(DeviceEvaluator):
    """`TrainStep.scanner(recordings, x_steps=T, stride_steps=s, ...)`: scan whole recordings with the step's detector on the device.

    recordings: a list of (N, L_r) float32 recordings, or (signals, rec_table, num_channels) of an earlier `RecordingDataset`.  Every
    recording of at least T whole steps is cut into windows of T steps every s steps (+ one tail window: `clip_table_scan`); the pass
    over that table IS `DeviceEvaluator`'s (zero labels, its sampler, its captured body), so a window's probability has the bits the
    evaluator gives that row.  `run(...)` = the pass + `postprocess(...)`; `postprocess` alone re-runs the three kernels on the
    probabilities of the last pass (other thresholds, same weights).  Limits: task detection, one shared graph or supports=None,
    P <= ops.EVAL_MAX_CLIPS windows per scanner, recordings shorter than T steps get no window (their bins stay uncovered), samples
    behind a recording's last whole step are ignored."""

    def __init__(self, step, recordings, x_steps: int, stride_steps: int, batch_size: int = 256, supports=None, cover_tail: bool = True,
                 max_events: int = 64, freq: int = 200, rank: Optional[int] = None, world: Optional[int] = None):
        if step.task != "detection":
            raise ValueError(f"Scanner: task={step.task!r}: a scan turns the detector's one probability per window into a timeline; evaluate "
                             f"this task per clip with TrainStep.evaluator" + (" / TrainStep.ssl_evaluator" if step.task == "ssl" else ""))
        classes = int(step.model.fc.weight.shape[0])
        if classes != 1:
            raise ValueError(f"Scanner: the model's head has {classes} outputs; a detector has one")
        if step.raw_window is None:
            raise ValueError("Scanner: the step has raw_window=None; whole recordings are raw signals: build it as TrainStep(raw_window=W, ...)")
        if int(max_events) < 1:
            raise ValueError(f"Scanner: max_events={max_events}: E_max < 1 holds no event")
        if int(batch_size) < 1:
            raise ValueError(f"Scanner: batch_size={batch_size}")
        dev, window = step.fp.flat.device, int(step.raw_window)
        if isinstance(recordings, tuple) and len(recordings) == 3 and torch.is_tensor(recordings[0]) and recordings[0].dim() == 1:
            signals, rec_table, channels = recordings
        else:
            recordings = list(recordings)
            signals, rec_table = layout_recordings(recordings, dev)
            channels = int(torch.as_tensor(recordings[0]).shape[0])
        rec_samples = torch.as_tensor(rec_table).cpu()[:, 2].tolist()
        table, clip_off = clip_table_scan(rec_samples, x_steps, stride_steps, window, cover_tail)
        if len(table) < 1:
            raise ValueError(f"Scanner: no recording holds x_steps={x_steps} whole steps of {window} samples (the longest has "
                             f"{max(rec_samples) // window}): nothing to scan")
        if len(table) > ops.EVAL_MAX_CLIPS:
            raise ValueError(f"Scanner: the scan has P={len(table)} windows, one pass takes at most {ops.EVAL_MAX_CLIPS} (ops.EVAL_MAX_CLIPS); "
                             f"scan the recordings in parts")
        dataset = RecordingDataset(signals, table, torch.zeros(len(table), dtype=torch.float32, device=signals.device), window=window,
                                   x_steps=int(x_steps), rec_table=rec_table, num_channels=int(channels))
        super().__init__(step, dataset, min(int(batch_size), len(table)), supports=supports, rank=rank, world=world)
        self.x_steps, self.stride_steps, self.window, self.freq, self.max_events = int(x_steps), int(stride_steps), window, int(freq), int(max_events)
        self.rec_steps = [int(n) // window for n in rec_samples]
        self.clip_off = torch.from_numpy(clip_off).to(dev)
        self.bin_off = ops.scan_buffers(self.rec_steps, self.max_events, dev).bin_off
        ops.scan_check_tables(dataset.clip_table, self.clip_off, self.bin_off, self.x_steps, window, len(table), sum(self.rec_steps), "Scanner")
        r = len(self.rec_steps)
        self._no_ref = (torch.zeros(r, 1, 2, dtype=torch.int32, device=dev), torch.zeros(r, dtype=torch.int32, device=dev))
        self._passed = False

    @torch.no_grad()
    def run(self, agg: str = "mean", smooth_bins: int = 1, th_on: float = 0.5, th_off: Optional[float] = None, merge_gap: int = 0,
            min_bins: int = 1, annotations=None, capture: bool = True) -> ScanResult:
        """One pass over every window, then `postprocess` with these arguments.  capture: replay the step's body as one HIP graph
        (captured at the first such call) instead of issuing it eagerly.  Leaves the model's mode, the step's counters, optimiser
        state, generators and sampler alone."""
        self._check_post(agg, smooth_bins, th_on, th_off, merge_gap, min_bins, annotations)           # refuse before the pass, not behind it
        s, model = self.sampler, self.step.model
        multi = s.world > 1
        if multi and not (dist.is_available() and dist.is_initialized() and dist.get_world_size() == s.world):
            raise RuntimeError(f"Scanner: world={s.world} needs a process group of that size for the all-reduce of the probabilities")
        was_training = model.training
        model.eval()
        try:
            self._replay(capture)
            if multi:
                dist.all_reduce(self._scores, op=dist.ReduceOp.SUM)
        finally:
            model.train(was_training)
        self._passed = True
        return self.postprocess(agg, smooth_bins, th_on, th_off, merge_gap, min_bins, annotations)

    def _check_post(self, agg, smooth_bins, th_on, th_off, merge_gap, min_bins, annotations):
        if agg not in ops.SCAN_AGG:
            raise ValueError(f"Scanner: agg={agg!r} (one of {sorted(ops.SCAN_AGG)})")
        if int(smooth_bins) < 1 or int(smooth_bins) % 2 == 0 or int(smooth_bins) > ops.SCAN_MAX_SMOOTH_BINS:
            raise ValueError(f"Scanner: smooth_bins={smooth_bins} must be odd, 1..{ops.SCAN_MAX_SMOOTH_BINS} (a centred window; 1 = no smoothing)")
        ops.scan_thresholds(th_on, th_off)
        if int(merge_gap) < 0 or int(min_bins) < 1:
            raise ValueError(f"Scanner: merge_gap={merge_gap} (>= 0), min_bins={min_bins} (>= 1)")
        if annotations is None:
            return self._no_ref
        ref, ref_count = (torch.as_tensor(a) for a in annotations)
        r = len(self.rec_steps)
        if ref.dim() != 3 or ref.shape[0] != r or ref.shape[1] < 1 or ref.shape[2] != 2 or tuple(ref_count.shape) != (r,):
            raise ValueError(f"Scanner: annotations must be (ref (R, A_max, 2), ref_count (R,)) for the R={r} recordings (annotation_bins), got "
                             f"{tuple(ref.shape)} and {tuple(ref_count.shape)}")
        dev = self.probs.device
        return ref.to(device=dev, dtype=torch.int32).contiguous(), ref_count.to(device=dev, dtype=torch.int32).contiguous()

    @torch.no_grad()
    def postprocess(self, agg: str = "mean", smooth_bins: int = 1, th_on: float = 0.5, th_off: Optional[float] = None, merge_gap: int = 0,
                    min_bins: int = 1, annotations=None) -> ScanResult:
        """Timeline, events and scores from the probabilities of the last pass: three kernels and one copy of the record, into
        buffers of the result's own.  annotations: (ref, ref_count) of `annotation_bins`, or None (no scores; the record still counts
        events and covered bins).  An event overflow raises ValueError and names the first recording and its count."""
        if not self._passed:
            raise ValueError("Scanner.postprocess: no pass has run yet: call run(...) first")
        ref, ref_count = self._check_post(agg, smooth_bins, th_on, th_off, merge_gap, min_bins, annotations)
        buf = ops.scan_buffers(self.rec_steps, self.max_events, self.probs.device, zeroed=False)
        probs = self.probs.clone()
        ops.scan_timeline(probs, self.dataset.clip_table, self.clip_off, buf.bin_off, buf.timeline, buf.cover, x_steps=self.x_steps,
                          window=self.window, agg=agg, validate=False)
        ops.scan_events(buf.timeline, buf.cover, buf.bin_off, buf.smoothed, buf.events, buf.event_count, smooth_bins=smooth_bins, th_on=th_on,
                        th_off=th_off, merge_gap=merge_gap, min_bins=min_bins, validate=False)
        ops.event_scores(buf.events, buf.event_count, ref, ref_count, buf.cover, buf.bin_off, buf.record, buf.rec_records, validate=False)
        return ScanResult(probs, self.clip_off, buf, self.window, self.freq, annotations is not None)
