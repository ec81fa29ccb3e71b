"""Epochs from a data set that stays in device memory (HBM): the reference's `DataLoader(dataset, shuffle=True, batch_size=...)`
(data/dataloader_detection.py:505-523, dataloader_classification.py:449-467, dataloader_ssl.py:441-459) without the host.

`TrainStep.capture` replays on static input tensors, so a host loader has to copy every batch over the link (117 MB of features
per cfg2 step, 233 MB of raw signals) -- the link, not the kernels, then sets the rate.  A 60-s clip is 456 KB as features and
912 KB raw and the card has 288 GB: the training sets of the reference's recipes fit.  `DeviceDataset` holds the pools, an
`EpochSampler` the epoch's permutation and a cursor, both on the device; `TrainStep.step_from` / `capture_epoch` gather each
step's batch out of the pools (`ops.gather_clips`: one launch + the cursor's) in front of the unchanged step.

The epoch's short last batch.  The reference's loaders keep it (`drop_last=False`): `EpochSampler(..., drop_last=False)` does the
same -- ceil(P / (batch_size * world)) steps, the last one on the P mod (batch_size * world) clips that remain.  A captured graph
has one batch size, but not one count of clips that matter: the gather wraps, so the slots behind the end of the epoch hold real
clips, and it writes which slots count (`clip_w`), the step's global count (`n_valid`) and the divisor of the rank's criterion
(`denom = max(n_valid, 1) / world`) into device memory; the criterion kernels select the other slots out (loss term and seed
exactly zero, hence a zero contribution to every gradient) and divide by `denom`.  Behind the summed all-reduce and its 1/world
the gradient is sum_valid g_b / n_valid: the mean over the clips that are there, what the reference's single process computes for
its short batch (on one rank the plain mean; the RMSE of the SSL task is the clip-weighted mean of the ranks' losses, a rank's loss
being that of its shard as everywhere here).  A rank whose slots all lie behind the end contributes zeros and still takes part in
the all-reduce.  The DEFAULT, `drop_last=True`, deviates from the reference: the short batch is dropped (other clips every epoch)
and the step runs the unweighted kernels.

Clips cut on the device.  The reference's loaders keep whole resampled recordings (num_channels, num_samples) and cut a clip out
by index arithmetic at `__getitem__` time.  `RecordingDataset` does the same in HBM: the recordings lie channel-major in one
signal buffer, a clip is a row (rec, x_start, x_samples, y_start) of an int64 table on the device, and `ops.gather_records` cuts
the step's batch -- raw signals (B, N, Tx*W), the SSL target (B, N, Ty*W), lengths, labels -- in front of the unchanged raw chain.
The SSL target is then no pool of its own, a classification clip needs no host padding, and overlapping or strided clips cost a
table row each.  `clip_table_detection` / `clip_table_ssl` / `clip_table_classification` restate the three loaders' arithmetic.
Both data sets hand their batch over through one method, `gather`.  Recordings that still have their native sampling rates go
through `RecordingDataset.from_native_rate`: each is resampled on the device straight into the signal buffer (resample.py); EDF files
go through `RecordingDataset.from_edf`, which decodes their payload bytes on the device in front of that (edf.py).

Class imbalance.  `BalancedEpochSampler` draws a balanced epoch out of the whole resident pool -- every epoch anew, or once per run
as the reference's detection loader does -- into a permutation shorter than the pool, which the gathers take as it is;
`TrainStep(class_weights=, sample_weights=)` weighs the clips of a step on the device (`ops.clip_weights`)."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
import torch.distributed as dist

from . import ops


class DeviceDataset:
    """Pools of P clips on the device, contiguous, never copied:
    x: features / windows (P, T, N, D) or raw signals (P, N, T*W), float32;
    y: labels (P,) (float32: detection, int64: classification) or the SSL target pool (P, ...) like x;
    seq_lengths: optional int64 (P,), the clips' valid steps (`TrainStep(padding_val=...)`)."""

    def __init__(self, x: torch.Tensor, y: torch.Tensor, seq_lengths: Optional[torch.Tensor] = None):
        pools = [("x", x), ("y", y)] + ([("seq_lengths", seq_lengths)] if seq_lengths is not None else [])
        for name, t in pools:
            if not torch.is_tensor(t):
                raise TypeError(f"DeviceDataset: {name} must be a tensor on the device, got {type(t).__name__}")
            if t.device != x.device:
                raise ValueError(f"DeviceDataset: {name} is on {t.device}, x on {x.device}: the pools live on one device")
            if not t.is_contiguous():
                raise ValueError(f"DeviceDataset: {name} must be contiguous (the pools are read in place, clip by clip)")
            if t.dim() < 1 or t.shape[0] != x.shape[0]:
                raise ValueError(f"DeviceDataset: {name} holds {t.shape[0] if t.dim() else 0} clips, x holds {x.shape[0]}: one leading "
                                 f"dimension P for all pools")
        if x.dim() not in (3, 4) or x.dtype != torch.float32 or x.shape[0] < 1:
            raise ValueError(f"DeviceDataset: x must be float32 features / windows (P, T, N, D) or raw signals (P, N, T*W), got "
                             f"{x.dtype} {tuple(x.shape)}")
        self.y_is_target = y.dim() > 1
        if self.y_is_target and y.dtype != torch.float32:
            raise ValueError(f"DeviceDataset: y {tuple(y.shape)} is a target pool and must be float32, got {y.dtype}")
        if not self.y_is_target and y.dtype not in (torch.float32, torch.int64):
            raise ValueError(f"DeviceDataset: y (P,) must hold float32 (detection) or int64 (classification) labels, got {y.dtype}")
        for name, t in (("x", x),) + ((("y", y),) if self.y_is_target else ()):
            row = t[0].numel() * t.element_size()
            if row == 0 or row % 16 != 0:
                raise ValueError(f"DeviceDataset: a clip of {name} has {row} bytes; the rows of a wide pool must be whole 16-byte pieces")
        if seq_lengths is not None and (seq_lengths.dtype != torch.int64 or seq_lengths.dim() != 1):
            raise ValueError(f"DeviceDataset: seq_lengths must be int64 (P,), got {seq_lengths.dtype} {tuple(seq_lengths.shape)}")
        self.x, self.y, self.seq_lengths = x, y, seq_lengths

    def __len__(self):
        return self.x.shape[0]

    @property
    def device(self):
        return self.x.device

    # what the call sites of a step's batch read (TrainStep._epoch_batch, DeviceEvaluator, DeviceSSLEvaluator) -- of this class and of
    # RecordingDataset alike: the shapes of one clip, whether a gather writes lengths, and the gather itself
    @property
    def x_shape(self):
        return tuple(self.x.shape[1:])

    @property
    def y_shape(self):
        return tuple(self.y.shape[1:])

    @property
    def y_dtype(self):
        return self.y.dtype

    @property
    def has_lengths(self):
        return self.seq_lengths is not None

    def check_step(self, step, who: str):
        """pools are taken as they are: features, windows or raw signals, whatever the step's chain expects"""

    def gather(self, sampler, x_out, y_out, len_out=None):
        """the sampler's next batch into the static batch tensors (`ops.gather_clips`; y_out: the labels or the target; len_out:
        only with a length pool); a drop_last=False sampler also gets its clip_w / denom / n_valid written"""
        wide = self.y_is_target
        ops.gather_clips(self.x, x_out, sampler.perm, sampler.cursor, sampler.rank, sampler.world,
                         y_pool=self.y if wide else None, y_out=y_out if wide else None,
                         label_pool=None if wide else self.y, label_out=None if wide else y_out,
                         len_pool=self.seq_lengths if len_out is not None else None, len_out=len_out,
                         clip_w=sampler.clip_w, denom=sampler.denom, n_valid=sampler.n_valid)     # (None, None, None: drop_last)

    def full_lengths(self, count: int, raw_window: Optional[int] = None, who: str = "DeviceDataset"):
        """The lengths of `count` clips of a label pool WITHOUT a length pool: every clip is whole, so the constant int64 (count,) the
        model's last-step gather reads (`encoder.run(lengths=None)` returns no top state) -- T for features / windows (P, T, N, D),
        T*W // raw_window for raw signals (P, N, T*W).  The one rule for the training side (`TrainStep._epoch_batch`) and the
        evaluation side (`batches`).  A target pool (ssl) has no lengths: None."""
        if self.y_is_target:
            return None
        if self.x.dim() == 4:
            steps = self.x.shape[1]
        else:
            if raw_window is None or int(raw_window) < 1 or self.x.shape[2] % int(raw_window) != 0:
                raise ValueError(f"{who}: x {tuple(self.x.shape)} holds raw signals (P, N, T*W) and there is no seq_lengths pool: the number "
                                 f"of steps of a whole clip is T*W // raw_window, and raw_window={raw_window} (a divisor of {self.x.shape[2]} "
                                 f"is needed)")
            steps = self.x.shape[2] // int(raw_window)
        return torch.full((int(count),), steps, dtype=torch.int64, device=self.device)

    def batches(self, batch_size: int, supports=None, raw_window: Optional[int] = None):
        """Sequential (x, y, seq_lengths, supports) views of the pools, the last partial batch included, no copy: what `predict`,
        `evaluate` and `evaluate_ssl` iterate over (supports: None = correlation graphs built on the device, or the shared graph).
        seq_lengths: views of the length pool; without one the constant full lengths of a label pool (`full_lengths`: a raw pool needs
        `raw_window` for them), None for a target pool."""
        if batch_size < 1:
            raise ValueError(f"DeviceDataset.batches: batch_size={batch_size}")
        lens = self.seq_lengths if self.seq_lengths is not None else self.full_lengths(len(self), raw_window, "DeviceDataset.batches")
        for i in range(0, len(self), batch_size):
            j = min(i + batch_size, len(self))
            yield self.x[i:j], self.y[i:j], None if lens is None else lens[i:j], supports


def layout_recordings(recordings, device):
    """whole recordings [(N, L_r) float32, ...] -> (signals, rec_table) on `device`: one flat float32 buffer, recording r
    channel-major at rec_table[r] = (offset, stride, samples) (int64 (R, 3)) with offset and stride padded to multiples of 4 floats
    (every channel row starts on a 16-byte piece) and the padding zero.  One upload per recording, no host copy of the whole set."""
    if len(recordings) < 1:
        raise ValueError("RecordingDataset: no recordings")
    shapes = []
    for r, rec in enumerate(recordings):
        t = torch.as_tensor(rec)
        if t.dim() != 2 or t.dtype != torch.float32 or t.shape[0] < 1 or t.shape[1] < 1 or t.shape[0] != torch.as_tensor(recordings[0]).shape[0]:
            raise ValueError(f"RecordingDataset: recording {r} must be float32 (N, L_r) with the N of recording 0, got {t.dtype} {tuple(t.shape)}")
        shapes.append(tuple(t.shape))
    n = shapes[0][0]
    table, offset = [], 0
    for _, samples in shapes:
        stride = -(-samples // 4) * 4
        table.append((offset, stride, samples))
        offset += n * stride
    signals = torch.zeros(offset, dtype=torch.float32, device=device)
    for rec, (off, stride, samples) in zip(recordings, table):
        signals[off:off + n * stride].view(n, stride)[:, :samples].copy_(torch.as_tensor(rec))
    return signals, torch.tensor(table, dtype=torch.int64, device=device)


class RecordingDataset:
    """Whole recordings in device memory and a table of the P clips to cut out of them (module docstring):
    recordings: a list of (N, L_r) float32 tensors / arrays, laid out by `layout_recordings` -- or the flat device buffer `signals` of
        an earlier data set together with rec_table= and num_channels= (load once, build several tables);
    clip_table: int64 (P, 4) = (rec, x_start, x_samples, y_start), numpy or tensor (`clip_table_detection` / `_ssl` /
        `_classification`), validated HERE on the host and uploaded;
    y: the labels (P,) (float32: detection, int64: classification), or None with y_steps > 0 (task ssl: the target is cut, too);
    window: samples per step (TrainStep(raw_window=window)); x_steps / y_steps: steps of the input clip and of the SSL target.
    A batch is x (B, N, x_steps*window), the whole steps of a clip's x_samples and zeros behind them, its lengths (B,) int64 -- what
    TrainStep(padding_val=...) and the length-aware graph read -- and the labels (B,) or the target (B, N, y_steps*window)."""

    has_lengths = True

    def __init__(self, recordings, clip_table, y=None, *, window: int, x_steps: int, y_steps: int = 0, device=None, rec_table=None,
                 num_channels: Optional[int] = None):
        self.window, self.x_steps, self.y_steps = int(window), int(x_steps), int(y_steps)
        if self.window < 4 or self.window % 4 != 0:
            raise ValueError(f"RecordingDataset: window={window} must be a positive multiple of 4 (rows of whole 16-byte pieces)")
        if self.x_steps < 1 or self.y_steps < 0:
            raise ValueError(f"RecordingDataset: x_steps={x_steps} (>= 1), y_steps={y_steps} (>= 0)")
        if torch.is_tensor(recordings) and recordings.dim() == 1:
            if rec_table is None or num_channels is None:
                raise ValueError("RecordingDataset: a ready signal buffer comes with rec_table= (R, 3) and num_channels=")
            self.signals, self.N = recordings, int(num_channels)
            self.rec_table = torch.as_tensor(rec_table, dtype=torch.int64).to(self.signals.device).contiguous()
            if self.signals.dtype != torch.float32 or not self.signals.is_contiguous() or self.signals.numel() < 4 or self.signals.numel() % 4 != 0:
                raise ValueError(f"RecordingDataset: signals must be a contiguous flat float32 buffer of whole 16-byte pieces, got "
                                 f"{self.signals.dtype} {tuple(self.signals.shape)}")
            if device is not None and torch.device(device) != self.signals.device:
                raise ValueError(f"RecordingDataset: signals is on {self.signals.device}, device={device}")
        else:
            if rec_table is not None:
                raise ValueError("RecordingDataset: rec_table= goes with a ready signal buffer, not with a list of recordings")
            if device is None:
                device = torch.device("cuda", torch.cuda.current_device())
            self.signals, self.rec_table = layout_recordings(list(recordings), device)
            self.N = int(torch.as_tensor(recordings[0]).shape[0])
        recs = self.rec_table.cpu().numpy()
        if recs.ndim != 2 or recs.shape[1] != 3 or recs.shape[0] < 1 or self.N < 1:
            raise ValueError(f"RecordingDataset: rec_table must be (R, 3) = (offset, stride, samples), got {recs.shape}; num_channels={self.N}")
        for r, (off, stride, samples) in enumerate(recs.tolist()):
            if off < 0 or samples < 1 or stride < samples or off + (self.N - 1) * stride + samples > self.signals.numel():
                raise ValueError(f"RecordingDataset: rec_table[{r}] = (offset={off}, stride={stride}, samples={samples}) with {self.N} channels "
                                 f"does not lie inside the {self.signals.numel()} floats of signals (stride >= samples >= 1)")
        table = clip_table.cpu().numpy() if torch.is_tensor(clip_table) else np.asarray(clip_table)
        if table.ndim != 2 or table.shape[1] != 4 or table.shape[0] < 1 or table.dtype.kind not in "iu":
            raise ValueError(f"RecordingDataset: clip_table must be an integer (P, 4) = (rec, x_start, x_samples, y_start), got {table.dtype} "
                             f"{table.shape}")
        table = table.astype(np.int64)
        rec, x_start, x_samples, y_start = table.T
        in_range = (rec >= 0) & (rec < recs.shape[0])
        samples = recs[np.where(in_range, rec, 0), 2]
        no_step = (x_start < 0) | (x_start > samples - self.window)          # (no sum of a table entry: none overflows)
        bad = ~in_range | (x_samples < self.window) | no_step | ((y_start < 0) if self.y_steps > 0 else False)
        if bad.any():                                                        # the first offending clip, by name
            p = int(np.argmax(bad))
            if not in_range[p]:
                raise ValueError(f"RecordingDataset: clip {p} names recording rec={rec[p]}, there are {recs.shape[0]}")
            if x_samples[p] < self.window:
                raise ValueError(f"RecordingDataset: clip {p} has x_samples={x_samples[p]}, less than one step of window={self.window}")
            if no_step[p]:
                raise ValueError(f"RecordingDataset: clip {p} starts at x_start={x_start[p]}: no whole step of {self.window} samples lies inside "
                                 f"recording {rec[p]} ({samples[p]} samples)")
            raise ValueError(f"RecordingDataset: clip {p} has y_start={y_start[p]} (>= 0)")
        dev = self.signals.device
        self.clip_table = torch.from_numpy(table).to(dev)
        self.y_is_target = self.y_steps > 0
        if self.y_is_target != (y is None):
            raise ValueError(f"RecordingDataset: y_steps={self.y_steps} and y={'None' if y is None else 'a label pool'} disagree: labels (P,) "
                             f"with y_steps=0 (detection, classification), y=None with y_steps > 0 (ssl: the target is cut from the recording)")
        if y is not None:
            if not torch.is_tensor(y) or y.device != dev or not y.is_contiguous() or tuple(y.shape) != (table.shape[0],) or \
                    y.dtype not in (torch.float32, torch.int64):
                got = f"{y.dtype} {tuple(y.shape)} on {y.device}" if torch.is_tensor(y) else type(y).__name__
                raise ValueError(f"RecordingDataset: y must be the contiguous labels ({table.shape[0]},) on {dev}, float32 (detection) or int64 "
                                 f"(classification), got {got}")
        self.y = y

    @classmethod
    def from_native_rate(cls, recordings, sample_freqs, clip_table, y=None, *, window: int, x_steps: int, y_steps: int = 0, to_freq=200, device=None):
        """the data set over recordings that still have their NATIVE sampling rates (sample_freqs[r] Hz): each is uploaded and resampled
        to `to_freq` Hz on the device, straight into the padded layout (`resample.resample_recordings`; the reference's offline
        resample_signals.py); the clip table counts samples at `to_freq`.  Sugar over the (signals, rec_table=, num_channels=) form."""
        from .resample import resample_recordings
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        recordings = list(recordings)
        signals, rec_table = resample_recordings(recordings, sample_freqs, to_freq=to_freq, device=device)      # (refuses an empty list)
        n = int((recordings[0] if torch.is_tensor(recordings[0]) else np.asarray(recordings[0])).shape[0])
        return cls(signals, clip_table, y, window=window, x_steps=x_steps, y_steps=y_steps, rec_table=rec_table, num_channels=n)

    @classmethod
    def from_edf(cls, paths, clip_table, y=None, *, window: int, x_steps: int, y_steps: int = 0, channels=None, to_freq=200, device=None):
        """the data set over EDF FILES (paths, bytes or uint8 arrays): each file's payload bytes are uploaded, the selected channels
        (default utils.INCLUDED_CHANNELS, the reference's order) decoded and resampled to `to_freq` Hz on the device, straight into
        the padded layout (`edf.load_edf_recordings`); the clip table counts samples at `to_freq`.  Sugar over the (signals,
        rec_table=, num_channels=) form."""
        from . import utils
        from .edf import load_edf_recordings
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        signals, rec_table, info = load_edf_recordings(paths, channels=channels, to_freq=to_freq, device=device)     # (refuses an empty list)
        n = len(utils.INCLUDED_CHANNELS) if channels is None else len(list(channels))
        return cls(signals, clip_table, y, window=window, x_steps=x_steps, y_steps=y_steps, rec_table=rec_table, num_channels=n)

    def __len__(self):
        return self.clip_table.shape[0]

    def clip_groups(self):
        """the recording of every clip (column 0 of the clip table) as (P,) int32 on the device: the by-recording clustering of
        `bootstrap_scores` / `DeviceEvaluator.bootstrap`"""
        return self.clip_table[:, 0].to(torch.int32).contiguous()

    @property
    def device(self):
        return self.signals.device

    @property
    def x_shape(self):
        return (self.N, self.x_steps * self.window)

    @property
    def y_shape(self):
        return (self.N, self.y_steps * self.window) if self.y_is_target else ()

    @property
    def y_dtype(self):
        return torch.float32 if self.y_is_target else self.y.dtype

    def check_step(self, step, who: str):
        """a batch of this data set is RAW signals in steps of `window`: the step must featurise / window them with the same window,
        and its task must match what the table cuts"""
        if step.raw_window is None:
            raise ValueError(f"{who}: a RecordingDataset yields raw signals (B, N, {self.x_steps}*{self.window}); the step has raw_window=None "
                             f"-- build it as TrainStep(raw_window={self.window}, ...)")
        if int(step.raw_window) != self.window:
            raise ValueError(f"{who}: TrainStep(raw_window={step.raw_window}) and RecordingDataset(window={self.window}) disagree: the lengths "
                             f"the gather writes count steps of {self.window} samples")
        if step.task == "ssl" and not self.y_is_target:
            raise ValueError(f"{who}: task='ssl' needs the target cut from the recordings: RecordingDataset(..., y=None, y_steps=Ty), got "
                             f"y_steps={self.y_steps}")
        if step.task != "ssl" and self.y_is_target:
            raise ValueError(f"{who}: task={step.task!r} needs labels: RecordingDataset(..., y=labels, y_steps=0), got y_steps={self.y_steps}")

    def gather(self, sampler, x_out, y_out, len_out=None):
        """the sampler's next batch, cut out of the recordings into the static batch tensors (`ops.gather_records`)"""
        wide = self.y_is_target
        ops.gather_records(self.signals, self.rec_table, self.clip_table, x_out, sampler.perm, sampler.cursor, sampler.rank, sampler.world,
                           window=self.window, y_out=y_out if wide else None, label_pool=None if wide else self.y,
                           label_out=None if wide else y_out, len_out=len_out, clip_w=sampler.clip_w, denom=sampler.denom,
                           n_valid=sampler.n_valid)

    def batches(self, *args, **kwargs):
        raise NotImplementedError("RecordingDataset.batches is not offered: there are no pre-cut pools to view.  Evaluate on the device with "
                                  "TrainStep.evaluator(dataset, batch_size) / TrainStep.ssl_evaluator(dataset, batch_size)")


# The three loaders' index arithmetic, on the host in numpy: one table row per clip.  freq: the resampled rate (constants.FREQUENCY).
def _table(rec_ids, x_start, x_samples, y_start):
    cols = np.broadcast_arrays(np.asarray(rec_ids, dtype=np.int64), np.asarray(x_start, dtype=np.int64),
                               np.asarray(x_samples, dtype=np.int64), np.asarray(y_start, dtype=np.int64))
    return np.ascontiguousarray(np.stack(cols, axis=1))


def clip_table_detection(rec_ids, clip_idx, clip_len_s, freq: int = 200):
    """data/dataloader_detection.py, computeSliceMatrix: physical_clip_len = int(FREQUENCY * clip_len), start_window = clip_idx *
    physical_clip_len, end_window = start_window + physical_clip_len -> (rec, start_window, physical_clip_len, 0)"""
    clip = int(freq * clip_len_s)
    return _table(rec_ids, np.asarray(clip_idx, dtype=np.int64) * clip, clip, 0)


def clip_table_ssl(rec_ids, clip_idx_x, clip_idx_y, input_len_s, freq: int = 200):
    """data/dataloader_ssl.py:52-58 for both halves, called with clip_len=self.input_len for x AND y (:303-310); the target is the
    first output_len steps of clip clip_idx_y (:341: `y_feature[:self.output_len]`) -> (rec, clip_idx_x * L, L, clip_idx_y * L) with
    L = int(FREQUENCY * input_len); the data set's y_steps cuts the target's length"""
    clip = int(freq * input_len_s)
    return _table(rec_ids, np.asarray(clip_idx_x, dtype=np.int64) * clip, clip, np.asarray(clip_idx_y, dtype=np.int64) * clip)


def clip_table_classification(rec_ids, seizure_times, seizure_idx, clip_len_s, freq: int = 200, offset_s: int = 2):
    """data/dataloader_classification.py:44-66.  seizure_times[k]: the (start_s, end_s) pairs of ALL seizures of clip k's recording in
    order (getSeizureTimes), seizure_idx[k] the one the clip shows:
        pre_seizure_end = int(FREQUENCY * seizure_times[idx - 1][1]) if idx > 0 else 0
        start_t = max(pre_seizure_end + 1, int(FREQUENCY * (seizure_times[idx][0] - offset)))
        end_t   = min(start_t + int(FREQUENCY * clip_len), int(FREQUENCY * seizure_times[idx][1]))
    -> (rec, start_t, end_t - start_t, 0).  The `while` loop of :68-81 (whole 1-s steps) and the zero padding to max_seq_len behind
    it are the gather's `keep` rule."""
    rows = []
    for times, idx in zip(seizure_times, seizure_idx):
        idx = int(idx)
        pre_seizure_end = int(freq * times[idx - 1][1]) if idx > 0 else 0
        start_t = max(pre_seizure_end + 1, int(freq * (times[idx][0] - offset_s)))
        end_t = min(start_t + int(freq * clip_len_s), int(freq * times[idx][1]))
        rows.append((start_t, end_t - start_t))
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 2)
    return _table(rec_ids, rows[:, 0], rows[:, 1], 0)


# Whole recordings (scan.py): the strided windows of every recording as one table, their clip labels, annotations as bin intervals.
def clip_table_scan(rec_samples, x_steps: int, stride_steps: int, window: int, cover_tail: bool = True):
    """The sliding windows of whole recordings as one clip table.  Recording r has S_r = rec_samples[r] // window whole steps (a step
    is one bin of `window` samples); with T = x_steps and s = stride_steps (1 <= s <= T) it gets no clip if S_r < T, else the
    K_r = (S_r - T) // s + 1 clips starting at the steps 0, s, 2s, .. and -- cover_tail, (S_r - T) % s != 0 -- one more starting at
    S_r - T, so that every whole step is covered.  -> (table (P, 4) int64 of rows (r, start_step*window, T*window, 0), ordered by
    recording, then start; clip_off (R + 1,) int64: the rows clip_off[r] .. clip_off[r+1] are recording r's)."""
    t, s, w = int(x_steps), int(stride_steps), int(window)
    if t < 1 or w < 1:
        raise ValueError(f"clip_table_scan: x_steps={x_steps}, window={window} (both >= 1)")
    if not 1 <= s <= t:
        raise ValueError(f"clip_table_scan: stride_steps={stride_steps} outside 1..x_steps={t} (a larger stride leaves steps uncovered)")
    samples = [int(v) for v in np.asarray(rec_samples).reshape(-1)]
    if not samples or min(samples) < 0:
        raise ValueError(f"clip_table_scan: rec_samples must name at least one recording, each >= 0 samples, got {samples[:8]}")
    rows, off = [], [0]
    for r, n in enumerate(samples):
        steps = n // w
        if steps >= t:
            starts = list(range(0, steps - t + 1, s))
            if cover_tail and (steps - t) % s != 0:
                starts.append(steps - t)
            rows += [(r, a * w, t * w, 0) for a in starts]
        off.append(len(rows))
    return np.asarray(rows, dtype=np.int64).reshape(-1, 4), np.asarray(off, dtype=np.int64)


def clip_labels_detection(table, seizure_times, freq: int = 200):
    """The reference's clip label (data/dataloader_detection.py, computeSliceMatrix) for every row of a clip table: with
    start_window = x_start and end_window = x_start + x_samples, 1 where `not (end_window < int(t0*freq) or start_window >
    int(t1*freq))` holds for some annotated (t0, t1) of the clip's recording (both boundary cases count as seizure), else 0.
    seizure_times[r]: the (start_s, end_s) pairs of recording r.  -> (P,) float32"""
    table = np.asarray(table.cpu() if torch.is_tensor(table) else table)
    if table.ndim != 2 or table.shape[1] != 4:
        raise ValueError(f"clip_labels_detection: table must be (P, 4) = (rec, x_start, x_samples, y_start), got {table.shape}")
    labels = np.zeros(table.shape[0], dtype=np.float32)
    for p, (rec, start_window, x_samples, _) in enumerate(table.tolist()):
        if not 0 <= rec < len(seizure_times):
            raise ValueError(f"clip_labels_detection: clip {p} names recording rec={rec}, seizure_times has {len(seizure_times)}")
        end_window = start_window + x_samples
        for t in seizure_times[rec]:
            start_t, end_t = int(t[0] * freq), int(t[1] * freq)
            if not ((end_window < start_t) or (start_window > end_t)):
                labels[p] = 1.0
                break
    return labels


def annotation_bins(seizure_times, rec_samples, window: int, freq: int = 200):
    """Annotated (start_s, end_s) pairs per recording as half-open BIN intervals [floor(t0*freq/window), ceil(t1*freq/window)), clipped
    to the recording's S_r = rec_samples[r] // window whole steps, empty ones dropped, overlapping or touching ones merged, sorted.
    -> (ref (R, A_max, 2) int32, zero rows behind a recording's intervals, A_max >= 1; ref_count (R,) int32): what `ops.event_scores`
    reads."""
    samples = [int(v) for v in np.asarray(rec_samples).reshape(-1)]
    if len(seizure_times) != len(samples) or not samples:
        raise ValueError(f"annotation_bins: seizure_times names {len(seizure_times)} recordings, rec_samples {len(samples)}")
    w = int(window)
    if w < 1 or freq <= 0:
        raise ValueError(f"annotation_bins: window={window}, freq={freq} (both positive)")
    per_rec = []
    for times, n in zip(seizure_times, samples):
        steps = n // w
        ivs = []
        for t0, t1 in times:
            a = min(max(int(np.floor(t0 * freq / w)), 0), steps)
            b = min(max(int(np.ceil(t1 * freq / w)), 0), steps)
            if b > a:
                ivs.append((a, b))
        merged = []
        for a, b in sorted(ivs):
            if merged and a <= merged[-1][1]:
                merged[-1] = (merged[-1][0], max(merged[-1][1], b))
            else:
                merged.append((a, b))
        per_rec.append(merged)
    ref = np.zeros((len(samples), max(1, max(len(m) for m in per_rec)), 2), dtype=np.int32)
    for r, m in enumerate(per_rec):
        if m:
            ref[r, :len(m)] = np.asarray(m, dtype=np.int32)
    return ref, np.asarray([len(m) for m in per_rec], dtype=np.int32)


class EpochSampler:
    """The epoch's shuffle and the position in it, on the device: `perm` (P,) int64, `cursor` (1,) int64, `epoch`.

    `begin_epoch(e)` draws P Philox keys from (seed, e) (`ops.epoch_keys`), sorts them -- stable, once per epoch -- INTO `perm` and
    zeroes the cursor; both tensors keep their addresses, so a captured graph sees the new epoch.  Every rank of a data-parallel
    run passes the same seed: one shared permutation, rank r takes positions cursor + r*batch_size .. + batch_size of every step
    (disjoint shards).  steps_per_epoch = P // (batch_size * world); the tail is dropped (module docstring).

    drop_last=False keeps the tail: steps_per_epoch = ceil(P / (batch_size * world)), and the sampler owns `clip_w` (batch_size,)
    float32, `denom` (1,) float32 and `n_valid` (1,) int64 at fixed addresses, which every gather of a step rewrites and the
    criterion reads (module docstring).  A constructor property: `state_dict` does not carry it.  Such a sampler keeps a HOST mirror
    of the cursor (`take`), so that the step counts its clips without reading the device: `begin_epoch` and `load_state_dict` set
    it; a caller that writes `cursor` itself says so with `seek`.  A step issued past the end of the epoch (cursor >= P) is the
    caller's error; it stays finite -- every weight 0: loss 0, zero gradients -- and no kernel raises."""

    def __init__(self, P: int, batch_size: int, seed: int, rank: Optional[int] = None, world: Optional[int] = None, device=None,
                 drop_last: bool = True):
        self._shard(rank, world, batch_size, seed)
        self.P = int(P)
        if self.batch_size < 1 or self.batch_size * self.world > self.P:
            raise ValueError(f"EpochSampler: batch_size*world = {self.batch_size}*{self.world} clips per step, the pool holds P={self.P} "
                             f"(1 <= batch_size*world <= P)")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self._allocate(self.P, device, drop_last)

    def _shard(self, rank, world, batch_size, seed):
        """this rank's place in the step, the batch size and the seed (refusals by the name of the class)"""
        who = type(self).__name__
        has_pg = dist.is_available() and dist.is_initialized()
        self.rank = int(rank) if rank is not None else (dist.get_rank() if has_pg else 0)
        self.world = int(world) if world is not None else (dist.get_world_size() if has_pg else 1)
        self.batch_size, self.seed = int(batch_size), int(seed)
        if self.world < 1 or not 0 <= self.rank < self.world:
            raise ValueError(f"{who}: rank={self.rank} of world={self.world}")
        if not 0 <= self.seed < 2 ** 63:
            raise ValueError(f"{who}: seed={seed} outside 0..2^63-1")

    def _allocate(self, epoch_len: int, device, drop_last: bool):
        """the device state of an epoch of `epoch_len` clips out of the pool's P (EpochSampler: all P; BalancedEpochSampler: its quotas):
        perm (epoch_len,), cursor, the key buffers over the pool and, for drop_last=False, the tail buffers -- fixed addresses"""
        self.epoch_len = int(epoch_len)
        self.drop_last = bool(drop_last)
        per_step = self.batch_size * self.world
        self.steps_per_epoch = self.epoch_len // per_step if self.drop_last else -(-self.epoch_len // per_step)
        self.perm = torch.arange(self.epoch_len, dtype=torch.int64, device=device)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=device)
        self._keys = torch.empty(self.P, dtype=torch.int64, device=device)
        self._sorted = torch.empty(self.P, dtype=torch.int64, device=device)
        self.epoch = None                 # no epoch begun: perm is the identity
        self.clip_w = self.denom = self.n_valid = None
        self._host_cursor = 0             # drop_last=False: the host's copy of `cursor`
        if not self.drop_last:            # a full batch until the first gather says otherwise
            self.clip_w = torch.ones(self.batch_size, dtype=torch.float32, device=device)
            self.denom = torch.full((1,), float(self.batch_size), dtype=torch.float32, device=device)
            self.n_valid = torch.full((1,), per_step, dtype=torch.int64, device=device)

    @property
    def device(self):
        return self.perm.device

    def begin_epoch(self, epoch: int):
        """outside any captured graph (the sort is the framework's and allocates)"""
        ops.epoch_keys(self._keys, self.seed, int(epoch))
        torch.sort(self._keys, stable=True, out=(self._sorted, self.perm))
        self.cursor.zero_()
        self._host_cursor = 0
        self.epoch = int(epoch)
        return self

    def seek(self, cursor: int):
        """put the cursor at `cursor` -- the device tensor and the host mirror of a drop_last=False sampler alike (outside any
        captured graph).  Writing `sampler.cursor` directly leaves that mirror behind: the step then counts the wrong clips."""
        self.cursor.fill_(int(cursor))
        self._host_cursor = int(cursor)
        return self

    def take(self) -> int:
        """the global number of clips that count in the step about to be issued; moves the host mirror of the cursor on by one
        step.  No device read: batch_size * world for the default sampler, clamp(epoch_len - cursor, 0, batch_size * world) from the mirror
        for drop_last=False."""
        per_step = self.batch_size * self.world
        if self.drop_last:
            return per_step
        n = min(max(self.epoch_len - self._host_cursor, 0), per_step)
        self._host_cursor += per_step
        return n

    def state_dict(self):
        return {"seed": self.seed, "epoch": self.epoch, "cursor": int(self.cursor.item())}

    def load_state_dict(self, state):
        """the permutation is a function of (seed, epoch): it is drawn again, and the cursor returns to where the run stopped"""
        self.seed = int(state["seed"])
        if state["epoch"] is None:
            self.perm.copy_(torch.arange(self.epoch_len, dtype=torch.int64, device=self.device))
            self.epoch = None
        else:
            self.begin_epoch(int(state["epoch"]))
        self.seek(int(state["cursor"]))


class BalancedEpochSampler(EpochSampler):
    """Balanced under-sampling per epoch, on the device: the reference's detection loader keeps int(scale_ratio * n_seizure) seizure clips
    and draws as many non-seizure clips at random, ONCE, when the loader is built (data/dataloader_detection.py:88-127,
    `parseTxtFiles`).  Here the pool stays whole in HBM and every epoch is a draw of `quotas[c]` clips of each class c.

    labels: the dataset's label pool on the device -- float32 0 / 1 (detection; class = label >= 0.5) or int64 classes 0..C-1.  The
    class counts n_c are read ONCE, here (the sampler's only synchronisation).  Default quotas: q_c = min(n_c, int(scale_ratio *
    n_rarest)), the reference's arithmetic with the rarest class present in the role of "seizure"; quotas=[q_0, ..] overrides them
    (one per class; q_c > n_c is refused).  `epoch_len` = sum_c q_c is the length of `perm` -- fixed size, fixed address -- and what
    steps_per_epoch and `take` count; `P` stays the pool size (what `TrainStep` checks against the dataset).

    begin_epoch(e), e < 2^30, outside any graph, no host read: selection keys k1 = epoch_keys(seed, 2 * e') with e' = e if redraw
    else 0, order keys k2 = epoch_keys(seed, 2 * e + 1); within each class the q_c clips with the smallest (k1_i, i) are selected, and
    perm is the selected clips sorted by (k2_i, i).  redraw=False is the reference -- one draw of the negatives per run, reshuffled
    every epoch; redraw=True (the default) is the point of keeping every recording resident: fresh negatives every epoch.  The sorts
    are the framework's, all sizes host integers.  Everything else -- shards, drop_last=False tail buffers, seek, state_dict -- is
    EpochSampler's; `redraw`, the quotas and drop_last are constructor properties, not state."""

    def __init__(self, labels: torch.Tensor, batch_size: int, seed: int, scale_ratio: float = 1.0, quotas=None, redraw: bool = True,
                 drop_last: bool = True, rank: Optional[int] = None, world: Optional[int] = None):
        who = "BalancedEpochSampler"
        if not torch.is_tensor(labels) or labels.dim() != 1 or labels.numel() < 1 or labels.dtype not in (torch.float32, torch.int64):
            got = f"{labels.dtype} {tuple(labels.shape)}" if torch.is_tensor(labels) else type(labels).__name__
            raise ValueError(f"{who}: labels must be the label pool (P,), float32 0 / 1 (detection) or int64 classes, got {got}")
        self._shard(rank, world, batch_size, seed)
        self.P, self.redraw = int(labels.numel()), bool(redraw)
        classes = (labels >= 0.5).to(torch.int64) if labels.dtype == torch.float32 else labels
        lo, hi = int(classes.min().item()), int(classes.max().item())          # the one synchronisation (with the counts below)
        if lo < 0:
            raise ValueError(f"{who}: labels hold the class {lo}; classes are 0..C-1")
        num_classes = 2 if labels.dtype == torch.float32 else hi + 1
        self.class_counts = torch.bincount(classes, minlength=num_classes).tolist()
        present = [n for n in self.class_counts if n > 0]
        if quotas is None:
            if not float(scale_ratio) > 0:
                raise ValueError(f"{who}: scale_ratio={scale_ratio} (> 0)")
            keep = int(float(scale_ratio) * min(present))
            quotas = [min(n, keep) for n in self.class_counts]
        quotas = [int(q) for q in quotas]
        if len(quotas) != num_classes:
            raise ValueError(f"{who}: {len(quotas)} quotas for the {num_classes} classes of the labels")
        for c, (q, n) in enumerate(zip(quotas, self.class_counts)):
            if q < 0 or q > n:
                raise ValueError(f"{who}: quota {q} for class {c}, which has {n} clips (0 <= quota <= count: no over-sampling)")
        self.quotas = quotas
        if self.batch_size < 1 or self.batch_size * self.world > sum(quotas):
            raise ValueError(f"{who}: batch_size*world = {self.batch_size}*{self.world} clips per step, a balanced epoch holds "
                             f"{sum(quotas)} (quotas {quotas} of class counts {self.class_counts})")
        self._allocate(sum(quotas), labels.device, drop_last)
        self._keys2 = torch.empty(self.P, dtype=torch.int64, device=labels.device)
        # the members of each class in pool order (ascending i: a stable sort of their keys breaks ties by i)
        self._members = [torch.nonzero(classes == c).view(-1) if q > 0 else None for c, q in enumerate(quotas)]

    def begin_epoch(self, epoch: int):
        """outside any captured graph (the sorts are the framework's and allocate); no host read"""
        epoch = int(epoch)
        if not 0 <= epoch < 2 ** 30:
            raise ValueError(f"BalancedEpochSampler: epoch={epoch} outside 0..2^30-1 (two key streams per epoch)")
        ops.epoch_keys(self._keys, self.seed, 2 * epoch if self.redraw else 0)
        ops.epoch_keys(self._keys2, self.seed, 2 * epoch + 1)
        chosen = []
        for members, q in zip(self._members, self.quotas):
            if q > 0:
                order = torch.sort(self._keys[members], stable=True).indices
                chosen.append(members[order[:q]])
        chosen = torch.sort(torch.cat(chosen)).values                           # ascending i: ties of k2 break by i below
        order = torch.sort(self._keys2[chosen], stable=True).indices
        torch.index_select(chosen, 0, order, out=self.perm)
        self.cursor.zero_()
        self._host_cursor = 0
        self.epoch = epoch
        return self
