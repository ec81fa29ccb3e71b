"""The fit of the input scaler on the device: the scalar mean and std of the un-standardised model inputs over the training clips.

`TrainStep(raw_window=..., raw_mean=m, raw_std=s)`, `feature_mean` / `feature_std` and the `scaler_mean` / `scaler_std` of the SSL
loss are the reference's `StandardScaler` (utils.py:393-428).  The reference reads its two numbers from files made offline for
one corpus, two clip lengths and the FFT domain only; another corpus, clip length, window or the time-domain mode has no number.
`fit_scaler` computes them where the clips already are: one pass over a device-resident data set in pool order, per step the
data set's gather and `ops.feature_moments` (the transform of `fft_features` without its feature writes, reduced per clip in
float64), then `ops.moments_record` and ONE device-to-host copy of seven words.  Nothing in the pass is a floating-point atomic and
a clip's words do not depend on where it sits, so every batch size, rank count and data-set kind gives the same bits."""
from __future__ import annotations

from collections import OrderedDict
from typing import Optional

import torch
import torch.distributed as dist

from . import ops, utils
from .device_data import EpochSampler, RecordingDataset


class ScalerFit:
    """What `fit_scaler` returns: `mean`, `std` (Python floats: the population std, np.std), `count` (values), `clips` (clips with at
    least one value), `bad` (always 0: a pool with NaN or infinite values is refused); `result`: the record's words by name
    (ops.MOMENTS_RECORD), `record` the float64 words on the host; `clip_sum`, `clip_sumsq`, `clip_count`: (P,) float64 on the device
    in pool order -- a flat or saturated clip shows there; `scaler()`: `utils.StandardScaler(mean, std)`."""

    def __init__(self, record, scores):
        self.record = record
        self.result = OrderedDict(zip(ops.MOMENTS_RECORD, (float(v) for v in record)))
        self.mean, self.std = self.result["mean"], self.result["std"]
        self.count, self.clips, self.bad = int(self.result["count"]), int(self.result["clips"]), int(self.result["bad"])
        self.scores = scores
        self.clip_sum, self.clip_sumsq, self.clip_count = scores[0], scores[1], scores[2]

    def scaler(self):
        return utils.StandardScaler(self.mean, self.std)

    def __repr__(self):
        return f"ScalerFit(mean={self.mean!r}, std={self.std!r}, count={self.count}, clips={self.clips})"


def fit_scaler(dataset, batch_size: int = 256, *, window: Optional[int] = None, use_fft: bool = True, rank: Optional[int] = None,
               world: Optional[int] = None) -> ScalerFit:
    """Mean and std of the un-standardised model inputs of `dataset`, computed on the device.

    dataset: a `RecordingDataset` (its own window; clips are cut by its gather, and only their valid steps count), a raw
    `DeviceDataset` pool (P, N, T*window) -- `window` is required --, or a pool of ready features / windows (P, T, N, D), always
    taken as given.  use_fft (raw signals only): True: the log|FFT| features of `fft_features`; False: the samples themselves, the
    reference's time-domain inputs.  A length pool is honoured; of an SSL data set only the input half counts.  batch_size: clips
    per step and rank (clamped to the pool; the result does not depend on it).  rank / world: as `EpochSampler` (default: the
    process group's): every rank takes its slots of every step, the per-clip words go through ONE summed all-reduce (disjoint slots)
    and every rank returns the same `ScalerFit`.  Raises ValueError for a pool with NaN or infinite values (with their count), with
    no values, or with std == 0."""
    who = "fit_scaler"
    if not hasattr(dataset, "gather") or not hasattr(dataset, "x_shape"):
        raise ValueError(f"{who}: dataset must be a RecordingDataset or a DeviceDataset, got {type(dataset).__name__}")
    p, dev, xs = len(dataset), dataset.device, tuple(dataset.x_shape)
    if p > ops.EVAL_MAX_CLIPS:
        raise ValueError(f"{who}: the pool holds P={p} clips, one pass takes at most {ops.EVAL_MAX_CLIPS} (ops.EVAL_MAX_CLIPS); fit it in parts")
    if isinstance(dataset, RecordingDataset):
        if window is not None and int(window) != dataset.window:
            raise ValueError(f"{who}: window={window} and RecordingDataset(window={dataset.window}) disagree")
        window = dataset.window
    elif len(xs) == 2:
        if window is None:
            raise ValueError(f"{who}: x {(p,) + xs} holds raw signals (P, N, T*window): pass window=")
        window = int(window)
        if window < 4 or window % 4 != 0 or xs[1] % window != 0:
            raise ValueError(f"{who}: window={window} must be a positive multiple of 4 that divides the {xs[1]} samples of a channel row")
    elif len(xs) == 3:
        window = None                                                # features / windows: the values as given
    else:
        raise ValueError(f"{who}: x {(p,) + xs} is neither raw signals (P, N, T*window) nor features / windows (P, T, N, D)")
    if window is not None and use_fft and window // 4 + 1 > 64:
        raise ValueError(f"{who}: window={window} unsupported with use_fft=True (a multiple of 4, at most 252)")
    has_pg = dist.is_available() and dist.is_initialized()
    n_ranks = int(world) if world is not None else (dist.get_world_size() if has_pg else 1)
    if int(batch_size) < 1:
        raise ValueError(f"{who}: batch_size={batch_size}")
    b = max(1, min(int(batch_size), p // max(n_ranks, 1)))
    # the pass's own sampler: never begun (perm = identity), the short last batch kept
    sampler = EpochSampler(p, b, seed=0, rank=rank, world=world, device=dev, drop_last=False)
    if sampler.world > 1 and not (has_pg and dist.get_world_size() == sampler.world):
        raise RuntimeError(f"{who}: world={sampler.world} needs a process group of that size for the all-reduce of the scores")
    scores, record = ops.moments_buffers(p, dev)
    x = torch.empty((b,) + xs, dtype=torch.float32, device=dev)
    y = torch.empty((b,) + tuple(dataset.y_shape), dtype=dataset.y_dtype, device=dev)
    lens = torch.empty(b, dtype=torch.int64, device=dev) if dataset.has_lengths else None
    with torch.no_grad():
        for _ in range(sampler.steps_per_epoch):
            dataset.gather(sampler, x, y, lens)
            ops.feature_moments(x, scores, sampler.clip_w, sampler.cursor, sampler.rank, sampler.world, window=window, use_fft=use_fft,
                                lengths=lens)
        if sampler.world > 1:
            dist.all_reduce(scores, op=dist.ReduceOp.SUM)
        ops.moments_record(scores, record)
        fit = ScalerFit(record.cpu(), scores)                        # the pass's one device-to-host copy
    if fit.bad:
        raise ValueError(f"{who}: {fit.bad} values of the pool are NaN or infinite, beside {fit.count} finite values of {fit.clips} clips")
    if fit.count == 0:
        raise ValueError(f"{who}: the pool of {p} clips holds no values")
    if fit.std == 0.0:
        raise ValueError(f"{who}: std == 0: all {fit.count} values of the pool equal {fit.mean!r}; a scaler cannot divide by it")
    return fit
