"""Native-rate recordings to the model's rate on the device: the reference's offline step `data/resample_signals.py:38-43` ->
`data/data_utils.py:158-170` (`resampleData` = `scipy.signal.resample` over the WHOLE recording, float64), as
`torch.ops.eeg_dcrnn.resample` (csrc/kernels_resample.h) writing float32 straight into the padded layout a `RecordingDataset` reads.

The number of output samples follows the reference's rule, `num = to_freq * int(L / sample_freq)`: it truncates, `sample_freq` may be a
float, and a recording whose length is not a whole number of seconds is squeezed as a whole (`resampled_length`).  A recording whose
`sample_freq == to_freq` is not resampled at all: it is copied as given (resample_signals.py:38).

What is uploaded here is the decoded native-rate (channels, L) array; EDF files themselves go through edf.py, which uploads their
payload bytes and decodes them on the device in front of this pass (`load_edf_recordings`, `RecordingDataset.from_edf`)."""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import ops

MAX_SAMPLES = ops.RESAMPLE_MAX_SAMPLES


def _check_freqs(what, sample_freq, to_freq):
    for name, f in (("sample_freq", sample_freq), ("to_freq", to_freq)):
        if isinstance(f, bool) or not isinstance(f, (int, float, np.integer, np.floating)) or not math.isfinite(float(f)) or float(f) <= 0:
            raise ValueError(f"{what}: {name}={f!r} must be a finite positive number")
    if int(to_freq) != to_freq:
        raise ValueError(f"{what}: to_freq={to_freq!r} must be a whole number of samples per second")


def resampled_length(samples: int, sample_freq, to_freq=200) -> int:
    """samples of a recording of `samples` samples at `sample_freq` Hz once resampled: to_freq * int(samples / sample_freq), the
    reference's rule (resample_signals.py:40-41 -> data_utils.py:167-168)"""
    _check_freqs("resampled_length", sample_freq, to_freq)
    if int(samples) != samples or samples < 0:
        raise ValueError(f"resampled_length: samples={samples!r} must be a non-negative integer")
    return int(to_freq) * int(int(samples) / sample_freq)


def _as_recording(what, x):
    """the 2-D float32 / float64 (channels, samples) tensor behind x (array or tensor, host or device), without a copy"""
    if not torch.is_tensor(x):
        a = np.asarray(x)
        if a.dtype not in (np.float32, np.float64):
            raise ValueError(f"{what}: dtype {a.dtype}; a recording is float32 or float64")
        if a.ndim != 2:
            raise ValueError(f"{what}: shape {a.shape}; a recording is 2-D (channels, samples)")
        x = torch.from_numpy(np.ascontiguousarray(a))
    if x.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what}: dtype {x.dtype}; a recording is float32 or float64")
    if x.dim() != 2 or x.shape[0] < 1:
        raise ValueError(f"{what}: shape {tuple(x.shape)}; a recording is 2-D (channels >= 1, samples)")
    if x.requires_grad:
        raise ValueError(f"{what}: the recording requires grad; resampling has no gradient formula (detach it)")
    return x


def _target_length(what, samples, sample_freq, to_freq, n_out=None):
    """output samples of one recording (None: copied as given), every refusal raised here"""
    _check_freqs(what, sample_freq, to_freq)
    if n_out is None and float(sample_freq) == float(to_freq):
        if samples < 1:
            raise ValueError(f"{what}: an empty recording")
        return None
    num = resampled_length(samples, sample_freq, to_freq) if n_out is None else int(n_out)
    if num < 1:
        raise ValueError(f"{what}: {samples} samples at {sample_freq} Hz are shorter than one second: nothing to resample to "
                         f"(num = to_freq * int(samples / sample_freq) = {num})" if n_out is None else f"{what}: n_out={n_out} (>= 1)")
    if not 2 <= samples <= MAX_SAMPLES:
        raise ValueError(f"{what}: {samples} samples per channel; 2..{MAX_SAMPLES} (EEG_RESAMPLE_MAX_SAMPLES = 2^22) are supported")
    if num > MAX_SAMPLES:
        raise ValueError(f"{what}: {num} output samples per channel; at most {MAX_SAMPLES} (EEG_RESAMPLE_MAX_SAMPLES = 2^22) are supported")
    return num


def _device(device):
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def resample_recording(x, sample_freq, to_freq=200, n_out: Optional[int] = None, workspace_bytes: Optional[int] = None) -> torch.Tensor:
    """x (N, L) float32 / float64 ON THE DEVICE at `sample_freq` Hz -> (N, num) float32 at `to_freq` Hz, num by `resampled_length`
    unless `n_out` names it (for instance round(L * to_freq / sample_freq)).  sample_freq == to_freq (and no n_out): x as float32."""
    what = "resample_recording"
    x = _as_recording(what, x)
    num = _target_length(what, int(x.shape[1]), sample_freq, to_freq, n_out)
    if num is None:
        return x.to(torch.float32, copy=True)
    return torch.ops.eeg_dcrnn.resample(x, num, workspace_bytes)


def resample_recordings(recordings, sample_freqs, to_freq=200, device=None, workspace_bytes: Optional[int] = None):
    """recordings [(N, L_r) float32 / float64 arrays or tensors, host or device] at sample_freqs[r] Hz -> (signals, rec_table) exactly as
    `layout_recordings` lays out the resampled set: one flat float32 buffer, recording r channel-major at rec_table[r] = (offset, stride,
    samples) with offset and stride padded to multiples of 4 floats and the padding zero.  Each recording is uploaded on its own through
    ONE staging buffer sized for the longest and resampled straight into its place: no host copy of the set, no second device copy."""
    what = "resample_recordings"
    recordings = list(recordings)
    sample_freqs = list(sample_freqs) if not isinstance(sample_freqs, (int, float)) else [sample_freqs] * len(recordings)
    if len(recordings) < 1:
        raise ValueError(f"{what}: no recordings")
    if len(sample_freqs) != len(recordings):
        raise ValueError(f"{what}: {len(sample_freqs)} sample_freqs for {len(recordings)} recordings")
    recs, nums = [], []
    for r, (rec, fs) in enumerate(zip(recordings, sample_freqs)):
        t = _as_recording(f"{what}: recording {r}", rec)
        if recs and t.shape[0] != recs[0].shape[0]:
            raise ValueError(f"{what}: recording {r} has {t.shape[0]} channels, recording 0 has {recs[0].shape[0]}")
        nums.append(_target_length(f"{what}: recording {r}", int(t.shape[1]), fs, to_freq))
        recs.append(t)
    dev = _device(device)
    n = int(recs[0].shape[0])
    table, offset = [], 0
    for t, num in zip(recs, nums):
        samples = int(t.shape[1]) if num is None else num
        stride = -(-samples // 4) * 4
        table.append((offset, stride, samples))
        offset += n * stride
    signals = torch.zeros(offset, dtype=torch.float32, device=dev)
    staging = {}                                                         # dtype -> the one staging buffer of host recordings of that dtype
    for t, num, (off, stride, samples) in zip(recs, nums, table):
        place = signals[off:off + n * stride].view(n, stride)[:, :samples]
        if num is None:
            place.copy_(t)                                               # already at to_freq: copied as given
            continue
        if t.device != dev:
            if t.dtype not in staging:
                longest = max(int(u.shape[1]) for u, k in zip(recs, nums) if k is not None and u.device != dev and u.dtype == t.dtype)
                staging[t.dtype] = torch.empty(n * longest, dtype=t.dtype, device=dev)
            up = staging[t.dtype][:n * t.shape[1]].view(n, t.shape[1])
            up.copy_(t)
            t = up
        elif t.stride(1) != 1 or (n > 1 and t.stride(0) < t.shape[1]):
            t = t.contiguous()
        ops.resample_into(t, place, workspace_bytes, what=what)
    return signals, torch.tensor(table, dtype=torch.int64, device=dev)
