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
and the step runs the unweighted kernels."""
from __future__ import annotations

from typing import Optional

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
        has_pg = dist.is_available() and dist.is_initialized()
        self.rank = int(rank) if rank is not None else (dist.get_rank() if has_pg else 0)
        self.world = int(world) if world is not None else (dist.get_world_size() if has_pg else 1)
        self.P, self.batch_size, self.seed = int(P), int(batch_size), int(seed)
        if self.world < 1 or not 0 <= self.rank < self.world:
            raise ValueError(f"EpochSampler: rank={self.rank} of world={self.world}")
        if self.batch_size < 1 or self.batch_size * self.world > self.P:
            raise ValueError(f"EpochSampler: batch_size*world = {self.batch_size}*{self.world} clips per step, the pool holds P={self.P} "
                             f"(1 <= batch_size*world <= P)")
        if not 0 <= self.seed < 2 ** 63:
            raise ValueError(f"EpochSampler: seed={seed} outside 0..2^63-1")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.drop_last = bool(drop_last)
        per_step = self.batch_size * self.world
        self.steps_per_epoch = self.P // per_step if self.drop_last else -(-self.P // per_step)
        self.perm = torch.arange(self.P, dtype=torch.int64, device=device)
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
        step.  No device read: batch_size * world for the default sampler, clamp(P - cursor, 0, batch_size * world) from the mirror
        for drop_last=False."""
        per_step = self.batch_size * self.world
        if self.drop_last:
            return per_step
        n = min(max(self.P - self._host_cursor, 0), per_step)
        self._host_cursor += per_step
        return n

    def state_dict(self):
        return {"seed": self.seed, "epoch": self.epoch, "cursor": int(self.cursor.item())}

    def load_state_dict(self, state):
        """the permutation is a function of (seed, epoch): it is drawn again, and the cursor returns to where the run stopped"""
        self.seed = int(state["seed"])
        if state["epoch"] is None:
            self.perm.copy_(torch.arange(self.P, dtype=torch.int64, device=self.device))
            self.epoch = None
        else:
            self.begin_epoch(int(state["epoch"]))
        self.seek(int(state["cursor"]))
