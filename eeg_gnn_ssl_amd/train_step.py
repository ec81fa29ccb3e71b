"""The reference's supervised/SSL optimisation step (train.py:222-224,253-275; train_ssl.py:147-178)
re-hosted for one-process-per-GPU data parallelism over RCCL.

Recipe per step:  zero_grad -> forward -> loss -> backward -> [all-reduce of ONE flat fp32
gradient bucket, mean over ranks] -> clip_grad_norm_(5.0) -> Adam(lr, weight_decay = coupled L2).

MI355X notes: the whole model is <= 2.8 MB, so parameters and gradients live in two flat
buffers (every `p` / `p.grad` is a view): the exchange is a single latency-bound all-reduce over
xGMI, the norm is one reduction, Adam runs over one tensor, and nothing in the step synchronises
with the host (the reference calls `loss.item()` and `lengths.cpu()` every step)."""
from __future__ import annotations

from typing import Optional, Sequence

import torch
import torch.distributed as dist

from . import ops


class FlatParameters:
    """Re-home a module's parameters (and their .grad) into two contiguous fp32 buffers.
    Shared parameters (the decoder's shared cell, model.py:126-143) appear once."""

    def __init__(self, module: torch.nn.Module):
        params, seen = [], set()
        for p in module.parameters():
            if id(p) not in seen:
                seen.add(id(p))
                params.append(p)
        self.params = params
        total = sum(p.numel() for p in params)
        dev, dt = params[0].device, params[0].dtype
        self.flat = torch.empty(total, device=dev, dtype=dt)
        self.flat_grad = torch.zeros(total, device=dev, dtype=dt)
        off = 0
        with torch.no_grad():
            for p in params:
                n = p.numel()
                self.flat[off:off + n].copy_(p.reshape(-1))
                p.data = self.flat[off:off + n].view(p.shape)
                p.grad = self.flat_grad[off:off + n].view(p.shape)
                off += n
        self.flat_param = torch.nn.Parameter(self.flat, requires_grad=True)
        self.flat_param.grad = self.flat_grad
        # the backward operators write these parameters' gradients straight into the bucket while `with self.sink:` is open
        self.sink = ops.GradSink(params)

    def zero_grad(self):
        ops.zero_(self.flat_grad)          # one memset node on the stream (no framework fill kernel in the captured step)


class TrainStep:
    """One optimisation step of the reference recipe on the local shard of the global batch."""

    def __init__(self, model: torch.nn.Module, task: str = "detection", lr: float = 3e-4,
                 weight_decay: float = 5e-4, max_grad_norm: float = 5.0,
                 scaler_mean: Optional[float] = None, scaler_std: Optional[float] = None,
                 always_reduce: bool = False, raw_window: Optional[int] = None, raw_mean: float = 0.0, raw_std: float = 1.0,
                 shared_graph: bool = True, data_augment: bool = False, swap_perm=None, reflected_supports=None,
                 feature_std: Optional[float] = None, use_fft: bool = True, feature_mean: Optional[float] = None,
                 padding_val: Optional[float] = None, class_weights=None, weight_norm: Optional[str] = None, sample_weights=None):
        """class_weights / sample_weights / weight_norm: the criterion of the supervised tasks with a weight per clip (class
        imbalance; `_step_weights`).  class_weights: one weight >= 0 per class, a sequence or a float32 tensor on the model's device
        -- (C,) for classification, `nn.CrossEntropyLoss(weight=)`; (2,) for detection, whose float labels are taken to be 0 or 1
        (class = label >= 0.5): (1, p) is `nn.BCEWithLogitsLoss(pos_weight=p)`.  sample_weights: a float32 (P,) pool on the model's
        device, one weight >= 0 per clip of the data set of `step_from` / `capture_epoch` (not for `step` / `capture`, which see no
        pool).  weight_norm: "sum" divides by the sum of the step's weights (the default for classification), "count" by the number
        of its clips (the default for detection); it has no effect without weights.  Every step then writes the clips' weights and
        the divisor on the device (`ops.clip_weights`, one launch, capturable) and runs the multiplicative criteria.  From a
        sampler the weights cover the step's clips on ALL ranks: the validity of a drop_last=False epoch's short last batch is part
        of them and the divisor is global (on a drop_last=True sampler a step issued past the end of the epoch has weight 0
        throughout).  `step` / `capture` weigh the rank's own batch: data-parallel, the mean of the ranks' weighted means.
        `samples_seen` counts clips, not weights, and `evaluator` stays unweighted, as the reference's evaluation loss is.
        shared_graph: batched supports whose clips all carry one and the same graph (the reference's trainers pass the distance
        graph that way) are handed to the model in their 2-D form, which lets the encoder run its hoisted GEMMs in the
        eigenbasis of that graph (`ops.collapse_shared_supports`: one comparison + one flag read per supports TENSOR, cached; a
        captured step keeps the decision of its capture -- refill a captured supports buffer with per-clip graphs only after
        re-capturing, or pass shared_graph=False).
        always_reduce: issue the gradient all-reduce whenever a process group exists, also at world size 1 (exercises
        the RCCL path on a single GPU; a sum over one rank is the identity).
        data_augment: the reference's training-set augmentation (`--data_augment`; dataloader_detection.py:233-256,384-389: per
        sample a fair coin -- reflect the electrodes along the midline or not -- and an amplitude factor uniform in [0.8, 1.2), which
        under use_fft is `+= log(factor)` before standardisation), drawn ON THE DEVICE every step (`ops.draw_augmentation`, a Philox
        state of this object: a captured step draws afresh at every replay).  With raw_window the draws are operands of the
        featurisation kernel; for feature inputs (already standardised) the step applies x[b, :, perm[b]] + log(factor_b) /
        feature_std, which is the same value (feature_std = the scaler's std, required then).  Graph side as in the reference:
        supports=None (correlation graph) is built from the UN-reflected, un-scaled clip (`_get_indiv_graphs` never reads its
        swapped name table); for the distance graph pass `reflected_supports` (`utils.reflected_supports`: the graph of
        `_get_combined_graph(swap_nodes)`) -- every clip then carries the plain or the reflected supports according to its coin
        (per-clip graphs: the general path, not the spectral form).  swap_perm: `utils.swap_permutation(num_nodes)` by default.
        y, per task and mode: detection -> (B,) float labels; classification -> (B,) int64 classes; ssl -> the clip to predict, as
        features (B, Ty, N, D) -- or, with raw_window, as RAW signals (B, N, Ty*raw_window) like x.  The SSL sample is a PAIR
        (dataloader_ssl.py:317-341): the clip's coin and scale factor apply to input AND target, then the scaler to both -- with
        raw_window one launch featurises both halves (`ops.fft_features_pair`), on feature inputs one launch augments both
        (`ops.augment_features`); decoder (teacher forcing) and loss see the augmented, standardised target.  Graph side as for the
        supervised tasks (dataloader_ssl.py:349,355): correlation graph of the un-augmented INPUT clip, or the plain / reflected
        distance graph per coin.
        use_fft=False: the reference's time-domain input mode (no `--use_fft`): a step of the clip is the 200 samples themselves
        (`computeSliceMatrix(is_fft=False)`, dataloader_detection.py:25-85; the model has input_dim = output_dim = raw_window) and
        `_random_scale` MULTIPLIES the signals (`EEG_seq *= scale_factor`, :247-256); the factor is exp(log_scale) of the same device
        draws (`self.last_scale`).  With raw_window, x (and for ssl y) are the raw signals as above and one launch windows, reflects,
        scales and standardises them (`ops.window_features` / `ops.window_features_pair`); supports=None is the correlation graph
        of the raw rows of the un-augmented INPUT (`ops.correlation_supports_raw`).  On ready windows (B, T, N, raw-window samples,
        already standardised) the step applies x[b, :, perm[b]] * s_b + (s_b - 1) * feature_mean / feature_std to x -- and for ssl
        to y -- in one launch (`ops.augment_windows`), which is the same value; feature_mean and feature_std are required then.
        raw_window: the step takes RAW resampled signals (B, N, T*raw_window) instead of features and runs the reference's
        DataLoader-side chain on the device in front of the model (dataloader_detection.py:57-71,346-354,384-393): log|FFT| of every
        raw_window-sample step (`eeg_dcrnn_fft_features`) -> z-score with (raw_mean, raw_std) = the model input; with
        supports=None the per-clip correlation graph is built from the UN-standardised features, as `_get_indiv_graphs` does.
        padding_val: variable-length clips, the classification loader (dataloader_classification.py:25-85,321-343,356-361: a clip of
        curr_len <= max_seq_len steps is augmented and standardised, THEN padded with `padding_val`, and its correlation graph is that
        of the unpadded, un-augmented clip).  None: every clip is taken at full length, as before.  A number, with `seq_lengths` at
        `step` / `forward_backward` / `capture` (int64, read on the device: a captured step replays with refilled lengths): with
        raw_window the steps t >= seq_lengths[b] of clip b are not featurised / windowed and the model input holds `padding_val`
        there (whatever the raw signals hold behind the clip); with supports=None the graph is built from the first seq_lengths[b]
        steps only -- of the un-augmented features, raw rows or windows.  Feature or ready-window inputs are taken as given (the
        caller padded them): only that graph changes.  seq_lengths=None: full length.  Not for task="ssl" (no lengths there)."""
        assert task in ("detection", "classification", "ssl")
        if padding_val is not None and task == "ssl":
            raise ValueError("TrainStep: padding_val (variable-length clips) is for the supervised tasks; the SSL pair has no seq_lengths")
        self.padding_val = None if padding_val is None else float(padding_val)
        self.class_weights, self.sample_weights, self.weight_norm = self._check_weights(model, task, class_weights, sample_weights, weight_norm)
        self._weight_buffers = {}         # batch size -> (clip_u, denom): fixed addresses, a captured step rewrites them
        self.model, self.task, self.max_grad_norm = model, task, max_grad_norm
        self.fp = FlatParameters(model)
        # optimiser state lives in flat buffers; the update is ONE fused HIP kernel (clip + Adam)
        self.lr, self.weight_decay, self.betas, self.eps = lr, weight_decay, (0.9, 0.999), 1e-8
        self.exp_avg = torch.zeros_like(self.fp.flat)
        self.exp_avg_sq = torch.zeros_like(self.fp.flat)
        self.ws = torch.zeros(64, device=self.fp.flat.device, dtype=torch.float32)
        self.grad_norm = torch.zeros(1, device=self.fp.flat.device, dtype=torch.float32)
        self.step_count = 0
        # the optimiser's step count and learning rate also live on the device (eeg_dcrnn_clip_adam_dev reads / advances them on
        # the stream): the update is then a graph node like everything else.  `step_count` / `lr` are the host mirrors.
        dev = self.fp.flat.device
        self.step_dev = torch.zeros(1, device=dev, dtype=torch.int32)
        self.lr_dev = torch.full((1,), float(lr), device=dev, dtype=torch.float32)
        # samples seen so far = the reference's `step += batch_size` (train_ssl.py:163,178): drives the scheduled-
        # sampling threshold of the SSL model under curriculum learning (global batch: every rank advances alike)
        self.samples_seen = 0
        self.samples_seen_dev = torch.zeros(1, device=dev, dtype=torch.int64)
        has_pg = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size() if has_pg else 1
        self.reduce = has_pg and (self.world > 1 or always_reduce)
        self.scaler_mean, self.scaler_std = scaler_mean, scaler_std
        self.raw_window, self.raw_mean, self.raw_std = raw_window, float(raw_mean), float(raw_std)
        self.shared_graph = bool(shared_graph)
        self.use_fft = bool(use_fft)
        self.feature_mean = None if feature_mean is None else float(feature_mean)
        self.last_scale = None            # time-domain steps: the clips' amplitude factors of the latest step (tests / logging)
        # detection / classification: head + criterion + head backward as ONE operator behind the encoder (ops.cls_head_loss) instead
        # of model.forward -> loss kernel -> autograd through the head (same values; False: that public path, launch by launch)
        self.fused_head = True
        self.last_logits = None
        self.data_augment = bool(data_augment)
        self.feature_std = None if feature_std is None else float(feature_std)
        self.swap_perm, self.reflected_supports, self._augment_rng = None, None, None
        if self.data_augment:
            from . import utils
            if not use_fft and raw_window is None and (feature_std is None or feature_mean is None):
                raise ValueError("TrainStep: data_augment on time-domain windows (use_fft=False) needs feature_mean and feature_std (the "
                                 "StandardScaler's: the reference multiplies the signals BEFORE it standardises)")
            if raw_window is None and feature_std is None:
                raise ValueError("TrainStep: data_augment on feature inputs needs feature_std (the StandardScaler's std: the reference "
                                 "adds log(scale) BEFORE it standardises)")
            sp = utils.swap_permutation(model.num_nodes) if swap_perm is None else torch.as_tensor(swap_perm)
            if sp.numel() != model.num_nodes:
                raise ValueError(f"TrainStep: swap_perm has {sp.numel()} entries for {model.num_nodes} nodes")
            self.swap_perm = sp.to(device=dev, dtype=torch.int32).contiguous()
            if reflected_supports is not None:
                self.reflected_supports = torch.stack([torch.as_tensor(r, dtype=torch.float32) for r in reflected_supports]).to(dev).contiguous()
            self._augment_rng = ops.make_rng_state(dev, stream_id=2)
        self.last_augmentation = None     # (flags, perm, log_scale) of the latest step (tests / logging)
        self._graphs = {}
        self.sampler, self._epoch_batches = None, {}   # epochs from a device-resident data set (step_from / capture_epoch)
        self._pending_sampler_state = None             # a checkpoint's sampler state loaded before any sampler was attached
        # curriculum learning (SSL, model.py:194-200): where the persistent decoder kernels apply, the teacher-forcing flags are
        # drawn on the device (`eeg_dcrnn_teacher_flags`) -- in eager steps and graph replays alike; elsewhere on the host
        self.device_curriculum = None     # decided at the first batch (needs the shapes)

    # `step_count` / `samples_seen`: host mirrors of the device-resident counters the kernels read (Adam's bias correction uses
    # step_dev, the scheduled-sampling threshold samples_seen_dev); assigning to them (a resumed or restarted run) rewrites the
    # device tensors too -- outside any captured graph, like `lr`.
    @property
    def step_count(self):
        return self._step_count

    @step_count.setter
    def step_count(self, value):
        self._step_count = int(value)
        if hasattr(self, "step_dev"):
            self.step_dev.fill_(self._step_count)

    @property
    def samples_seen(self):
        return self._samples_seen

    @samples_seen.setter
    def samples_seen(self, value):
        self._samples_seen = int(value)
        if hasattr(self, "samples_seen_dev"):
            self.samples_seen_dev.fill_(self._samples_seen)

    def _advance(self, steps: int = 0, samples: int = 0):
        """the kernels of a step advanced the device counters themselves: move the host mirrors only"""
        self._step_count += int(steps)
        self._samples_seen += int(samples)

    @property
    def lr(self):
        return self._lr

    @lr.setter
    def lr(self, value):
        self._lr = float(value)
        if hasattr(self, "lr_dev"):
            self.lr_dev.fill_(self._lr)   # (outside any captured graph: the graph reads the tensor)

    def _use_device_curriculum(self, t_out: int, batch: int) -> bool:
        m = self.model
        if self.task != "ssl" or not getattr(m, "use_curriculum_learning", False):
            return False
        if self.device_curriculum is None:
            dec = m.decoder
            self.device_curriculum = ops.decoder_is_persistent(t_out, batch, dec.num_nodes, dec.hid_dim, dec.output_dim,
                                                               dec.decoding_cells[0].num_matrices, dec.num_rnn_layers)
        return self.device_curriculum

    def set_epoch(self, epoch: int, num_epochs: int, eta_min: float = 0.0):
        """Cosine learning-rate schedule of the reference, stepped per epoch (train.py:224,329)."""
        from . import utils
        if not hasattr(self, "base_lr"):
            self.base_lr = self.lr
        self.lr = utils.cosine_annealing_lr(self.base_lr, epoch, num_epochs, eta_min)
        return self.lr

    def loss(self, out, y):
        if self.task == "detection":        # train.py:203-204,266-267
            return ops.bce_with_logits(out.view(-1), y)
        if self.task == "classification":   # train.py:205-206,268
            return ops.cross_entropy(out, y)
        from . import utils                 # train_ssl.py:165-170 ("MAE" -> masked RMSE, Q9)
        sc = None if self.scaler_mean is None else utils.StandardScaler(self.scaler_mean, self.scaler_std)
        return utils.compute_regression_loss(y_true=y, y_predicted=out, standard_scaler=sc, loss_fn="MAE")

    @staticmethod
    def _check_weights(model, task, class_weights, sample_weights, weight_norm):
        """the weights of the criterion as device tensors, or the ValueError that names what is wrong with them -- before anything is
        launched.  -> (class_weights (C,) | None, sample_weights (P,) | None, weight_norm)"""
        if weight_norm is not None and weight_norm not in ops.WEIGHT_NORMS:
            raise ValueError(f"TrainStep: weight_norm={weight_norm!r} ('sum': divide by the sum of the step's weights; 'count': by the number "
                             f"of its clips)")
        if class_weights is None and sample_weights is None:
            return None, None, weight_norm
        if task == "ssl":
            raise ValueError("TrainStep: class_weights / sample_weights weigh the clips of the supervised criteria; task='ssl' has a "
                             "regression loss and no classes")
        dev = next(model.parameters()).device

        def vector(value, name, length, what):
            if torch.is_tensor(value):
                if value.dtype != torch.float32 or value.device != dev:
                    raise ValueError(f"TrainStep: {name} must be float32 on {dev} (the model's device), got {value.dtype} on {value.device}")
                t = value
            else:
                t = torch.tensor([float(v) for v in value], dtype=torch.float32)
            if t.dim() != 1 or (length is not None and t.numel() != length) or t.numel() < 1:
                raise ValueError(f"TrainStep: {name} has shape {tuple(t.shape)}, expected ({length if length is not None else 'P'},): {what}")
            host = t.detach().cpu()
            if not bool(torch.isfinite(host).all()) or bool((host < 0).any()):
                raise ValueError(f"TrainStep: {name} must be finite and >= 0 (a weight of 0 selects the clips out)")
            return host, t.detach().to(dev).contiguous()

        cw = sw = None
        if class_weights is not None:
            classes = 2 if task == "detection" else int(model.fc.weight.shape[0])
            host, cw = vector(class_weights, "class_weights", classes,
                              "one weight per class" + (" of the 0 / 1 labels: (1, p) is pos_weight=p" if task == "detection" else ""))
            if not bool((host > 0).any()):
                raise ValueError("TrainStep: class_weights are all zero: no clip would count")
        if sample_weights is not None:
            if not torch.is_tensor(sample_weights):
                raise ValueError(f"TrainStep: sample_weights must be a float32 (P,) tensor on {dev}, one weight per clip of the pool, got "
                                 f"{type(sample_weights).__name__}")
            _, sw = vector(sample_weights, "sample_weights", None, "one weight per clip of the pool")
        return cw, sw, weight_norm if weight_norm is not None else ("count" if task == "detection" else "sum")

    def _step_weights(self, y, sampler, label_pool):
        """this step's clip_u (B,) / denom (1,) in the buffers the step owns (`ops.clip_weights`, one launch).  With a sampler: from the
        label pool through the sampler's perm and the cursor its gather has just advanced; else from the batch's own labels."""
        b = int(y.shape[0])
        if b not in self._weight_buffers:
            dev = self.fp.flat.device
            self._weight_buffers[b] = (torch.zeros(b, dtype=torch.float32, device=dev), torch.ones(1, dtype=torch.float32, device=dev))
        clip_u, denom = self._weight_buffers[b]
        if sampler is None:
            labels = y.to(torch.float32 if self.task == "detection" else torch.int64).contiguous().view(-1)
            ops.clip_weights(labels, clip_u, denom, class_w=self.class_weights, norm=self.weight_norm)
        else:
            ops.clip_weights(label_pool, clip_u, denom, class_w=self.class_weights, sample_w=self.sample_weights, norm=self.weight_norm,
                             perm=sampler.perm, cursor=sampler.cursor, back=sampler.batch_size * sampler.world, rank=sampler.rank,
                             world=sampler.world)
        return clip_u, denom

    def _check_step_weights(self, y, sampler, label_pool):
        """what a weighted step refuses, before its first launch"""
        if sampler is None:
            if self.sample_weights is not None:
                raise ValueError("TrainStep(sample_weights=...): the weights belong to the clips of a pool; step() / capture() see a batch "
                                 "only -- use step_from() / capture_epoch() with the dataset and a sampler")
            return
        if label_pool is None or label_pool.dim() != 1:
            raise ValueError("TrainStep(class_weights / sample_weights): a step from a sampler weighs its clips through the dataset's label "
                             "pool (P,): forward_backward(..., sampler=, label_pool=dataset.y)")
        if self.sample_weights is not None and self.sample_weights.numel() != label_pool.numel():
            raise ValueError(f"TrainStep: sample_weights holds {self.sample_weights.numel()} weights, the pool {label_pool.numel()} clips")
        if y.shape[0] != sampler.batch_size:
            raise ValueError(f"TrainStep: a batch of {y.shape[0]} clips from a sampler of batch_size={sampler.batch_size}")

    def loss_and_grad(self, out, y, clip_w=None, denom=None, clip_u=None):
        """(loss, d loss / d out) of the task's criterion from the fused HIP loss kernels (same values as `self.loss`).
        clip_w / denom (device tensors of a drop_last=False sampler): over the clips that count, divided by denom; clip_u / denom
        (`_step_weights`, supervised tasks): a multiplier per clip instead"""
        E = torch.ops.eeg_dcrnn
        weights = () if clip_w is None else (clip_w, denom)
        if clip_u is not None:
            return E.bce_logits_cw(out.view(-1), y, clip_u, denom) if self.task == "detection" else E.ce_logits_cw(out, y, clip_u, denom)
        if self.task == "detection":
            return (E.bce_logits_w if weights else E.bce_logits)(out.view(-1), y, *weights)
        if self.task == "classification":
            return (E.ce_logits_w if weights else E.ce_logits)(out, y, *weights)
        scaled = self.scaler_mean is not None
        # train_ssl.py:165-170: loss_fn "MAE" != "mae" selects the masked RMSE (kind 1), Q9
        return (E.masked_loss_w if weights else E.masked_loss)(out, y, scaled, float(self.scaler_mean) if scaled else 0.0,
                                                               float(self.scaler_std) if scaled else 1.0, 0.0, 1, *weights)

    def forward_backward(self, x, y, seq_lengths, supports, sampler=None, label_pool=None):
        """supports=None: build the per-clip correlation graph and its dual random-walk supports from
        the clips on the device (the DataLoader-side `_get_indiv_graphs` of the reference).
        sampler: the `EpochSampler` whose gather filled x / y (`step_from` / `capture_epoch` pass theirs).  One that keeps the
        epoch's short last batch (drop_last=False) hands its device-resident `clip_w` / `denom` to the criterion and, for ssl, its
        `n_valid` to the curriculum counter; everything in front of the criterion sees the B real clips of the batch tensors.
        label_pool: the data set's labels (P,), read by a step with class / sample weights through the sampler (`_step_weights`)."""
        tail = sampler is not None and not sampler.drop_last
        clip_w, denom = (sampler.clip_w, sampler.denom) if tail else (None, None)
        clip_u = None
        weighted = self.class_weights is not None or self.sample_weights is not None
        if weighted:
            self._check_step_weights(y, sampler, label_pool)
        self.fp.zero_grad()
        if weighted:                      # the multipliers carry the validity of a short last batch: they take the selector's place
            clip_u, denom = self._step_weights(y, sampler, label_pool)
            clip_w = None
        perm, log_scale = None, None
        if self.data_augment and self.model.training:
            supports, perm, log_scale = self._draw_augmentation(x.shape[0], supports)
        x, y, supports = self._data_chain(x, y, seq_lengths, supports, perm, log_scale)
        if self.task == "ssl":
            if self._use_device_curriculum(y.shape[1], y.shape[0]):
                self.model.batches_seen_increment = sampler.n_valid if tail else x.shape[0] * self.world
                out = self.model(x, y, supports, batches_seen=self.samples_seen_dev)
            else:
                out = self.model(x, y, supports, batches_seen=self.samples_seen)    # train_ssl.py:163
        elif self.fused_head and hasattr(self.model, "encode_last"):
            # encoder -> [head, criterion and the head's backward: two launches] -> encoder backward seeded with d loss / d last
            m = self.model
            last = m.encode_last(x, seq_lengths, supports)
            drop_p = m._drop_p()
            with self.fp.sink:
                loss, self.last_logits, dz = ops.cls_head_loss(last, m.fc.weight, m.fc.bias, y, self.task, drop_p,
                                                               m._rng_state(last.device) if drop_p > 0 else None, clip_w=clip_w, denom=denom,
                                                               clip_u=clip_u)
                last.backward(dz)
            return loss.detach()
        else:
            out = self.model(x, seq_lengths, supports)
        # The loss kernels return value AND gradient (d loss / d out) from one pass: backward is seeded with that gradient
        # directly -- `loss.backward()` would first fill a ones tensor and multiply the saved gradient by it (two framework
        # kernels per step for a factor of exactly 1).  `self.loss(out, y).backward()` remains the equivalent public path.
        loss, seed = self.loss_and_grad(out.detach(), y, clip_w, denom, clip_u)
        with self.fp.sink:                       # backward operators write into the flat gradient bucket
            out.backward(seed.view_as(out))
        return loss.detach()

    def _data_chain(self, x, y, seq_lengths, supports, perm=None, log_scale=None):
        """the data side of a step in front of the model: raw signals -> log|FFT| or windows -> z-score, the padding of variable-length
        clips, the correlation graph of the un-augmented, un-standardised clip (supports=None) or the shared graph in its 2-D form
        -> (model input, target, supports).  perm / log_scale: this step's augmentation draws; None (a step without augmentation,
        and the evaluation pass of `DeviceEvaluator`): no draw is applied and none is taken."""
        # variable-length clips: the data side stops at the clip's own length (None: every step, the calls below as they always were)
        lens, pad = None, 0.0
        if self.padding_val is not None and seq_lengths is not None:
            lens, pad = seq_lengths.to(device=x.device, dtype=torch.int64), self.padding_val
        if not self.use_fft:
            x, y, supports = self._time_domain_inputs(x, y, supports, perm, log_scale, lens, pad)
        elif self.task == "ssl" and (self.raw_window is not None or perm is not None):
            # the SSL sample is a pair: the target takes the clip's draws and the scaler like the input (dataloader_ssl.py:317-341)
            x, y, supports = self._ssl_pair(x, y, supports, perm, log_scale)
        elif self.raw_window is not None:            # raw signals in: featurise on the device (x becomes the standardised log|FFT|)
            feat_raw, x = ops.fft_features(x, window=self.raw_window, mean=self.raw_mean, std=self.raw_std, perm=perm, log_scale=log_scale,
                                           lengths=lens, padding_val=pad)
            if supports is None:
                supports = ops.correlation_supports(feat_raw, top_k=3, lengths=lens)   # (feat_raw: un-reflected, un-scaled, un-standardised)
        elif perm is not None:
            plain = x
            idx = perm.to(torch.int64)[:, None, :, None].expand(-1, x.shape[1], -1, x.shape[3])
            x = x.gather(2, idx) + (log_scale / self.feature_std)[:, None, None, None]
            if supports is None:
                supports = ops.correlation_supports(plain, top_k=3, lengths=lens)
        if supports is None:
            supports = ops.correlation_supports(x, top_k=3, lengths=lens)
        elif self.shared_graph:
            supports = ops.collapse_shared_supports(supports)
        return x, y, supports

    def _ssl_target_steps(self, y) -> int:
        """decoder steps of an SSL target: feature steps, or whole windows of a raw target (refused otherwise)"""
        if self.raw_window is None:
            return y.shape[1]
        w = self.raw_window
        if y.dim() != 3 or y.shape[2] == 0 or y.shape[2] % w != 0:
            raise ValueError(f"TrainStep(task='ssl', raw_window={w}): y is the RAW target (B, num_nodes, Ty*{w}) -- the signals "
                             f"of the seconds to predict, a whole number of {w}-sample windows -- got {tuple(y.shape)}")
        return y.shape[2] // w

    def _ssl_pair(self, x, y, supports, perm, log_scale):
        """data side of the SSL step (dataloader_ssl.py:317-355): (model input, target, supports) with this step's draws (or none)
        on BOTH halves; the correlation graph comes from the un-reflected, un-scaled INPUT clip, the target plays no part in it"""
        if self.raw_window is not None:
            self._ssl_target_steps(y)
            if y.shape[:2] != x.shape[:2]:
                raise ValueError(f"TrainStep(task='ssl', raw_window={self.raw_window}): the raw target must be (B, num_nodes, Ty*"
                                 f"{self.raw_window}) with the input's {x.shape[0]} clips and {x.shape[1]} nodes, got {tuple(y.shape)}")
            plain, x, y = ops.fft_features_pair(x, y, window=self.raw_window, mean=self.raw_mean, std=self.raw_std, perm=perm,
                                                log_scale=log_scale)
        else:
            plain = x
            x, y = ops.augment_features(x, y, perm, log_scale, self.feature_std)
        if supports is None:
            supports = ops.correlation_supports(plain, top_k=3)
        return x, y, supports

    def _time_domain_inputs(self, x, y, supports, perm, log_scale, lens=None, pad=0.0):
        """data side of a use_fft=False step (dataloader_detection.py:25-85,233-256,384-393; dataloader_ssl.py:317-355): (model
        input, target, supports) with this step's draws (or none) -- on BOTH halves of an SSL pair; the correlation graph comes
        from the un-reflected, un-scaled INPUT clip.  lens (supervised tasks): the clips' valid steps -- raw signals are windowed up
        to them and padded with `pad` behind, and the graph is that of the unpadded clip (dataloader_classification.py:321-361)"""
        scale = None
        if log_scale is not None:
            scale = torch.exp(log_scale)             # B floats, a framework op (capturable): `EEG_seq *= scale_factor`
            self.last_scale = scale
        pair = self.task == "ssl"
        if self.raw_window is not None:
            raw = x
            if pair:
                self._ssl_target_steps(y)
                if y.shape[:2] != x.shape[:2]:
                    raise ValueError(f"TrainStep(task='ssl', raw_window={self.raw_window}): the raw target must be (B, num_nodes, Ty*"
                                     f"{self.raw_window}) with the input's {x.shape[0]} clips and {x.shape[1]} nodes, got {tuple(y.shape)}")
                x, y = ops.window_features_pair(x, y, self.raw_window, self.raw_mean, self.raw_std, perm=perm, scale=scale)
            else:
                x = ops.window_features(x, self.raw_window, self.raw_mean, self.raw_std, perm=perm, scale=scale, lengths=lens, padding_val=pad)
            if supports is None:
                supports = ops.correlation_supports_raw(raw, top_k=3, lengths=lens, window=self.raw_window)
        elif perm is not None:
            plain = x
            x, ya = ops.augment_windows(x, y if pair else None, perm, scale, self.feature_mean, self.feature_std)
            y = ya if pair else y
            if supports is None:
                supports = ops.correlation_supports(plain, top_k=3, lengths=lens)
        return x, y, supports

    def _draw_augmentation(self, batch, supports):
        """this step's draws; with a distance graph and its reflected partner, the per-clip supports"""
        plain = None
        if supports is not None and self.reflected_supports is not None:
            shared = ops.collapse_shared_supports(supports) if self.shared_graph else supports
            if any(s_.dim() != 2 for s_ in shared):
                raise RuntimeError("TrainStep(data_augment, reflected_supports): the supports of the step must be ONE graph shared by all "
                                   "clips (2-D tensors, or batched copies of it): the reflected partner is chosen per clip")
            if len(shared) != self.reflected_supports.shape[0]:
                raise RuntimeError(f"TrainStep: {len(shared)} supports, {self.reflected_supports.shape[0]} reflected partners")
            plain = torch.stack([s_.to(torch.float32) for s_ in shared])
        flags, perm, log_scale, sel = ops.draw_augmentation(self._augment_rng, batch, self.swap_perm, plain,
                                                            None if plain is None else self.reflected_supports)
        self.last_augmentation = (flags, perm, log_scale)
        return (supports if sel is None else sel), perm, log_scale

    # -- HIP-graph replay of forward + loss + backward -------------------------------------------
    def capture(self, x, y, seq_lengths, supports, warmup: int = 2, slot: int = 0, include_update: bool = False):
        """include_update: also capture the exchange + optimiser tail (the RCCL all-reduce of the flat bucket when a process
        group exists -- RCCL collectives are capturable -- and the fused clip + Adam, whose step count and learning rate are
        device-resident): the WHOLE optimisation step is then one graph launch per rank.  The warm-up launches and the upload
        replay below then apply real updates; a caller that minds restores the state afterwards (`snapshot()` / `restore()`).

        Capture zero_grad -> forward -> loss -> backward on the given (static) input tensors into
        one HIP graph (torch.cuda.CUDAGraph: the library launches on torch's current stream, never
        synchronises and allocates only through torch, so the ~60 launches of a step replay as one
        graph launch).  The exchange + optimiser tail stay outside the graph: the RCCL all-reduce is
        issued eagerly between the replay and the fused clip+Adam kernel.  New data is fed by
        copying into the captured tensors (`x.copy_(batch)`) -- or, without any device-side copy, by capturing the step
        on TWO input sets (`slot` 0 and 1) and alternating `replay_step(slot)`: the host-to-device copy of batch k+1
        then lands directly in the tensors the next replay reads while batch k computes."""
        # (the decoder's steps: feature steps of y, or the whole windows of a raw target)
        on_device = self.task == "ssl" and self._use_device_curriculum(self._ssl_target_steps(y), y.shape[0])
        if self.task == "ssl" and getattr(self.model, "use_curriculum_learning", False) and not on_device:
            # host-side teacher-forcing coin flips (model.py:194-200) select which launches are issued: a captured graph would
            # freeze one draw for ever.  (Where the persistent decoder kernels apply the flags are drawn on the device instead.)
            raise RuntimeError("TrainStep.capture: this decoder shape is outside the persistent decoder kernels, so curriculum "
                               "learning draws its teacher-forcing flags on the host every step; use step() (eager launches)")
        keep = self.snapshot() if on_device and not include_update else None

        def body():
            loss = self.forward_backward(x, y, seq_lengths, supports)
            if include_update:
                self.reduce_and_update(count=False)
            return loss

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):                       # populate the allocator before capture
                body()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loss = body()
        # one untimed replay: the first launch of an instantiated graph also uploads it to the device (torch exposes no
        # hipGraphUpload); it recomputes the gradients of the captured batch (and, with include_update, applies one more update)
        graph.replay()
        if include_update:
            self._advance(warmup + 1, (warmup + 1) * x.shape[0] * self.world)
        elif keep is not None:
            self.restore(keep, counters_only=True)        # the warm-up draws advanced the device-side sample counter
        self._graphs[slot] = (graph, loss, (x, y, seq_lengths, supports), include_update, None)
        return graph

    def snapshot(self):
        """everything a step changes besides the gradients: parameters, Adam moments, counters (device and host)"""
        return {"flat": self.fp.flat.detach().clone(), "exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone(),
                "step_dev": self.step_dev.clone(), "samples_seen_dev": self.samples_seen_dev.clone(),
                "step_count": self.step_count, "samples_seen": self.samples_seen}

    def restore(self, snap, counters_only: bool = False):
        with torch.no_grad():
            if not counters_only:
                self.fp.flat.copy_(snap["flat"])
                self.exp_avg.copy_(snap["exp_avg"])
                self.exp_avg_sq.copy_(snap["exp_avg_sq"])
                self.step_dev.copy_(snap["step_dev"])
                self.step_count = snap["step_count"]
            self.samples_seen_dev.copy_(snap["samples_seen_dev"])
            self.samples_seen = snap["samples_seen"]

    def replay_step(self, slot: int = 0):
        """One optimisation step on the captured tensors of `slot`: graph replay + all-reduce + clip/Adam."""
        graph, loss, inputs, whole, sampler = self._graphs[slot]
        graph.replay()
        # (a sampler that keeps the short last batch counts the clips that were there, from its host mirror of the cursor)
        self._advance(0, inputs[0].shape[0] * self.world if sampler is None else sampler.take())
        if whole:
            self._advance(1)
        else:
            self.reduce_and_update()
        return loss

    def reduce_and_update(self, count: bool = True):
        g = self.fp.flat_grad
        if self.reduce:
            dist.all_reduce(g, op=dist.ReduceOp.SUM)        # RCCL over xGMI: one flat bucket
        if count:
            self._advance(1)
        # mean over ranks (grad_scale), clip_grad_norm_(max_norm) and Adam in one pass over the buffers; the kernel advances
        # the device-resident step count itself
        ops.clip_adam_step_dev(self.fp.flat, g, self.exp_avg, self.exp_avg_sq, self.step_dev, self.lr_dev, self.betas,
                               self.eps, self.weight_decay, self.max_grad_norm, 1.0 / self.world, self.ws, self.grad_norm)
        return self.grad_norm

    def step(self, x, y, seq_lengths, supports):
        loss = self.forward_backward(x, y, seq_lengths, supports)
        self._advance(0, x.shape[0] * self.world)
        self.reduce_and_update()
        return loss

    # -- epochs from a device-resident data set (device_data.py: DeviceDataset, EpochSampler) ---------------------
    # The DataLoader's shuffle and collate (dataloader_detection.py:505-523 and its classification / SSL twins) on the device: the
    # step's batch is gathered out of the pools through the sampler's device-resident permutation and cursor (`ops.gather_clips`,
    # two launches) in front of the unchanged step -- in a captured graph as its first nodes, so an epoch replays with no host data
    # traffic.  Everything behind the gather (augmentation, featurisation, padding, graphs) acts on the gathered batch as before.
    def attach_sampler(self, sampler):
        """the sampler whose (seed, epoch, cursor) `state_dict` carries and `begin_epoch` advances (step_from / capture_epoch attach
        theirs themselves).  A sampler state that `load_state_dict` found with no sampler attached is applied to the first one
        attached afterwards: loading the checkpoint before or after the first step_from / capture_epoch resumes on the same clips."""
        self.sampler = sampler
        if self._pending_sampler_state is not None:
            state, self._pending_sampler_state = self._pending_sampler_state, None
            sampler.load_state_dict(state)
        return sampler

    def _epoch_batch(self, dataset, sampler):
        """the static batch tensors (x, y, seq_lengths) of this (dataset, batch size): allocated once, refilled by every gather"""
        dev = self.fp.flat.device
        if dataset.device != dev or sampler.device != dev:
            raise ValueError(f"TrainStep: dataset on {dataset.device}, sampler on {sampler.device}, model on {dev}: one device")
        if len(dataset) != sampler.P:
            raise ValueError(f"TrainStep: the dataset holds {len(dataset)} clips, the sampler permutes P={sampler.P}")
        dataset.check_step(self, "TrainStep")
        if self.padding_val is not None and not dataset.has_lengths:
            raise ValueError("TrainStep(padding_val=...): variable-length clips need the dataset's seq_lengths pool (DeviceDataset(x, y, "
                             "seq_lengths=...)); it has none")
        if (self.task == "ssl") != dataset.y_is_target:
            raise ValueError(f"TrainStep(task={self.task!r}): y of the dataset is {(len(dataset),) + dataset.y_shape} -- labels (P,) for the supervised "
                             f"tasks, the target pool (P, ...) for ssl")
        self.attach_sampler(sampler)
        key = (id(dataset), sampler.batch_size)
        if key not in self._epoch_batches:
            b = sampler.batch_size
            x = torch.empty((b,) + dataset.x_shape, dtype=torch.float32, device=dev)
            y = torch.empty((b,) + dataset.y_shape, dtype=dataset.y_dtype, device=dev)
            if dataset.has_lengths:
                lens, gathered = torch.empty(b, dtype=torch.int64, device=dev), True
            else:                         # whole clips: the constant lengths the model's last-step gather reads (ssl: None); a raw
                lens, gathered = dataset.full_lengths(b, self.raw_window, "TrainStep(raw_window=...)"), False      # pool needs raw_window
            self._epoch_batches[key] = (dataset, x, y, lens, gathered)    # (the dataset is held: its id stays its own)
        if self.class_weights is not None or self.sample_weights is not None:      # refused here, in front of the gather
            self._check_step_weights(self._epoch_batches[key][2], sampler, self._label_pool(dataset))
        return self._epoch_batches[key][1:]

    @staticmethod
    def _label_pool(dataset):
        """the data set's labels (P,) for a weighted step (None for a target pool: ssl, which takes no weights)"""
        return None if dataset.y_is_target else dataset.y

    def _gather_batch(self, dataset, sampler, batch):
        x, y, lens, gathered = batch
        dataset.gather(sampler, x, y, lens if gathered else None)

    def step_from(self, dataset, sampler, supports=None):
        """One eager step on the sampler's next batch of the dataset: gather into the batch tensors kept for it, then `step`.
        supports: None (correlation graphs built on the device) or the shared graph.  With a drop_last=False sampler the last step of
        the epoch trains on the clips that remain, normalised by their number (device_data.py); a step issued past the end of the
        epoch is the caller's error and applies a zero gradient."""
        batch = self._epoch_batch(dataset, sampler)
        self._gather_batch(dataset, sampler, batch)
        if sampler.drop_last and self.class_weights is None and self.sample_weights is None:
            return self.step(batch[0], batch[1], batch[2], supports)
        # the epoch's short last batch is kept: the criterion runs over the clips that count, and so does `samples_seen`
        loss = self.forward_backward(batch[0], batch[1], batch[2], supports, sampler=sampler, label_pool=self._label_pool(dataset))
        self._advance(0, sampler.take())
        self.reduce_and_update()
        return loss

    def capture_epoch(self, dataset, sampler, supports=None, warmup: int = 2, slot: int = 0, include_update: bool = False):
        """`capture` with the gather as the first nodes of the graph body, all on the one capture stream: every `replay_step(slot)`
        then trains on the sampler's next batch -- the cursor advances inside the graph -- and `begin_epoch` (outside the graph)
        starts the next epoch in the same tensors.  The warm-up launches and the upload replay run real gathers (and, with
        include_update, real updates, as in `capture`); the cursor is put back to where it was."""
        batch = self._epoch_batch(dataset, sampler)
        x, y, lens, _ = batch
        on_device = self.task == "ssl" and self._use_device_curriculum(self._ssl_target_steps(y), y.shape[0])
        if self.task == "ssl" and getattr(self.model, "use_curriculum_learning", False) and not on_device:
            raise RuntimeError("TrainStep.capture_epoch: this decoder shape is outside the persistent decoder kernels, so curriculum "
                               "learning draws its teacher-forcing flags on the host every step; use step_from() (eager launches)")
        keep = self.snapshot() if on_device and not include_update else None
        cursor0, host0 = sampler.cursor.clone(), sampler._host_cursor     # (host0: the host mirror a drop_last=False sampler keeps)

        def body():
            self._gather_batch(dataset, sampler, batch)
            loss = self.forward_backward(x, y, lens, supports, sampler=sampler, label_pool=self._label_pool(dataset))
            if include_update:
                self.reduce_and_update(count=False)
            return loss

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):                       # populate the allocator before capture
                body()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loss = body()
        graph.replay()                                    # the untimed upload replay of `capture`
        sampler.cursor.copy_(cursor0)
        seen = (warmup + 1) * x.shape[0] * self.world             # the clips the warm-up launches and the upload replay counted
        if not sampler.drop_last:
            seen = sum(sampler.take() for _ in range(warmup + 1))
            sampler._host_cursor = host0
        if include_update:
            self._advance(warmup + 1, seen)
        elif keep is not None:
            self.restore(keep, counters_only=True)
        self._graphs[slot] = (graph, loss, (x, y, lens, supports), include_update, None if sampler.drop_last else sampler)
        return graph

    def begin_epoch(self, epoch: int, num_epochs: int, sampler=None, eta_min: float = 0.0):
        """Start epoch `epoch`: the sampler draws and sorts its permutation in place and zeroes the cursor, the learning rate takes
        its cosine value (`set_epoch`).  Outside any captured graph; the graph of `capture_epoch` reads the same tensors."""
        if sampler is not None:
            self.attach_sampler(sampler)
        if self.sampler is None:
            raise RuntimeError("TrainStep.begin_epoch: no sampler attached (pass sampler=, or call step_from / capture_epoch first)")
        self.sampler.begin_epoch(epoch)
        return self.set_epoch(epoch, num_epochs, eta_min)

    def evaluator(self, dataset, batch_size: int, supports=None, rank: Optional[int] = None, world: Optional[int] = None):
        """the evaluation pass of this step's model and data chain over a device-resident pool, on the device
        (`evaluation.DeviceEvaluator`): `ev = step.evaluator(dev_ds, B); res = ev.run(is_test=False, eval_set="dev")`"""
        from .evaluation import DeviceEvaluator
        return DeviceEvaluator(self, dataset, batch_size, supports=supports, rank=rank, world=world)

    def ssl_evaluator(self, dataset, batch_size: int, supports=None, rank: Optional[int] = None, world: Optional[int] = None,
                      keep_predictions: bool = False, loss_batch: Optional[int] = None):
        """the SSL evaluation pass (train_ssl.py:232-280) of this step's model and pair chain over device-resident input and target
        pools, on the device (`evaluation.DeviceSSLEvaluator`): `ev = step.ssl_evaluator(dev_ds, B); eval_loss = ev.run()`"""
        from .evaluation import DeviceSSLEvaluator
        return DeviceSSLEvaluator(self, dataset, batch_size, supports=supports, rank=rank, world=world, keep_predictions=keep_predictions,
                                  loss_batch=loss_batch)

    def scanner(self, recordings, x_steps: int, stride_steps: int, batch_size: int = 256, supports=None, cover_tail: bool = True,
                max_events: int = 64, freq: int = 200, rank: Optional[int] = None, world: Optional[int] = None):
        """scan WHOLE recordings with this step's detector and data chain on the device (`scan.Scanner`): sliding windows of x_steps
        steps every stride_steps, the evaluator's pass over them, then a per-second timeline, seizure events and event scores:
        `sc = step.scanner(recordings, x_steps=60, stride_steps=12); res = sc.run(th_on=0.6, th_off=0.4, annotations=(ref, ref_count))`"""
        from .scan import Scanner
        return Scanner(self, recordings, x_steps, stride_steps, batch_size=batch_size, supports=supports, cover_tail=cover_tail,
                       max_events=max_events, freq=freq, rank=rank, world=world)

    def fit_scaler(self, dataset, batch_size: int = 256):
        """Fit this step's input scaler on the device (`statistics.fit_scaler`): the mean and std of the un-standardised inputs the
        step's raw chain produces for `dataset` -- log|FFT| features, or with use_fft=False the samples -- over its clips (valid steps
        only, of an SSL data set the input half), on the process group's ranks.  Sets `raw_mean` / `raw_std` and returns the
        `ScalerFit`.  Before any capture: a captured graph holds the scaler as kernel arguments.  A step without raw_window takes
        features that are already standardised: there is nothing to fit."""
        from .statistics import fit_scaler
        if self.raw_window is None:
            raise ValueError("TrainStep.fit_scaler: the step has raw_window=None: its inputs are features / windows taken as already "
                             "standardised; fit a pool of un-standardised features with eeg_gnn_ssl_amd.fit_scaler(dataset)")
        if self._graphs:
            raise ValueError(f"TrainStep.fit_scaler: {len(self._graphs)} graph(s) captured: raw_mean / raw_std are kernel arguments baked into "
                             f"them; fit the scaler in front of capture / capture_epoch")
        dataset.check_step(self, "TrainStep.fit_scaler")
        dev = self.fp.flat.device
        if dataset.device != dev:
            raise ValueError(f"TrainStep.fit_scaler: dataset on {dataset.device}, model on {dev}: one device")
        if len(dataset.x_shape) != 2:
            raise ValueError(f"TrainStep.fit_scaler: TrainStep(raw_window={self.raw_window}) takes raw signals (P, N, T*{self.raw_window}), the "
                             f"pool holds {(len(dataset),) + tuple(dataset.x_shape)}")
        fit = fit_scaler(dataset, batch_size, window=int(self.raw_window), use_fft=self.use_fft)
        self.raw_mean, self.raw_std = fit.mean, fit.std
        return fit

    def occlusion_maps(self, x, seq_lengths, supports=None, **kw):
        """occlusion maps (`interpret.occlusion_maps`) of this step's model on the inputs of an evaluation step: x as the step takes
        it (features, windows or raw signals) goes through the data chain WITHOUT augmentation draws -- with supports=None the
        correlation graph of the unpadded clip, built once and held fixed for every variant -- and the maps are taken on what the
        model would see.  Keywords: time_window, node_groups, fill, target, clips_per_pass, return_logits.  Leaves the model's mode,
        the step's counters, generators, optimiser state and sampler alone."""
        from .interpret import _check_options, occlusion_maps
        if self.task == "ssl":
            raise ValueError("TrainStep.occlusion_maps: task='ssl' predicts signals, not a probability; occlusion maps exist for the "
                             "detection and classification models (its evaluation pass is TrainStep.ssl_evaluator / evaluate_ssl)")
        classes = int(self.model.fc.weight.shape[0])
        if (self.task == "detection") != (classes == 1):
            raise ValueError(f"TrainStep.occlusion_maps(task={self.task!r}): the model's head has {classes} outputs")
        if not torch.is_tensor(x):
            raise ValueError(f"TrainStep.occlusion_maps: x must be a tensor, got {type(x).__name__}")
        _check_options(self.model, int(self.model.num_nodes), x.device, kw.get("time_window", 1), kw.get("node_groups"), kw.get("clips_per_pass", 16))
        with torch.no_grad():
            feats, _, sup = self._data_chain(x, None, seq_lengths, supports)
        return occlusion_maps(self.model, feats, seq_lengths, sup, **kw)

    # -- checkpointing (utils.CheckpointSaver / load_model_checkpoint use these like an optimizer's) -------
    def state_dict(self):
        """with a sampler attached also its (seed, epoch, cursor): a resumed run continues mid-epoch on the same clips"""
        state = {"step": self.step_count, "samples_seen": self.samples_seen, "lr": self.lr, "exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone()}
        if self.sampler is not None:
            state["sampler"] = self.sampler.state_dict()
        return state

    def load_state_dict(self, state):
        self.step_count, self.lr = int(state["step"]), float(state["lr"])
        self.samples_seen = int(state.get("samples_seen", 0))
        self.step_dev.fill_(self.step_count)
        self.samples_seen_dev.fill_(self.samples_seen)
        self.exp_avg.copy_(state["exp_avg"])
        self.exp_avg_sq.copy_(state["exp_avg_sq"])
        if "sampler" in state:            # no sampler attached yet: kept for `attach_sampler` (never dropped)
            if self.sampler is not None:
                self.sampler.load_state_dict(state["sampler"])
            else:
                self._pending_sampler_state = dict(state["sampler"])


def _all_gather_uneven(t: torch.Tensor) -> torch.Tensor:
    """Concatenation over the ranks of tensors whose FIRST dimension differs from rank to rank (evaluation shards of a
    data set are uneven whenever its size is not a multiple of the world size): the lengths travel first, every rank
    pads its shard to the longest one, one all_gather, and the padding is cut away again.  Same result on every rank."""
    world = dist.get_world_size()
    n = torch.tensor([t.shape[0]], device=t.device, dtype=torch.int64)
    sizes = [torch.empty_like(n) for _ in range(world)]
    dist.all_gather(sizes, n)
    sizes = [int(s.item()) for s in sizes]
    longest = max(sizes)
    if t.shape[0] < longest:
        t = torch.cat([t, t.new_zeros((longest - t.shape[0],) + tuple(t.shape[1:]))])
    parts = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(parts, t.contiguous())
    return torch.cat([p[:k] for p, k in zip(parts, sizes)])


@torch.no_grad()
def predict(model, batches, task: str = "detection"):
    """Evaluation forward passes (train.py:343-404 without the host round trip per batch): returns
    (y_prob, y_true) as numpy arrays gathered from ALL ranks on every rank (RCCL all_gather when launched
    data-parallel).  batches: iterable of (x, y, seq_lengths, supports) device tensors."""
    was_training = model.training
    model.eval()
    probs, labels = [], []
    for x, y, seq_lengths, supports in batches:
        if supports is None:
            supports = ops.correlation_supports(x, top_k=3)
        logits = model(x, seq_lengths, supports)
        probs.append(torch.sigmoid(logits.view(-1)) if task == "detection" else torch.softmax(logits, dim=1))
        labels.append(y.view(-1))
    multi = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    if probs:
        prob, lab = torch.cat(probs), torch.cat(labels)
    elif multi:
        # a rank whose shard of the evaluation set is empty still takes part in the gather (the others are waiting in it)
        dev = next(model.parameters()).device
        prob = torch.empty((0,) if task == "detection" else (0, model.fc.out_features), device=dev)
        lab = torch.empty((0,), dtype=torch.float32 if task == "detection" else torch.int64, device=dev)
    else:
        model.train(was_training)
        raise ValueError("predict: no batches")
    if multi:
        prob, lab = _all_gather_uneven(prob), _all_gather_uneven(lab)
    model.train(was_training)
    return prob.cpu().numpy(), lab.cpu().numpy()


@torch.no_grad()
def evaluate_ssl(model, batches, scaler_mean: Optional[float] = None, scaler_std: Optional[float] = None,
                 return_predictions: bool = False):
    """The reference's SSL evaluation pass (train_ssl.py:232-280): eval mode (no dropout, no teacher forcing -- `model(x, y,
    supports)` without `batches_seen`), per batch the masked MAE in original units (`loss_fn="mae"` with the StandardScaler,
    utils.py:431-495) from the HIP loss kernel, averaged over the data set weighted by batch size (the reference's
    `AverageMeter`, train_ssl.py:262-263,276).  Launched data-parallel, every rank evaluates its shard and all ranks
    return the loss of the union (all-reduce of the weighted sum and the count; no host round trip per batch).
    batches: iterable of (x, y, supports) or (x, y, seq_lengths, supports) device tensors (supports None: built on the
    device).  Returns eval_loss (float) -- and, with return_predictions, the predictions and targets of THIS rank's shard
    as the reference collects them (train_ssl.py:266-274)."""
    was_training = model.training
    model.eval()
    tot, preds, truths = None, [], []
    for batch in batches:
        x, y, supports = batch[0], batch[1], batch[-1]
        if supports is None:
            supports = ops.correlation_supports(x, top_k=3)
        pred = model(x, y, supports)
        loss = ops.masked_regression_loss(pred, y, scaler_mean, scaler_std, loss_fn="mae")
        w = torch.stack([loss.reshape(()).double() * x.shape[0], torch.tensor(float(x.shape[0]), device=x.device, dtype=torch.float64)])
        tot = w if tot is None else tot + w
        if return_predictions:
            preds.append(pred)
            truths.append(y)
    multi = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    if tot is None:
        if not multi:
            model.train(was_training)
            raise ValueError("evaluate_ssl: no batches")
        tot = torch.zeros(2, dtype=torch.float64, device=next(model.parameters()).device)    # an empty shard still joins the all-reduce
    if multi:
        dist.all_reduce(tot)
    model.train(was_training)
    if float(tot[1].item()) == 0.0:
        raise ValueError("evaluate_ssl: no batches on any rank")
    eval_loss = float((tot[0] / tot[1]).item())
    if return_predictions:
        return eval_loss, torch.cat(preds).cpu().numpy(), torch.cat(truths).cpu().numpy()
    return eval_loss


@torch.no_grad()
def evaluate(model, batches, task: str = "detection", is_test: bool = False, eval_set: str = "dev",
             best_thresh: float = 0.5):
    """The reference's evaluation pass (train.py:332-431) on device tensors: forward in eval mode, sample-weighted
    mean loss (BCE-with-logits / cross-entropy, computed by the HIP loss kernels), predictions at `best_thresh`
    (detection; on the dev set of a test run the threshold is re-chosen by `utils.thresh_max_f1`,
    train.py:406-412) or arg-max (classification), and the score dictionary in the reference's order:
    loss, acc, F1, recall, precision, best_thresh[, auroc].  Launched data-parallel, every rank evaluates its
    shard and all ranks return the scores of the union (all_gather of probabilities, labels and loss sums).
    batches: iterable of (x, y, seq_lengths, supports) device tensors (supports None: built on the device)."""
    from collections import OrderedDict
    import numpy as np
    from . import utils
    was_training = model.training
    model.eval()
    probs, labels = [], []
    loss_sum = None
    n_seen = 0
    for x, y, seq_lengths, supports in batches:
        if supports is None:
            supports = ops.correlation_supports(x, top_k=3)
        logits = model(x, seq_lengths, supports)
        if task == "detection":
            lg = logits.view(-1)
            loss = ops.bce_with_logits(lg, y.view(-1).float())
            probs.append(torch.sigmoid(lg))
        else:
            loss = ops.cross_entropy(logits, y.view(-1))
            probs.append(torch.softmax(logits, dim=1))
        labels.append(y.view(-1))
        loss_sum = loss * x.shape[0] if loss_sum is None else loss_sum + loss * x.shape[0]
        n_seen += x.shape[0]
    prob, lab = torch.cat(probs), torch.cat(labels)
    tot = torch.stack([loss_sum.reshape(()).double(), torch.tensor(float(n_seen), device=prob.device, dtype=torch.float64)])
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        prob, lab = _all_gather_uneven(prob), _all_gather_uneven(lab)
        dist.all_reduce(tot)
    model.train(was_training)
    y_prob, y_true = prob.cpu().numpy(), lab.cpu().numpy().astype(int)
    eval_loss = float((tot[0] / tot[1]).item())
    if task == "detection":
        if eval_set == "dev" and is_test:
            best_thresh = float(utils.thresh_max_f1(y_true=y_true, y_prob=y_prob))
        y_pred = (y_prob > best_thresh).astype(int)
    else:
        y_pred = np.argmax(y_prob, axis=1).reshape(-1)
    scores, _, _ = utils.eval_dict(y_pred=y_pred, y=y_true, y_prob=y_prob if task == "detection" else None,
                                   average="binary" if task == "detection" else "weighted")
    res = [("loss", eval_loss), ("acc", scores["acc"]), ("F1", scores["F1"]), ("recall", scores["recall"]),
           ("precision", scores["precision"]), ("best_thresh", best_thresh)]
    if "auroc" in scores:
        res.append(("auroc", scores["auroc"]))
    return OrderedDict(res)
