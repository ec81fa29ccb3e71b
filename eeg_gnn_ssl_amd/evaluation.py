"""The reference's evaluation pass (train.py:289-326,332-431: after every epoch, for checkpoint selection and early stopping) on the
device, for the detection and classification tasks.

`evaluate` / `predict` (train_step.py) run the model on whatever batches they are handed and finish on the host (`.cpu()` + sklearn):
they have no data chain -- a raw or time-domain pool cannot be evaluated -- and no lengths for the correlation graph.  A
`DeviceEvaluator` hangs off the `TrainStep`, which owns both: a pass walks a `DeviceDataset` IN ORDER through an evaluator-owned
`EpochSampler` (identity permutation, short last batch kept), runs the step's data chain without augmentation, the `save=False`
forward and the head, and writes every clip's probability and criterion term into fixed buffers (`ops.eval_scores`).  The body of a
step is captured once as one HIP graph and replayed; the graph reads the parameters in place, so it stays valid while training
updates them.  Behind the last step `ops.eval_metrics` reduces the buffers to one small integer record (the project's own sort, AUROC
numerator, max-F1 threshold, confusion counts) which the host reads in a single copy and finishes in float64.

A `DeviceSSLEvaluator` (`TrainStep.ssl_evaluator`) is the same pass for self-supervised pre-training (train_ssl.py:232-280): the pair
chain of the step on the input and target pools, the decoder without teacher forcing, and per clip the float64 masked-MAE sum and
count (`ops.ssl_eval_scores`); `ops.ssl_eval_metrics` reduces them to the loss the reference selects its checkpoint by.

`evaluate`, `predict` and `evaluate_ssl` are unchanged and remain the yardstick."""
from __future__ import annotations

from collections import OrderedDict
from typing import Optional

import numpy as np
import torch
import torch.distributed as dist

from . import ops
from .device_data import EpochSampler

# words of the record (include/eeg_dcrnn.h: eeg_dcrnn_eval_metrics)
_N, _POS, _NEG, _NUM, _THRESH, _TP, _FP_, _FN, _TN, _BAD_LABELS, _BAD_PROBS, _LOSS, _SEARCHED, _FOUND = range(14)


def _ratio(a, b):
    return float(a) / float(b) if b else 0.0       # (a class without predictions / support scores 0: sklearn's zero_division default)


def scores_from_record(record, task: str, best_thresh: float = 0.5):
    """The reference's score dictionary (the keys and order of `evaluate`) from the int64 record of `ops.eval_metrics`, in float64 on the
    host.  Non-zero flag counters (labels outside the task's classes, probabilities outside [0, 1] or NaN) raise ValueError."""
    rec = np.asarray(record.cpu() if torch.is_tensor(record) else record, dtype=np.int64)
    n = int(rec[_N])
    if rec[_BAD_LABELS] or rec[_BAD_PROBS]:
        raise ValueError(f"eval_metrics: {int(rec[_BAD_LABELS])} labels outside the task's classes and {int(rec[_BAD_PROBS])} probabilities "
                         f"outside [0, 1] (or NaN) among {n} clips")
    loss = float(rec[_LOSS:_LOSS + 1].view(np.float64)[0]) / n
    if task == "detection":
        n_pos, n_neg = int(rec[_POS]), int(rec[_NEG])
        tp, fp, fn, tn = (int(rec[i]) for i in (_TP, _FP_, _FN, _TN))
        if rec[_SEARCHED]:
            if not rec[_FOUND]:
                raise ValueError("eval_metrics: the threshold search has no candidate (no positive clip: F1 is undefined everywhere, "
                                 "as in utils.thresh_max_f1)")
            best_thresh = float(rec[_THRESH:_THRESH + 1].view(np.float64)[0])
        if n_pos == 0 or n_neg == 0:
            # one class only: whatever utils.eval_dict does on such labels (sklearn's AUROC is undefined there), from the same counts
            from . import utils
            y = np.array([1] * n_pos + [0] * n_neg)
            y_pred = np.array([1] * tp + [0] * fn + [1] * fp + [0] * tn)
            scores, _, _ = utils.eval_dict(y_pred=y_pred, y=y, y_prob=y_pred.astype(np.float64), average="binary")
        else:
            scores = {"acc": (tp + tn) / n, "F1": _ratio(2 * tp, 2 * tp + fp + fn), "precision": _ratio(tp, tp + fp),
                      "recall": _ratio(tp, tp + fn), "auroc": int(rec[_NUM]) / (2.0 * n_pos * n_neg)}
    else:
        c = int(round((rec.size - ops.EVAL_RECORD_HEAD) ** 0.5))
        cm = rec[ops.EVAL_RECORD_HEAD:].reshape(c, c)                # row = label, column = prediction
        support, predicted, hit = cm.sum(axis=1), cm.sum(axis=0), np.diag(cm)
        w = support / float(support.sum())
        scores = {"acc": float(hit.sum()) / n,
                  "F1": float(sum(w[k] * _ratio(2 * hit[k], support[k] + predicted[k]) for k in range(c))),
                  "precision": float(sum(w[k] * _ratio(hit[k], predicted[k]) for k in range(c))),
                  "recall": float(sum(w[k] * _ratio(hit[k], support[k]) for k in range(c)))}
    res = [("loss", loss), ("acc", scores["acc"]), ("F1", scores["F1"]), ("recall", scores["recall"]), ("precision", scores["precision"]),
           ("best_thresh", best_thresh)]
    if "auroc" in scores:
        res.append(("auroc", scores["auroc"]))
    return OrderedDict(res)


class _CapturedPass:
    """what the evaluators share: the body of a step as one HIP graph"""

    def _capture(self, warmup: int = 2):
        """the body as one HIP graph (the model is in eval mode here); the warm-up launches and the upload replay run real steps
        whose scores `run` zeroes again"""
        if self._scores.device.type != "cuda":
            raise RuntimeError(type(self).__name__ + ".run(capture=True) needs HIP graphs: the pools are on " + str(self._scores.device) +
                               "; pass capture=False")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self._body()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self._body()
        graph.replay()
        self._graph = graph
        return graph

    def _replay(self, capture: bool):
        """zero the scores, put the sampler at the start of the pool and issue the steps of one pass"""
        s = self.sampler
        graph = (self._graph or self._capture()) if capture else None
        ops.zero_(self._scores)
        s.seek(0)
        for _ in range(s.steps_per_epoch):
            if graph is not None:
                graph.replay()
            else:
                self._body()


class DeviceEvaluator(_CapturedPass):
    """`TrainStep.evaluator(dataset, batch_size, supports=None)`: evaluation passes of the step's model over `dataset` on the device.

    supports: None (correlation graphs built on the device -- of the unpadded clip when the step has `padding_val` and the dataset a
    length pool) or the shared graph: the rule of `TrainStep.step_from`.  A pass is ceil(P / (batch_size * world)) steps over the pool
    in order; rank r takes the slots cursor + r * batch_size .. of every step, and `probs` / `losses` go through one summed
    all-reduce behind the last step (disjoint slots, zeros elsewhere).  After `run`:
        probs   (P,) float32 (detection) / (P, C) (classification), pool order, on the device
        losses  (P,) float32, the per-clip criterion terms
        record  the integer record of the pass (`ops.eval_metrics`), on the host
    The buffers keep their addresses; the next `run` overwrites them.  P <= ops.EVAL_MAX_CLIPS (2^20)."""

    def __init__(self, step, dataset, batch_size: int, supports=None, rank: Optional[int] = None, world: Optional[int] = None):
        if step.task == "ssl":
            raise ValueError("DeviceEvaluator: task='ssl' has no per-clip scores; its evaluation pass is train_step.evaluate_ssl")
        dev = step.fp.flat.device
        if dataset.device != dev:
            raise ValueError(f"DeviceEvaluator: dataset on {dataset.device}, model on {dev}: one device")
        if len(dataset) > ops.EVAL_MAX_CLIPS:
            raise ValueError(f"DeviceEvaluator: the pool holds P={len(dataset)} clips, one pass takes at most {ops.EVAL_MAX_CLIPS} "
                             f"(ops.EVAL_MAX_CLIPS); evaluate it in parts")
        dataset.check_step(step, "DeviceEvaluator")
        want = torch.float32 if step.task == "detection" else torch.int64
        if dataset.y_is_target or dataset.y_dtype != want:
            raise ValueError(f"DeviceEvaluator(task={step.task!r}): y of the dataset must be the labels (P,) as {want}, got {dataset.y_dtype} "
                             f"{(len(dataset),) + dataset.y_shape}")
        if step.padding_val is not None and not dataset.has_lengths:
            raise ValueError("DeviceEvaluator: TrainStep(padding_val=...) evaluates variable-length clips: the dataset needs a seq_lengths "
                             "pool (DeviceDataset(x, y, seq_lengths=...))")
        self.classes = int(step.model.fc.weight.shape[0])
        if (step.task == "detection") != (self.classes == 1):
            raise ValueError(f"DeviceEvaluator(task={step.task!r}): the model's head has {self.classes} outputs")
        self.step, self.dataset, self.supports = step, dataset, supports
        # the pass's own sampler: never begun (perm = identity), never attached to the step
        self.sampler = EpochSampler(len(dataset), batch_size, seed=0, rank=rank, world=world, device=dev, drop_last=False)
        p, b, c = len(dataset), int(batch_size), self.classes
        self._scores = torch.zeros(p * c + p, dtype=torch.float32, device=dev)      # probs | losses: one zero_, one all-reduce
        self.probs = self._scores[:p * c].view((p,) if c == 1 else (p, c))
        self.losses = self._scores[p * c:]
        self._ws, self._record = ops.eval_metrics_buffers(p, c, dev)
        self.record = None
        self._x = torch.empty((b,) + dataset.x_shape, dtype=torch.float32, device=dev)
        self._y = torch.empty((b,), dtype=dataset.y_dtype, device=dev)
        if dataset.has_lengths:
            self._lens, self._gather_lens = torch.empty(b, dtype=torch.int64, device=dev), True
        else:
            self._lens, self._gather_lens = dataset.full_lengths(b, step.raw_window, "DeviceEvaluator"), False
        self._graph = None

    def _body(self):
        """one step of the pass: gather -> data chain without augmentation -> save=False forward -> head (p = 0) -> scores"""
        st, ds, s, m = self.step, self.dataset, self.sampler, self.step.model
        ds.gather(s, self._x, self._y, self._lens if self._gather_lens else None)
        x, _, supports = st._data_chain(self._x, self._y, self._lens, self.supports)
        last = m.encode_last(x, self._lens, supports)
        logits = ops.cls_head(last, m.fc.weight, m.fc.bias, 0.0, None)
        ops.eval_scores(logits.view(self._x.shape[0], self.classes), ds.y, s.clip_w, s.cursor, self.probs, self.losses, s.rank, s.world)

    @torch.no_grad()
    def run(self, is_test: bool = False, eval_set: str = "dev", best_thresh: float = 0.5, capture: bool = True):
        """One pass -> the OrderedDict of `evaluate` (loss, acc, F1, recall, precision, best_thresh[, auroc]).  detection: the
        predictions are prob > best_thresh; on the dev set of a test run (is_test, eval_set == "dev") the threshold is searched on the
        device (max F1, `utils.thresh_max_f1`).  capture: replay the step's body as one HIP graph (captured at the first such call)
        instead of issuing it eagerly.  Leaves the model's mode, the step's counters, optimiser state, generators and sampler alone."""
        st, s, model = self.step, self.sampler, self.step.model
        multi = s.world > 1
        if multi and not (dist.is_available() and dist.is_initialized() and dist.get_world_size() == s.world):
            raise RuntimeError(f"DeviceEvaluator: world={s.world} needs a process group of that size for the all-reduce of the scores")
        was_training = model.training
        model.eval()
        try:
            self._replay(capture)
            if multi:
                dist.all_reduce(self._scores, op=dist.ReduceOp.SUM)
            search = st.task == "detection" and eval_set == "dev" and bool(is_test)
            ops.eval_metrics(self.probs, self.dataset.y, self.losses, search, best_thresh, self._ws, self._record)
            self.record = self._record.cpu()                         # the pass's one device-to-host copy
        finally:
            model.train(was_training)
        return scores_from_record(self.record, st.task, best_thresh)

    @torch.no_grad()
    def bootstrap(self, groups=None, n_boot: int = 2000, seed: int = 0):
        """Clustered-bootstrap replicates of the last pass's scores -> `BootstrapResult` (bootstrap.py).  groups: (P,) integer cluster
        ids (`RecordingDataset.clip_groups()`: by recording) or None: every clip its own cluster.  Uses the pass's `probs`, `losses`,
        the labels of the dataset and the threshold of the pass's record, and only reads them: `probs`, `losses`, `record` and the
        captured graph stay as they are.  With several ranks every rank holds the all-reduced buffers and computes the same result,
        with no communication."""
        from .bootstrap import bootstrap_scores
        if self.record is None:
            raise ValueError("DeviceEvaluator.bootstrap: no pass has run yet (run() first)")
        thresh = 0.5
        if self.step.task == "detection":
            thresh = float(self.record[_THRESH:_THRESH + 1].numpy().view(np.float64)[0])
        return bootstrap_scores(self.probs, self.dataset.y, self.step.task, groups=groups, n_boot=n_boot, seed=seed, best_thresh=thresh,
                                losses=self.losses)


class DeviceSSLEvaluator(_CapturedPass):
    """`TrainStep.ssl_evaluator(dataset, batch_size, supports=None)`: the SSL evaluation pass (train_ssl.py:232-280) of the step's
    model over `dataset` on the device -- the value `evaluate_ssl` returns, from pools `evaluate_ssl` cannot be handed.

    dataset: `DeviceDataset(x, y)` with y the TARGET pool: features / windows (P, Ty, N, D), or -- `TrainStep(raw_window=W)` -- raw
    signals (P, N, Ty*W) like x.  A step of the pass gathers B clips of both pools in order, runs the step's pair chain without
    augmentation (`fft_features_pair` / `window_features_pair` / the features as they are; supports=None: the correlation graph of
    the plain input clip), the model in eval mode (no dropout, no `batches_seen`: no teacher forcing) and `ops.ssl_eval_scores`
    with the step's scaler_mean / scaler_std.  rank r takes the slots cursor + r * batch_size .. of every step; the (3, P) scores
    go through one summed all-reduce behind the last step (disjoint slots, zeros elsewhere).

    `run` returns the reference's AverageMeter loss over consecutive batches of `loss_batch` clips (default: batch_size, the
    PER-RANK batch size: every rank of any world size returns the single-process result of that batch size).  After `run`:
        record       the pass's record (`ops.ssl_eval_metrics`), float64, on the host; `result`: its words by name
        clip_abs, clip_count, clip_mae   (P,) float64 in pool order, on the device (clip_mae: 0 for a fully masked clip)
        predictions  (P, Ty, N, D) with keep_predictions: THIS rank's slots, zeros elsewhere (not reduced), standardised like
                     the predictions `evaluate_ssl(return_predictions=True)` returns for the rank's shard
    The buffers keep their addresses; the next `run` overwrites them.  Limits: P <= ops.EVAL_MAX_CLIPS, a clip below
    ops.SSL_EVAL_MAX_CLIP_ELEMS elements, output_dim a multiple of 4 (16-byte pieces)."""

    def __init__(self, step, dataset, batch_size: int, supports=None, rank: Optional[int] = None, world: Optional[int] = None,
                 keep_predictions: bool = False, loss_batch: Optional[int] = None):
        if step.task != "ssl":
            raise ValueError(f"DeviceSSLEvaluator: task={step.task!r} has labels and scores per clip; its evaluation pass is TrainStep.evaluator")
        dataset.check_step(step, "DeviceSSLEvaluator")
        if not dataset.y_is_target:
            raise ValueError(f"DeviceSSLEvaluator: y of the dataset is a label pool {(len(dataset),) + dataset.y_shape}; the pass needs the TARGET pool, "
                             f"DeviceDataset(x, y) with y the clips to predict (P, Ty, N, D) or raw (P, N, Ty*raw_window)")
        dev = step.fp.flat.device
        if dataset.device != dev:
            raise ValueError(f"DeviceSSLEvaluator: dataset on {dataset.device}, model on {dev}: one device")
        p, b, m = len(dataset), int(batch_size), step.model
        if p > ops.EVAL_MAX_CLIPS:
            raise ValueError(f"DeviceSSLEvaluator: the pool holds P={p} clips, one pass takes at most {ops.EVAL_MAX_CLIPS} "
                             f"(ops.EVAL_MAX_CLIPS); evaluate it in parts")
        xs, ys = (p,) + dataset.x_shape, (p,) + dataset.y_shape       # the shapes of the pools, held or cut
        if step.raw_window is not None:
            w = int(step.raw_window)
            if len(xs) != 3 or len(ys) != 3 or ys[1] != xs[1] or ys[2] == 0 or ys[2] % w != 0:
                raise ValueError(f"DeviceSSLEvaluator: TrainStep(raw_window={w}) evaluates RAW pools: x (P, N, T*{w}) and the target "
                                 f"(P, N, Ty*{w}) -- whole windows of the same nodes -- got x {xs}, y {ys}")
            steps = ys[2] // w
        else:
            if len(xs) != 4 or len(ys) != 4:
                raise ValueError(f"DeviceSSLEvaluator: without raw_window the pools hold features / windows, x (P, T, N, D) and the target "
                                 f"(P, Ty, N, D), got x {xs}, y {ys}; raw signals need TrainStep(raw_window=W)")
            steps = ys[1]
        if m.output_dim % 4 != 0:
            raise ValueError(f"DeviceSSLEvaluator: the model's output_dim={m.output_dim} is no multiple of 4 (ops.ssl_eval_scores reads "
                             f"16-byte pieces); evaluate with train_step.evaluate_ssl")
        if loss_batch is not None and int(loss_batch) < 1:
            raise ValueError(f"DeviceSSLEvaluator: loss_batch={loss_batch} (the batch size of the reference's loss, >= 1)")
        self.step, self.dataset, self.supports = step, dataset, supports
        # the pass's own sampler: never begun (perm = identity), never attached to the step
        self.sampler = EpochSampler(p, b, seed=0, rank=rank, world=world, device=dev, drop_last=False)
        self.loss_batch = b if loss_batch is None else int(loss_batch)
        self._scores, self._record, self.predictions = ops.ssl_eval_buffers(
            p, dev, (steps, m.num_nodes, m.output_dim) if keep_predictions else None)
        self.clip_abs, self.clip_count = self._scores[0], self._scores[1]
        self.clip_mae, self.record, self.result = None, None, None
        self._x = torch.empty((b,) + dataset.x_shape, dtype=torch.float32, device=dev)
        self._y = torch.empty((b,) + dataset.y_shape, dtype=torch.float32, device=dev)
        self._graph = None

    def _body(self):
        """one step of the pass: gather the pair -> pair chain without augmentation -> the model without teacher forcing -> scores"""
        st, ds, s = self.step, self.dataset, self.sampler
        ds.gather(s, self._x, self._y)
        x, y, supports = st._data_chain(self._x, self._y, None, self.supports)
        pred = st.model(x, y, supports).contiguous()                 # (the decoder's output is time-major)
        ops.ssl_eval_scores(pred, y, s.clip_w, s.cursor, self._scores, s.rank, s.world, st.scaler_mean, st.scaler_std, 0.0, self.predictions)

    @torch.no_grad()
    def run(self, capture: bool = True) -> float:
        """One pass -> eval_loss, the value of `evaluate_ssl` over batches of `loss_batch` clips.  capture: replay the step's body as
        one HIP graph (captured at the first such call; it reads the parameters in place) instead of issuing it eagerly.  A
        prediction that is NaN or infinite where the target is masked in raises ValueError (the reference turns such a batch's loss
        into 0).  Leaves the model's mode, the step's counters, optimiser state, generators and sampler alone."""
        st, s, model = self.step, self.sampler, self.step.model
        multi = s.world > 1
        if multi and not (dist.is_available() and dist.is_initialized() and dist.get_world_size() == s.world):
            raise RuntimeError(f"DeviceSSLEvaluator: world={s.world} needs a process group of that size for the all-reduce of the scores")
        was_training = model.training
        model.eval()
        try:
            if self.predictions is not None:
                ops.zero_(self.predictions)
            self._replay(capture)
            if multi:
                dist.all_reduce(self._scores, op=dist.ReduceOp.SUM)
            ops.ssl_eval_metrics(self._scores, self.loss_batch, self._record)
            self.record = self._record.cpu()                         # the pass's one device-to-host copy
        finally:
            model.train(was_training)
        self.result = OrderedDict(zip(ops.SSL_EVAL_RECORD, (float(v) for v in self.record)))
        if self.result["bad"]:
            raise ValueError(f"ssl_eval_scores: {int(self.result['bad'])} predictions are NaN or infinite where the target counts, among "
                             f"{int(self.result['count'])} elements of {int(self.result['n'])} clips")
        self.clip_mae = torch.where(self.clip_count > 0, self.clip_abs / self.clip_count.clamp(min=1.0), torch.zeros_like(self.clip_abs))
        return self.result["loss"]
