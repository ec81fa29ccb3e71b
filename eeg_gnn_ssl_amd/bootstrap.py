"""Confidence intervals of the scores, on the device: the clustered bootstrap.

The clips of an evaluation set are not independent -- a recording gives dozens of clips, a patient several recordings -- so the
resampling unit is the CLUSTER (`RecordingDataset.clip_groups()`: by recording; any (P,) int32 labelling: by patient).  A replicate is
a row of integer counts over the G clusters (`ops.boot_counts`: Philox draws, row 0 all ones = the point estimate); a clip of cluster
g weighs counts[r, g], and every score of the replicate is the weighted form of the score the evaluator computes:
    detection       `ops.boot_detection`: one sort per call, then one workgroup per replicate -> an int64 record per replicate
                    (weighted N, positives, negatives, the AUROC numerator, tp / fp / fn / tn at the fixed threshold, the bits of the
                    float64 average precision and of the weighted loss sum)
    classification  `ops.boot_classification`: the weighted confusion matrix per replicate
    scans           `ops.boot_records`: weighted sums of the per-recording records of `ops.event_scores`
The host reads the records in one copy and finishes in float64 with the formulas of `scores_from_record` (+ auprc).  A replicate in
which a score has no support (AUROC without a positive or without a negative) is NaN and COUNTED, never dropped silently:
`BootstrapResult.interval` refuses when too many are.  DESIGN.md §4.3 states the kernels and the integer forms, §8 the limits."""
from __future__ import annotations

from collections import OrderedDict
from typing import Optional

import numpy as np
import torch

from . import ops

_W = {name: i for i, name in enumerate(ops.BOOT_RECORD)}


def _safe_div(a, b, empty):
    """a / b elementwise in float64; `empty` where b == 0"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.where(b != 0, a / np.where(b != 0, b, 1.0), empty)


def detection_scores_from_records(records, with_loss: bool):
    """name -> (rows,) float64 from the int64 records of `ops.boot_detection`: the formulas of `scores_from_record` on weighted counts
    (a precision / recall / F1 without support is 0, sklearn's zero_division default, as there) + auprc; auroc and auprc are NaN where
    a class has no weight, every score where the replicate has no weight at all."""
    rec = np.asarray(records, dtype=np.int64)
    w, pos, neg = (rec[:, _W[k]].astype(np.float64) for k in ("weight", "pos", "neg"))
    tp, fp, fn, tn = (rec[:, _W[k]].astype(np.float64) for k in ("tp", "fp", "fn", "tn"))
    nan = float("nan")
    out = OrderedDict()
    if with_loss:
        out["loss"] = _safe_div(np.ascontiguousarray(rec[:, _W["loss_bits"]]).view(np.float64), w, nan)
    out["acc"] = _safe_div(tp + tn, w, nan)
    out["F1"] = np.where(w > 0, _safe_div(2 * tp, 2 * tp + fp + fn, 0.0), nan)
    out["recall"] = np.where(w > 0, _safe_div(tp, tp + fn, 0.0), nan)
    out["precision"] = np.where(w > 0, _safe_div(tp, tp + fp, 0.0), nan)
    # the numerator is below 2^63 and a float64 holds 53 bits: divide the exact integers (Python), not their roundings
    out["auroc"] = np.array([int(n) / (2 * int(p) * int(q)) if p and q else nan for n, p, q in
                             zip(rec[:, _W["auroc_num"]].tolist(), rec[:, _W["pos"]].tolist(), rec[:, _W["neg"]].tolist())], dtype=np.float64)
    out["auprc"] = np.where(pos > 0, np.ascontiguousarray(rec[:, _W["ap_bits"]]).view(np.float64), nan)
    return out


def classification_scores_from_records(records):
    """name -> (rows,) float64 from the (rows, C * C) weighted confusion matrices of `ops.boot_classification`: acc and the
    support-weighted F1 / precision / recall of `scores_from_record`"""
    rec = np.asarray(records, dtype=np.int64)
    c = int(round(rec.shape[1] ** 0.5))
    cm = rec.reshape(-1, c, c).astype(np.float64)                        # row = label, column = prediction
    support, predicted, hit = cm.sum(axis=2), cm.sum(axis=1), np.diagonal(cm, axis1=1, axis2=2)
    n = support.sum(axis=1)
    nan = float("nan")
    wk = _safe_div(support, n[:, None], nan)
    return OrderedDict([
        ("acc", _safe_div(hit.sum(axis=1), n, nan)),
        ("F1", (wk * _safe_div(2 * hit, support + predicted, 0.0)).sum(axis=1)),
        ("recall", (wk * _safe_div(hit, support, 0.0)).sum(axis=1)),
        ("precision", (wk * _safe_div(hit, predicted, 0.0)).sum(axis=1))])


class BootstrapResult:
    """The replicates of a bootstrap.  point: OrderedDict of the scores of row 0 (all counts one: the point estimate); samples[name]:
    (n_boot,) float64, NaN where the score is undefined in a replicate; n_undefined[name]: how many are; records: the integer records
    (n_boot + 1, words) on the host; draw: what identifies the resamples (`paired_difference` compares it)."""

    def __init__(self, scores, records, draw):
        self.records = records
        self.point = OrderedDict((k, float(v[0])) for k, v in scores.items())
        self.samples = OrderedDict((k, np.ascontiguousarray(v[1:], dtype=np.float64)) for k, v in scores.items())
        self.n_undefined = OrderedDict((k, int(np.isnan(v).sum())) for k, v in self.samples.items())
        self.n_boot = int(len(next(iter(self.samples.values()))))
        self.draw = draw

    def _defined(self, name, max_undefined, what):
        v = self.samples[name]
        share = self.n_undefined[name] / float(self.n_boot)
        if share > max_undefined:
            raise ValueError(f"{what}: {name} is undefined in {self.n_undefined[name]} of {self.n_boot} replicates ({share:.3f} > max_undefined="
                             f"{max_undefined}): the set has too few clusters of one class for an interval of this score")
        return v[~np.isnan(v)]

    def interval(self, level: float = 0.95, max_undefined: float = 0.05):
        """name -> (lo, hi): the percentile interval of every score over its defined replicates (`numpy.percentile` at 100 * (1 -
        level) / 2 and 100 * (1 + level) / 2).  ValueError when more than `max_undefined` of a score's replicates are undefined."""
        if not 0.0 < level < 1.0:
            raise ValueError(f"BootstrapResult.interval: level={level} outside (0, 1)")
        q = [100.0 * (1.0 - level) / 2.0, 100.0 * (1.0 + level) / 2.0]
        out = OrderedDict()
        for name in self.samples:
            lo, hi = np.percentile(self._defined(name, max_undefined, "BootstrapResult.interval"), q)
            out[name] = (float(lo), float(hi))
        return out

    def se(self, max_undefined: float = 0.05):
        """name -> the bootstrap standard error (standard deviation of the defined replicates, ddof = 1)"""
        out = OrderedDict()
        for name in self.samples:
            v = self._defined(name, max_undefined, "BootstrapResult.se")
            out[name] = float(np.std(v, ddof=1)) if len(v) > 1 else float("nan")
        return out


def paired_difference(a: BootstrapResult, b: BootstrapResult, level: float = 0.95, max_undefined: float = 0.05):
    """Two models on the SAME resamples: per score of both results, OrderedDict(diff = a.point - b.point, lo, hi = the percentile
    interval of a.samples - b.samples, p = the two-sided bootstrap p-value 2 * min(share of differences <= 0, share >= 0), capped at
    1; n_undefined = replicates where either score is undefined).  Refuses results whose draws differ (groups, seed, n_boot, counts)."""
    if a.draw != b.draw:
        raise ValueError(f"paired_difference: the two results were not made on the same resamples ({a.draw} against {b.draw}): "
                         f"use the same groups, seed and n_boot (or the same counts)")
    if not 0.0 < level < 1.0:
        raise ValueError(f"paired_difference: level={level} outside (0, 1)")
    q = [100.0 * (1.0 - level) / 2.0, 100.0 * (1.0 + level) / 2.0]
    out = OrderedDict()
    for name in a.samples:
        if name not in b.samples:
            continue
        d = a.samples[name] - b.samples[name]
        und = int(np.isnan(d).sum())
        if und / float(a.n_boot) > max_undefined:
            raise ValueError(f"paired_difference: {name} is undefined in {und} of {a.n_boot} replicates (max_undefined={max_undefined})")
        d = d[~np.isnan(d)]
        lo, hi = np.percentile(d, q)
        p = min(1.0, 2.0 * min(float(np.mean(d <= 0)), float(np.mean(d >= 0))))
        out[name] = OrderedDict([("diff", a.point[name] - b.point[name]), ("lo", float(lo)), ("hi", float(hi)), ("p", p), ("n_undefined", und)])
    return out


def _check_counts(what, counts, device):
    """explicit counts: (n_boot + 1, G) int32, non-negative, row 0 all ones (row 0 is the point estimate)"""
    counts = torch.as_tensor(counts)
    if counts.dim() != 2 or counts.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: counts must be an integer tensor of shape (n_boot + 1, G), got {counts.dtype} {tuple(counts.shape)}")
    counts = counts.to(device=device, dtype=torch.int32).contiguous()
    if counts.shape[0] < 2 or counts.shape[1] < 1:
        raise ValueError(f"{what}: counts must be (n_boot + 1, G) with n_boot >= 1 and G >= 1, got {tuple(counts.shape)}")
    if int(counts.min()) < 0 or not bool((counts[0] == 1).all()):
        raise ValueError(f"{what}: counts must be non-negative with row 0 all ones (row 0 is the point estimate)")
    return counts


def _draw_key(groups, counts, seed, p):
    """what `paired_difference` compares: the clustering and the counts, by size, seed and two integer checksums each"""
    g = int(counts.shape[1])
    key = [("P", int(p)), ("G", g), ("n_boot", int(counts.shape[0]) - 1), ("seed", seed)]
    if groups is not None:
        pos = torch.arange(1, groups.numel() + 1, device=groups.device, dtype=torch.int64) % 8191 + 1
        key.append(("groups", int((groups.long() * pos).sum())))
    if seed is None:
        rows = counts.sum(dim=1, dtype=torch.int64) * torch.arange(1, counts.shape[0] + 1, device=counts.device, dtype=torch.int64)
        cols = counts.sum(dim=0, dtype=torch.int64) * (torch.arange(1, g + 1, device=counts.device, dtype=torch.int64) % 8191 + 1)
        key.append(("counts", (int(rows.sum()), int(cols.sum()))))
    return tuple(key)


def bootstrap_scores(probs, labels, task: str, groups=None, n_boot: int = 2000, seed: int = 0, best_thresh: float = 0.5, losses=None, counts=None):
    """The clustered bootstrap of the evaluator's scores -> `BootstrapResult`.

    probs (P,) float32 (task "detection") or (P, C) (task "classification") and labels (float32 {0, 1} / int64 classes) on the device,
    as `DeviceEvaluator` leaves them; groups: (P,) integer cluster ids 0..G-1 (G = the largest id + 1; with `counts`, its width) or None:
    every clip its own cluster; counts: explicit (n_boot + 1, G) integer counts with row 0 all ones in place of the draw of
    `ops.boot_counts(G, n_boot, seed)`.  detection: the predictions are (double)prob > best_thresh, held fixed over the replicates;
    scores loss (with `losses` (P,) float32), acc, F1, recall, precision, auroc, auprc.  classification: acc, F1, recall, precision
    (support-weighted).  Limits (ValueError before any launch): P <= ops.EVAL_MAX_CLIPS, 1 <= G <= ops.BOOT_MAX_GROUPS, 1 <= n_boot <=
    ops.BOOT_MAX_REPLICATES, 0 <= groups[i] < G, G * (largest cluster) < 2^31, best_thresh not NaN."""
    what = "bootstrap_scores"
    if task not in ("detection", "classification"):
        raise ValueError(f"{what}: task={task!r} (detection or classification)")
    if not torch.is_tensor(probs) or probs.dim() != (1 if task == "detection" else 2) or probs.shape[0] < 1:
        got = f"{tuple(probs.shape)}" if torch.is_tensor(probs) else type(probs).__name__
        raise ValueError(f"{what}: probs must be a (P,) (detection) or (P, C) (classification) tensor, got {got}")
    p, dev = int(probs.shape[0]), probs.device
    if p > ops.EVAL_MAX_CLIPS:
        raise ValueError(f"{what}: P={p} clips exceed the limit of one call, {ops.EVAL_MAX_CLIPS} (ops.EVAL_MAX_CLIPS)")
    if best_thresh != best_thresh:
        raise ValueError(f"{what}: best_thresh is NaN")
    label_dtype = torch.float32 if task == "detection" else torch.int64
    for name, t, dtype, shape in (("probs", probs, torch.float32, tuple(probs.shape)), ("labels", labels, label_dtype, (p,)),
                                  ("losses", losses, torch.float32, (p,))):
        if t is not None and (not torch.is_tensor(t) or t.device != dev or tuple(t.shape) != shape or t.dtype != dtype):
            got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if torch.is_tensor(t) else type(t).__name__
            raise ValueError(f"{what}: {name} must be a {dtype} tensor of shape {shape} on {dev}, got {got}")
    if groups is not None:
        groups = torch.as_tensor(groups)
        if groups.dim() != 1 or groups.numel() != p or groups.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{what}: groups must be an integer tensor of shape ({p},), got {groups.dtype} {tuple(groups.shape)}")
        lo, hi = int(groups.min()), int(groups.max())
        groups = groups.to(device=dev, dtype=torch.int32).contiguous()
    if counts is not None:
        counts = _check_counts(what, counts, dev)
        g, n_boot, seed = int(counts.shape[1]), int(counts.shape[0]) - 1, None
    else:
        g = p if groups is None else hi + 1
    if groups is not None and (lo < 0 or hi >= g):
        raise ValueError(f"{what}: groups holds cluster ids {lo}..{hi}, outside 0..G-1 = {g - 1}")
    if groups is None and g != p:
        raise ValueError(f"{what}: groups is None (every clip its own cluster): counts rows must be P={p} wide, got {g}")
    if not 1 <= g <= ops.BOOT_MAX_GROUPS:
        raise ValueError(f"{what}: G={g} clusters outside 1..{ops.BOOT_MAX_GROUPS} (ops.BOOT_MAX_GROUPS)")
    if not 1 <= int(n_boot) <= ops.BOOT_MAX_REPLICATES:
        raise ValueError(f"{what}: n_boot={n_boot} replicates outside 1..{ops.BOOT_MAX_REPLICATES} (ops.BOOT_MAX_REPLICATES)")
    largest = 1 if groups is None else int(torch.bincount(groups.long()).max())
    weight = g * largest if counts is None else int(counts.sum(dim=1, dtype=torch.int64).max()) * largest
    if weight >= 1 << 31:
        raise ValueError(f"{what}: G={g} clusters, the largest of {largest} clips: a replicate can weigh {weight} >= 2^31; use fewer, smaller clusters")
    # the evaluator raises on such a pool (scores_from_record); here it is refused before the kernels see it
    if task == "detection":
        ok = bool(((probs >= 0) & (probs <= 1)).all()) and bool(((labels == 0) | (labels == 1)).all())
    else:
        ok = bool(((probs >= 0) & (probs <= 1)).all()) and bool(((labels >= 0) & (labels < probs.shape[1])).all())
    if not ok:
        raise ValueError(f"{what}: labels outside the task's classes or probabilities outside [0, 1] (or NaN) among {p} clips")
    if counts is None:
        counts = ops.boot_counts(g, int(n_boot), int(seed), dev)
    # (explicit counts may sum to more than G per row: the weight bound above is what the kernels need)
    max_cluster = max(1, min(largest, ((1 << 31) - 1) // g))
    if task == "detection":
        records = ops.boot_detection(probs, labels, groups, counts, float(best_thresh), losses, max_cluster=max_cluster).cpu().numpy()
        scores = detection_scores_from_records(records, losses is not None)
    else:
        records = ops.boot_classification(probs, labels, groups, counts, max_cluster=max_cluster).cpu().numpy()
        scores = classification_scores_from_records(records)
    return BootstrapResult(scores, records, _draw_key(groups, counts, seed, p))


def bootstrap_scan(result, n_boot: int = 2000, seed: int = 0, groups=None):
    """`ScanResult.bootstrap`: resample the R recordings of a scan (or patients through groups (R,): integer ids 0..G-1) and score
    every replicate's summed record with `scores_from_scan_record`."""
    from .scan import scores_from_scan_record
    what = "ScanResult.bootstrap"
    if result.scores is None:
        raise ValueError(f"{what}: the scan has no annotations: there are no scores to resample")
    recs = result.rec_records
    r, dev = int(recs.shape[0]), recs.device
    if groups is not None:
        groups = torch.as_tensor(groups)
        if groups.dim() != 1 or groups.numel() != r or groups.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{what}: groups must be an integer tensor of shape ({r},), got {groups.dtype} {tuple(groups.shape)}")
        lo, hi = int(groups.min()), int(groups.max())
        if lo < 0:
            raise ValueError(f"{what}: groups holds cluster ids {lo}..{hi}, outside 0..G-1")
        groups = groups.to(device=dev, dtype=torch.int32).contiguous()
        recs = torch.zeros((hi + 1, recs.shape[1]), dtype=torch.int64, device=dev).index_add_(0, groups.long(), recs)
    g = int(recs.shape[0])
    if not 1 <= g <= ops.BOOT_MAX_GROUPS:
        raise ValueError(f"{what}: G={g} clusters outside 1..{ops.BOOT_MAX_GROUPS} (ops.BOOT_MAX_GROUPS)")
    if not 1 <= int(n_boot) <= ops.BOOT_MAX_REPLICATES:
        raise ValueError(f"{what}: n_boot={n_boot} replicates outside 1..{ops.BOOT_MAX_REPLICATES} (ops.BOOT_MAX_REPLICATES)")
    counts = ops.boot_counts(g, int(n_boot), int(seed), dev)
    records = ops.boot_records(recs.contiguous(), counts).cpu().numpy()
    rows = [scores_from_scan_record(row.tolist(), result.window, result.freq) for row in records]
    scores = OrderedDict((k, np.array([float(row[k]) for row in rows], dtype=np.float64)) for k in rows[0])
    return BootstrapResult(scores, records, _draw_key(groups, counts, int(seed), r))
