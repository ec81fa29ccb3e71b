"""dev aid (GPU box): wall-clock timing of the clustered bootstrap of the scores (eeg_gnn_ssl_amd/bootstrap.py, csrc/kernels_boot.h) on
synthetic pools: P = 2^16 and 2^20 clips, G = P / 64 clusters and G = P (every clip its own), n_boot = 2000 replicates.  Candidates:
    boot_counts          `ops.boot_counts(G, n_boot, seed)`
    boot_detection       `ops.boot_detection` on drawn counts, without and with the per-clip losses (sort + pack + one workgroup per
                         replicate); per replicate the bytes it streams (two passes over the packed words, the counts row, with losses
                         the losses and the cluster ids) against the measured time
    boot_classification  `ops.boot_classification`, C = 4
    aten                 the same AUROC numerators and average precisions from ATen kernels on the same device: ONE `torch.sort`, then
                         per chunk of replicates the gathered weights and `cumsum` along the sorted order (ties through the run bounds,
                         found once); its results are compared with the kernel's before anything is timed
    sklearn              `roc_auc_score` + `average_precision_score(sample_weight=)` on the host for --sk-reps replicates: the cost of
                         ONE replicate (the probabilities are copied to the host once, outside the clock)
A call ends in a synchronisation, so a host clock around it measures it whole.  Fresh process, every candidate warmed once, `--rounds`
rounds alternating between the device candidates; median and spread (min..max).
usage: python tools/time_boot_ops.py [--rounds 5] [--n-boot 2000] [--sk-reps 3] [--out profiles/boot_ops.txt]"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from eeg_gnn_ssl_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--n-boot", type=int, default=2000)
ap.add_argument("--sk-reps", type=int, default=3)
ap.add_argument("--seed", type=int, default=11)
ap.add_argument("--pools", type=int, nargs="+", default=[1 << 16, 1 << 20])
ap.add_argument("--aten-chunk", type=int, default=16)
ap.add_argument("--out", default=None)
opt = ap.parse_args()

assert torch.cuda.is_available(), "time_boot_ops.py measures on an MI355X; there is no other path"
warnings.simplefilter("ignore")
dev = "cuda"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(cands, rounds):
    for fn in cands.values():
        fn()
    got = {name: [] for name in cands}
    for _ in range(rounds):
        for name, fn in cands.items():
            got[name].append(timed(fn))
    return {name: dict(median=statistics.median(v), min=min(v), max=max(v)) for name, v in got.items()}


def aten_detection(probs, labels, groups, counts, chunk):
    """-> (AUROC numerators int64 (rows,), average precisions float64 (rows,)) with ATen kernels: one sort, cumsums per chunk of rows"""
    order = torch.sort(probs, stable=True).indices
    sp, lab = probs[order], labels[order] == 1
    grp = order if groups is None else groups.long()[order]
    p = sp.numel()
    idx = torch.arange(p, device=sp.device)
    is_start = torch.ones(p, dtype=torch.bool, device=sp.device)
    is_start[1:] = sp[1:] != sp[:-1]
    start = torch.cummax(torch.where(is_start, idx, torch.zeros_like(idx)), 0).values                     # first index of the clip's run
    is_end = torch.ones(p, dtype=torch.bool, device=sp.device)
    is_end[:-1] = is_start[1:]
    end = torch.flip(torch.cummin(torch.flip(torch.where(is_end, idx, torch.full_like(idx, p)), [0]), 0).values, [0])     # last index of it
    nums, aps = [], []
    for r0 in range(0, counts.shape[0], chunk):
        w = counts[r0:r0 + chunk].long()[:, grp]
        posw, negw = w * lab, w * ~lab
        cpos, cneg = torch.cumsum(posw, 1), torch.cumsum(negw, 1)
        w_pos, w_neg = cpos[:, -1:], cneg[:, -1:]
        nb = (cneg - negw)[:, start]                                     # negative weight below the run
        pb = (cpos - posw)[:, start]
        n_in = cneg[:, end] - nb
        nums.append((posw * (2 * nb + n_in)).sum(1))
        tp, fp = (w_pos - pb).double(), (w_neg - nb).double()
        aps.append((posw.double() * (tp / (tp + fp).clamp_min(1.0))).sum(1) / w_pos[:, 0].double())
    return torch.cat(nums), torch.cat(aps)


result = {"device": torch.cuda.get_device_name(0), "command": f"python tools/time_boot_ops.py --rounds {opt.rounds} --n-boot {opt.n_boot} --sk-reps {opt.sk_reps} --seed {opt.seed} --pools " +
          " ".join(str(v) for v in opt.pools) + f" --aten-chunk {opt.aten_chunk}",
          "rounds": opt.rounds, "n_boot": opt.n_boot, "unit": "ms per call of n_boot + 1 replicates, host clock around a call that ends in a synchronisation",
          "shapes": []}
rows = opt.n_boot + 1
for p in opt.pools:
    g0 = torch.Generator(device=dev).manual_seed(opt.seed)
    probs = torch.rand(p, generator=g0, device=dev)
    labels = (torch.rand(p, generator=g0, device=dev) < 0.1 + 0.3 * probs).float()      # imbalanced, informative
    losses = torch.rand(p, generator=g0, device=dev)
    cprobs = torch.softmax(torch.randn(p, 4, generator=g0, device=dev), 1)
    clabels = torch.randint(0, 4, (p,), generator=g0, device=dev)
    for g in (p // 64, p):
        groups = None if g == p else (torch.arange(p, device=dev) // 64).int()
        largest = 1 if g == p else 64
        counts = ops.boot_counts(g, opt.n_boot, opt.seed, dev)
        ws = ops.boot_workspace(p, dev)
        rec = ops.boot_detection(probs, labels, groups, counts, 0.5, losses, ws=ws, max_cluster=largest)
        # the ATen composition computes what the kernel computes
        check_rows = min(rows, 2 * opt.aten_chunk)
        a_num, a_ap = aten_detection(probs, labels, groups, counts[:check_rows], opt.aten_chunk)
        k_ap = rec[:check_rows, 8].contiguous().view(torch.float64)
        assert torch.equal(a_num, rec[:check_rows, 3]), "the ATen composition and boot_detection disagree on the AUROC numerator"
        ap_diff = float((a_ap - k_ap).abs().max())
        assert ap_diff <= 2.0 ** -32, ap_diff
        dev_ms = alternate({
            "boot_counts": lambda: ops.boot_counts(g, opt.n_boot, opt.seed, dev),
            "boot_detection": lambda: ops.boot_detection(probs, labels, groups, counts, 0.5, None, ws=ws, max_cluster=largest),
            "boot_detection_with_losses": lambda: ops.boot_detection(probs, labels, groups, counts, 0.5, losses, ws=ws, max_cluster=largest),
            "boot_classification": lambda: ops.boot_classification(cprobs, clabels, groups, counts, ws=ws, max_cluster=largest),
            "aten": lambda: aten_detection(probs, labels, groups, counts, opt.aten_chunk),
        }, opt.rounds)
        # the sort and the pack alone: a call of one replicate
        one = ops.boot_counts(g, 1, opt.seed, dev)
        dev_ms["boot_detection_two_rows"] = alternate({"x": lambda: ops.boot_detection(probs, labels, groups, one, 0.5, None, ws=ws, max_cluster=largest)},
                                                      opt.rounds)["x"]
        words = ((p + 1023) // 1024) * 1024
        stream = 2 * 4 * words + 4 * g                                   # two passes over the packed words + the counts row
        stream_l = stream + 4 * p + (4 * p if groups is not None else 0)
        per_rep = (dev_ms["boot_detection"]["median"] - dev_ms["boot_detection_two_rows"]["median"]) / (rows - 2)
        per_rep_l = (dev_ms["boot_detection_with_losses"]["median"] - dev_ms["boot_detection_two_rows"]["median"]) / (rows - 2)
        # sklearn on the host
        from sklearn.metrics import average_precision_score, roc_auc_score
        y, pr = labels.cpu().numpy().astype(int), probs.cpu().numpy().astype(np.float64)
        grp = np.arange(p) if groups is None else groups.cpu().numpy()
        host_counts = counts[1:1 + opt.sk_reps].cpu().numpy()
        rec_host = rec.cpu().numpy()
        sk = []
        for r in range(opt.sk_reps):
            t0 = time.perf_counter()
            w = host_counts[r][grp]
            auc, apv = roc_auc_score(y, pr, sample_weight=w), average_precision_score(y, pr, sample_weight=w)
            sk.append((time.perf_counter() - t0) * 1e3)
            row = rec_host[r + 1]
            assert abs(auc - int(row[3]) / (2 * int(row[1]) * int(row[2]))) <= 1e-9 and abs(apv - row[8:9].view(np.float64)[0]) <= 1e-9
        result["shapes"].append({
            "P": p, "G": g, "counts_in_lds": g <= ops.BOOT_LDS_GROUPS, "ms": dev_ms,
            "ap_max_abs_difference_aten_to_kernel": ap_diff,
            "bytes_streamed_per_replicate": stream, "us_per_replicate": per_rep * 1e3, "stream_GB_per_s": stream * 1e-6 / per_rep,
            "with_losses": {"bytes_streamed_per_replicate": stream_l, "us_per_replicate": per_rep_l * 1e3, "stream_GB_per_s": stream_l * 1e-6 / per_rep_l},
            "boot_detection_over_aten": dev_ms["boot_detection"]["median"] / dev_ms["aten"]["median"],
            "sklearn_ms_per_replicate": dict(median=statistics.median(sk), min=min(sk), max=max(sk), replicates=opt.sk_reps),
            "sklearn_ms_for_n_boot_extrapolated": statistics.median(sk) * opt.n_boot})
        del counts, rec
        torch.cuda.empty_cache()
text = json.dumps(result, indent=1)
print(text)
if opt.out:
    with open(opt.out, "w") as f:
        f.write(text + "\n")
