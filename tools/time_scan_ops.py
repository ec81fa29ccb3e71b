"""dev aid (GPU box): timing of whole-recording scans (eeg_gnn_ssl_amd/scan.py, csrc/kernels_scan.h) at a user's size: --recordings
(64) recordings of --minutes (20) at 200 Hz, the cfg2 / cfg3 detector (2 x 64 units, T = 60, raw signals -> log|FFT|), B = 256, windows
every 1 s and every 12 s, with the distance graph and with supports=None (correlation graphs).  Per case, after a warm-up:
    pass_captured   the captured pass alone: `Scanner._replay(True)`, device events around `--passes` passes
    postprocess     `Scanner.postprocess` (three kernels + the one copy of the record), device events around enough calls to fill a
                    fraction of a second
    host_numpy      the same post-processing the way a user does it without these kernels: `clip_probs.cpu()` + the numpy
                    restatement below (overlap mean by np.bincount, smoothing, hysteresis, merge, minimum length, any-overlap and
                    bin scores), host clock
The numpy path's events and record are compared with the kernels' before anything is timed.  Nothing here is a gate.
usage: python tools/time_scan_ops.py [--recordings 64] [--minutes 20] [--passes 2] [--out profiles/scan_ops.txt]"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402  (workload table, model arguments, the distance graph)
from eeg_gnn_ssl_amd import DCRNNModel_classification, annotation_bins, layout_recordings, ops  # noqa: E402
from eeg_gnn_ssl_amd.train_step import TrainStep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--recordings", type=int, default=64)
ap.add_argument("--minutes", type=float, default=20.0)
ap.add_argument("--passes", type=int, default=2)
ap.add_argument("--seed", type=int, default=11)
ap.add_argument("--out", default=None)
opt = ap.parse_args()

assert torch.cuda.is_available(), "time_scan_ops.py measures on an MI355X; there is no other path"
warnings.simplefilter("ignore")
dev, W, T, B, FREQ = "cuda", bench.RAW_WINDOW, 60, 256, 200
POST = dict(agg="mean", smooth_bins=5, th_on=0.55, th_off=0.45, merge_gap=2, min_bins=3)
samples = int(opt.minutes * 60 * FREQ)
g = torch.Generator(device=dev).manual_seed(opt.seed)
signals, rec_table = layout_recordings([torch.randn(19, samples, generator=g, device=dev) * (1.0 + 0.5 * (r % 3)) for r in range(opt.recordings)], dev)
rng = np.random.default_rng(opt.seed)
seizures = [sorted((float(a), float(a + d)) for a, d in zip(rng.uniform(0, opt.minutes * 60 - 90, 3), rng.uniform(10, 90, 3))) for _ in range(opt.recordings)]
ann = annotation_bins(seizures, [samples] * opt.recordings, W, FREQ)


def host_numpy(probs, table, clip_off, steps, ref, ref_count, agg, smooth_bins, th_on, th_off, merge_gap, min_bins):
    """what a user writes today: numpy over the clip probabilities -> (events per recording, the ten-word record)"""
    th_on, th_off, h = np.float32(th_on), np.float32(th_off), (smooth_bins - 1) // 2
    events, rec = [], np.zeros(10, dtype=np.int64)
    for r, s_r in enumerate(steps):
        rows = slice(int(clip_off[r]), int(clip_off[r + 1]))
        starts, p = table[rows, 1] // W, probs[rows]
        idx = (starts[:, None] + np.arange(T)[None, :]).reshape(-1)
        cover = np.bincount(idx, minlength=s_r)[:s_r]
        if agg == "mean":
            tl = np.bincount(idx, weights=np.repeat(p, T), minlength=s_r)[:s_r] / np.maximum(cover, 1)
        else:
            tl = np.zeros(s_r)
            np.maximum.at(tl, idx, np.repeat(p, T))
        cov = cover > 0
        num = np.convolve(np.where(cov, tl, 0.0), np.ones(smooth_bins), "same")
        q = np.where(cov, num / np.maximum(np.convolve(cov.astype(np.float64), np.ones(smooth_bins), "same"), 1), 0.0).astype(np.float32)
        code = np.where(~cov | (q < th_off), 1, 0)
        code = np.where(cov & (q >= th_on), 2, code)                      # 0 keep, 1 off, 2 on
        last = np.maximum.accumulate(np.where(code > 0, np.arange(s_r), -1))
        on = np.where(last >= 0, code[np.maximum(last, 0)] == 2, False)
        edge = np.diff(np.concatenate([[0], on.astype(np.int8), [0]]))
        runs = list(zip(np.nonzero(edge == 1)[0].tolist(), np.nonzero(edge == -1)[0].tolist()))
        merged = []
        for a, b in runs:
            if merged and a - merged[-1][1] <= merge_gap:
                merged[-1] = (merged[-1][0], b)
            else:
                merged.append((a, b))
        ev = [(a, b) for a, b in merged if b - a >= min_bins]
        events.append(ev)
        refs = [tuple(x) for x in ref[r, :ref_count[r]].tolist()]
        pos, pred = np.zeros(s_r, dtype=bool), np.zeros(s_r, dtype=bool)
        for a, b in refs:
            pos[a:b] = True
        for a, b in ev:
            pred[a:b] = True
        over = lambda x, ys: any(max(x[0], y[0]) < min(x[1], y[1]) for y in ys)     # noqa: E731
        rec += [len(refs), len(ev), sum(over(x, ev) for x in refs), sum(over(x, refs) for x in ev), int(cov.sum()), int((pos & pred & cov).sum()),
                int((~pos & pred & cov).sum()), int((pos & ~pred & cov).sum()), int((~pos & ~pred & cov).sum()), 0]
    return events, rec


def device_ms(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


result = {"device": torch.cuda.get_device_name(0), "recordings": opt.recordings, "minutes": opt.minutes, "x_steps": T, "batch": B, "post": POST,
          "unit": "ms", "cases": {}}
for graph in ("distance", "none"):
    task, filt, _, _, classes = bench.WORKLOADS["cfg2" if graph == "distance" else "cfg3"]
    torch.manual_seed(opt.seed)
    model = DCRNNModel_classification(bench.make_args(filt), classes, device=dev).to(dev).eval()
    st = TrainStep(model, task=task, raw_window=W, raw_mean=0.0, raw_std=1.0)
    supports = None
    if graph == "distance":
        _, _, _, hs = bench.synthetic_batch(task, filt, T, B, classes, seed=opt.seed)
        supports = ops.collapse_shared_supports([s.to(dev) for s in hs])
    for stride in (12, 1):
        sc = st.scanner((signals, rec_table, 19), x_steps=T, stride_steps=stride, batch_size=B, supports=supports, max_events=256)
        res = sc.run(annotations=ann, **POST)                              # captures, warms up
        sc.run(annotations=ann, **POST)
        table, clip_off = sc.dataset.clip_table.cpu().numpy(), sc.clip_off.cpu().numpy()
        ev_h, rec_h = host_numpy(res.clip_probs.cpu().numpy(), table, clip_off, sc.rec_steps, ann[0], ann[1], **POST)
        counts = res.event_count.cpu().tolist()
        ev_d = [[tuple(e) for e in res.events[r, :counts[r]].cpu().tolist()] for r in range(opt.recordings)]
        agree = ev_d == ev_h and res.record.tolist() == [int(v) for v in rec_h]     # (float64 numpy sums: a q within rounding of a threshold may differ)

        def replay():
            sc._replay(True)

        pass_ms = device_ms(replay, opt.passes)
        one = device_ms(lambda: sc.postprocess(annotations=ann, **POST), 3)
        post_ms = device_ms(lambda: sc.postprocess(annotations=ann, **POST), max(5, int(300.0 / max(one, 0.05))))
        times = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_numpy(sc.probs.cpu().numpy(), table, clip_off, sc.rec_steps, ann[0], ann[1], **POST)
            times.append((time.perf_counter() - t0) * 1e3)
        result["cases"][f"graph={graph},stride={stride}s"] = {
            "windows": len(sc.dataset), "steps_per_pass": sc.sampler.steps_per_epoch, "bins": sum(sc.rec_steps), "events": int(res.record[1]),
            "host_numpy_agrees": bool(agree), "pass_captured_ms": pass_ms, "windows_per_s": len(sc.dataset) / pass_ms * 1e3,
            "postprocess_ms": post_ms, "host_numpy_ms": float(np.median(times)), "postprocess_over_host_numpy": post_ms / float(np.median(times)),
            "scores": dict(res.scores)}
        print(json.dumps({k: v for k, v in result["cases"][f"graph={graph},stride={stride}s"].items() if k != "scores"}), flush=True)
text = json.dumps(result, indent=1)
print(text)
if opt.out:
    with open(opt.out, "w") as f:
        f.write(text + "\n")
