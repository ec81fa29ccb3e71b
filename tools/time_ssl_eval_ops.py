"""dev aid (GPU box): wall-clock timing of one SSL evaluation pass over a device-resident dev set (eeg_gnn_ssl_amd/evaluation.py:
DeviceSSLEvaluator, csrc/kernels_eval.h) at cfg5's shapes: 60 s in, 12 s out, correlation graphs, B = 512, a pool of --pool clips
(default 2048).  Candidates, each a whole pass from the first launch to the loss on the host:
    evaluate_ssl        `evaluate_ssl(model, ds.batches(B), mean, std)` over the ready feature pool: eager forwards, the float32 loss
                        kernel per batch.  The code of the parent commit, unchanged here: its number is the parent's.
    evaluator_eager     `DeviceSSLEvaluator.run(capture=False)`, same feature pool
    evaluator_captured  `DeviceSSLEvaluator.run(capture=True)` (the graph captured before the timed rounds), same feature pool
    raw_eager / raw_captured   the same two from a RAW pool (P, 19, 60 * 200) / (P, 19, 12 * 200) through `fft_features_pair`: what
                        `evaluate_ssl` cannot be handed
and the scores kernel alone (`ops.ssl_eval_scores`, one batch per launch out of six in rotation so that none is served from the
Infinity Cache, device events around --reps launches) against the time its bytes, 2 * B * Ty * N * D * 4, take at the achievable HBM
rate (6.3 TB/s).
A pass ends in a device-to-host copy, so a host clock around it measures it whole.  Fresh process, every candidate warmed, `--rounds`
rounds alternating between the candidates; median and spread (min..max) over the rounds.  The passes' results are compared before
anything is timed.
usage: python tools/time_ssl_eval_ops.py [--rounds 7] [--seed 11] [--pool 2048] [--out profiles/ssl_eval_ops.txt]"""
import argparse
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402  (workload table, model arguments)
from eeg_gnn_ssl_amd import DCRNNModel_nextTimePred, DeviceDataset, ops  # noqa: E402
from eeg_gnn_ssl_amd.train_step import TrainStep, evaluate_ssl  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--seed", type=int, default=11)
ap.add_argument("--pool", type=int, default=2048)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--out", default=None)
opt = ap.parse_args()

assert torch.cuda.is_available(), "time_ssl_eval_ops.py measures on an MI355X; there is no other path"
warnings.simplefilter("ignore")
HBM_BYTES_PER_S = 6.3e12          # achievable (float4 copy), not the 8 TB/s of the data sheet
dev = "cuda"
task, filt, t_in, B, _ = bench.WORKLOADS["cfg5"]
t_out, n, d, w = bench.T_OUT, 19, 100, bench.RAW_WINDOW
MEAN, STD = 5.68, 0.87            # the scaler of bench.py's synthetic raw signals
g = torch.Generator(device=dev).manual_seed(opt.seed)
torch.manual_seed(opt.seed)
model = DCRNNModel_nextTimePred(bench.make_args(filt), device=dev).to(dev).train()
feat = DeviceDataset(torch.randn(opt.pool, t_in, n, d, generator=g, device=dev), torch.randn(opt.pool, t_out, n, d, generator=g, device=dev))
raw = DeviceDataset(20.0 * torch.randn(opt.pool, n, t_in * w, generator=g, device=dev), 20.0 * torch.randn(opt.pool, n, t_out * w, generator=g, device=dev))
st_feat = TrainStep(model, task=task, scaler_mean=MEAN, scaler_std=STD)
st_raw = TrainStep(model, task=task, scaler_mean=MEAN, scaler_std=STD, raw_window=w, raw_mean=MEAN, raw_std=STD)
ev_eager, ev_graph = st_feat.ssl_evaluator(feat, B), st_feat.ssl_evaluator(feat, B)
raw_eager, raw_graph = st_raw.ssl_evaluator(raw, B), st_raw.ssl_evaluator(raw, B)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(cands, rounds):
    for fn in cands.values():
        for _ in range(2):
            fn()
    got = {name: [] for name in cands}
    for _ in range(rounds):
        for name, fn in cands.items():
            got[name].append(timed(fn))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in got.items()}


def parent():
    return evaluate_ssl(model, feat.batches(B), MEAN, STD)


want = parent()
got_e, got_g = ev_eager.run(capture=False), ev_graph.run(capture=True)
assert got_e == got_g and torch.equal(ev_eager._scores, ev_graph._scores), (got_e, got_g)
assert abs(got_g - want) <= 2e-5 * abs(want), (got_g, want)
raw_e, raw_g = raw_eager.run(capture=False), raw_graph.run(capture=True)
assert raw_e == raw_g and torch.equal(raw_eager._scores, raw_graph._scores), (raw_e, raw_g)
res = alternate({"evaluate_ssl": parent, "evaluator_eager": lambda: ev_eager.run(capture=False), "evaluator_captured": lambda: ev_graph.run(capture=True),
                 "raw_eager": lambda: raw_eager.run(capture=False), "raw_captured": lambda: raw_graph.run(capture=True)}, opt.rounds)

# the scores kernel alone: device events around `reps` launches that rotate over ROTATE batches (together above the 256 MiB the
# Infinity Cache holds, so that every launch reads from HBM); the cursor stays put: every launch writes the same slots
ROTATE = 6
batches = [(torch.randn(B, t_out, n, d, generator=g, device=dev), torch.randn(B, t_out, n, d, generator=g, device=dev)) for _ in range(ROTATE)]
clip_w, cursor = torch.ones(B, device=dev), torch.tensor([B], dtype=torch.int64, device=dev)
scores, _, keep = ops.ssl_eval_buffers(opt.pool, dev, (t_out, n, d))


def kernel_us(keep_buf):
    for i in range(10):
        ops.ssl_eval_scores(*batches[i % ROTATE], clip_w, cursor, scores, mean=MEAN, std=STD, keep=keep_buf)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(opt.reps):
        ops.ssl_eval_scores(*batches[i % ROTATE], clip_w, cursor, scores, mean=MEAN, std=STD, keep=keep_buf)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / opt.reps


k_us = [kernel_us(None) for _ in range(opt.rounds)]
k_keep_us = [kernel_us(keep) for _ in range(opt.rounds)]
nbytes = 2 * B * t_out * n * d * 4
floor_us = nbytes / HBM_BYTES_PER_S * 1e6
base = res["evaluate_ssl"]
lines = [f"device: {torch.cuda.get_device_name(0)}; cfg5 shapes: B = {B}, pool of {opt.pool} clips ({ev_graph.sampler.steps_per_epoch} steps per pass), "
         f"{t_in} s in, {t_out} s out, N = {n}, D = {d}; rounds = {opt.rounds}, seed = {opt.seed}",
         f"loss: evaluate_ssl {want!r}, evaluator (eager = captured) {got_g!r}, rel. difference {abs(got_g - want) / abs(want):.2e}; raw pool {raw_g!r}",
         "ms per pass (host clock around a pass that ends in a device-to-host copy): median (min .. max), ratio to evaluate_ssl's median"]
for name, (med, lo, hi) in res.items():
    lines.append(f"  {name:<20s} {med:9.3f} ({lo:9.3f} .. {hi:9.3f})  {med / base[0]:6.3f}")
lines += [f"spread of evaluate_ssl over the rounds: {(base[2] - base[1]) / base[0] * 100:.2f} % of its median",
          f"ssl_eval_scores alone, one batch per launch ({nbytes / 1e6:.1f} MB read, {ROTATE} batches in rotation; back-to-back launches, device events, "
          f"us per launch over {opt.reps}): "
          f"median {statistics.median(k_us):.2f} (min {min(k_us):.2f} .. max {max(k_us):.2f}); {floor_us:.2f} us at {HBM_BYTES_PER_S / 1e12:.1f} TB/s: "
          f"{floor_us / statistics.median(k_us) * 100:.0f} % of the achievable HBM rate",
          f"  with keep (+{nbytes / 2e6:.1f} MB written): median {statistics.median(k_keep_us):.2f} (min {min(k_keep_us):.2f} .. max {max(k_keep_us):.2f}); "
          f"{1.5 * floor_us:.2f} us at that rate"]
text = "\n".join(lines)
print(text)
if opt.out:
    with open(opt.out, "w") as f:
        f.write(text + "\n")
