"""dev aid (GPU box): HIP-event timing of clips cut out of device-resident recordings (eeg_gnn_ssl_amd/device_data.py: RecordingDataset,
csrc/kernels_records.h), by the protocol of tools/time_epoch_ops.py.
  (a) one batch of B = 256 raw clips (19, 12000) plus the (19, 2400) SSL target out of --recs recordings of 19 x --samples samples:
        `ops.gather_records` on the aligned path (every start a multiple of 4 samples: 16-byte loads);
        `ops.gather_records` with every start = 1 mod 4 (dword loads through LDS);
        `ops.gather_clips` on the pre-cut pools of the same (aligned) clips -- the yardstick: unchanged code that moves the same bytes
        in the same 16-byte pieces -- and, with --lib PATH, the same call on ANOTHER build of the library (the parent commit's).
      TB/s of 2 x batch bytes (one read, one write); the cursor is zeroed once per epoch of the table, as `begin_epoch` does.  The
      aligned path is expected within the yardstick's max-of-rounds plus 10 % (two table reads per block, 19 row descriptors per
      clip instead of one); the unaligned path has no bar.
  (b) the captured raw detection step (correlation graphs, T = 60, B = 256, optimiser tail inside the graph) and the captured SSL pair
      step (T = 60 + 12) from a `RecordingDataset` against the same step from the pre-cut `DeviceDataset`; `begin_epoch` once per
      epoch inside the timed loop.  The steps behind the gather are the same launches: the two should agree within their spreads.
Every figure: warm, `--rounds` rounds alternating between the candidates, each round ~0.1 s per candidate (steps: 20 steps); median
and spread (min..max) over the rounds.
usage: python tools/time_record_ops.py [--lib PATH] [--rounds 7] [--seed 11] [--out profiles/record_pool_time.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402  (model arguments)
from eeg_gnn_ssl_amd import (DCRNNModel_classification, DCRNNModel_nextTimePred, DeviceDataset, EpochSampler, RecordingDataset, _lib,  # noqa: E402
                             clip_table_ssl)
from eeg_gnn_ssl_amd.train_step import TrainStep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None, help="another build of libeeg_dcrnn_hip.so on which gather_clips is timed beside this tree's")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--seed", type=int, default=11)
ap.add_argument("--recs", type=int, default=16)
ap.add_argument("--samples", type=int, default=240000, help="samples per recording (20 min at 200 Hz)")
ap.add_argument("--pool", type=int, default=2048, help="clips in the table")
ap.add_argument("--skip-steps", action="store_true")
ap.add_argument("--out", default=None)
opt = ap.parse_args()

dev = "cuda"
B, N, T, W, TY, POOL = 256, 19, 60, 200, 12, opt.pool
EPOCH = POOL // B
other = _lib.EegDcrnnLib(opt.lib, strict=False) if opt.lib else None


def ms_per_call(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(cands, rounds, reps=None):
    """cands: {name: callable}; returns {name: (median ms, min ms, max ms)} over alternating rounds"""
    n = {}
    for name, fn in cands.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        n[name] = reps or max(5, int(100.0 / max(ms_per_call(fn, 5), 1e-3)))            # ~0.1 s per round
    got = {name: [] for name in cands}
    for _ in range(rounds):
        for name, fn in cands.items():
            got[name].append(ms_per_call(fn, n[name]))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in got.items()}


def with_lib(lib, fn):
    def run(*a, **k):
        keep = _lib._LIB
        _lib._LIB = lib
        try:
            return fn(*a, **k)
        finally:
            _lib._LIB = keep
    return run


def stats(res):
    return {k: dict(median=v[0], min=v[1], max=v[2]) for k, v in res.items()}


result = {"device": torch.cuda.get_device_name(0), "rounds": opt.rounds, "seed": opt.seed, "recordings": opt.recs, "samples": opt.samples,
          "table_clips": POOL, "batch": B, "other_lib": opt.lib}
g = torch.Generator(device=dev).manual_seed(opt.seed)
rng = np.random.RandomState(opt.seed)
recordings = [torch.randn(N, opt.samples, generator=g, device=dev) * 20.0 for _ in range(opt.recs)]
clips_per_rec = opt.samples // (T * W) - 1                         # (the target is the head of the following clip)
rec_ids = rng.randint(0, opt.recs, POOL)
clip_idx = rng.randint(0, clips_per_rec, POOL)
table = clip_table_ssl(rec_ids, clip_idx, clip_idx + 1, T)          # 60-s clips, the target cut to TY steps by the data set
odd = table.copy()
odd[:, 1] += 1
odd[:, 3] += 1
ssl_ds = RecordingDataset(recordings, table, None, window=W, x_steps=T, y_steps=TY, device=dev)
odd_ds = RecordingDataset(ssl_ds.signals, odd, None, window=W, x_steps=T, y_steps=TY, rec_table=ssl_ds.rec_table, num_channels=N)
x_pool = torch.stack([recordings[r][:, s:s + T * W] for r, s in zip(table[:, 0], table[:, 1])])
y_pool = torch.stack([recordings[r][:, s:s + TY * W] for r, s in zip(table[:, 0], table[:, 3])])
del recordings
pools = DeviceDataset(x_pool, y_pool)

# ---- (a) the gather ----------------------------------------------------------------------------------------------------------------
sampler = EpochSampler(POOL, B, opt.seed, 0, 1, device=dev).begin_epoch(0)
x_out, y_out, n_out = torch.empty(B, N, T * W, device=dev), torch.empty(B, N, TY * W, device=dev), torch.empty(B, dtype=torch.int64, device=dev)


def epochs(fn):
    calls = {"k": 0}

    def run():
        if calls["k"] % EPOCH == 0:
            sampler.cursor.zero_()
        calls["k"] += 1
        fn()
    return run


index = sampler.perm[:B].clone()
sampler.cursor.zero_()
ssl_ds.gather(sampler, x_out, y_out, n_out)
assert torch.equal(x_out, x_pool[index]) and torch.equal(y_out, y_pool[index]) and n_out.tolist() == [T] * B
sampler.cursor.zero_()
odd_ds.gather(sampler, x_out, y_out, n_out)
assert torch.equal(x_out[:, :, :-1], x_pool[index][:, :, 1:]) and torch.equal(y_out[:, :, :-1], y_pool[index][:, :, 1:])
cands = {"gather_records_aligned": epochs(lambda: ssl_ds.gather(sampler, x_out, y_out, n_out)),
         "gather_records_start_1_mod_4": epochs(lambda: odd_ds.gather(sampler, x_out, y_out, n_out)),
         "gather_clips_pre_cut": epochs(lambda: pools.gather(sampler, x_out, y_out))}
if other is not None:
    cands["gather_clips_pre_cut_other_lib"] = with_lib(other, epochs(lambda: pools.gather(sampler, x_out, y_out)))
res = alternate(cands, opt.rounds)
nbytes = 2.0 * 4 * (x_out.numel() + y_out.numel())
yard = res["gather_clips_pre_cut"]
result["gather"] = {"ms": stats(res), "MB_moved": nbytes / 1e6, "TBps": {k: nbytes / (v[0] * 1e-3) / 1e12 for k, v in res.items()},
                    "aligned_over_gather_clips": res["gather_records_aligned"][0] / yard[0],
                    "unaligned_over_gather_clips": res["gather_records_start_1_mod_4"][0] / yard[0],
                    "aligned_median_within_yardstick_max_plus_10_percent": bool(res["gather_records_aligned"][0] <= 1.1 * yard[2])}
print(json.dumps(result["gather"], indent=1), flush=True)

# ---- (b) the captured steps --------------------------------------------------------------------------------------------------------
if not opt.skip_steps:
    raw_kw = dict(raw_window=W, raw_mean=5.68, raw_std=0.87)
    labels = (torch.rand(POOL, generator=g, device=dev) > 0.5).float()
    det_table = table.copy()
    det_table[:, 3] = 0
    det_rec = RecordingDataset(ssl_ds.signals, det_table, labels, window=W, x_steps=T, rec_table=ssl_ds.rec_table, num_channels=N)
    det_pool = DeviceDataset(x_pool, labels)

    def epoch_stepper(task, data):
        torch.manual_seed(opt.seed)
        if task == "ssl":
            model = DCRNNModel_nextTimePred(bench.make_args("dual_random_walk"), device=dev).to(dev).train()
        else:
            model = DCRNNModel_classification(bench.make_args("dual_random_walk"), 1, device=dev).to(dev).train()
        st = TrainStep(model, task=task, lr=3e-4, weight_decay=5e-4, max_grad_norm=5.0, **raw_kw)
        sm = EpochSampler(POOL, B, opt.seed, 0, 1, device=dev)
        st.begin_epoch(0, 1000, sampler=sm)
        keep = st.snapshot()
        st.capture_epoch(data, sm, None, include_update=True)
        st.restore(keep)
        calls = {"k": 0}

        def run():
            if calls["k"] % sm.steps_per_epoch == 0:
                st.begin_epoch((calls["k"] // sm.steps_per_epoch) % 1000, 1000)
            calls["k"] += 1
            return st.replay_step(0)
        return run

    steps = {}
    for task, rec_data, pool_data in (("detection", det_rec, det_pool), ("ssl", ssl_ds, pools)):
        a, b = epoch_stepper(task, rec_data), epoch_stepper(task, pool_data)
        la, lb = [float(a()) for _ in range(3)], [float(b()) for _ in range(3)]
        res = alternate({"from_recordings": a, "from_pre_cut_pools": b}, opt.rounds, reps=20)
        r, p = res["from_recordings"], res["from_pre_cut_pools"]
        steps[task] = {"ms": stats(res), "first_losses_equal": la == lb,      # (the same clips, the same launches behind the gather)
                       "recordings_minus_pools_ms": r[0] - p[0],
                       "recordings_median_within_pools_range_widened_by_own_spread": bool(p[1] - (r[2] - r[1]) <= r[0] <= p[2] + (r[2] - r[1]))}
        print(json.dumps({task: steps[task]}, indent=1), flush=True)
    result["captured_raw_steps"] = steps
torch.cuda.synchronize()
text = json.dumps(result, indent=1)
if opt.out:
    with open(opt.out, "w") as f:
        f.write(text + "\n")
    print("wrote", opt.out)
