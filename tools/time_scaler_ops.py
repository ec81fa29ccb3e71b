"""dev aid (GPU box): timing of the scaler fit on the device (eeg_gnn_ssl_amd/statistics.py: fit_scaler, csrc/kernels_moments.h) at
cfg2's shapes: 60-s clips of 19 channels, W = 200, B = 256, a pool of --pool clips (default 1024).  Per pass over the pool, from the
first launch to the two floats on the host:
    (a) fit_recordings   `fit_scaler(RecordingDataset)`: the cut (`gather_records`) + `feature_moments` per step
    (b) fit_pool         `fit_scaler(DeviceDataset(raw pool), window=200)`: `gather_clips` + `feature_moments` per step
    (c) parent_way       what the parent commit offers: the same gather, then `ops.fft_features(batch)` (both outputs, as the operator
                         writes them) followed by `feat_raw.double().sum()` and `.double().square().sum()` per batch, added up on
                         the device, one copy at the end
and per launch on one batch, device events around --reps back-to-back launches that rotate over two batches (467 MB together,
above the 256 MiB of the Infinity Cache, so every launch reads from HBM):
    (d) fft_features     `ops.fft_features` alone (reads the batch, writes feat_raw and feat_std) -- with --lib PATH also on ANOTHER
                         build of the library (the parent commit's), bit-compared first
        feature_moments  the reducing kernel (use_fft=True) and the values-as-given kernel (use_fft=False), fold launch included
    (e) hbm_floor        the time to read the batch once at the achievable HBM rate (6.3 TB/s)
Every step runs in a process of its own under its own time limit (--limit seconds); the first step that fails or runs out of time
ends the run.  Inside a step every candidate is warmed, then --rounds rounds alternate between the candidates; median and spread
(min..max) over the rounds.  Results are compared before anything is timed.
usage: python tools/time_scaler_ops.py [--lib PATH] [--rounds 7] [--seed 11] [--pool 1024] [--out profiles/scaler_fit.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None, help="another build of libeeg_dcrnn_hip.so whose fft_features is timed beside this tree's")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--seed", type=int, default=11)
ap.add_argument("--pool", type=int, default=1024)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--seconds", type=int, default=60, help="steps of a clip")
ap.add_argument("--reps", type=int, default=40, help="launches per timed sample of a kernel")
ap.add_argument("--passes", type=int, default=5, help="passes per timed sample of a pass")
ap.add_argument("--limit", type=int, default=240, help="time limit of one step, seconds")
ap.add_argument("--out", default=None)
ap.add_argument("--step", default=None, choices=["passes", "kernels"], help="(internal) run this one step and print its JSON line")
opt = ap.parse_args()

HBM_BYTES_PER_S = 6.3e12          # achievable (float4 copy), not the 8 TB/s of the data sheet
N, W = 19, 200
B, T, P = opt.batch, opt.seconds, opt.pool
STEPS = ("passes", "kernels")


def driver():
    """every step in a fresh process under its own time limit; stop at the first failure"""
    results = {}
    for step in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + [a for a in sys.argv[1:] if a != "--step"]
        try:
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=opt.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"time_scaler_ops: step {step!r} ran past its limit of {opt.limit} s; nothing further is started")
        if done.returncode != 0:
            sys.exit(f"time_scaler_ops: step {step!r} ended with status {done.returncode}; nothing further is started")
        results[step] = json.loads(done.stdout.strip().splitlines()[-1])
    text = "\n".join(report(results))
    print(text)
    if opt.out:
        with open(opt.out, "w") as f:
            f.write(text + "\n")


def report(res):
    pa, ke = res["passes"], res["kernels"]
    fmt = lambda v: f"{v[0]:9.3f} ({v[1]:9.3f} .. {v[2]:9.3f})"     # noqa: E731
    lines = [f"device: {pa['device']}; cfg2 shapes: B = {B}, {T}-s clips of {N} channels, W = {W}, pool of {P} clips ({pa['steps']} steps per pass); "
             f"rounds = {opt.rounds}, seed = {opt.seed}",
             f"fit: mean {pa['mean']!r}, std {pa['std']!r} over {pa['count']} values; recordings and raw pool give the same bits: {pa['same_bits']}; "
             f"the parent's way (float32 features, framework sums): mean differs by {pa['parent_mean_diff']:.2e}, std by {pa['parent_std_diff']:.2e}",
             f"ms per pass (host clock around {opt.passes} passes in a row, each ending in a device-to-host copy): median (min .. max), ratio to (c)"]
    for name in ("fit_recordings", "fit_pool", "parent_way"):
        lines.append(f"  {name:<16s} {fmt(pa['ms'][name])}  {pa['ms'][name][0] / pa['ms']['parent_way'][0]:6.3f}")
    base = pa["ms"]["parent_way"]
    lines += [f"spread of parent_way over the rounds: {(base[2] - base[1]) / base[0] * 100:.2f} % of its median",
              f"us per launch on one batch ({ke['batch_MB']:.1f} MB of raw signals; two batches in rotation, device events over {opt.reps} back-to-back launches): "
              f"median (min .. max), share of the HBM floor"]
    floor = ke["floor_us"]
    for name, v in ke["us"].items():
        lines.append(f"  {name:<28s} {fmt(v)}  {floor / v[0] * 100:5.1f} %")
    lines.append(f"  {'hbm_floor (read once)':<28s} {floor:9.3f}  at {HBM_BYTES_PER_S / 1e12:.1f} TB/s")
    if "other_lib_same_bits" in ke:
        lines.append(f"fft_features of this tree and of {opt.lib}: same bits (feat_raw and feat_std): {ke['other_lib_same_bits']}")
    return lines


def timed(torch, fn):
    """ms per pass over opt.passes passes in a row (each ends in its own device-to-host copy)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(opt.passes):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / opt.passes


def spread(v):
    return (statistics.median(v), min(v), max(v))


def step_passes():
    import torch
    from eeg_gnn_ssl_amd import DeviceDataset, EpochSampler, RecordingDataset, clip_table_detection, fit_scaler, ops
    assert torch.cuda.is_available(), "time_scaler_ops.py measures on an MI355X; there is no other path"
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(opt.seed)
    per_rec = 64 if P % 64 == 0 else 1                               # recordings of 64 clips each
    recs = [20.0 * torch.randn(N, per_rec * T * W, generator=g, device=dev) for _ in range(P // per_rec)]
    table = clip_table_detection([p // per_rec for p in range(P)], [p % per_rec for p in range(P)], T, W)
    labels = torch.zeros(P, device=dev)
    rec_ds = RecordingDataset(recs, table, labels, window=W, x_steps=T, device=dev)
    pool = torch.stack([r.view(N, per_rec, T * W).transpose(0, 1) for r in recs]).reshape(P, N, T * W).contiguous()
    pool_ds = DeviceDataset(pool, labels)
    del recs

    def parent_way():
        s = EpochSampler(P, B, seed=0, rank=0, world=1, device=dev, drop_last=False)
        x, y = torch.empty((B, N, T * W), device=dev), torch.empty(B, device=dev)
        tot = torch.zeros(3, dtype=torch.float64, device=dev)
        for _ in range(s.steps_per_epoch):
            pool_ds.gather(s, x, y)
            feat_raw, _ = ops.fft_features(x, window=W, mean=0.0, std=1.0)
            f = feat_raw.double() * s.clip_w.double()[:, None, None, None]
            tot[0] += f.sum()
            tot[1] += f.square().sum()
            tot[2] += s.clip_w.double().sum() * feat_raw[0].numel()
        s_, q, n = tot.cpu().tolist()
        return s_ / n, (q / n - (s_ / n) ** 2) ** 0.5

    fit_a, fit_b = fit_scaler(rec_ds, B), fit_scaler(pool_ds, B, window=W)
    same = bool(torch.equal(fit_a.scores, fit_b.scores) and torch.equal(fit_a.record, fit_b.record))
    pm, ps = parent_way()
    cands = {"fit_recordings": lambda: fit_scaler(rec_ds, B), "fit_pool": lambda: fit_scaler(pool_ds, B, window=W), "parent_way": parent_way}
    for fn in cands.values():
        fn()
    got = {name: [] for name in cands}
    for _ in range(opt.rounds):
        for name, fn in cands.items():
            got[name].append(timed(torch, fn))
    print(json.dumps({"device": torch.cuda.get_device_name(0), "steps": -(-P // B), "mean": fit_a.mean, "std": fit_a.std, "count": fit_a.count,
                      "same_bits": same, "parent_mean_diff": abs(pm - fit_a.mean), "parent_std_diff": abs(ps - fit_a.std),
                      "ms": {k: spread(v) for k, v in got.items()}}))


def step_kernels():
    import torch
    from eeg_gnn_ssl_amd import _lib, ops
    assert torch.cuda.is_available(), "time_scaler_ops.py measures on an MI355X; there is no other path"
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(opt.seed)
    batches = [20.0 * torch.randn(B, N, T * W, generator=g, device=dev) for _ in range(2)]
    clip_w, cursor = torch.ones(B, device=dev), torch.tensor([B], dtype=torch.int64, device=dev)
    scores, _ = ops.moments_buffers(P, dev)
    other = _lib.EegDcrnnLib(os.path.abspath(opt.lib), strict=False) if opt.lib else None

    def with_lib(lib, fn):
        def run(x):
            keep = _lib._LIB
            _lib._LIB = lib
            try:
                return fn(x)
            finally:
                _lib._LIB = keep
        return run

    cands = {"fft_features": lambda x: ops.fft_features(x, window=W, mean=5.68, std=0.87),
             "feature_moments (log|FFT|)": lambda x: ops.feature_moments(x, scores, clip_w, cursor, window=W, use_fft=True),
             "feature_moments (samples)": lambda x: ops.feature_moments(x, scores, clip_w, cursor, window=W, use_fft=False)}
    out = {}
    if other is not None:
        cands["fft_features, other lib"] = with_lib(other, cands["fft_features"])
        a, b = cands["fft_features"](batches[0]), cands["fft_features, other lib"](batches[0])
        out["other_lib_same_bits"] = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
        del a, b

    def us_per_launch(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(opt.reps):
            fn(batches[i % 2])
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / opt.reps

    for fn in cands.values():
        for i in range(4):
            fn(batches[i % 2])
    torch.cuda.synchronize()
    got = {name: [] for name in cands}
    for _ in range(opt.rounds):
        for name, fn in cands.items():
            got[name].append(us_per_launch(fn))
    nbytes = batches[0].numel() * 4
    out.update({"batch_MB": nbytes / 1e6, "floor_us": nbytes / HBM_BYTES_PER_S * 1e6, "us": {k: spread(v) for k, v in got.items()}})
    print(json.dumps(out))


if opt.step == "passes":
    step_passes()
elif opt.step == "kernels":
    step_kernels()
else:
    driver()
