"""dev aid (GPU box): HIP-event timing of the length-aware data side (variable-length clips, the classification loader) at
B = 256, N = 19, T = 60, W = 200.  Four operators -- `fft_features`, `window_features`, `corr_graph` on features (B,60,N,100) and
`corr_graph_rows` on the raw rows (B,N,12000) -- and three candidates each:
  (a) the plain call of this tree -- and, with --lib PATH, of ANOTHER build of the library (the parent commit's): the plain calls run
      the instructions they ran before, so the two must agree within their spreads;
  (b) the length-aware call with every length at 60;
  (c) the length-aware call with seeded integer lengths uniform in 1..60 (seed and sum of lengths are recorded).
Every figure: warm, `--rounds` rounds alternating between the candidates, each round ~0.1 s per candidate; median and spread
(min..max) over the rounds.  Achieved TB/s are against ALGORITHMIC bytes over the VALID steps only (fft: 4*N*W read + 2*4*N*W/2 written
per step; windows: 8*N*W; graphs: 4*N*D) plus, for the featurisation, the padding written.
Kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/time_varlen_ops.py` and summarise the result with
tools/rocpd_stats.py.
usage: python tools/time_varlen_ops.py [--lib PATH] [--rounds 7] [--seed 11] [--out profiles/varlen_time_ops.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from eeg_gnn_ssl_amd import _lib, ops, utils  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None, help="another build of libeeg_dcrnn_hip.so whose plain calls are timed beside this tree's")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--seed", type=int, default=11)
ap.add_argument("--out", default=None)
opt = ap.parse_args()

dev = "cuda"
B, N, T, W = 256, 19, 60, 200
MEAN, STD = 0.37, 21.3
here = _lib.get_lib()
other = _lib.EegDcrnnLib(opt.lib, strict=False) if opt.lib else None


def ms_per_call(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(cands, rounds):
    """cands: {name: callable}; returns {name: (median ms, min ms, max ms)} over alternating rounds"""
    reps = {}
    for name, fn in cands.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        reps[name] = max(5, int(100.0 / max(ms_per_call(fn, 5), 1e-3)))            # ~0.1 s per round
    got = {name: [] for name in cands}
    for _ in range(rounds):
        for name, fn in cands.items():
            got[name].append(ms_per_call(fn, reps[name]))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in got.items()}


def with_lib(lib, fn):
    def run():
        keep = _lib._LIB
        _lib._LIB = lib
        try:
            return fn()
        finally:
            _lib._LIB = keep
    return run


g = torch.Generator().manual_seed(opt.seed)
raw = (20.0 * torch.randn(B, N, T * W, generator=g)).to(dev)
full = torch.full((B,), T, dtype=torch.int64, device=dev)
mixed = torch.randint(1, T + 1, (B,), generator=g).to(dev)
valid = int(mixed.sum().item())
rng = ops.make_rng_state(dev, stream_id=2)
_, perm, ls, _ = ops.draw_augmentation(rng, B, utils.swap_permutation(N).to(dev))
scale = torch.exp(ls)
feats = ops.fft_features(raw, window=W)[0]                                              # (B, T, N, 100)

OPS = {
    # name: (plain call, length-aware call, algorithmic bytes per valid step, bytes written per padded step)
    "fft_features": (lambda: ops.fft_features(raw, W, MEAN, STD, perm, ls), lambda le: ops.fft_features(raw, W, MEAN, STD, perm, ls, lengths=le),
                     4.0 * N * W + 8.0 * N * (W // 2), 8.0 * N * (W // 2)),
    "window_features": (lambda: ops.window_features(raw, W, MEAN, STD, perm, scale),
                        lambda le: ops.window_features(raw, W, MEAN, STD, perm, scale, lengths=le), 8.0 * N * W, 4.0 * N * W),
    "corr_graph": (lambda: ops.correlation_supports(feats), lambda le: ops.correlation_supports(feats, lengths=le), 4.0 * N * (W // 2), 0.0),
    "corr_graph_rows": (lambda: ops.correlation_supports_raw(raw), lambda le: ops.correlation_supports_raw(raw, lengths=le, window=W), 4.0 * N * W, 0.0),
}

result = {"device": torch.cuda.get_device_name(0), "rounds": opt.rounds, "shape": dict(B=B, N=N, T=T, W=W), "seed": opt.seed,
          "sum_of_lengths": valid, "share_of_valid_steps": valid / (B * T), "other_lib": opt.lib}
for name, (plain, aware, step_bytes, pad_bytes) in OPS.items():
    cands = {"a_plain": plain, "b_lengths_all_60": lambda aware=aware: aware(full), "c_lengths_uniform_1_60": lambda aware=aware: aware(mixed)}
    if other is not None:
        cands["a_plain_other_lib"] = with_lib(other, plain)
    res = alternate(cands, opt.rounds)
    row = {"ms": {k: dict(median=v[0], min=v[1], max=v[2]) for k, v in res.items()}}
    a, b_, c = res["a_plain"][0], res["b_lengths_all_60"][0], res["c_lengths_uniform_1_60"][0]
    row["b_over_a"], row["c_over_a"] = b_ / a, c / a
    for key, steps, ms in (("a_plain", B * T, a), ("b_lengths_all_60", B * T, b_), ("c_lengths_uniform_1_60", valid, c)):
        nbytes = steps * step_bytes + (B * T - steps) * pad_bytes
        row.setdefault("algorithmic", {})[key] = dict(MB=nbytes / 1e6, TBps=nbytes / (ms * 1e-3) / 1e12)
    if other is not None:
        o = res["a_plain_other_lib"]
        spread = res["a_plain"][2] - res["a_plain"][1]
        row["plain_median_within_other_libs_range_widened_by_own_spread"] = bool(o[1] - spread <= a <= o[2] + spread)
    result[name] = row
text = json.dumps(result, indent=1)
print(text)
if opt.out:
    with open(opt.out, "w") as f:
        f.write(text + "\n")
