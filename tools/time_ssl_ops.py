"""dev aid (GPU box): HIP-event timing of the SSL step's data side at cfg5 size (B = 512, 60 s in / 12 s out, 19 nodes, W = 200).
  1. paired featurisation (`ops.fft_features_pair`, one launch) against `ops.fft_features(x)` + `ops.fft_features(y)` (two launches);
     with --lib PATH also the two launches of ANOTHER build of the library (e.g. the parent commit's), all alternating in one process;
  2. `ops.augment_features` against the ATen expression of the supervised feature path on the same tensors;
  3. the whole captured SSL step from raw signals with data_augment (correlation graph) beside the step from features without
     augmentation, in clips/s.
Every figure: warm, `--rounds` rounds alternating between the candidates, each round long enough to last ~0.1 s per candidate;
median and spread (min..max) over the rounds.
usage: python tools/time_ssl_ops.py [--lib PATH] [--rounds 7] [--skip-step]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from eeg_gnn_ssl_amd import DCRNNModel_nextTimePred, _lib, ops  # noqa: E402
from eeg_gnn_ssl_amd.train_step import TrainStep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None, help="another build of libeeg_dcrnn_hip.so whose fft_features is timed beside this tree's")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--skip-step", action="store_true")
opt = ap.parse_args()

dev = "cuda"
B, N, TX, TY, W, D = 512, 19, 60, 12, 200, 100
MEAN, STD = 3.924, 1.56
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


out = {"device": torch.cuda.get_device_name(0), "shape": dict(B=B, N=N, Tx=TX, Ty=TY, W=W), "rounds": opt.rounds}
g = torch.Generator().manual_seed(3)
raw_x = (20.0 * torch.randn(B, N, TX * W, generator=g)).to(dev)
raw_y = (20.0 * torch.randn(B, N, TY * W, generator=g)).to(dev)
rng = ops.make_rng_state(dev, stream_id=2)
from eeg_gnn_ssl_amd import utils  # noqa: E402
flags, perm, ls, _ = ops.draw_augmentation(rng, B, utils.swap_permutation(N).to(dev))


# 1. featurisation
def two_launches():
    a = ops.fft_features(raw_x, W, MEAN, STD, perm, ls)
    b = ops.fft_features(raw_y, W, MEAN, STD, perm, ls)
    return a, b


cands = {"pair_one_launch": lambda: ops.fft_features_pair(raw_x, raw_y, W, MEAN, STD, perm, ls), "two_launches": two_launches}
if other is not None:
    cands["two_launches_other_lib"] = with_lib(other, two_launches)
    (fr0, fs0), (_, ys0) = two_launches()
    (fr1, fs1), (_, ys1) = cands["two_launches_other_lib"]()
    out["fft_features_bit_identical_to_other_lib"] = bool(torch.equal(fr0, fr1) and torch.equal(fs0, fs1) and torch.equal(ys0, ys1))
fr, xs, ys = cands["pair_one_launch"]()
(fr0, fs0), (_, ys0) = two_launches()
out["pair_bit_identical_to_two_launches"] = bool(torch.equal(fr, fr0) and torch.equal(xs, fs0) and torch.equal(ys, ys0))
res = alternate(cands, opt.rounds)
fft_bytes = 4.0 * B * N * ((TX + TY) * W + (2 * TX + TY) * (W // 2))          # windows read once; feat_raw_x, x_std, y_std written
out["featurisation_ms"] = {k: dict(median=v[0], min=v[1], max=v[2]) for k, v in res.items()}
out["featurisation_algorithmic_MB"] = fft_bytes / 1e6
out["pair_over_two_launches"] = res["pair_one_launch"][0] / res["two_launches"][0]
del fr0, fs0, ys0

# 2. augmentation of standardised features
x, y = xs, ys


def aten():
    outs = []
    for t in (x, y):
        idx = perm.to(torch.int64)[:, None, :, None].expand(-1, t.shape[1], -1, t.shape[3])
        outs.append(t.gather(2, idx) + (ls / STD)[:, None, None, None])
    return outs


xa, ya = ops.augment_features(x, y, perm, ls, STD)
ref = aten()
out["augment_bit_identical_to_aten"] = bool(torch.equal(xa, ref[0]) and torch.equal(ya, ref[1]))
del ref, xa, ya
res = alternate({"augment_features": lambda: ops.augment_features(x, y, perm, ls, STD), "aten_expression": aten}, opt.rounds)
aug_bytes = 8.0 * B * (TX + TY) * N * D
out["augment_ms"] = {k: dict(median=v[0], min=v[1], max=v[2]) for k, v in res.items()}
out["augment_algorithmic_MB"] = aug_bytes / 1e6
out["augment_TBps"] = aug_bytes / (res["augment_features"][0] * 1e-3) / 1e12
out["augment_fraction_of_8TBps"] = out["augment_TBps"] / 8.0
out["augment_speedup_over_aten"] = res["aten_expression"][0] / res["augment_features"][0]

# 3. the whole step (captured forward + backward + update; clips/s)
if not opt.skip_step:
    def step_rate(raw, augment):
        torch.manual_seed(5)
        model = DCRNNModel_nextTimePred(bench.make_args("dual_random_walk"), device=dev).to(dev).train()
        kw = dict(raw_window=W, raw_mean=MEAN, raw_std=STD) if raw else {}
        st = TrainStep(model, task="ssl", data_augment=augment, **kw)
        xi, yi = (raw_x, raw_y) if raw else (xs, ys)
        st.capture(xi, yi, None, None)
        for _ in range(3):
            st.replay_step()
        torch.cuda.synchronize()
        v = []
        for _ in range(opt.rounds):
            v.append(ms_per_call(st.replay_step, 10))
        return {"clips_per_s_median": B / (statistics.median(v) * 1e-3), "ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)}

    out["ssl_step_raw_pair_augmented"] = step_rate(True, True)
    out["ssl_step_features_no_augmentation"] = step_rate(False, False)
print(json.dumps(out, indent=1))
