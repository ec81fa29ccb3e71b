"""dev aid (GPU box): HIP-event timing of the time-domain data side (`use_fft=False`: a step of a clip is its 200 samples), at
B = 512 with 60 s in / 12 s out (the SSL pair) and at B = 256 with 60 s (a supervised batch); 19 nodes, W = 200.  Per shape:
  1. `ops.window_features_pair` (one launch) against the two single launches of `ops.window_features` and against the ATen
     expression (gather, multiply, subtract, divide, permute-contiguous) on the same tensors;
  2. `ops.augment_windows` against its ATen expression `x.gather(2, idx) * a + c` (x and y);
  3. `ops.correlation_supports_raw` on the raw rows (B, N, 12000) against the existing `corr_graph` kernel on a (B, 120, N, 100)
     tensor of equal bytes;
  4. the captured raw time-domain step against the captured step from ready windows (both augmented, correlation graph), clips/s;
     `--curriculum`: the SSL step once more with `use_curriculum_learning=True` (teacher-forcing flags drawn inside the graph).  Where
     the decoder shape is outside the persistent decoder kernels the capture is refused and the row reads "not available".
Every figure: warm, `--rounds` rounds alternating between the candidates, each round ~0.1 s per candidate; median and spread
(min..max) over the rounds.  Achieved TB/s are against ALGORITHMIC bytes (8*B*N*(Tx+Ty)*W for the two streaming kernels, 4*B*N*L for
the Gram) beside the 8 TB/s of the data sheet; the rate of a plain device copy of the same bytes is given as a footnote.
Kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/time_timedomain_ops.py --skip-step`.
usage: python tools/time_timedomain_ops.py [--rounds 7] [--skip-step] [--curriculum] [--out profiles/timedomain_time_ops.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from eeg_gnn_ssl_amd import DCRNNModel_classification, DCRNNModel_nextTimePred, ops, utils  # noqa: E402
from eeg_gnn_ssl_amd.train_step import TrainStep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--skip-step", action="store_true")
ap.add_argument("--curriculum", action="store_true")
ap.add_argument("--out", default=None)
opt = ap.parse_args()

dev = "cuda"
N, W = 19, 200
MEAN, STD = 0.37, 21.3


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


def table(res):
    return {k: dict(median=v[0], min=v[1], max=v[2]) for k, v in res.items()}


def rates(nbytes, ms):
    tbps = nbytes / (ms * 1e-3) / 1e12
    return dict(algorithmic_MB=nbytes / 1e6, TBps=tbps, fraction_of_8TBps=tbps / 8.0)


def one_shape(B, TX, TY):
    out = {"shape": dict(B=B, N=N, Tx=TX, Ty=TY, W=W)}
    g = torch.Generator().manual_seed(3)
    raw_x = (20.0 * torch.randn(B, N, TX * W, generator=g)).to(dev)
    raw_y = (20.0 * torch.randn(B, N, max(TY, 1) * W, generator=g)).to(dev) if TY else None
    rng = ops.make_rng_state(dev, stream_id=2)
    _, perm, ls, _ = ops.draw_augmentation(rng, B, utils.swap_permutation(N).to(dev))
    scale = torch.exp(ls)
    halves = [raw_x] + ([raw_y] if TY else [])
    stream_bytes = 8.0 * B * N * (TX + TY) * W

    # 1. raw signals -> standardised, augmented windows
    def single_launches():
        return [ops.window_features(r, W, MEAN, STD, perm, scale) for r in halves]

    def aten_windows():
        outs = []
        for r in halves:
            idx = perm.to(torch.int64)[:, :, None].expand(-1, -1, r.shape[2])
            v = (r.gather(1, idx) * scale[:, None, None] - MEAN) / STD
            outs.append(v.view(B, N, r.shape[2] // W, W).permute(0, 2, 1, 3).contiguous())
        return outs

    cands = {"single_launches": single_launches, "aten_expression": aten_windows}
    if TY:
        cands = {"pair_one_launch": lambda: ops.window_features_pair(raw_x, raw_y, W, MEAN, STD, perm, scale), **cands}
        pr, sg = cands["pair_one_launch"](), single_launches()
        out["pair_bit_identical_to_single_launches"] = bool(torch.equal(pr[0], sg[0]) and torch.equal(pr[1], sg[1]))
    sg, at = single_launches(), aten_windows()
    out["window_features_max_abs_diff_to_aten"] = max(float((a - b_).abs().max()) for a, b_ in zip(sg, at))
    del sg, at
    res = alternate(cands, opt.rounds)
    ours = "pair_one_launch" if TY else "single_launches"
    out["window_features_ms"] = table(res)
    out["window_features"] = dict(kernel=ours, **rates(stream_bytes, res[ours][0]), speedup_over_aten=res["aten_expression"][0] / res[ours][0])
    if TY:
        out["window_features"]["pair_over_single_launches"] = res["pair_one_launch"][0] / res["single_launches"][0]

    # 2. ready windows -> augmented windows
    xs = ops.window_features(raw_x, W, MEAN, STD)
    ys = ops.window_features(raw_y, W, MEAN, STD) if TY else None
    c = (scale - 1.0) * (MEAN / STD)

    def aten_augment():
        outs = []
        for t in (xs, ys)[: 2 if TY else 1]:
            idx = perm.to(torch.int64)[:, None, :, None].expand(-1, t.shape[1], -1, t.shape[3])
            outs.append(t.gather(2, idx) * scale[:, None, None, None] + c[:, None, None, None])
        return outs

    got, ref = ops.augment_windows(xs, ys, perm, scale, MEAN, STD), aten_augment()
    out["augment_windows_bit_identical_to_aten"] = bool(torch.equal(got[0], ref[0]) and (not TY or torch.equal(got[1], ref[1])))
    del got, ref
    res = alternate({"augment_windows": lambda: ops.augment_windows(xs, ys, perm, scale, MEAN, STD), "aten_expression": aten_augment}, opt.rounds)
    out["augment_windows_ms"] = table(res)
    out["augment_windows"] = dict(**rates(stream_bytes, res["augment_windows"][0]), speedup_over_aten=res["aten_expression"][0] / res["augment_windows"][0])

    # footnote: a plain device copy of the same bytes (read + write)
    src = torch.empty(int(stream_bytes // 8), device=dev)
    dst = torch.empty_like(src)
    res = alternate({"copy": lambda: dst.copy_(src)}, opt.rounds)
    out["copy_footnote"] = dict(ms=table(res)["copy"], **rates(stream_bytes, res["copy"][0]))
    del src, dst

    # 3. correlation graph: wide raw rows against the existing kernel on 100-wide steps of equal bytes
    steps = raw_x.view(B, N, TX * W // 100, 100).permute(0, 2, 1, 3).contiguous()
    res = alternate({"corr_graph_rows_raw": lambda: ops.correlation_supports_raw(raw_x),
                     "corr_graph_existing_100wide": lambda: torch.ops.eeg_dcrnn.corr_graph(steps, 3),
                     "corr_graph_rows_windows": lambda: ops.correlation_supports(xs)}, opt.rounds)
    gram_bytes = 4.0 * B * N * TX * W
    out["corr_graph_ms"] = table(res)
    out["corr_graph_rows"] = dict(**rates(gram_bytes, res["corr_graph_rows_raw"][0]),
                                  over_existing_kernel=res["corr_graph_rows_raw"][0] / res["corr_graph_existing_100wide"][0])
    out["corr_graph_existing"] = rates(gram_bytes, res["corr_graph_existing_100wide"][0])
    del steps

    # 4. the whole captured step (forward + backward + update; clips/s): raw signals against ready windows
    if not opt.skip_step:
        def step_rate(raw, curriculum=False):
            torch.manual_seed(5)
            args = bench.make_args("dual_random_walk")
            args.input_dim = args.output_dim = W
            args.use_curriculum_learning = curriculum
            if TY:
                model, task = DCRNNModel_nextTimePred(args, device=dev).to(dev).train(), "ssl"
                yi = raw_y if raw else ys
            else:
                model, task = DCRNNModel_classification(args, 1, device=dev).to(dev).train(), "detection"
                yi = (torch.rand(B, generator=g) > 0.5).float().to(dev)
            kw = dict(raw_window=W, raw_mean=MEAN, raw_std=STD) if raw else dict(feature_mean=MEAN, feature_std=STD)
            st = TrainStep(model, task=task, use_fft=False, data_augment=True, **kw)
            lengths = torch.full((B,), TX, dtype=torch.int64, device=dev)
            try:
                st.capture(raw_x if raw else xs, yi, lengths, None)
            except RuntimeError as e:
                if curriculum and "outside the persistent decoder kernels" in str(e):
                    return "not available"
                raise
            for _ in range(3):
                st.replay_step()
            torch.cuda.synchronize()
            v = [ms_per_call(st.replay_step, 5) for _ in range(opt.rounds)]
            return {"clips_per_s_median": B / (statistics.median(v) * 1e-3), "ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)}

        out["step_from_raw_signals"] = step_rate(True)
        out["step_from_ready_windows"] = step_rate(False)
        if opt.curriculum and TY:
            out["step_from_raw_signals_curriculum"] = step_rate(True, curriculum=True)
            out["step_from_ready_windows_curriculum"] = step_rate(False, curriculum=True)
    return out


result = {"device": torch.cuda.get_device_name(0), "rounds": opt.rounds, "ssl_pair_B512": one_shape(512, 60, 12), "supervised_B256": one_shape(256, 60, 0)}
text = json.dumps(result, indent=1)
print(text)
if opt.out:
    with open(opt.out, "w") as f:
        f.write(text + "\n")
