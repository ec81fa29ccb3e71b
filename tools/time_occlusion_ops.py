"""dev aid (GPU box): wall-clock timing of occlusion maps (eeg_gnn_ssl_amd/interpret.py, csrc/kernels_occlude.h) at B = 16 clips of
T = 60 s, N = 19, D = 100, 64 units, two layers, one channel per group and one step per window (1140 variants per clip), for the
distance graph (laplacian, the shared 2-D support: the spectral form) and for per-clip correlation graphs (dual_random_walk).
Candidates, each from the first launch to the maps on the host:
    occlusion_maps      one pass of `occlusion_maps(model, x, lengths, supports)`: a baseline pass, then per window the variants from
                        the baseline's states at the window's start
    from_scratch        the same maps the way a user had to make them before: per window the B * G occluded copies built with ATen,
                        each run through `model.forward` from step 0, probabilities and their difference with ATen
and the expand kernel alone (`ops.occlude_expand`, windows of t0 = 0 in rotation over buffers that together exceed the Infinity
Cache, device events around --reps launches) against the time the bytes it WRITES take at the achievable HBM rate (6.29 TB/s, the
float4-copy rate).  Op counts put the prefix-shared pass at (T + 1) / 2T = 0.51 of the recurrent work of from_scratch.
Fresh process, every candidate warmed, `--rounds` rounds alternating between the candidates; median and spread (min..max).  The two
candidates' maps are compared before anything is timed.  --trace adds the launches of one pass by role (the event recorder).
usage: python tools/time_occlusion_ops.py [--rounds 5] [--seed 11] [--clips 16] [--trace] [--out profiles/occlusion_ops.txt]"""
import argparse
import ctypes
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402  (model arguments)
from eeg_gnn_ssl_amd import DCRNNModel_classification, _lib, occlusion_maps, ops, utils  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--seed", type=int, default=11)
ap.add_argument("--clips", type=int, default=16)
ap.add_argument("--reps", type=int, default=60)
ap.add_argument("--trace", action="store_true")
ap.add_argument("--out", default=None)
opt = ap.parse_args()

assert torch.cuda.is_available(), "time_occlusion_ops.py measures on an MI355X; there is no other path"
warnings.simplefilter("ignore")
HBM_BYTES_PER_S = 6.29e12         # achievable (float4 copy), not the 8 TB/s of the data sheet
dev = "cuda"
B, T, N, D, H = opt.clips, 60, 19, 100, 64
g = torch.Generator(device=dev).manual_seed(opt.seed)
torch.manual_seed(opt.seed)
x = torch.randn(B, T, N, D, generator=g, device=dev)
lens = torch.full((B,), T, dtype=torch.int64, device=dev)


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
    return {name: (statistics.median(v), min(v), max(v)) for name, v in got.items()}


@torch.no_grad()
def from_scratch(model, supports):
    """the maps with ATen and `model.forward`: every variant built on the device as a copy of the clip, run from step 0"""
    was = model.training
    model.eval()
    eye = torch.eye(N, dtype=torch.bool, device=dev)
    sup = [s if s.dim() == 2 else s.repeat_interleave(N, dim=0) for s in supports]
    lens_v = lens.repeat_interleave(N)
    pb = torch.sigmoid(model(x, lens, supports).double().view(B))
    maps = torch.empty(B, T, N, device=dev)
    for k in range(T):
        xv = x[:, None].repeat(1, N, 1, 1, 1)                        # (B, G, T, N, D)
        xv[:, :, k] = torch.where(eye[None, :, :, None], torch.zeros((), device=dev), xv[:, :, k])
        pv = torch.sigmoid(model(xv.view(B * N, T, N, D), lens_v, sup).double().view(B, N))
        maps[:, k] = (pb[:, None] - pv).float()
    model.train(was)
    return maps.cpu()


def launches(fn):
    lib = _lib.get_lib()
    lib.query("eeg_dcrnn_prof_enable", 1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.query("eeg_dcrnn_prof_enable", 0)
    buf = ctypes.create_string_buffer(1 << 16)
    lib.call("eeg_dcrnn_prof_report", buf, len(buf))
    by_role = {}
    for line in buf.value.decode().strip().splitlines():
        role, cnt, ms, _ = line.split(None, 3)
        n_, t_ = by_role.get(role, (0, 0.0))
        by_role[role] = (n_ + int(cnt), t_ + float(ms))
    return by_role


lines = [f"device: {torch.cuda.get_device_name(0)}; B = {B} clips, T = {T}, N = {N}, D = {D}, {H} units, 2 layers, K = 2; time_window = 1, one channel "
         f"per group: {T * N} variants per clip; rounds = {opt.rounds}, seed = {opt.seed}"]
adj = np.load(os.path.join(ROOT, "eeg_gnn_ssl_amd", "data", "electrode_adj_3d.npy"))
for graph, filt in (("distance graph", "laplacian"), ("correlation graphs", "dual_random_walk")):
    model = DCRNNModel_classification(bench.make_args(filt), 1, device=dev).to(dev).train()
    if filt == "laplacian":
        supports = [s.to(dev) for s in utils.compute_supports(adj, "laplacian")]
    else:
        supports = list(ops.correlation_supports(x, top_k=3))
    ours = lambda: occlusion_maps(model, x, lens, supports, clips_per_pass=B).maps.cpu()     # noqa: E731
    ref = lambda: from_scratch(model, supports)     # noqa: E731
    a, b = ours(), ref()
    diff = float((a - b).abs().max())
    assert diff <= 2e-5, (graph, diff)
    res = alternate({"occlusion_maps": ours, "from_scratch": ref}, opt.rounds)
    lines.append(f"{graph} ({filt}): largest |map| {float(b.abs().max()):.3e}, largest difference between the two candidates {diff:.2e}")
    lines.append("  ms per pass (host clock around a pass that ends in a device-to-host copy): median (min .. max), ratio to from_scratch's median")
    for name, (med, lo, hi) in res.items():
        lines.append(f"    {name:<16s} {med:10.2f} ({lo:10.2f} .. {hi:10.2f})  {med / res['from_scratch'][0]:6.3f}")
    if opt.trace:
        lines.append("  launches of one occlusion_maps pass by role (event recorder: count, ms between the events around the launches):")
        for role, (cnt, ms) in sorted(launches(ours).items(), key=lambda kv: -kv[1][1]):
            lines.append(f"    {role:<24s} {cnt:6d} {ms:10.3f}")

# the expand kernel alone, window 0 (the largest): ROTATE output buffers, together above the 256 MiB the Infinity Cache holds
G, L = N, 2
hext = [torch.randn(T + 1, B, N * H, generator=g, device=dev) for _ in range(L)]
eye = torch.eye(N, dtype=torch.int32, device=dev)
ROTATE = 3
bufs = [(torch.empty(T, B * G, N, D, device=dev), torch.empty(L, B * G, N * H, device=dev), torch.empty(B * G, dtype=torch.int64, device=dev))
        for _ in range(ROTATE)]


def kernel_us():
    for i in range(ROTATE):
        ops.occlude_expand(x, hext, eye, lens, 0, 1, 0.0, *bufs[i % ROTATE])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(opt.reps):
        ops.occlude_expand(x, hext, eye, lens, 0, 1, 0.0, *bufs[i % ROTATE])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / opt.reps


k_us = [kernel_us() for _ in range(opt.rounds)]
written = sum(t.numel() * t.element_size() for t in bufs[0])
floor_us = written / HBM_BYTES_PER_S * 1e6
lines.append(f"occlude_expand alone, window 0 ({written / 1e6:.1f} MB written, {ROTATE} output buffers in rotation; back-to-back launches, device events, "
             f"us per launch over {opt.reps}): median {statistics.median(k_us):.2f} (min {min(k_us):.2f} .. max {max(k_us):.2f}); {floor_us:.2f} us at "
             f"{HBM_BYTES_PER_S / 1e12:.2f} TB/s: {floor_us / statistics.median(k_us) * 100:.0f} % of the achievable HBM rate")
text = "\n".join(lines)
print(text)
if opt.out:
    with open(opt.out, "w") as f:
        f.write(text + "\n")
