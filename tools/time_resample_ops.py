"""dev aid (GPU box): HIP-event timing of the device resampling of whole native-rate recordings (eeg_gnn_ssl_amd/resample.py,
csrc/kernels_resample.h), by the protocol of tools/time_record_ops.py.  Three shapes, 19 channels of float64 samples each:
    300 000 samples (250 Hz, 20 min), 921 600 samples (256 Hz, 1 h), 400 * 1200 + 137 samples (400 Hz, a ragged length);
for each
    the device pass `torch.ops.eeg_dcrnn.resample` in ms (all channels at once, and chunked through one channel's workspace);
    its algorithmic HBM bytes -- what the launches read and write by their shapes, counted below from the plan rule -- and the time
        those bytes take at the measured copy rate of 6.29 TB/s;
    the ATen composition on the same device: torch.fft.rfft / irfft in float64, then .float() (the baseline, as aten_gpu_baseline is
        for the step);
    the numpy restatement on the host (one repeat: what the offline step costs per recording).
The two device results are compared with each other and with the host's before anything is timed.  Every device figure: warm,
`--rounds` rounds alternating between the candidates, each round ~0.2 s per candidate; median and spread (min..max) over the rounds.
There is no pass/fail threshold on time.
usage: python tools/time_resample_ops.py [--rounds 7] [--out profiles/resample_ops.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from eeg_gnn_ssl_amd import _lib, resampled_length  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=None)
opt = ap.parse_args()
assert torch.cuda.is_available(), "time_resample_ops.py measures on an MI355X; there is nothing to measure without one"
dev = "cuda"
N, COPY_TBPS = 19, 6.29
SHAPES = (("250 Hz, 20 min", 300000, 250), ("256 Hz, 1 h", 921600, 256), ("400 Hz, ragged", 400 * 1200 + 137, 400))
TILE_BITS, PASS_BITS, MIN_BITS = 12, 8, 6          # the plan rule of csrc/kernels_resample.h


def fft_bits(need):
    return max(MIN_BITS, int(need - 1).bit_length())


def passes(lm):
    return 1 if lm <= TILE_BITS else -(-lm // PASS_BITS)


def algorithmic_bytes(nx, num, channels, in_bytes=8):
    """bytes the launches of one call read and write, by their shapes: 16 per float64 complex point"""
    lm1, lm2 = fft_bits(nx + min(nx, num) // 2), fft_bits(num // 2 + num)
    total = 0
    for lm in (lm1, lm2):                                                  # the chirp filters: written, then transformed in place
        total += 16 * (1 << lm) * (1 + 2 * passes(lm))
    per_channel = nx * in_bytes + 16 * (1 << lm1)                           # load: samples in, padded chirped row out
    for lm in (lm1, lm2):                                                  # a convolution: 2p - 1 in-place passes, one reads the filter too
        total_passes = 2 * passes(lm) - 1
        per_channel += 16 * (1 << lm) * (2 * total_passes + 1)
    per_channel += 16 * (min(nx, num) // 2 + 1) + 16 * (1 << lm2)           # bridge: the kept bins in, the padded row out
    per_channel += 16 * num + 4 * num                                       # store: the row in, float32 out
    return total + channels * per_channel


def restate(x, num):
    nx = x.shape[-1]
    X = np.fft.rfft(x, axis=-1)
    n = min(num, nx)
    Y = np.zeros(x.shape[:-1] + (num // 2 + 1,), dtype=np.complex128)
    Y[..., :n // 2 + 1] = X[..., :n // 2 + 1]
    if n % 2 == 0:
        Y[..., n // 2] *= 2.0 if num < nx else (0.5 if nx < num else 1.0)
    return np.fft.irfft(Y, num, axis=-1) * (float(num) / float(nx))


def aten(x, num):
    nx = x.shape[-1]
    X = torch.fft.rfft(x, dim=-1)
    n = min(num, nx)
    Y = torch.zeros(x.shape[0], num // 2 + 1, dtype=torch.complex128, device=x.device)
    Y[:, :n // 2 + 1] = X[:, :n // 2 + 1]
    if n % 2 == 0:
        Y[:, n // 2] *= 2.0 if num < nx else (0.5 if nx < num else 1.0)
    return (torch.fft.irfft(Y, num, dim=-1) * (float(num) / float(nx))).float()


def ms_per_call(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(cands, rounds):
    n = {}
    for name, fn in cands.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        n[name] = max(3, int(200.0 / max(ms_per_call(fn, 3), 1e-3)))            # ~0.2 s per round
    got = {name: [] for name in cands}
    for _ in range(rounds):
        for name, fn in cands.items():
            got[name].append(ms_per_call(fn, n[name]))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in got.items()}


lib = _lib.get_lib()
lines = [f"device: {torch.cuda.get_device_name(0)}; {N} channels of float64 samples; rounds: {opt.rounds}; HIP events, median (min..max) ms",
         "no threshold on time: these are the first measurements of the pass"]
for what, nx, fs in SHAPES:
    num = resampled_length(nx, fs)
    t = np.arange(nx)[None, :]
    c = np.arange(N)[:, None]
    x = 50.0 * np.sin(0.086 * t + 0.7 * c) + 31.0 * np.sin(0.4677 * t + 1.3 * c) + 17.0 * np.sin(1.7945 * t - 0.9 * c) + (40.0 + 3.0 * c) * (t / nx - 0.3)
    xd = torch.from_numpy(x).to(dev)
    one = int(lib.query("eeg_dcrnn_resample_ws_bytes", nx, num, 1))
    full = int(lib.query("eeg_dcrnn_resample_ws_bytes", nx, num, N))
    t0 = time.perf_counter()
    ref = restate(x, num)
    host_s = time.perf_counter() - t0
    y = torch.ops.eeg_dcrnn.resample(xd, num)
    ya = aten(xd, num)
    torch.cuda.synchronize()
    scale = float(np.abs(x).max())
    err = float(np.abs(y.cpu().numpy().astype(np.float64) - ref).max())
    err_aten = float(np.abs(ya.cpu().numpy().astype(np.float64) - ref).max())
    chunked_equal = bool(torch.equal(torch.ops.eeg_dcrnn.resample(xd, num, one), y))
    res = alternate({"device": lambda: torch.ops.eeg_dcrnn.resample(xd, num), "device_chunked": lambda: torch.ops.eeg_dcrnn.resample(xd, num, one),
                     "aten": lambda: aten(xd, num)}, opt.rounds)
    nbytes = algorithmic_bytes(nx, num, N)
    floor_ms = nbytes / (COPY_TBPS * 1e12) * 1e3
    d, k, a = res["device"], res["device_chunked"], res["aten"]
    slower = d[0] - a[0] > a[2] - a[1]
    lines += ["",
              f"{what}: {N} x {nx} -> {N} x {num} (transforms of 2^{fft_bits(nx + min(nx, num) // 2)} and 2^{fft_bits(num // 2 + num)} points; workspace {full / 2**20:.0f} MiB, "
              f"one channel {one / 2**20:.0f} MiB)",
              f"  device pass            {d[0]:9.3f} ({d[1]:.3f}..{d[2]:.3f}) ms",
              f"  device pass, chunked   {k[0]:9.3f} ({k[1]:.3f}..{k[2]:.3f}) ms   (workspace of one channel; same bits: {chunked_equal})",
              f"  algorithmic HBM bytes  {nbytes / 1e6:9.1f} MB = {floor_ms:.3f} ms at {COPY_TBPS} TB/s -> the pass runs at {floor_ms / d[0] * 100:.1f} % of that rate",
              f"  ATen rfft/irfft f64    {a[0]:9.3f} ({a[1]:.3f}..{a[2]:.3f}) ms   device / ATen = {d[0] / a[0]:.2f}"
              f"{' (slower by more than the ATen spread)' if slower else ''}",
              f"  numpy restatement      {host_s * 1e3:9.1f} ms on the host (one repeat)",
              f"  max |y - restatement|: device {err:.3e}, ATen {err_aten:.3e} (float32 ulp at max|x| = {scale:.1f}: {np.spacing(np.float32(scale)):.3e})"]
    print("\n".join(lines[-8:]), flush=True)
    del xd, y, ya
text = "\n".join(lines) + "\n"
if opt.out:
    with open(opt.out, "w") as f:
        f.write(text)
    print("wrote", opt.out)
