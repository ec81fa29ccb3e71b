"""dev aid (GPU box): timing of the device EDF decode (eeg_gnn_ssl_amd/edf.py, csrc/kernels_edf.h), by the protocol of
tools/time_resample_ops.py.  One shape, a synthetic one-hour EDF file: 33 signals at 256 Hz in records of 1 s (R = 8448 int16, a
payload of 60.8 MB), the 19 montage channels selected in the montage's order (L = 921 600 samples per channel).
    (a) `torch.ops.eeg_dcrnn.edf_decode` to float64 and to float32, as an eager call (allocation and the Python layer included) and as
        the kernel alone (`ops.edf_decode_into` a fixed buffer, GRAPH_LAUNCHES launches captured in one graph, per launch: no host
        time between them); the bytes the kernel reads and writes by its shapes (2 per selected sample in, 8 or 4 out) and the time
        those bytes take at the measured copy rate of 6.29 TB/s.  Payload (60.8 MB) and output (140 / 70 MB) together fit the 256 MB
        Infinity Cache, as they do for every real file of this kind;
    (b) the same result from stock ATen ops on the device (the yardstick): the int16 view as (records, R), one column slice per channel
        copied into its float64 row, then add and multiply over the whole array -- and, because every signal of THIS file has the same
        samples per record, also as one index_select over a (records, signals, n) view;
    (c) the path the decode replaces: numpy on the host to the float64 (19, L) array plus its upload -- against the upload of the
        payload bytes plus (a);  host clock around a device synchronise, pageable memory;
    (d) `load_edf_recordings` per file (two files of this shape through the reused buffers) against `resample_recordings` fed the
        ready host float64 arrays (the host decode of (c) is NOT in that figure).
All device results are compared bit for bit with the host's before anything is timed.  (a), (b): HIP events, warm, `--rounds` rounds
alternating between the candidates, each round ~0.2 s per candidate; median and spread (min..max).  There is no pass/fail threshold on
time.
usage: python tools/time_edf_ops.py [--rounds 7] [--out profiles/edf_ops.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from eeg_gnn_ssl_amd import load_edf_recordings, ops, read_edf_header, resample_recordings, select_channels, utils  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--records", type=int, default=3600)
ap.add_argument("--out", default=None)
opt = ap.parse_args()
assert torch.cuda.is_available(), "time_edf_ops.py measures on an MI355X; there is nothing to measure without one"
dev = "cuda"
COPY_TBPS = 6.29
NS, FS, RECORDS = 33, 256, opt.records
GRAPH_LAUNCHES = 20


def synthetic_file():
    """33 signals of 256 samples per 1-s record: the 19 montage channels in reversed order with 14 others between them"""
    others = [f"EEG X{k}-REF" for k in range(NS - 19)]
    labels = []
    for k, name in enumerate(reversed(utils.INCLUDED_CHANNELS)):
        labels.append(name + "-REF")
        if k < len(others):
            labels.append(others[k])
    field = lambda v, w: str(v).ljust(w).encode("ascii")     # noqa: E731
    head = [field("0", 8), field("X", 80), field("Startdate X", 80), field("01.01.01", 8), field("00.00.00", 8), field(256 * (NS + 1), 8), field("", 44),
            field(RECORDS, 8), field(1, 8), field(NS, 4)]
    for values, w in ((labels, 16), ([""] * NS, 80), (["uV"] * NS, 8), ([round(-5482.28 - k, 2) for k in range(NS)], 8), ([5482.288] * NS, 8), ([-32767] * NS, 8),
                      ([32767] * NS, 8), ([""] * NS, 80), ([FS] * NS, 8), ([""] * NS, 32)):
        head += [field(v, w) for v in values]
    t = np.arange(RECORDS * NS * FS, dtype=np.int64)
    data = ((t * 7919 + (t * t) % 8191 * 13 + (t // 5) * 331) % 65536 - 32768).astype("<i2")
    return np.concatenate([np.frombuffer(b"".join(head), dtype=np.uint8), data.view(np.uint8)])


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


def host_ms(fn, repeats=3):
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


file = synthetic_file()
header = read_edf_header(file)
picked = select_channels(header)
C, R, n = len(picked), header.record_len, header.nsamp[picked[0]]
L = RECORDS * n
off = [header.chan_off(s) for s in picked]
gain = [header.gain_offset(s)[0] for s in picked]
offset = [header.gain_offset(s)[1] for s in picked]
payload_host = file[header.header_bytes:]
payload = torch.from_numpy(payload_host.copy()).to(dev)
gain_d = torch.tensor(gain, dtype=torch.float64, device=dev)[:, None]
offset_d = torch.tensor(offset, dtype=torch.float64, device=dev)[:, None]
picked_d = torch.tensor(picked, device=dev)


def numpy_decode():
    d = payload_host.view("<i2").reshape(RECORDS, R)
    x = np.empty((C, L), dtype=np.float64)
    for c in range(C):
        x[c] = gain[c] * (offset[c] + d[:, off[c]:off[c] + n].reshape(-1).astype(np.float64))
    return x


def aten_slices(dtype=torch.float64):
    v = payload.view(torch.int16).view(RECORDS, R)
    out = torch.empty(C, L, dtype=torch.float64, device=dev)
    for c in range(C):
        out[c].view(RECORDS, n).copy_(v[:, off[c]:off[c] + n])
    out.add_(offset_d).mul_(gain_d)
    return out if dtype == torch.float64 else out.float()


def aten_index_select(dtype=torch.float64):
    v = payload.view(torch.int16).view(RECORDS, NS, n)
    out = v.index_select(1, picked_d).permute(1, 0, 2).to(torch.float64).reshape(C, L)
    out = out.add_(offset_d).mul_(gain_d)
    return out if dtype == torch.float64 else out.float()


def kernel(dtype):
    return torch.ops.eeg_dcrnn.edf_decode(payload, RECORDS, R, n, off, gain, offset, dtype)


_graph_buffers = []      # the captured launches keep the ADDRESS of their output: the buffers live as long as the graphs (a later capture
#                          empties the allocator's cache, which would hand a dead buffer's memory back to the driver under the first graph)


def captured(dtype):
    """GRAPH_LAUNCHES launches of the kernel into one buffer, captured once; -> a callable that replays them"""
    out = torch.empty(C, L, dtype=dtype, device=dev)
    _graph_buffers.append(out)
    ops.edf_decode_into(payload, RECORDS, R, n, off, gain, offset, out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(GRAPH_LAUNCHES):
            ops.edf_decode_into(payload, RECORDS, R, n, off, gain, offset, out)
    _graph_buffers.append(graph)
    return graph.replay


ref = numpy_decode()
ref_d = torch.from_numpy(ref).to(dev)
for dtype in (torch.float64, torch.float32):
    want = ref_d.to(dtype)
    for name, fn in (("edf_decode", kernel), ("ATen slices", aten_slices), ("ATen index_select", aten_index_select)):
        assert torch.equal(fn(dtype), want), f"{name} {dtype} differs from the host's result"
torch.cuda.synchronize()

res = alternate({"k64": lambda: kernel(torch.float64), "k32": lambda: kernel(torch.float32), "g64": captured(torch.float64), "g32": captured(torch.float32), "s64": lambda: aten_slices(), "i64": lambda: aten_index_select(),
                 "s32": lambda: aten_slices(torch.float32), "i32": lambda: aten_index_select(torch.float32)}, opt.rounds)
lines = [f"device: {torch.cuda.get_device_name(0)}; one synthetic EDF file: {NS} signals x {n} samples x {RECORDS} records of 1 s (R = {R} int16, payload "
         f"{payload_host.size / 1e6:.1f} MB), {C} channels selected, L = {L}; rounds: {opt.rounds}; median (min..max) ms",
         "no threshold on time: these are the first measurements of the decode; every device result was bit-equal to the host's first",
         "",
         "(a) torch.ops.eeg_dcrnn.edf_decode (one launch; HIP events)"]
for key, gkey, what, width in (("k64", "g64", "float64", 8), ("k32", "g32", "float32", 4)):
    nbytes = C * L * (2 + width)
    floor = nbytes / (COPY_TBPS * 1e12) * 1e3
    m, g = res[key], tuple(v / GRAPH_LAUNCHES for v in res[gkey])
    lines.append(f"  -> {what}, eager call    {m[0]:8.4f} ({m[1]:.4f}..{m[2]:.4f}) ms")
    lines.append(f"  -> {what}, kernel alone  {g[0]:8.4f} ({g[1]:.4f}..{g[2]:.4f}) ms   kernel bytes {nbytes / 1e6:7.1f} MB (2 in + {width} out per sample) = "
                 f"{floor:.4f} ms at {COPY_TBPS} TB/s -> {floor / g[0] * 100:.1f} % of the copy rate")
lines += ["", "(b) the same arrays from stock ATen ops on the device (the yardstick; HIP events)"]
for key, what in (("s64", "column slices      -> float64"), ("i64", "index_select       -> float64"), ("s32", "column slices      -> float32"),
                  ("i32", "index_select       -> float32")):
    m = res[key]
    k = res["k64" if key.endswith("64") else "k32"]
    faster = m[1] - k[2] > m[2] - m[1]
    lines.append(f"  {what}   {m[0]:8.4f} ({m[1]:.4f}..{m[2]:.4f}) ms   ATen / edf_decode = {m[0] / k[0]:.2f}"
                 f"{' (the kernel is faster by more than the ATen spread)' if faster else ' (NOT faster beyond the ATen spread)'}")

up64 = host_ms(lambda: torch.from_numpy(ref).to(dev))
dec = host_ms(numpy_decode)
both = host_ms(lambda: torch.from_numpy(numpy_decode()).to(dev))
ours = host_ms(lambda: torch.ops.eeg_dcrnn.edf_decode(torch.from_numpy(payload_host).to(dev), RECORDS, R, n, off, gain, offset, torch.float64))
lines += ["", "(c) what the decode replaces (host clock around a device synchronise, pageable host memory, 3 repeats)",
          f"  numpy decode to float64 (19, L) on the host          {dec[0]:9.2f} ({dec[1]:.2f}..{dec[2]:.2f}) ms",
          f"  upload of that array ({ref.nbytes / 1e6:.1f} MB)                      {up64[0]:9.2f} ({up64[1]:.2f}..{up64[2]:.2f}) ms",
          f"  both                                                 {both[0]:9.2f} ({both[1]:.2f}..{both[2]:.2f}) ms",
          f"  upload of the payload bytes ({payload_host.size / 1e6:.1f} MB) + edf_decode      {ours[0]:9.2f} ({ours[1]:.2f}..{ours[2]:.2f}) ms   "
          f"-> {both[0] / ours[0]:.1f} x"]

files = [file, file]
arrays = [ref, ref]
load = host_ms(lambda: load_edf_recordings(files))
rs = host_ms(lambda: resample_recordings(arrays, [float(FS)] * 2))
a, _, _ = load_edf_recordings(files)
b, _ = resample_recordings(arrays, [float(FS)] * 2)
same = bool(torch.equal(a, b))
lines += ["", f"(d) whole chain to the 200 Hz layout, per file (two files of this shape; host clock; same bits: {same})",
          f"  load_edf_recordings (header, payload upload, decode, resample)      {load[0] / 2:9.2f} ({load[1] / 2:.2f}..{load[2] / 2:.2f}) ms per file",
          f"  resample_recordings fed ready host float64 arrays (no host decode)  {rs[0] / 2:9.2f} ({rs[1] / 2:.2f}..{rs[2] / 2:.2f}) ms per file",
          f"  the same with the host decode of (c) in front                       {rs[0] / 2 + dec[0]:9.2f} ms per file"]
text = "\n".join(lines) + "\n"
print(text, flush=True)
if opt.out:
    with open(opt.out, "w") as f:
        f.write(text)
    print("wrote", opt.out)
