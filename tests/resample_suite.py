"""Checks of the device resampling of native-rate recordings (`torch.ops.eeg_dcrnn.resample`, eeg_gnn_ssl_amd/resample.py,
`RecordingDataset.from_native_rate`), run by tests/test_resample.py on the emulator build ("cpu") and on the MI355X library ("cuda").

Reference: `restate`, the float64 restatement of scipy.signal.resample the reference calls (data/data_utils.py:158-170), pinned to the
genuine function by tests/golden/golden_resample_v1.npz (`make_golden_resample.py`).  Inputs are the closed form `signal`: no draws.

Bound, per element, against the restatement of the same (float32-rounded, where applicable) input:
    |y - ref| <= 2^-24 |ref| + 1e-12 max|x_row|
the single rounding to float32 plus the float64 algorithm (a numpy Bluestein of this structure measured 1.4e-15 max|x| at 300 007
samples)."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_resample_v1.npz")
TO_FREQ = 200
# case -> (Nx, sample_freq): one per branch of the definition (num = 200 * int(Nx / sample_freq))
CASES = {"a": (757, 250), "b": (768, 256), "c": (1000, 250), "d": (1203, 400), "e": (4099, 1000), "f": (515, 100), "g": (500, 100), "h": (251, 250)}
GOLDEN_CHANNELS = 2
MAX_SAMPLES = 1 << 22
# the plan rule of csrc/kernels_resample.h, restated: a transform of 2^lm points is one LDS tile up to 2^TILE_BITS, else
# ceil(lm / PASS_BITS) global passes
TILE_BITS, PASS_BITS, MIN_BITS, MAX_BITS = 12, 8, 6, 23
# (Nx, num): single-channel cases just above each boundary of the plan (and the largest single tile)
PASS_CASES = {"tile_4096": (2926, 2340), "two_passes": (2927, 2340), "three_passes": (46813, 37448)}
LARGEST = (MAX_SAMPLES, TO_FREQ * int(MAX_SAMPLES / 250), 2)          # (Nx, num, channels): M1 = M2 = 2^23


def num_of(nx, fs, to_freq=TO_FREQ):
    return to_freq * int(nx / fs)


def signal(channels, nx, dtype=np.float64):
    """a few sines of incommensurate frequencies (cycles per sample) and a linear trend, so that the ends do not match; amplitudes
    about 50, another phase per channel"""
    t = np.arange(nx, dtype=np.float64)[None, :]
    c = np.arange(channels, dtype=np.float64)[:, None]
    x = 50.0 * np.sin(2 * np.pi * 0.0137 * t + 0.7 * c) + 31.0 * np.sin(2 * np.pi * np.sqrt(2.0) / 19.0 * t + 1.3 * c + 0.4) \
        + 17.0 * np.sin(2 * np.pi * np.pi / 11.0 * t - 0.9 * c) + 9.0 * np.cos(2 * np.pi * 0.41 * t + 2.1 * c) + (40.0 + 3.0 * c) * (t / nx - 0.3)
    return np.ascontiguousarray(x.astype(dtype))


def restate(x, num):
    """scipy.signal.resample(x, num, axis=1) for real float64 x, restated on numpy's FFT"""
    x = np.asarray(x, dtype=np.float64)
    nx = x.shape[-1]
    X = np.fft.rfft(x, axis=-1)
    n = min(num, nx)
    Y = np.zeros(x.shape[:-1] + (num // 2 + 1,), dtype=np.complex128)
    Y[..., :n // 2 + 1] = X[..., :n // 2 + 1]
    if n % 2 == 0:
        if num < nx:
            Y[..., n // 2] *= 2.0
        elif nx < num:
            Y[..., n // 2] *= 0.5
    return np.fft.irfft(Y, num, axis=-1) * (float(num) / float(nx))


def assert_within_bound(got, x, num, what):
    """got (C, num) float32 against the restatement of x (C, Nx)"""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    x = np.asarray(x, dtype=np.float64)
    ref = restate(x, num)
    assert got.shape == ref.shape and got.dtype == np.float32, (what, got.shape, got.dtype)
    err = np.abs(got.astype(np.float64) - ref)
    bound = 2.0 ** -24 * np.abs(ref) + 1e-12 * np.abs(x).max(axis=1, keepdims=True)
    worst = float((err / bound).max())
    print(f"{what}: max |y - ref| = {err.max():.3e}, worst error / bound = {worst:.4f}")
    assert np.isfinite(got).all() and worst <= 1.0, f"{what}: error {err.max():.3e} is {worst:.3f} x the bound"


def plan_passes(lm):
    return 1 if lm <= TILE_BITS else -(-lm // PASS_BITS)


def fft_bits(nx, num):
    """log2 of the two transforms of a resample of Nx -> num samples: Nx inputs and N/2 + 1 bins, M1 >= Nx + N/2; num/2 + 1 bins and
    num outputs, M2 >= num/2 + num"""
    bits = lambda need: max(MIN_BITS, int(need - 1).bit_length())     # noqa: E731
    return bits(nx + min(nx, num) // 2), bits(num // 2 + num)


# ---- no GPU, no library -------------------------------------------------------------------------------------------------------------
def check_golden():
    """the restatement equals the reference's own `resampleData` on the small cases (float64 outputs stored by make_golden_resample.py)"""
    with np.load(GOLDEN) as z:
        for name, (nx, fs) in CASES.items():
            x = signal(GOLDEN_CHANNELS, nx)
            num = num_of(nx, fs)
            want = z[f"resample/{name}"]
            assert want.shape == (GOLDEN_CHANNELS, num) and want.dtype == np.float64, name
            diff = float(np.abs(restate(x, num) - want).max())
            print(f"case {name}: restatement - reference = {diff:.3e}")
            assert diff <= 1e-13 * float(np.abs(x).max()), (name, diff)


def check_case_branches():
    """the small cases are what the table of the issue says: lengths, branches, transform sizes"""
    want = {"a": 600, "b": 600, "c": 800, "d": 600, "e": 800, "f": 1000, "g": 1000, "h": 200}
    for name, (nx, fs) in CASES.items():
        assert num_of(nx, fs) == want[name], name
    assert fft_bits(757, 600) == (11, 10) and fft_bits(1203, 600) == (11, 10) and fft_bits(4099, 800) == (13, 11) and fft_bits(515, 1000) == (10, 11)
    assert min(600, 757) % 2 == 0 and min(1000, 515) % 2 == 1 and min(1000, 500) % 2 == 0
    from eeg_gnn_ssl_amd import resampled_length
    for nx, fs in CASES.values():
        assert resampled_length(nx, fs) == num_of(nx, fs)
    assert resampled_length(1203, 400.0) == 600 and resampled_length(999, 250) == 600 and resampled_length(1000, 256.0) == 600
    assert resampled_length(249, 250) == 0 and resampled_length(300007, 250, 100) == 120000


def check_plan_completeness():
    """every pass count the plan can produce for M = 2^6 .. 2^23 is reached by a case of the GPU suite"""
    possible = {plan_passes(lm) for lm in range(MIN_BITS, MAX_BITS + 1)}
    assert possible == {1, 2, 3}
    reached = {}
    for name, (nx, num) in list(PASS_CASES.items()) + [("largest", LARGEST[:2])]:
        for lm in fft_bits(nx, num):
            assert MIN_BITS <= lm <= MAX_BITS
            reached.setdefault(plan_passes(lm), []).append(name)
    assert set(reached) == possible, reached
    # just above the boundaries: the first length of each pass count, and the last single tile
    assert fft_bits(*PASS_CASES["tile_4096"])[0] == TILE_BITS and fft_bits(*PASS_CASES["two_passes"])[0] == TILE_BITS + 1
    assert fft_bits(*PASS_CASES["three_passes"])[0] == 2 * PASS_BITS + 1 and plan_passes(2 * PASS_BITS) == 2
    assert fft_bits(*LARGEST[:2]) == (MAX_BITS, MAX_BITS)


# ---- the operator -------------------------------------------------------------------------------------------------------------------
def _nan(*shape, device, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=device)


def check_cases(device, channels):
    """every small case, float32 and float64 input, contiguous and with a row stride above Nx, into a fresh tensor and into rows of a
    stride padded to 4 floats"""
    from eeg_gnn_ssl_amd import ops
    for name, (nx, fs) in CASES.items():
        num = num_of(nx, fs)
        for dtype in (np.float32, np.float64):
            x = signal(channels, nx, dtype)
            xd = torch.from_numpy(x).to(device)
            y = torch.ops.eeg_dcrnn.resample(xd, num)
            assert tuple(y.shape) == (channels, num) and y.dtype == torch.float32 and y.is_contiguous()
            assert_within_bound(y, x, num, f"case {name} {np.dtype(dtype).name} x{channels}")
            wide = _nan(channels, nx + 5, device=device, dtype=xd.dtype)          # a row stride above Nx: the same bits
            wide[:, :nx] = xd
            stride = -(-num // 4) * 4 + 4
            out = _nan(channels, stride, device=device)
            ops.resample_into(wide[:, :nx], out[:, :num])
            assert torch.equal(out[:, :num], y), f"case {name}: strided rows changed the result"
            assert bool(torch.isnan(out[:, num:]).all()), f"case {name}: the padding behind a row was written"


def check_pass_counts(device):
    """one single-channel case just above each boundary of the FFT plan"""
    for name, (nx, num) in PASS_CASES.items():
        x = signal(1, nx)
        y = torch.ops.eeg_dcrnn.resample(torch.from_numpy(x).to(device), num)
        assert_within_bound(y, x, num, f"{name} ({nx} -> {num}, transforms of 2^{fft_bits(nx, num)})")


def check_largest(device):
    """GPU: the largest supported length, 2^22 samples (both transforms 2^23 points, three passes), two channels"""
    nx, num, channels = LARGEST
    x = signal(channels, nx)
    y = torch.ops.eeg_dcrnn.resample(torch.from_numpy(x).to(device), num)
    assert_within_bound(y, x, num, f"largest ({nx} -> {num})")


def _call_c(lib, x, num, out, ws, ws_bytes=None, in_stride=None, out_stride=None, n_in=None):
    """the C entry as it is (no Python refusals in front); returns its status"""
    from eeg_gnn_ssl_amd.ops import _p, _stream
    return lib.query("eeg_dcrnn_resample", _p(x), 1 if x.dtype == torch.float64 else 0, int(x.shape[0]), int(x.shape[1] if n_in is None else n_in),
                     int(x.stride(0) if in_stride is None else in_stride), int(num), _p(out), int(out.stride(0) if out_stride is None else out_stride),
                     _p(ws), int(ws.numel() * ws.element_size() if ws_bytes is None else ws_bytes), _stream(x))


def check_invariance(device):
    """bits do not depend on the company, the chunking, what the buffers held, or the call before"""
    from eeg_gnn_ssl_amd import _lib, resample_recording, resample_recordings
    lib = _lib.get_lib()
    channels = 5
    (nx_a, fs_a), (nx_d, fs_d), (nx_e, fs_e) = CASES["a"], CASES["d"], CASES["e"]
    recs = [signal(channels, nx_a, np.float32), signal(channels, 800, np.float32) * 0.5, signal(channels, nx_e, np.float64), signal(channels, nx_d, np.float32)]
    freqs = [fs_a, TO_FREQ, fs_e, fs_d]
    alone = [resample_recording(torch.from_numpy(r).to(device), f) for r, f in zip(recs, freqs)]
    again = [resample_recording(torch.from_numpy(r).to(device), f) for r, f in zip(recs, freqs)]
    for a, b in zip(alone, again):
        assert torch.equal(a, b), "two calls in a row differ"
    # among others, through the staging buffer, into the padded layout
    signals, table = resample_recordings(recs, freqs, device=device)
    offset = 0
    for r, (a, (off, stride, samples)) in enumerate(zip(alone, table.tolist())):
        assert off == offset and stride == -(-samples // 4) * 4 and samples == a.shape[1], (r, off, stride, samples)
        block = signals[off:off + channels * stride].view(channels, stride)
        assert torch.equal(block[:, :samples], a), f"recording {r} differs inside the set"
        assert bool((block[:, samples:] == 0).all()), f"recording {r}: the padding is not zero"
        offset += channels * stride
    assert signals.numel() == offset and signals.dtype == torch.float32
    assert torch.equal(alone[1], torch.from_numpy(recs[1]).to(device)), "a recording at to_freq must be copied as given"
    # the same layout as layout_recordings of the resampled set
    from eeg_gnn_ssl_amd import layout_recordings
    want_signals, want_table = layout_recordings([a.cpu() for a in alone], device)
    assert torch.equal(want_table, table) and torch.equal(want_signals, signals)
    # all channels at once against the one-channel minimum (chunked)
    num_e = num_of(nx_e, fs_e)
    one = int(lib.query("eeg_dcrnn_resample_ws_bytes", nx_e, num_e, 1))
    full = int(lib.query("eeg_dcrnn_resample_ws_bytes", nx_e, num_e, channels))
    assert 0 < one < full
    xe = torch.from_numpy(recs[2]).to(device)
    for cap in (one, one + (full - one) // 2, full, 2 * full):
        assert torch.equal(resample_recording(xe, fs_e, workspace_bytes=cap), alone[2]), f"workspace_bytes={cap} changed the bits"
    # poisoned workspace and output, the C entry as it is: every sample written, nothing else
    stride = -(-num_e // 4) * 4 + 4
    for ws_bytes in (one, full):
        ws = _nan(ws_bytes // 8, device=device, dtype=torch.float64)
        flat = _nan(channels * stride + 8, device=device)
        before = flat.clone()
        out = flat[:channels * stride].view(channels, stride)
        assert _call_c(lib, xe, num_e, out, ws, out_stride=stride) == 0, lib.last_error()
        assert torch.equal(out[:, :num_e], alone[2]), "a poisoned workspace / output changed the bits"
        keep = torch.ones_like(flat, dtype=torch.bool)
        keep[:channels * stride].view(channels, stride)[:, :num_e] = False
        assert torch.equal(flat.view(torch.int32)[keep], before.view(torch.int32)[keep]), "something outside the output rows was written"


def check_layout_end_to_end(device):
    """`RecordingDataset.from_native_rate` over cases a and d and a recording already at 200 Hz: one gathered batch against the same
    clips cut out of the restatement"""
    from eeg_gnn_ssl_amd import EpochSampler, RecordingDataset
    channels, window, x_steps = 3, 200, 2
    (nx_a, fs_a), (nx_d, fs_d) = CASES["a"], CASES["d"]
    recs = [signal(channels, nx_a, np.float64), signal(channels, nx_d, np.float32), signal(channels, 1000, np.float32)]
    freqs = [fs_a, float(fs_d), TO_FREQ]
    table = np.array([[0, 0, 400, 0], [1, 200, 400, 0], [2, 600, 400, 0], [0, 200, 400, 0], [2, 0, 400, 0]], dtype=np.int64)
    y = torch.arange(len(table), dtype=torch.float32, device=device)
    ds = RecordingDataset.from_native_rate(recs, freqs, table, y, window=window, x_steps=x_steps, device=device)
    assert ds.N == channels and ds.rec_table[:, 2].tolist() == [600, 600, 1000]
    sampler = EpochSampler(len(table), len(table), 7, 0, 1, device=device)           # no epoch begun: the identity permutation
    x_out, y_out = _nan(len(table), channels, x_steps * window, device=device), _nan(len(table), device=device)
    len_out = torch.zeros(len(table), dtype=torch.int64, device=device)
    ds.gather(sampler, x_out, y_out, len_out)
    assert torch.equal(y_out, y) and len_out.tolist() == [x_steps] * len(table)
    for p, (rec, start, samples, _) in enumerate(table.tolist()):
        if rec == 2:
            assert torch.equal(x_out[p].cpu(), torch.from_numpy(recs[2][:, start:start + samples])), "the 200 Hz recording is not bit-equal"
            continue
        x64 = recs[rec].astype(np.float64)
        ref = restate(x64, 600)[:, start:start + samples]
        err = np.abs(x_out[p].cpu().numpy().astype(np.float64) - ref)
        bound = 2.0 ** -24 * np.abs(ref) + 1e-12 * np.abs(x64).max(axis=1, keepdims=True)
        print(f"clip {p}: max |x - ref| = {err.max():.3e}, worst error / bound = {(err / bound).max():.4f}")
        assert (err <= bound).all(), (p, float(err.max()))


def check_refusals(device):
    """every ValueError of the host layer and of the operator, by message and BEFORE any launch (the event recorder sees none); the C
    entry refuses the same and names the argument"""
    from parity_suite import kernels_run
    from eeg_gnn_ssl_amd import RecordingDataset, _lib, ops, resample_recording, resample_recordings, resampled_length
    lib = _lib.get_lib()
    x = torch.from_numpy(signal(3, 757, np.float32)).to(device)
    h = signal(3, 757, np.float32)

    def refused():
        for fn, text in (
                (lambda: resample_recording(x.half(), 250), r"dtype torch.float16; a recording is float32 or float64"),
                (lambda: resample_recording(x.long(), 250), r"dtype torch.int64"),
                (lambda: resample_recording(x[0], 250), r"shape \(757,\); a recording is 2-D"),
                (lambda: resample_recording(x[None], 250), r"a recording is 2-D"),
                (lambda: resample_recording(x, 0), r"sample_freq=0 must be a finite positive number"),
                (lambda: resample_recording(x, -250.0), r"sample_freq=-250.0 must be a finite positive number"),
                (lambda: resample_recording(x, float("nan")), r"sample_freq=nan must be a finite positive"),
                (lambda: resample_recording(x, float("inf")), r"sample_freq=inf must be a finite positive"),
                (lambda: resample_recording(x, 250, to_freq=0), r"to_freq=0 must be a finite positive"),
                (lambda: resample_recording(x, 1000), r"757 samples at 1000 Hz are shorter than one second"),
                (lambda: resample_recording(x, 250, n_out=0), r"n_out=0 \(>= 1\)"),
                (lambda: resample_recording(x, 250, n_out=MAX_SAMPLES + 1), r"4194305 output samples per channel; at most 4194304 \(EEG_RESAMPLE_MAX_SAMPLES"),
                (lambda: resample_recording(x[:, :1], 250, n_out=4), r"1 samples per channel; 2\.\.4194304 \(EEG_RESAMPLE_MAX_SAMPLES"),
                (lambda: resample_recording(torch.zeros(1, MAX_SAMPLES + 1, device="meta"), 250), r"4194305 samples per channel; 2\.\.4194304"),
                (lambda: resample_recording(x, 250, workspace_bytes=1024), r"workspace_bytes=1024 is below the \d+ bytes one channel"),
                (lambda: resample_recording(x.clone().requires_grad_(), 250), r"requires grad; resampling has no gradient formula"),
                (lambda: resample_recording(x.t().contiguous().t(), 250), r"rows of x must be contiguous"),
                (lambda: torch.ops.eeg_dcrnn.resample(x, 0), r"n_out=0 output samples"),
                (lambda: torch.ops.eeg_dcrnn.resample(x[0], 600), r"x must be a 2-D"),
                (lambda: torch.ops.eeg_dcrnn.resample(x.int(), 600), r"x must be a 2-D \(channels, samples\) tensor of torch.float32 or torch.float64"),
                (lambda: torch.ops.eeg_dcrnn.resample(x.clone().requires_grad_(), 600), r"requires grad"),
                (lambda: ops.resample_into(x, torch.zeros(2, 600, device=device)), r"out is \(2, 600\)"),
                (lambda: ops.resample_into(x, torch.zeros(3, 600, device=device, dtype=torch.float64)), r"out must be a 2-D .* torch.float32"),
                (lambda: resample_recordings([h, h], [250], device=device), r"1 sample_freqs for 2 recordings"),
                (lambda: resample_recordings([], [], device=device), r"no recordings"),
                (lambda: resample_recordings([h, h[:2]], [250, 250], device=device), r"recording 1 has 2 channels, recording 0 has 3"),
                (lambda: resample_recordings([h, h.astype(np.int16)], [250, 250], device=device), r"recording 1: dtype int16"),
                (lambda: resample_recordings([h, h[0]], [250, 250], device=device), r"recording 1: shape \(757,\)"),
                (lambda: resample_recordings([h, h], [250, 0.0], device=device), r"recording 1: sample_freq=0.0"),
                (lambda: resample_recordings([h, h[:, :100]], [250, 250], device=device), r"recording 1: 100 samples at 250 Hz are shorter than one second"),
                (lambda: RecordingDataset.from_native_rate([h], [250, 256], np.array([[0, 0, 400, 0]]), torch.zeros(1, device=device), window=200,
                                                           x_steps=2, device=device), r"2 sample_freqs for 1 recordings"),
                (lambda: resampled_length(-1, 250), r"samples=-1 must be a non-negative integer"),
        ):
            with pytest.raises(ValueError, match=text):
                fn()
    assert kernels_run(refused) == {}, "a refused call launched a kernel"

    # the C entry and its size query
    q = lambda *a: int(lib.query("eeg_dcrnn_resample_ws_bytes", *a))     # noqa: E731
    need = q(757, 600, 3)
    assert need > q(757, 600, 1) > 0 and need == (2048 + 1024 + 3 * 2048) * 16 and q(1203, 600, 1) == (2048 + 1024 + 2048) * 16
    for shape in ((1, 600, 3), (0, 600, 3), (-5, 600, 3), (MAX_SAMPLES + 1, 600, 3), (757, 0, 3), (757, MAX_SAMPLES + 1, 3), (757, 600, 0), (757, 600, -1)):
        assert q(*shape) == 0, shape
    assert q(MAX_SAMPLES, MAX_SAMPLES, 1) == 3 * (1 << 23) * 16 and q(2, 1, 1) > 0
    ws = _nan(need // 8 + 2, device=device, dtype=torch.float64)
    out = _nan(3, 600, device=device)

    def c_refused():
        for kwargs, text in (
                (dict(ws_bytes=q(757, 600, 1) - 16), r"resample: ws_bytes=\d+ below the \d+ bytes of one channel"),
                (dict(in_stride=756), r"resample: in_stride=756 below n_in=757"),
                (dict(out_stride=599), r"resample: out_stride=599 below n_out=600"),
                (dict(n_in=1), r"resample: n_in=1 samples unsupported \(2\.\.4194304\)"),
                (dict(n_in=MAX_SAMPLES + 1, in_stride=MAX_SAMPLES + 1), r"resample: n_in=4194305 samples unsupported"),
        ):
            assert _call_c(lib, x, 600, out, ws, **kwargs) != 0, kwargs
            assert re.search(text, lib.last_error()), (kwargs, lib.last_error())
        assert _call_c(lib, x, 0, out, ws, out_stride=600) != 0 and "n_out=0" in lib.last_error()
        assert _call_c(lib, x, 600, out, ws[1:].view(torch.float32)[1:]) != 0 and "16-byte aligned" in lib.last_error()
        from eeg_gnn_ssl_amd.ops import _p, _stream
        assert lib.query("eeg_dcrnn_resample", None, 0, 3, 757, 757, 600, _p(out), 600, _p(ws), need, _stream(x)) != 0 and "null" in lib.last_error()
    assert kernels_run(c_refused) == {}, "a refused C call launched a kernel"
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(ws).all()), "a refused call wrote"
    assert _call_c(lib, x, 600, out, ws, ws_bytes=need) == 0 and bool(torch.isfinite(out).all())      # and the same arguments, accepted, run


def check_fake():
    """the operator under FakeTensorMode: shape and dtype, no data"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    import eeg_gnn_ssl_amd  # noqa: F401
    with FakeTensorMode():
        for dtype in (torch.float32, torch.float64):
            y = torch.ops.eeg_dcrnn.resample(torch.empty(19, 757, dtype=dtype), 600)
            assert tuple(y.shape) == (19, 600) and y.dtype == torch.float32
        y = torch.ops.eeg_dcrnn.resample(torch.empty(19, 757), 600, 1 << 20)
        assert tuple(y.shape) == (19, 600)
