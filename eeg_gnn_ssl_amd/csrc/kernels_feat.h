// Input featurisation on the GPU: 1-second windows -> log|FFT| of the positive
// frequencies -> optional augmentation (left/right reflection = node permutation, amplitude jitter =
// additive log scale) -> z-score.  Reference (CPU, in the DataLoader): data_utils.py:13-35 computeFFT
// (scipy.fftpack, float64), dataloader_detection.py:57-71 (windowing), :233-256 (augmentation),
// utils.py:393-428 (StandardScaler).
//
// The reference transforms float64 signals; log amplitudes of weak bins amplify any error of the
// transform, so the DFT here runs in fp64 (the MI355X vector unit does 39 T fp64 FMA/s; the whole
// kernel is ~0.5 ms for 256 one-minute clips).  One wave per (clip, node, window group): the W samples
// of a window sit in LDS as doubles (broadcast reads), lane k < W/4+1 owns the frequency pair
// (k, W/2-k), whose twiddles differ only by (-1)^n: four sums over even / odd samples give both bins.
// Twiddles advance by complex rotation (error ~W*eps).  Needs W % 4 == 0, W/4 + 1 <= 64.
#pragma once
#include "common.h"

namespace eeg {

// source channel of node nd under the reflection augmentation; an entry outside 0..N-1 (not a permutation: caller error) falls back to
// the node itself instead of addressing another clip's signals / features
__device__ __forceinline__ int perm_source(const int* __restrict__ perm, int b, int N, int nd) {
    if (perm == nullptr) return nd;
    const int s = perm[b * N + nd];
    return (unsigned)s < (unsigned)N ? s : nd;
}

// The window body of the direct DFT, shared by the storing kernel below and the reducing kernel of kernels_moments.h (the same
// instructions on the same operands: both see the same values).  xs: the W samples of the window as doubles (LDS, wave-private);
// lane k <= W/4 owns the frequency pair (k, W/2 - k), (c1, s1) = (cos, sin) of 2 pi k / W; emit(bin, log amplitude) is called for
// the lane's one or two bins.
template <class Emit>
__device__ __forceinline__ void dft_window(const double* xs, int W, int lane, double c1, double s1, Emit&& emit) {
    const int H2 = W / 2;
    double ec = 0.0, es = 0.0, oc = 0.0, os = 0.0, c = 1.0, s = 0.0;
    for (int n = 0; n < W; n += 2) {
        const double x0 = xs[n], x1 = xs[n + 1];
        ec = fma(x0, c, ec); es = fma(x0, s, es);
        double cn = c * c1 - s * s1, sn = s * c1 + c * s1;
        oc = fma(x1, cn, oc); os = fma(x1, sn, os);
        c = cn * c1 - sn * s1; s = sn * c1 + cn * s1;
    }
    auto bin = [&](int k, double re, double im) {
        double amp = sqrt(re * re + im * im);
        if (amp == 0.0) amp = 1e-8;                // computeFFT: avoid log of 0
        emit(k, log(amp));
    };
    if (lane < H2) bin(lane, ec + oc, es + os);
    if (lane > 0 && H2 - lane > lane && H2 - lane < H2) bin(H2 - lane, ec - oc, es - os);
}

// LEN (variable-length clips, dataloader_classification.py:25-85,321-343: a clip has curr_len <= max_seq_len steps, is augmented and
// standardised as it is and THEN padded with padding_val): clip b has clip_steps(lengths, b, T) valid windows; a window behind them is
// not transformed -- its feat_std row is pad_val (the padding behind the scaler), its feat_raw row 0 (adds nothing to a Gram).
template <bool LEN>
__global__ __launch_bounds__(64) void fft_features_kernel(const float* __restrict__ raw, int N, int T, int W, int tchunk,
                                                          const int* __restrict__ perm, const float* __restrict__ log_scale,
                                                          float mean, float inv_std, float* __restrict__ feat_raw,
                                                          float* __restrict__ feat_std, const long long* __restrict__ lengths,
                                                          float pad_val) {
    EEG_DYN_SMEM(sm);
    double* xs = reinterpret_cast<double*>(sm);          // [W]
    const int lane = threadIdx.x, b = blockIdx.x / N, nd = blockIdx.x % N, H2 = W / 2;
    const int src = perm_source(perm, b, N, nd);            // EEG_seq_reflect[:, pair] = EEG_seq[:, swapped pair]
    const double ls = log_scale != nullptr ? (double)log_scale[b] : 0.0;
    const float* sig = raw + ((size_t)b * N + src) * (size_t)T * W;
    const bool active = lane <= W / 4;
    double c1 = 1.0, s1 = 0.0;
    if (active) sincos(6.283185307179586476925286766559 * (double)lane / (double)W, &s1, &c1);
    const int t0 = blockIdx.y * tchunk, t1 = (t0 + tchunk < T) ? t0 + tchunk : T;
    int tv = T;
    if constexpr (LEN) tv = clip_steps(lengths, b, T);
    for (int t = t0; t < t1; ++t) {
        if constexpr (LEN) {
            if (t >= tv) {                                // padding (wave-uniform): the un-augmented zero row stays at the source channel
                const size_t o_raw = (((size_t)b * T + t) * N + src) * H2, o_std = (((size_t)b * T + t) * N + nd) * H2;
                for (int k = lane; k < H2; k += 64) {
                    if (feat_raw != nullptr) feat_raw[o_raw + k] = 0.f;
                    if (feat_std != nullptr) feat_std[o_std + k] = pad_val;
                }
                continue;
            }
        }
        EEG_WAVE_SYNC();                                  // previous window fully consumed
        for (int i = lane; i < W; i += 64) xs[i] = (double)sig[(size_t)t * W + i];
        EEG_WAVE_SYNC();
        if (active) {
            // the un-augmented features stay at the source channel (perm is a permutation: every slot is written once)
            const size_t o_raw = (((size_t)b * T + t) * N + src) * H2, o_std = (((size_t)b * T + t) * N + nd) * H2;
            dft_window(xs, W, lane, c1, s1, [&](int k, double v) {
                if (feat_raw != nullptr) feat_raw[o_raw + k] = (float)v;
                if (feat_std != nullptr) feat_std[o_std + k] = (float)(((v + ls) - (double)mean) * (double)inv_std);
            });
        }
    }
}


// ---- W = 200 (the reference's 200 Hz x 1-s steps, dataloader_detection.py:54-67): mixed-radix real transform -----------------
// The direct DFT above does 2 x 200 x 100 multiply-adds per window (23 GFLOP fp64 for 256 one-minute clips = 5 x the HBM floor
// of this kernel).  Here: z[n] = x[2n] + i x[2n+1] (n < 100), Z = DFT_100(z) as 10 x 10 Cooley-Tukey with every 10-point DFT done
// in registers as a 2 x 5 prime-factor transform (no twiddles inside), then the real-input split
//     2 X[k] = (Z[k] + conj Z[100-k]) - i e^{-2 pi i k / 200} (Z[k] - conj Z[100-k]),   k = 0..99,
// all in fp64 (the log of a weak bin amplifies any error of the transform, see above): ~3 k fp64 operations per window instead of
// 160 k.  Ten lanes own one window, six windows per wave (lanes 60..63 idle); a wave walks 6 CONSECUTIVE (b, t, node) windows, whose
// outputs are one contiguous 2400-byte stretch of feat_std: the log amplitudes leave through a wave-private LDS tile as full
// 16-byte pieces.  Wave-private LDS (11.3 KB), wave-level syncs only, no workgroup barrier.
struct cplx { double re, im; };
__device__ __forceinline__ cplx cadd(cplx a, cplx b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cplx csub(cplx a, cplx b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
// forward 5-point DFT (kernel e^{-2 pi i n k / 5})
__device__ __forceinline__ void dft5(const cplx (&x)[5], cplx (&X)[5]) {
    constexpr double C1 = 0.30901699437494742410, C2 = -0.80901699437494742410;    // cos(2 pi / 5), cos(4 pi / 5)
    constexpr double S1 = 0.95105651629515357212, S2 = 0.58778525229247312917;     // sin(2 pi / 5), sin(4 pi / 5)
    const cplx s1 = cadd(x[1], x[4]), s2 = cadd(x[2], x[3]), d1 = csub(x[1], x[4]), d2 = csub(x[2], x[3]);
    X[0] = {x[0].re + s1.re + s2.re, x[0].im + s1.im + s2.im};
    const cplx a1 = {x[0].re + C1 * s1.re + C2 * s2.re, x[0].im + C1 * s1.im + C2 * s2.im};
    const cplx a2 = {x[0].re + C2 * s1.re + C1 * s2.re, x[0].im + C2 * s1.im + C1 * s2.im};
    const cplx b1 = {S1 * d1.re + S2 * d2.re, S1 * d1.im + S2 * d2.im};
    const cplx b2 = {S2 * d1.re - S1 * d2.re, S2 * d1.im - S1 * d2.im};
    X[1] = {a1.re + b1.im, a1.im - b1.re};        // a1 - i b1
    X[4] = {a1.re - b1.im, a1.im + b1.re};        // a1 + i b1
    X[2] = {a2.re + b2.im, a2.im - b2.re};
    X[3] = {a2.re - b2.im, a2.im + b2.re};
}
// forward 10-point DFT as a 2 x 5 prime-factor transform: n = 5 n1 + 2 n2, k = 5 k1 + 6 k2 (mod 10) => W10^{nk} = (-1)^{n1 k1} W5^{n2 k2}
__device__ __forceinline__ void dft10(const cplx (&x)[10], cplx (&X)[10]) {
    cplx u[5], y0[5], y1[5];
#pragma unroll
    for (int n2 = 0; n2 < 5; ++n2) u[n2] = x[(2 * n2) % 10];
    dft5(u, y0);
#pragma unroll
    for (int n2 = 0; n2 < 5; ++n2) u[n2] = x[(5 + 2 * n2) % 10];
    dft5(u, y1);
#pragma unroll
    for (int k2 = 0; k2 < 5; ++k2) {
        X[(6 * k2) % 10] = cadd(y0[k2], y1[k2]);
        X[(5 + 6 * k2) % 10] = csub(y0[k2], y1[k2]);
    }
}

#ifndef EEG_FFT_MINW
#define EEG_FFT_MINW 2          // waves per SIMD the kernel is compiled for (176 registers; 3 = 168 + 9 spilled: measured)
#endif
constexpr int kFftWin = 200, kFftBins = 100, kFftPerWave = 6, kFftWgPerCu = EEG_FFT_MINW;
constexpr int kFftRow = 11;                                              // transposed tile: 16-byte entries, row stride 11 (conflict-free)
constexpr int kFftWaveDoubles = kFftPerWave * 10 * kFftRow * 2;          // 1320 doubles = 10.3 KB per wave (the Z and output tiles alias it)

// twiddles of a lane: stage 1 -> 2: W100^{q k1}, k1 = 0..9; real-input split: W200^{q + 10 k2}, k2 = 0..9
__device__ __forceinline__ void fft200_twiddles(int q, cplx (&tw1)[10], cplx (&tw2)[10]) {
    // two sincos per lane; the other 18 twiddles by complex rotation (error ~10 eps; twenty library sincos calls were 3 000
    // instructions = 5 us in front of every wave's first window)
    double sn, cs;
    sincos(6.283185307179586476925286766559 * (double)q / 100.0, &sn, &cs);
    const cplx r1 = {cs, -sn};                                           // W100^q
    sincos(6.283185307179586476925286766559 * (double)q / 200.0, &sn, &cs);
    const cplx r2 = {cs, sn};                                            // (cos, sin) of 2 pi q / 200
    const cplx s2 = {0.95105651629515357212, 0.30901699437494742410};    // (cos, sin) of 2 pi 10 / 200
    tw1[0] = {1.0, 0.0};
    tw2[0] = r2;
#pragma unroll
    for (int j = 1; j < 10; ++j) {
        tw1[j] = cmul(tw1[j - 1], r1);
        tw2[j] = cmul(tw2[j - 1], s2);                                   // (cos, sin) of 2 pi (q + 10 j) / 200: the split uses both signs explicitly
    }
}

// the 16-byte piece at `pos` of a PADDED window wj = (bt, nd) of clip b: pad_val in feat_std at the window's own slot, 0 in feat_raw
// at the source node's slot (where a transformed window's un-augmented row goes)
__device__ __forceinline__ void fft200_store_pad(int N, const int* __restrict__ perm, float* __restrict__ feat_raw, float* __restrict__ feat_std,
                                                 long long wj, long long bt, int b, int nd, int pos, float pad_val) {
    if (feat_raw != nullptr) {
        const int src = perm_source(perm, b, N, nd);
        *reinterpret_cast<f32x4*>(feat_raw + ((size_t)bt * N + src) * kFftBins + pos) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (feat_std != nullptr) *reinterpret_cast<f32x4*>(feat_std + (size_t)wj * kFftBins + pos) = f32x4{pad_val, pad_val, pad_val, pad_val};
}

// The transform of the wave's six windows, shared by the storing item below and the reducing kernel of kernels_moments.h (the same
// instructions on the same operands: both see the same values).  Lane (w, q) of a LIVE window reads its samples at sig_of() (the
// 200 floats of the window; called by live lanes only) and leaves with v[k2] = the float32 log amplitude of bin q + 10 k2; the ten
// lanes of a window that is not live sit the transform out.  tile: the wave's kFftWaveDoubles doubles of LDS; the caller syncs the
// wave before it reuses them.
template <class Sig>
__device__ __forceinline__ void fft200_windows(Sig&& sig_of, bool live, int w, int q, cplx* tile, const cplx (&tw1)[10], const cplx (&tw2)[10],
                                               double log_floor, float (&v)[10]) {
    cplx a[10], A[10];
    if (live) {
        const float* sig = sig_of();
#pragma unroll
        for (int n1 = 0; n1 < 10; ++n1) {
            const f32x2 z = *reinterpret_cast<const f32x2*>(sig + 20 * n1 + 2 * q);        // z[10 n1 + q]
            a[n1] = {(double)z[0], (double)z[1]};
        }
        dft10(a, A);                                                 // over n1 -> k1
#pragma unroll
        for (int k1 = 0; k1 < 10; ++k1) tile[(w * 10 + q) * kFftRow + k1] = cmul(A[k1], tw1[k1]);
    }
    EEG_WAVE_SYNC();
    if (live) {
#pragma unroll
        for (int n2 = 0; n2 < 10; ++n2) a[n2] = tile[(w * 10 + n2) * kFftRow + q];
        dft10(a, A);                                                 // over n2 -> k2: A[k2] = Z[q + 10 k2]
    }
    EEG_WAVE_SYNC();
    if (live) {
#pragma unroll
        for (int k2 = 0; k2 < 10; ++k2) tile[w * 110 + q + 10 * k2] = A[k2];              // Z[k] at [w][k]
    }
    EEG_WAVE_SYNC();
    if (live) {
#pragma unroll
        for (int k2 = 0; k2 < 10; ++k2) {
            const int k = q + 10 * k2;
            const cplx zp = tile[w * 110 + (k == 0 ? 0 : 100 - k)];
            const double ar = A[k2].re + zp.re, ai = A[k2].im - zp.im;                    // Z[k] + conj Z[100-k]
            const double br = A[k2].re - zp.re, bi = A[k2].im + zp.im;                    // Z[k] - conj Z[100-k]
            const double xr = ar + (tw2[k2].re * bi - tw2[k2].im * br);
            const double xi = ai - (tw2[k2].re * br + tw2[k2].im * bi);
            const double pw = 0.25 * (xr * xr + xi * xi);
            // log|X| = ln2/2 * (e + log2 m), |X|^2 = m 2^e with m in [0.5, 1): the exponent split is exact in fp64, the mantissa's
            // log2 is one v_log_f32 (absolute error ~1e-7 on a value in (-1, 0]) and the two parts are combined in fp64 -- the fp64
            // library log (~70 fp64 instructions per bin) was 60 % of this kernel's instructions
            int ex;
            const double mant = frexp(pw, &ex);
            const double lg = 0.34657359027997264 * ((double)ex + (double)fast_log2((float)mant));
            v[k2] = (float)(pw == 0.0 ? log_floor : lg);
        }
    }
}

// One item = 6 consecutive (b, t, node) windows of ONE (B, N, T*200) buffer, transformed by one wave (the body shared by the
// single-buffer and the paired kernel: the same instructions on the same operands, so both give the same bits).
// LEN: windows (b, t >= clip_steps(lengths, b, T)) are padding (see fft_features_kernel).  `vmask` = the valid windows of the item, the
// same value in every lane: an item wholly in padding stores its 150 pad pieces and returns (a wave-uniform branch: no load, no
// transform); in an item that straddles the end of a clip -- or two rows or clips when 6 does not divide N -- the ten lanes of a
// padded window sit the transform out and its pieces leave as padding.  A valid window takes the instructions of the plain item.
template <bool LEN = false>
__device__ __forceinline__ void fft200_item(const float* __restrict__ raw, int N, int T, long long n_windows, const int* __restrict__ perm,
                                            const float* __restrict__ log_scale, float mean, float inv_std, float* __restrict__ feat_raw,
                                            float* __restrict__ feat_std, long long item, cplx* tile, int lane, const cplx (&tw1)[10],
                                            const cplx (&tw2)[10], double log_floor, const long long* __restrict__ lengths = nullptr,
                                            float pad_val = 0.f) {
    float* ftile = reinterpret_cast<float*>(tile);                       // [6][100] log amplitudes (aliases the tile, behind a wave sync)
    const int w = lane / 10, q = lane - 10 * w;                          // window of the wave, position (n2 in stage 1, k1 in stage 2)
    const bool active = w < kFftPerWave;
    const long long w0 = item * kFftPerWave, wg = w0 + w;
    unsigned vmask = (1u << kFftPerWave) - 1u;
    if constexpr (LEN) {
        vmask = 0u;
        const long long bt0 = w0 / N;
        int nd = (int)(w0 % N), t = (int)(bt0 % T), b = (int)(bt0 / T);
        for (int j = 0; j < kFftPerWave && w0 + j < n_windows; ++j) {    // (b < B while w0 + j < n_windows: lengths is read in bounds)
            if (t < clip_steps(lengths, b, T)) vmask |= 1u << j;
            if (++nd == N) { nd = 0; if (++t == T) { t = 0; ++b; } }
        }
        vmask = (unsigned)wave_uniform((int)vmask);
        if (vmask == 0u) {
            for (int c = lane; c < kFftPerWave * kFftBins / 4; c += 64) {
                const int j = c / 25, pos = 4 * (c - 25 * j);
                const long long wj = w0 + j;
                if (wj >= n_windows) continue;
                const long long bt = wj / N;
                fft200_store_pad(N, perm, feat_raw, feat_std, wj, bt, (int)(bt / T), (int)(wj % N), pos, pad_val);
            }
            return;
        }
    }
    const bool live = active && wg < n_windows && (!LEN || ((vmask >> w) & 1u) != 0u);
    auto sig_of = [&]() {
        const int nd = (int)(wg % N);
        const long long bt = wg / N;
        const int t = (int)(bt % T), b = (int)(bt / T);
        const int src = perm_source(perm, b, N, nd);     // EEG_seq_reflect[:, pair] = EEG_seq[:, swapped pair]
        return raw + (((size_t)b * N + src) * T + t) * kFftWin;
    };
    float v[10];
    fft200_windows(sig_of, live, w, q, tile, tw1, tw2, log_floor, v);
    EEG_WAVE_SYNC();                                                 // every partner read is done: the tile becomes the output tile
    if (live) {
#pragma unroll
        for (int k2 = 0; k2 < 10; ++k2) ftile[w * kFftBins + q + 10 * k2] = v[k2];
    }
    EEG_WAVE_SYNC();
    // 6 windows x 100 floats leave as 16-byte pieces: feat_std at the window's own (b, t, node) slot (6 windows = one 2400-byte
    // stretch), feat_raw at the SOURCE node's slot (perm is a permutation: every slot is written once)
    for (int c = lane; c < kFftPerWave * kFftBins / 4; c += 64) {
        const int j = c / 25, pos = 4 * (c - 25 * j);
        const long long wj = w0 + j;
        if (wj >= n_windows) continue;
        const f32x4 val = *reinterpret_cast<const f32x4*>(ftile + 4 * c);
        const int nd = (int)(wj % N);
        const long long bt = wj / N;
        const int b = (int)(bt / T);
        if constexpr (LEN) {
            if (((vmask >> j) & 1u) == 0u) {
                fft200_store_pad(N, perm, feat_raw, feat_std, wj, bt, b, nd, pos, pad_val);
                continue;
            }
        }
        if (feat_raw != nullptr) {
            const int src = perm_source(perm, b, N, nd);
            *reinterpret_cast<f32x4*>(feat_raw + ((size_t)bt * N + src) * kFftBins + pos) = val;
        }
        if (feat_std != nullptr) {
            const double ls = log_scale != nullptr ? (double)log_scale[b] : 0.0;
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (float)((((double)val[e] + ls) - (double)mean) * (double)inv_std);
            *reinterpret_cast<f32x4*>(feat_std + (size_t)wj * kFftBins + pos) = o;
        }
    }
    EEG_WAVE_SYNC();                                                 // the output tile is free again
}

template <bool LEN>
__global__ __launch_bounds__(256, EEG_FFT_MINW) void fft200_features_kernel(const float* __restrict__ raw, int N, int T, long long n_windows,
                                                              const int* __restrict__ perm, const float* __restrict__ log_scale,
                                                              float mean, float inv_std, float* __restrict__ feat_raw,
                                                              float* __restrict__ feat_std, const long long* __restrict__ lengths,
                                                              float pad_val) {
    EEG_DYN_SMEM(sm);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    cplx* tile = reinterpret_cast<cplx*>(sm) + (size_t)wave * (kFftWaveDoubles / 2);
    cplx tw1[10], tw2[10];
    fft200_twiddles(lane % 10, tw1, tw2);
    const double log_floor = log(1e-8);                                  // computeFFT: amp == 0 -> 1e-8
    const long long n_items = (n_windows + kFftPerWave - 1) / kFftPerWave;
    for (long long item = (long long)blockIdx.x * 4 + wave; item < n_items; item += (long long)gridDim.x * 4)
        fft200_item<LEN>(raw, N, T, n_windows, perm, log_scale, mean, inv_std, feat_raw, feat_std, item, tile, lane, tw1, tw2, log_floor, lengths,
                         pad_val);
}

// The SSL sample is a PAIR (dataloader_ssl.py:317-341): 60 s of input and the first seconds of the following clip as target, ONE
// coin and ONE scale factor per sample applied to both halves, then the scaler on both.  One grid walks the items of raw_x
// (B, N, Tx*200) and behind them those of raw_y (B, N, Ty*200) with the clip's perm[b] / log_scale[b]: one twiddle set-up per wave
// and one ramp for both halves; every item is fft200_item on its half, so each output equals the single-buffer kernel's bit for
// bit.  The target has no un-augmented output: the correlation graph is built from the input clip alone (dataloader_ssl.py:349).
// Only W = 200 has a paired kernel: for any other window the host runs fft_features_kernel once per half (nobody trains with one).
struct FftHalf {
    const float* raw;          // (B, N, T*200)
    int T;
    long long n_windows;       // B * N * T
    float* feat_raw;           // (B, T, N, 100), nullable
    float* feat_std;           // (B, T, N, 100), nullable
};
__global__ __launch_bounds__(256, EEG_FFT_MINW) void fft200_features_pair_kernel(FftHalf hx, FftHalf hy, int N, const int* __restrict__ perm,
                                                                                 const float* __restrict__ log_scale, float mean, float inv_std) {
    EEG_DYN_SMEM(sm);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    cplx* tile = reinterpret_cast<cplx*>(sm) + (size_t)wave * (kFftWaveDoubles / 2);
    cplx tw1[10], tw2[10];
    fft200_twiddles(lane % 10, tw1, tw2);
    const double log_floor = log(1e-8);
    const long long nix = (hx.n_windows + kFftPerWave - 1) / kFftPerWave, niy = (hy.n_windows + kFftPerWave - 1) / kFftPerWave;
    for (long long item = (long long)blockIdx.x * 4 + wave; item < nix + niy; item += (long long)gridDim.x * 4) {
        const bool second = item >= nix;                                 // wave-uniform: each half ends with its own partial item
        fft200_item(second ? hy.raw : hx.raw, N, second ? hy.T : hx.T, second ? hy.n_windows : hx.n_windows, perm, log_scale, mean, inv_std,
                    second ? hy.feat_raw : hx.feat_raw, second ? hy.feat_std : hx.feat_std, second ? item - nix : item, tile, lane, tw1, tw2,
                    log_floor);
    }
}

// Augmentation of already standardised features, the pair in one launch: out[b, t, n, :] = in[b, t, perm[b][n], :] + shift[b] for
// x (B, Tx, N, D) and y (B, Ty, N, D), shift[b] = log(scale_b) / std (adding log(scale) before the scaler = adding it over std
// behind it).  blockIdx.x = clip, blockIdx.y = a stretch of kAugPerBlock 16-byte pieces of the clip's (Tx + Ty) * N rows (x rows
// first): consecutive lanes hold consecutive pieces, so stores are whole lines and loads are whole 400-byte rows (D = 100: a row
// covers 3 1/8 lines of 128 bytes, the partial lines are shared with the neighbouring row of the same step).  One read, one write.
constexpr int kAugThreads = 256, kAugUnroll = 4, kAugPerBlock = kAugThreads * kAugUnroll;
template <int D4C>              // 16-byte pieces per row when known at compile time (25: D = 100), 0 = read D4
__global__ __launch_bounds__(kAugThreads) void augment_features_kernel(const float* __restrict__ x, const float* __restrict__ y, int N, int Tx,
                                                                       int Ty, int D4, const int* __restrict__ perm,
                                                                       const float* __restrict__ shift, float* __restrict__ x_out,
                                                                       float* __restrict__ y_out) {
    const int d4 = D4C > 0 ? D4C : D4, b = blockIdx.x;
    const unsigned rows_x = (unsigned)Tx * N, total = (rows_x + (unsigned)Ty * N) * d4;
    const float sh = shift[b];
    const unsigned e0 = blockIdx.y * (unsigned)kAugPerBlock + threadIdx.x;
    f32x4 v[kAugUnroll];
    size_t dst[kAugUnroll];
    bool in_y[kAugUnroll], on[kAugUnroll];
#pragma unroll
    for (int u = 0; u < kAugUnroll; ++u) {
        const unsigned e = e0 + u * kAugThreads;
        on[u] = e < total;
        if (!on[u]) continue;
        unsigned row = e / d4;
        const unsigned c = e - row * d4;
        in_y[u] = row >= rows_x;
        if (in_y[u]) row -= rows_x;
        const unsigned t = row / N, nd = row - t * N;
        const int src = perm_source(perm, b, N, (int)nd);
        const size_t clip = (size_t)b * (in_y[u] ? Ty : Tx) * N;
        dst[u] = ((clip + row) * d4 + c) * 4;
        v[u] = *reinterpret_cast<const f32x4*>((in_y[u] ? y : x) + ((clip + (size_t)t * N + src) * d4 + c) * 4);
    }
#pragma unroll
    for (int u = 0; u < kAugUnroll; ++u) {
        if (!on[u]) continue;
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = v[u][k] + sh;
        *reinterpret_cast<f32x4*>((in_y[u] ? y_out : x_out) + dst[u]) = o;
    }
}

// ---- time-domain inputs (the reference without --use_fft) -----------------------------------------------------------------------
// computeSliceMatrix(is_fft=False) (dataloader_detection.py:25-85) cuts the clip's channel rows into 1-s windows and nothing else:
// clip[t, n, :] = raw[n, t*W : (t+1)*W]; `_random_reflect` permutes the channels (:233-245), `_random_scale` MULTIPLIES the signals
// (`EEG_seq *= scale_factor`, :247-256), then the scaler (utils.py:393-428); the SSL loader does the same to both halves of its pair
// with one coin and one factor (dataloader_ssl.py:159-182,317-341).  Two routes to the model input, one kernel:
//   RAW  = true : in = raw signals (B, N, T*W) -> out[b, t, n, :] = (in[b, perm[b][n], t*W ..] * a[b] - mean) / std, the product and
//                 the difference as ONE fused multiply-add (one rounding, on the GPU and in any other build of this source)
//                 (a = the clip's scale factor, null = 1): windowing, augmentation and scaler in one read and one write; no
//                 un-augmented copy is written -- the correlation graph of a time-domain clip is that of the raw rows themselves;
//   RAW  = false: in = standardised windows (B, T, N, W) -> out[b, t, n, :] = in[b, t, perm[b][n], :] * a[b] + c[b], the product
//                 rounded before the sum like the framework's two kernels (a = s, c = (s - 1) * mean / std: the same augmentation
//                 applied behind the scaler).
// Launch shape of augment_features_kernel above: blockIdx.x = clip, blockIdx.y = a stretch of kAugPerBlock 16-byte pieces of the
// clip's (Tx + Ty) * N output rows (x rows first, Ty = 0: no second half), kAugUnroll pieces in flight per thread; consecutive
// lanes hold consecutive pieces, so stores are whole lines and loads whole rows of 4*W bytes.  Every element takes the same
// instructions whether its half travels alone or in a pair: the paired launch is a re-scheduling, bit for bit.
// LEN (single clip, Ty = 0; dataloader_classification.py:321-343: the short clip is scaled and standardised, then padded): the pieces
// of the steps t >= clip_steps(lengths, b, Tx) are not loaded, pad_val is stored in their place; every other piece as without LEN.
template <bool RAW, int D4C, bool LEN = false>    // D4C: 16-byte pieces per row when known at compile time (50: W = 200), 0 = read D4
__global__ __launch_bounds__(kAugThreads) void window_stream_kernel(const float* __restrict__ x, const float* __restrict__ y, int N, int Tx,
                                                                    int Ty, int D4, const int* __restrict__ perm, const float* __restrict__ a,
                                                                    const float* __restrict__ c, float mean, float std_,
                                                                    float* __restrict__ x_out, float* __restrict__ y_out,
                                                                    const long long* __restrict__ lengths, float pad_val) {
    const int d4 = D4C > 0 ? D4C : D4, b = blockIdx.x;
    unsigned tv = (unsigned)Tx;
    if constexpr (LEN) tv = (unsigned)clip_steps(lengths, b, Tx);
    bool pad[kAugUnroll];
    const unsigned rows_x = (unsigned)Tx * N, total = (rows_x + (unsigned)Ty * N) * d4;
    const float ab = a != nullptr ? a[b] : 1.0f, cb = (!RAW && c != nullptr) ? c[b] : 0.0f;
    const unsigned e0 = blockIdx.y * (unsigned)kAugPerBlock + threadIdx.x;
    f32x4 v[kAugUnroll];
    size_t dst[kAugUnroll];
    bool in_y[kAugUnroll], on[kAugUnroll];
#pragma unroll
    for (int u = 0; u < kAugUnroll; ++u) {
        const unsigned e = e0 + u * kAugThreads;
        on[u] = e < total;
        if (!on[u]) continue;
        unsigned row = e / d4;
        const unsigned p = e - row * d4;
        in_y[u] = row >= rows_x;
        if (in_y[u]) row -= rows_x;
        const unsigned t = row / N, nd = row - t * N;
        const unsigned T = in_y[u] ? Ty : Tx;
        const int src = perm_source(perm, b, N, (int)nd);
        const size_t clip = (size_t)b * T * N;
        dst[u] = ((clip + row) * d4 + p) * 4;
        pad[u] = LEN && t >= tv;
        if (pad[u]) { v[u] = f32x4{0.f, 0.f, 0.f, 0.f}; continue; }
        const size_t from = RAW ? (((size_t)b * N + src) * T + t) : (clip + (size_t)t * N + src);
        v[u] = *reinterpret_cast<const f32x4*>((in_y[u] ? y : x) + (from * d4 + p) * 4);
    }
#pragma unroll
    for (int u = 0; u < kAugUnroll; ++u) {
        if (!on[u]) continue;
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = (LEN && pad[u]) ? pad_val : RAW ? __builtin_fmaf(v[u][k], ab, -mean) / std_ : unfused_mul_add(v[u][k], ab, cb);
        *reinterpret_cast<f32x4*>((in_y[u] ? y_out : x_out) + dst[u]) = o;
    }
}

// Data augmentation drawn on the device (dataloader_detection.py:384-389: `_random_reflect` then `_random_scale` per sample, in the
// DataLoader workers): clip b takes Philox counter used[1] + b of the {seed, offset} pair `used` (eeg_dcrnn_rng_take): word 0 is the
// fair coin of `np.random.choice([True, False])` (top bit), word 1 the uniform of `np.random.uniform(0.8, 1.2)`.  Outputs, all
// read by later launches of the same step: flags[b]; perm[b][n] = the source channel of node n (swap_perm[n] if reflected, else n)
// and log_scale[b] = log(scale) -- the `perm` / `log_scale` operands of the featurisation kernels above; and, for the distance
// graph (`_get_combined_graph(swap_nodes)`, :405-409), the per-clip supports S_out[s][b] = flags[b] ? S_refl[s] : S_plain[s].
__global__ __launch_bounds__(128) void augment_draw_kernel(const unsigned long long* __restrict__ used, int N, const int* __restrict__ swap_perm,
                                                            int* __restrict__ flags, int* __restrict__ perm, float* __restrict__ log_scale,
                                                            const float* __restrict__ S_plain, const float* __restrict__ S_refl, int nsup,
                                                            float* __restrict__ S_out) {
    const int b = blockIdx.x, B = gridDim.x;
    const unsigned long long seed = used[0], c = used[1] + (unsigned long long)b;
    unsigned w[4];
    philox4x32_10((unsigned)c, (unsigned)(c >> 32), 0u, 0u, (unsigned)seed, (unsigned)(seed >> 32), w);
    const int reflect = (int)(w[0] >> 31);
    if (threadIdx.x == 0) {
        flags[b] = reflect;
        const double scale = 0.8 + 0.4 * ((double)w[1] * (1.0 / 4294967296.0));
        log_scale[b] = (float)log(scale);
    }
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        const int s = swap_perm[n];
        perm[b * N + n] = (reflect && (unsigned)s < (unsigned)N) ? s : n;
    }
    if (S_out != nullptr) {
        const int NN = N * N;
        for (int e = threadIdx.x; e < nsup * NN; e += blockDim.x) {
            const int s = e / NN, r = e - s * NN;
            S_out[((size_t)s * B + b) * NN + r] = reflect ? S_refl[e] : S_plain[e];
        }
    }
}

}  // namespace eeg
