// Fourier resampling of whole native-rate recordings to the model's rate (the reference's data/resample_signals.py:38-43 ->
// data/data_utils.py:158-170 `resampleData` = scipy.signal.resample over the whole recording): per channel row x of Nx samples and
// `num` output samples, in float64,
//   X = rfft(x);  N = min(num, Nx);  Y[0 .. N/2] = X[0 .. N/2], zero above;  N even: Y[N/2] *= 2 (num < Nx) or 0.5 (Nx < num);
//   y = irfft(Y, num) * num / Nx, rounded ONCE to float32 on the store.
// Lengths are arbitrary (prime ones included), so both transforms are Bluestein chirp-z transforms on power-of-two float64 complex
// FFTs:   sum_n a[n] e^{s i 2 pi n k / L} = c[k] * sum_n (a[n] c[n]) conj(c)[k - n],   c[m] = e^{s i pi m^2 / L},
// a circular convolution of length M >= (inputs + outputs - 1) with the chirp filter conj(c), whose spectrum is built once per call and
// shared by the channels.  Forward: Nx inputs and only the bins 0 .. N/2 out (M1 >= Nx + N/2); inverse: the K = num/2 + 1 one-sided bins in,
// num samples out, y = Re(sum_k Z[k] e^{+i 2 pi j k / num}) / Nx with Z = 2 Y (Z[0] = Re Y[0]; num even: Z[num/2] = Re Y[num/2]).
//
// The phase of a chirp is reduced exactly in integers, r = m^2 mod 2L (m < 2^22: no overflow in 64 bits), then sincos(pi r / L).
//
// The power-of-two FFT (rs_fft_pass_kernel): the convolution needs no ordered spectrum, so the forward transform is decimation in
// frequency (natural in, digit-reversed out), the inverse its exact mirror (decimation in time), and every global pass works IN PLACE:
// a pass splits each sub-block of Mp = L * S points into S interleaved L-point transforms (element j of transform `rest` at rest + j * S),
// multiplies output k1 by w_Mp^(rest * k1) and leaves S-point sub-blocks to the next pass.  A workgroup holds a tile of 2^kRsPassTileBits
// points (G = tile / L transforms of adjacent `rest`, g fastest in LDS and in global memory) and runs the L-point radix-2 stages in LDS with
// a twiddle table of L/2 entries it builds itself.  The pass at S = 1 is shared by the forward and the inverse transform: load, FFT,
// multiply by the filter spectrum, inverse FFT, store (MODE kRsBoth).  Plan: M <= kRsTile is one pass; else ceil(log2 M / kRsPassBits)
// passes of evenly split bits (rs_plan).  No atomics, one fixed order of operations per element: a channel's bits depend on its samples
// and (Nx, num) alone.  Every index is masked / tested against the extents the host passed; nothing outside out rows and the workspace
// is written.
#pragma once
#include <cmath>

#include "common.h"

namespace eeg {

constexpr int kRsThreads = 256;
constexpr int kRsTileBits = 12;                         // the largest one-pass transform: 4096 float64 complex = 64 KiB of LDS
constexpr int kRsTile = 1 << kRsTileBits;
constexpr int kRsPassBits = 8;                          // a global pass of a transform above one tile takes at most 256-point sub-transforms
constexpr int kRsPassTileBits = 10;                     // ... on tiles of 1024 points (16 KiB: eight workgroups share a CU's LDS and overlap
                                                        // their load, LDS and store phases; measured 4096 -> 1024: the passes take 0.57 x)
constexpr int kRsMinBits = 6;                           // the smallest transform (64 points)
constexpr int kRsMaxBits = 23;                          // EEG_RESAMPLE_MAX_SAMPLES = 2^22 -> M <= 2^23
constexpr int kRsMaxPasses = 3;
constexpr double kRsPi = 3.14159265358979323846;
enum RsMode { kRsFwd = 0, kRsInv = 1, kRsBoth = 2 };

struct alignas(16) rs_c64 { double re, im; };
__host__ __device__ inline rs_c64 rs_mul(rs_c64 a, rs_c64 b) { return rs_c64{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__host__ __device__ inline rs_c64 rs_mulc(rs_c64 a, rs_c64 b) { return rs_c64{a.re * b.re + a.im * b.im, a.im * b.re - a.re * b.im}; }   // a * conj(b)

// the passes of an M = 2^lm point transform, first (largest stride) to last (stride 1): bits[p] = log2 of the sub-transform length
struct RsPlan { int lm = 0, passes = 0, bits[kRsMaxPasses] = {0, 0, 0}; };
inline RsPlan rs_plan(int lm) {
    RsPlan p;
    p.lm = lm;
    if (lm <= kRsTileBits) { p.passes = 1; p.bits[0] = lm; return p; }
    p.passes = (lm + kRsPassBits - 1) / kRsPassBits;
    for (int i = 0; i < p.passes; ++i) p.bits[i] = lm / p.passes + (i < lm % p.passes ? 1 : 0);
    return p;
}
// log2 of the transform length of a chirp-z with `need` = inputs + outputs - 1 points
inline int rs_log2_len(long long need) {
    int lm = kRsMinBits;
    while ((1ll << lm) < need) ++lm;
    return lm;
}
// LDS of a pass: the tile of 2^(lbits + gbits) points and the L/2 twiddles
inline size_t rs_pass_lds(int lbits, int gbits) { return (((size_t)1 << (lbits + gbits)) + ((size_t)1 << lbits) / 2) * sizeof(rs_c64); }
constexpr size_t kRsMaxLds = ((size_t)kRsTile + kRsTile / 2) * sizeof(rs_c64);     // 96 KiB: the one-pass transform of 4096 points

// e^{sign * i * pi * m^2 / n}, the phase reduced exactly: r = m^2 mod 2n in [-n, n)
__device__ __forceinline__ rs_c64 rs_chirp(long long m, long long n, int sign) {
    const unsigned long long a = (unsigned long long)(m < 0 ? -m : m);
    long long r = (long long)((a * a) % (unsigned long long)(2 * n));
    if (r >= n) r -= 2 * n;
    double s, c;
    sincos(kRsPi * ((double)r / (double)n), &s, &c);
    return rs_c64{c, sign < 0 ? -s : s};
}
// w_len^e = e^{-2 pi i e / len}, len a power of two, 0 <= e < len
__device__ __forceinline__ rs_c64 rs_twiddle(long long e, long long len) {
    if (e >= len / 2) e -= len;
    double s, c;
    sincos(-2.0 * kRsPi * ((double)e / (double)len), &s, &c);
    return rs_c64{c, s};
}
__device__ __forceinline__ int rs_bitrev(int v, int bits) {
    unsigned x = (unsigned)v;
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0f0f0f0fu) | ((x & 0x0f0f0f0fu) << 4);
    x = ((x >> 8) & 0x00ff00ffu) | ((x & 0x00ff00ffu) << 8);
    x = (x >> 16) | (x << 16);
    return bits == 0 ? 0 : (int)(x >> (32 - bits));
}

// ---- the chirp filter: h[i] = e^{sign i pi m^2 / n} at i = m mod M for m in -(lo - 1) .. hi - 1, zero elsewhere (M >= lo + hi - 1) ----
__global__ __launch_bounds__(kRsThreads) void rs_filter_kernel(rs_c64* __restrict__ h, long long M, long long n, long long lo, long long hi, int sign) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    rs_c64 v{0.0, 0.0};
    if (i < hi) v = rs_chirp(i, n, sign);
    else if (M - i < lo) v = rs_chirp(M - i, n, sign);
    h[i] = v;
}

// ---- forward input: buf[c][i] = x[c][i] * e^{-i pi i^2 / Nx} for i < Nx, zero up to M ----
template <class T>
__global__ __launch_bounds__(kRsThreads) void rs_load_kernel(const T* __restrict__ x, long long in_stride, long long Nx, rs_c64* __restrict__ buf,
                                                             long long buf_stride, long long M) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const int c = blockIdx.y;
    rs_c64 v{0.0, 0.0};
    if (i < Nx) {
        const double s = (double)x[(size_t)c * in_stride + i];
        const rs_c64 w = rs_chirp(i, Nx, -1);
        v = rs_c64{s * w.re, s * w.im};
    }
    buf[(size_t)c * buf_stride + i] = v;
}

// ---- bridge: bin k of the forward chirp-z (conv[k] * scale1 * e^{-i pi k^2 / Nx}) -> the inverse chirp-z's input, in place:
// buf[c][k] = Z[k] * e^{+i pi k^2 / num} for k < K, zero up to M2.  Z as in the head comment: nothing above N/2, factor 2 (1 at k = 0,
// where the imaginary part is dropped, as at k = num/2 for even num, which also counts once), the Nyquist factor of an even N. ----
__global__ __launch_bounds__(kRsThreads) void rs_bridge_kernel(rs_c64* __restrict__ buf, long long buf_stride, long long Nx, long long num, double scale1,
                                                               long long M2) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= M2) return;
    rs_c64* p = buf + (size_t)blockIdx.y * buf_stride + k;
    const long long N = num < Nx ? num : Nx;
    rs_c64 v{0.0, 0.0};
    if (k <= N / 2) {                                                    // (N/2 <= num/2: inside the K one-sided bins)
        rs_c64 y = rs_mul(*p, rs_chirp(k, Nx, -1));
        double f = (k == 0 ? 1.0 : 2.0) * scale1;
        if (N % 2 == 0 && k == N / 2) f *= num < Nx ? 2.0 : (Nx < num ? 0.5 : 1.0);
        bool real_only = k == 0;
        if (num % 2 == 0 && k == num / 2) { real_only = true; f *= 0.5; }
        y.re *= f;
        y.im = real_only ? 0.0 : y.im * f;
        v = rs_mul(y, rs_chirp(k, num, +1));
    }
    *p = v;
}

// ---- output: out[c][j] = float(Re(conv[j] * e^{+i pi j^2 / num}) * scale) for j < num ----
__global__ __launch_bounds__(kRsThreads) void rs_store_kernel(const rs_c64* __restrict__ buf, long long buf_stride, long long num, double scale,
                                                              float* __restrict__ out, long long out_stride) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= num) return;
    const int c = blockIdx.y;
    const rs_c64 v = buf[(size_t)c * buf_stride + j], w = rs_chirp(j, num, +1);
    out[(size_t)c * out_stride + j] = (float)((v.re * w.re - v.im * w.im) * scale);
}

// L-point radix-2 stages over the tile t[j * G + g] (G transforms side by side), tw[i] = w_L^i for i < L/2.  Forward: decimation in
// frequency, natural in -> bit-reversed out; inverse: decimation in time with conjugate twiddles, bit-reversed in -> natural out (unscaled).
__device__ __forceinline__ void rs_tile_dif(rs_c64* t, const rs_c64* tw, int lbits, int gbits) {
    const int nbf = 1 << (lbits + gbits - 1), gmask = (1 << gbits) - 1;
    for (int hb = lbits - 1; hb >= 0; --hb) {
        __syncthreads();
        for (int u = threadIdx.x; u < nbf; u += blockDim.x) {
            const int g = u & gmask, bb = u >> gbits, i = bb & ((1 << hb) - 1);
            const int j0 = ((bb >> hb) << (hb + 1)) + i, p0 = (j0 << gbits) + g, p1 = ((j0 + (1 << hb)) << gbits) + g;
            const rs_c64 a = t[p0], b = t[p1];
            t[p0] = rs_c64{a.re + b.re, a.im + b.im};
            t[p1] = rs_mul(rs_c64{a.re - b.re, a.im - b.im}, tw[i << (lbits - 1 - hb)]);
        }
    }
    __syncthreads();
}
__device__ __forceinline__ void rs_tile_dit_inv(rs_c64* t, const rs_c64* tw, int lbits, int gbits) {
    const int nbf = 1 << (lbits + gbits - 1), gmask = (1 << gbits) - 1;
    for (int hb = 0; hb < lbits; ++hb) {
        __syncthreads();
        for (int u = threadIdx.x; u < nbf; u += blockDim.x) {
            const int g = u & gmask, bb = u >> gbits, i = bb & ((1 << hb) - 1);
            const int j0 = ((bb >> hb) << (hb + 1)) + i, p0 = (j0 << gbits) + g, p1 = ((j0 + (1 << hb)) << gbits) + g;
            const rs_c64 a = t[p0], b = rs_mulc(t[p1], tw[i << (lbits - 1 - hb)]);
            t[p0] = rs_c64{a.re + b.re, a.im + b.im};
            t[p1] = rs_c64{a.re - b.re, a.im - b.im};
        }
    }
    __syncthreads();
}

// One pass of the transform of buf[c][0 .. M) (M = 2^lm), in place; grid (M / tile, channels), tile = 2^(lbits + gbits) points.
// lbits: log2 L of the sub-transforms, sbits: log2 S of their stride (sub-blocks of 2^(lbits + sbits) points), gbits: log2 of the
// transforms in a tile.  MODE kRsFwd / kRsInv as in the head comment; kRsBoth (sbits = 0): forward, times filt at the same (permuted)
// place, inverse.  LDS: the tile, then the L/2 twiddles.
template <int MODE>
__global__ __launch_bounds__(kRsThreads) void rs_fft_pass_kernel(rs_c64* __restrict__ buf, long long buf_stride, const rs_c64* __restrict__ filt, int lm,
                                                                 int lbits, int sbits, int gbits) {
    EEG_DYN_SMEM(smf);
    rs_c64* t = reinterpret_cast<rs_c64*>(smf);
    rs_c64* tw = t + ((size_t)1 << (lbits + gbits));
    const int tid = threadIdx.x, nt = blockDim.x, L = 1 << lbits, npts = 1 << (lbits + gbits);
    const long long M = 1ll << lm, tile = blockIdx.x;
    rs_c64* row = buf + (size_t)blockIdx.y * buf_stride;
    for (int i = tid; i < L / 2; i += nt) tw[i] = rs_twiddle(i, L);
    // element (j, g) of the tile in global memory: transform `rest` of sub-block blk, adjacent g = adjacent rest, then adjacent blk
    const int gsb = gbits < sbits ? gbits : sbits;                       // log2 of the adjacent transforms of one sub-block in a tile
    const long long blk0 = (tile >> (sbits - gsb)) << (gbits - gsb), rest0 = (tile & ((1ll << (sbits - gsb)) - 1)) << gsb;
    auto place = [&](int j, int g, long long& rest) {
        rest = rest0 + (g & ((1 << gsb) - 1));
        return ((((blk0 + (g >> gsb)) << (lbits + sbits)) + rest + ((long long)j << sbits)) & (M - 1));
    };
    // the twiddles w_Mp^(rest * j) of this thread's elements: its g (so its rest) is the same for all of them (the block's threads are
    // a multiple of G) and j advances by nt / G, so w advances by one fixed factor: two sincos per thread, then products
    rs_c64 w0{1.0, 0.0}, wstep{1.0, 0.0};
    if (MODE != kRsBoth && sbits > 0) {
        long long rest;
        place(0, tid & ((1 << gbits) - 1), rest);
        const long long Mp = 1ll << (lbits + sbits);
        w0 = rs_twiddle((rest * (tid >> gbits)) & (Mp - 1), Mp);
        wstep = rs_twiddle((rest * (nt >> gbits)) & (Mp - 1), Mp);
    }
    rs_c64 w = w0;
#pragma unroll 4
    for (int e = tid; e < npts; e += nt) {
        const int g = e & ((1 << gbits) - 1), j = e >> gbits;
        long long rest;
        const long long at = place(j, g, rest);
        rs_c64 v = row[at];
        if (MODE == kRsInv) {
            if (sbits > 0) {
                v = rs_mulc(v, w);
                w = rs_mul(w, wstep);
            }
            t[(rs_bitrev(j, lbits) << gbits) + g] = v;
        } else {
            t[e] = v;
        }
    }
    if (MODE != kRsInv) {
        rs_tile_dif(t, tw, lbits, gbits);                                // (its first barrier orders the loads and the table)
        if (MODE == kRsBoth) {
            for (int e = tid; e < npts; e += nt) {
                const int g = e & ((1 << gbits) - 1), p = e >> gbits;
                long long rest;
                const long long at = place(rs_bitrev(p, lbits), g, rest);
                t[e] = rs_mul(t[e], filt[at]);
            }
        }
    }
    if (MODE != kRsFwd) rs_tile_dit_inv(t, tw, lbits, gbits);
    w = w0;
#pragma unroll 4
    for (int e = tid; e < npts; e += nt) {
        const int g = e & ((1 << gbits) - 1), j = e >> gbits;
        long long rest;
        const long long at = place(j, g, rest);
        if (MODE == kRsFwd) {
            rs_c64 v = t[(rs_bitrev(j, lbits) << gbits) + g];
            if (sbits > 0) {
                v = rs_mul(v, w);
                w = rs_mul(w, wstep);
            }
            row[at] = v;
        } else {
            row[at] = t[e];
        }
    }
}

}  // namespace eeg
