// The fit of the input scaler on the device (the reference's StandardScaler, utils.py:393-428, whose mean and std it unpickles from
// files made offline): the scalar moments of the UN-standardised model inputs over a pool of clips, without writing the inputs.
// feature_moments (one pass step behind the gather): per clip the float64 sum, sum of squares, count and the count of non-finite
// values of
//   kind 0: the float32 log|FFT| features fft_features writes to feat_raw for the clip without augmentation -- the window bodies of
//           kernels_feat.h (fft200_windows for W = 200, dft_window else), so the values are those numbers bit for bit;
//   kind 1: the float32 samples as given: the time-domain windows of computeSliceMatrix(is_fft=False), or ready features read as
//           one row per clip.
// A clip's values are cut into chunks of a fixed size; grid = (chunks, B), one workgroup per (clip, chunk).  A thread adds its values
// in a fixed order ((double)v and (double)v * (double)v: the square of a float32 is exact in float64), the workgroup folds them with
// the fixed LDS tree of ssl_eval_block_sum, the chunk's four words go to a workspace and moments_fold_kernel adds a clip's chunks in
// chunk order into scores (4, P) = sum | sumsq | count | bad.  No floating-point atomics.  Which thread of which chunk takes which
// value depends on (N, T, W, kind) alone -- not on B, the slot, the rank, the cursor or the clip's length (a shorter clip only leaves
// values out) -- so a clip's four words have the same bits wherever it sits.  Slot -> pool position and its bound are those of
// ssl_eval_scores_kernel (unsigned; a slot writes only if clip_w[b] != 0 AND 0 <= pos < P).  With lengths, clip b counts its first
// clip_steps(lengths, b, T) steps only.  moments_record_kernel folds the scores of the pool into one float64 record.
#pragma once
#include "common.h"
#include "kernels_eval.h"
#include "kernels_feat.h"

namespace eeg {

constexpr int kMomThreads = 256;
constexpr int kMomFftItemsPerWave = 12;                         // W = 200: six-window items a wave walks
constexpr int kMomFftChunk = 4 * kMomFftItemsPerWave;           //          items of one workgroup
constexpr int kMomDftPerWave = 16;                              // any other W: windows a wave walks
constexpr int kMomDftChunk = 4 * kMomDftPerWave;                //          windows of one workgroup
constexpr int kMomPiecesPerThread = 16;                         // kind 1: 16-byte pieces of a thread
constexpr int kMomPieceChunk = kMomThreads * kMomPiecesPerThread;
constexpr int kMomPiecesInFlight = 4;
constexpr long long kMomMaxClipElems = 1ll << 31;               // a clip holds fewer elements: counts stay exact in an int per thread
constexpr int kMomMaxBatch = 65535;                             // blockIdx.y
constexpr int kMomRecordWords = 7;                              // EEG_MOMENTS_RECORD_WORDS
enum MomRec { kMomRecClips = 0, kMomRecCount = 1, kMomRecSum = 2, kMomRecSumsq = 3, kMomRecMean = 4, kMomRecStd = 5, kMomRecBad = 6 };

// chunks of a clip: a function of (N, T, W, kind) alone
inline long long moments_chunks(int N, int T, int W, int kind) {
    const long long windows = (long long)N * T;
    if (kind != 0) return (windows * (W / 4) + kMomPieceChunk - 1) / kMomPieceChunk;
    if (W == kFftWin) return ((windows + kFftPerWave - 1) / kFftPerWave + kMomFftChunk - 1) / kMomFftChunk;
    return (windows + kMomDftChunk - 1) / kMomDftChunk;
}

// pool position of batch slot b; false: the slot does not count (its weight is 0, or the position lies outside the pool)
__device__ __forceinline__ bool moments_slot(const float* __restrict__ clip_w, const long long* __restrict__ cursor, long long step, long long slot0,
                                             long long P, int b, unsigned long long& pos) {
    if (clip_w != nullptr && clip_w[b] == 0.f) return false;
    const unsigned long long cur = cursor != nullptr ? (unsigned long long)cursor[0] : (unsigned long long)step;
    pos = cur - (unsigned long long)step + (unsigned long long)slot0 + (unsigned long long)b;
    return pos < (unsigned long long)P;
}

struct MomAcc {
    double sum = 0.0, sumsq = 0.0;
    int cnt = 0, bad = 0;
    __device__ __forceinline__ void add(float v) {
        if (fabsf(v) <= 3.402823466e+38f) {                              // (NaN and Inf fail the comparison)
            const double d = (double)v;
            sum += d;
            sumsq += d * d;
            ++cnt;
        } else {
            ++bad;
        }
    }
};

// the workgroup's four words -> out; s: kMomThreads doubles of LDS (the tree starts behind a barrier: s may alias what the waves used)
__device__ __forceinline__ void moments_finish(double* s, const MomAcc& a, double* __restrict__ out) {
    const double sum = ssl_eval_block_sum(s, a.sum), sq = ssl_eval_block_sum(s, a.sumsq);
    const double c = ssl_eval_block_sum(s, (double)a.cnt), bd = ssl_eval_block_sum(s, (double)a.bad);   // (integers below 2^31: exact)
    if (threadIdx.x != 0) return;
    out[0] = sum; out[1] = sq; out[2] = c; out[3] = bd;
}

// kind 0, W = 200.  The clip's N*T windows are taken in (step, node) order, so the valid windows of a short clip are a prefix; item i
// = the windows 6 i .. 6 i + 5 of the CLIP (items never straddle two clips); wave w of chunk c walks the items c * 48 + 4 k + w.
__global__ __launch_bounds__(kMomThreads, EEG_FFT_MINW) void moments_fft200_kernel(const float* __restrict__ raw, int N, int T,
                                                                                   const long long* __restrict__ lengths,
                                                                                   const float* __restrict__ clip_w,
                                                                                   const long long* __restrict__ cursor, long long step,
                                                                                   long long slot0, long long P, double* __restrict__ ws) {
    EEG_DYN_SMEM(sm);
    const int b = blockIdx.y, chunk = blockIdx.x;
    unsigned long long pos;
    if (!moments_slot(clip_w, cursor, step, slot0, P, b, pos)) return;   // (the whole workgroup leaves: no barrier is left waiting)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    cplx* tile = reinterpret_cast<cplx*>(sm) + (size_t)wave * (kFftWaveDoubles / 2);
    cplx tw1[10], tw2[10];
    fft200_twiddles(lane % 10, tw1, tw2);
    const double log_floor = log(1e-8);                                  // computeFFT: amp == 0 -> 1e-8
    const int w = lane / 10, q = lane - 10 * w;
    const int n_live = (lengths != nullptr ? clip_steps(lengths, b, T) : T) * N;
    MomAcc acc;
    for (int k = 0; k < kMomFftItemsPerWave; ++k) {
        const int j0 = (chunk * kMomFftChunk + 4 * k + wave) * kFftPerWave;
        if (j0 >= n_live) break;                                         // (wave-uniform; the wave's later items lie further back)
        const int j = j0 + w;
        const bool live = w < kFftPerWave && j < n_live;
        auto sig_of = [&]() {
            const int t = j / N, nd = j - t * N;
            return raw + (((size_t)b * N + nd) * T + t) * kFftWin;
        };
        float v[10];
        fft200_windows(sig_of, live, w, q, tile, tw1, tw2, log_floor, v);
        EEG_WAVE_SYNC();                                                 // every partner read is done: the tile is free again
        if (live) {
#pragma unroll
            for (int k2 = 0; k2 < 10; ++k2) acc.add(v[k2]);
        }
    }
    moments_finish(reinterpret_cast<double*>(sm), acc, ws + ((size_t)b * gridDim.x + chunk) * 4);
}

// kind 0, any other W: the direct DFT, one window per wave at a time (fft_features_kernel); windows in (step, node) order, wave w of
// chunk c walks the windows c * 64 + 4 k + w.  LDS: 4 * W doubles, at least kMomThreads.
__global__ __launch_bounds__(kMomThreads) void moments_dft_kernel(const float* __restrict__ raw, int N, int T, int W,
                                                                  const long long* __restrict__ lengths, const float* __restrict__ clip_w,
                                                                  const long long* __restrict__ cursor, long long step, long long slot0,
                                                                  long long P, double* __restrict__ ws) {
    EEG_DYN_SMEM(sm);
    const int b = blockIdx.y, chunk = blockIdx.x;
    unsigned long long pos;
    if (!moments_slot(clip_w, cursor, step, slot0, P, b, pos)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* xs = reinterpret_cast<double*>(sm) + (size_t)wave * W;       // [W], wave-private
    const bool active = lane <= W / 4;
    double c1 = 1.0, s1 = 0.0;
    if (active) sincos(6.283185307179586476925286766559 * (double)lane / (double)W, &s1, &c1);
    const int n_live = (lengths != nullptr ? clip_steps(lengths, b, T) : T) * N;
    MomAcc acc;
    for (int k = 0; k < kMomDftPerWave; ++k) {
        const int j = chunk * kMomDftChunk + 4 * k + wave;
        if (j >= n_live) break;                                          // (wave-uniform)
        const int t = j / N, nd = j - t * N;
        const float* sig = raw + (((size_t)b * N + nd) * T + t) * W;
        EEG_WAVE_SYNC();                                                 // previous window fully consumed
        for (int i = lane; i < W; i += 64) xs[i] = (double)sig[i];
        EEG_WAVE_SYNC();
        if (active) dft_window(xs, W, lane, c1, s1, [&](int, double v) { acc.add((float)v); });
    }
    moments_finish(reinterpret_cast<double*>(sm), acc, ws + ((size_t)b * gridDim.x + chunk) * 4);
}

// kind 1: the clip is `rows` rows of row4 16-byte pieces, of which the first clip_steps * step4 of every row count.  Thread t of chunk
// c takes the pieces c * 4096 + t + 256 u, u = 0 .. 15, in that order (four loads in flight).
__global__ __launch_bounds__(kMomThreads) void moments_values_kernel(const float* __restrict__ raw, unsigned rows, unsigned row4, unsigned step4,
                                                                     int T, const long long* __restrict__ lengths,
                                                                     const float* __restrict__ clip_w, const long long* __restrict__ cursor,
                                                                     long long step, long long slot0, long long P, double* __restrict__ ws) {
    EEG_DYN_SMEM(sm);
    const int b = blockIdx.y, chunk = blockIdx.x;
    unsigned long long pos;
    if (!moments_slot(clip_w, cursor, step, slot0, P, b, pos)) return;
    const unsigned total = rows * row4;                                  // (below 2^29: the host checks)
    const unsigned live4 = (unsigned)(lengths != nullptr ? clip_steps(lengths, b, T) : T) * step4;
    const float* clip = raw + (size_t)b * total * 4;
    MomAcc acc;
    const unsigned e0 = (unsigned)chunk * kMomPieceChunk + threadIdx.x;
    for (int u0 = 0; u0 < kMomPiecesPerThread; u0 += kMomPiecesInFlight) {
        f32x4 x[kMomPiecesInFlight];
        bool on[kMomPiecesInFlight];
#pragma unroll
        for (int u = 0; u < kMomPiecesInFlight; ++u) {
            const unsigned e = e0 + (unsigned)(u0 + u) * kMomThreads;
            on[u] = e < total && e % row4 < live4;
            if (on[u]) x[u] = ld4(clip + 4 * (size_t)e);
        }
#pragma unroll
        for (int u = 0; u < kMomPiecesInFlight; ++u) {
            if (!on[u]) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc.add(x[u][r]);
        }
    }
    moments_finish(reinterpret_cast<double*>(sm), acc, ws + ((size_t)b * gridDim.x + chunk) * 4);
}

// the chunks of every slot that counts, added in chunk order -> scores (4, P) at the slot's pool position; one thread per slot
__global__ void moments_fold_kernel(const double* __restrict__ ws, int chunks, const float* __restrict__ clip_w, const long long* __restrict__ cursor,
                                    long long step, long long slot0, long long P, int B, double* __restrict__ scores) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long pos;
    if (b >= B || !moments_slot(clip_w, cursor, step, slot0, P, b, pos)) return;
    const double* part = ws + (size_t)b * chunks * 4;
    double sum = 0.0, sq = 0.0, c = 0.0, bd = 0.0;
    for (int k = 0; k < chunks; ++k) { sum += part[4 * k]; sq += part[4 * k + 1]; c += part[4 * k + 2]; bd += part[4 * k + 3]; }
    scores[pos] = sum;
    scores[(size_t)P + pos] = sq;
    scores[2 * (size_t)P + pos] = c;
    scores[3 * (size_t)P + pos] = bd;
}

// sumsq / count - mean^2 with every operation rounded on its own (no fused multiply-add: the same bits in every build of this source)
__device__ __forceinline__ double moments_variance(double sumsq, double count, double mean) {
#pragma clang fp contract(off)
    const double m2 = mean * mean;
    const double q = sumsq / count;
    return q - m2;
}

// The record of the pool from its (4, P) scores, ONE block, float64: thread t adds the positions t, t + 256, .. in that order, then
// the tree -- an order that depends on P alone.  std is the population std (np.std) = sqrt(sumsq / count - mean^2).  That difference
// cannot be told from 0 where it lies inside the rounding of the sums: sum and sumsq are each within count * 2^-52 of their exact
// values relative to sum|v| and sumsq (any order of float64 additions), so the variance carries up to 3 * count * 2^-52 *
// sumsq / count, and one more for the record's own operations.  A variance at or below 2^-50 * sumsq -- negative ones among them --
// counts as 0: a pool of equal values (every window silent) reports std = 0 whatever its partial sums rounded to, and the host
// refuses it instead of dividing by noise.  count == 0: mean = std = 0 (the host refuses).
__global__ __launch_bounds__(kMomThreads) void moments_record_kernel(const double* __restrict__ scores, int P, double* __restrict__ rec) {
    EEG_DYN_SMEM(smf);
    double* s = reinterpret_cast<double*>(smf);                          // kMomThreads words
    const double* sum = scores;
    const double* sumsq = scores + P;
    const double* count = scores + 2 * (size_t)P;
    const double* bad = scores + 3 * (size_t)P;
    double ts = 0.0, tq = 0.0, tc = 0.0, tb = 0.0, tn = 0.0;
    for (int i = threadIdx.x; i < P; i += blockDim.x) {
        ts += sum[i]; tq += sumsq[i]; tc += count[i]; tb += bad[i];
        tn += count[i] > 0.0 ? 1.0 : 0.0;
    }
    ts = ssl_eval_block_sum(s, ts);
    tq = ssl_eval_block_sum(s, tq);
    tc = ssl_eval_block_sum(s, tc);
    tb = ssl_eval_block_sum(s, tb);
    tn = ssl_eval_block_sum(s, tn);
    if (threadIdx.x != 0) return;
    const double mean = tc > 0.0 ? ts / tc : 0.0;
    const double var = tc > 0.0 ? moments_variance(tq, tc, mean) : 0.0;
    rec[kMomRecClips] = tn; rec[kMomRecCount] = tc; rec[kMomRecSum] = ts; rec[kMomRecSumsq] = tq;
    rec[kMomRecMean] = mean; rec[kMomRecStd] = var > 0x1p-50 * tq ? sqrt(var) : 0.0; rec[kMomRecBad] = tb;
}

}  // namespace eeg
