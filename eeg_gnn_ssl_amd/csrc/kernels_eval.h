// The evaluation pass of train.py:332-431 on the device: per-clip scores behind the head (eval_scores_kernel, one launch per step
// of the pass) and, behind the last step, the scores of the whole pool (eval_metrics: sort keys, the project's own bitonic sort, one
// scan) as ONE small integer record the host reads.  Plain C++: vector stores, integer arithmetic in int64, the one float64 sum in a
// fixed order -- the record reproduces bit for bit.  No framework sort, no allocation: everything sits on the stream.
#pragma once
#include "common.h"
#include "kernels_tail.h"

namespace eeg {

constexpr long long kEvalMaxClips = 1ll << 20;   // EEG_EVAL_MAX_CLIPS: the pool of one pass (the scan's counters are int32 inside)
constexpr int kEvalRecordHead = 16;              // EEG_EVAL_RECORD_HEAD: int64 words in front of the confusion matrix
constexpr int kEvalSortTile = 2048;              // keys of one LDS tile of the sort
constexpr int kEvalSortThreads = 256;
constexpr int kEvalScanThreads = 1024;
constexpr unsigned kEvalPadKey = 0xFFFFFFFFu;    // above every real key ((0x3F800000 << 1) | 1)

// record words (int64; float64 values travel as their bit patterns)
enum EvalRec {
    kRecN = 0, kRecPos = 1, kRecNeg = 2, kRecAurocNum = 3, kRecThreshBits = 4, kRecTp = 5, kRecFp = 6, kRecFn = 7, kRecTn = 8,
    kRecBadLabels = 9, kRecBadProbs = 10, kRecLossSumBits = 11, kRecSearched = 12, kRecFound = 13, kRecBestTp = 14, kRecBestF1Bits = 15
};

__device__ __forceinline__ unsigned eval_f2u(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
__device__ __forceinline__ float eval_u2f(unsigned u) { float f; memcpy(&f, &u, 4); return f; }
__device__ __forceinline__ long long eval_d2ll(double d) { long long u; memcpy(&u, &d, 8); return u; }

// One launch behind the head of every step of the pass.  Slot b of the batch is pool position pos = cursor - B*world + rank*B + b
// (the gather in front has already advanced the cursor).  A slot writes only if clip_w[b] != 0 AND 0 <= pos < P: whatever the
// cursor holds, nothing is written outside probs (P, C) / losses (P) -- the arithmetic runs unsigned (exact modulo 2^64), so a
// negative or huge cursor gives a pos outside [0, P).  The label is read from the pool at pos (every rank holds the pool).
// C = 1: sigmoid + the BCE-with-logits term of bce_logits_kernel; C > 1: the float32 softmax row + the cross-entropy term of
// ce_logits_kernel (a label outside 0..C-1: NaN, counted by the metrics as a bad label).
__global__ void eval_scores_kernel(const float* __restrict__ logits, const void* __restrict__ label_pool, const float* __restrict__ clip_w,
                                   const long long* __restrict__ cursor, long long step, long long slot0, long long P, int B, int C,
                                   float* __restrict__ probs, float* __restrict__ losses) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B || clip_w[b] == 0.f) return;
    const unsigned long long pos = (unsigned long long)cursor[0] - (unsigned long long)step + (unsigned long long)slot0 + (unsigned long long)b;
    if (pos >= (unsigned long long)P) return;
    if (C == 1) {
        const float v = logits[b], t = static_cast<const float*>(label_pool)[pos];
        probs[pos] = 1.f / (1.f + expf(-v));
        losses[pos] = bce_logits_term(v, t);
        return;
    }
    const float* r = logits + (size_t)b * C;
    float mx = r[0];
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, r[c]);
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += expf(r[c] - mx);
    float* out = probs + (size_t)pos * C;
    for (int c = 0; c < C; ++c) out[c] = expf(r[c] - mx) / se;
    losses[pos] = ce_logits_term(r, C, static_cast<const long long*>(label_pool)[pos], ce_row_lse(r, C));
}

// ---- detection: sort keys -----------------------------------------------------------------------------------------------------------
// key = (bits(prob) << 1) | label for the P clips, the pad key behind them up to npad (a power of two).  For 0 <= prob <= 1 the bit
// pattern of a float is order-preserving and at most 0x3F800000, so the key fits 32 bits; -0 counts as 0.  A probability outside
// [0, 1] (or NaN) and a label outside {0, 1} are COUNTED by the scan (the host raises); here they only have to stay in range.
__global__ void eval_keys_kernel(const float* __restrict__ probs, const float* __restrict__ labels, int P, int npad,
                                 unsigned* __restrict__ keys) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npad) return;
    unsigned k = kEvalPadKey;
    if (i < P) {
        const float p = probs[i];
        unsigned bits = (p > 0.f && p <= 1.f) ? eval_f2u(p) : (p > 1.f ? 0x3F800000u : 0u);
        k = (bits << 1) | (labels[i] == 1.f ? 1u : 0u);
    }
    keys[i] = k;
}

// The bitonic network over npad keys, ascending: stage k = 2, 4, .. npad, step j = k/2 .. 1: element i meets i ^ j, ascending where
// (i & k) == 0.  Steps with j < kEvalSortTile stay inside a tile-aligned tile: eval_sort_tile_kernel runs ALL of them for the stages
// k_first .. k_last in LDS (one tile per block); a step with j >= the tile is one launch of eval_sort_step_kernel over global memory.
__global__ __launch_bounds__(kEvalSortThreads) void eval_sort_tile_kernel(unsigned* __restrict__ keys, int npad, int k_first, int k_last) {
    EEG_DYN_SMEM(smf);
    unsigned* sm = reinterpret_cast<unsigned*>(smf);
    const int n = npad < kEvalSortTile ? npad : kEvalSortTile;          // keys of this tile
    const int base = blockIdx.x * kEvalSortTile;
    for (int t = threadIdx.x; t < n; t += kEvalSortThreads) sm[t] = keys[base + t];
    __syncthreads();
    for (int k = k_first; k <= k_last; k <<= 1) {
        for (int j = (k >> 1) < (n >> 1) ? (k >> 1) : (n >> 1); j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (n >> 1); t += kEvalSortThreads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned a = sm[i], b = sm[l];
                const bool asc = ((base + i) & k) == 0;
                if ((a > b) == asc) { sm[i] = b; sm[l] = a; }
            }
            __syncthreads();
        }
    }
    for (int t = threadIdx.x; t < n; t += kEvalSortThreads) keys[base + t] = sm[t];
}
constexpr int kEvalStepPairs = 4;                // pairs per thread of the global step
__global__ __launch_bounds__(kEvalSortThreads) void eval_sort_step_kernel(unsigned* __restrict__ keys, int npad, int j, int k) {
    const int t0 = (blockIdx.x * kEvalSortThreads + threadIdx.x) * kEvalStepPairs;
    for (int u = 0; u < kEvalStepPairs; ++u) {
        const int t = t0 + u;
        if (t >= (npad >> 1)) return;
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const unsigned a = keys[i], b = keys[l];
        const bool asc = (i & k) == 0;
        if ((a > b) == asc) { keys[i] = b; keys[l] = a; }
    }
}

// F1 of a threshold candidate as utils.thresh_max_f1 computes it from sklearn's precision_recall_curve: p = tp / (tp + fp),
// r = tp / n_pos, f1 = 2 * p * r / (p + r), every operation rounded to float64 on its own (2 * p is exact; no product feeds a sum, so
// nothing here can contract into an fma).  Two candidates whose F1 are EQUAL as rationals can differ in the last bit here, and the
// reference's argmax then prefers the one that rounded up: the value is reproduced, not corrected.
__device__ __forceinline__ double eval_f1_as_reference(long long tp, long long fp, long long n_pos) {
    const double p = (double)tp / (double)(tp + fp), r = (double)tp / (double)n_pos;
    return ((2.0 * p) * r) / (p + r);
}

// first index in [lo, hi) whose key is >= want (hi if none); keys ascending
__device__ __forceinline__ int eval_lower_bound(const unsigned* __restrict__ keys, int lo, int hi, unsigned want) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < want) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// sum of the block's long long values, fixed order (tree over the thread index); s: kEvalScanThreads words of LDS
__device__ __forceinline__ long long eval_block_sum(long long* s, long long v) {
    __syncthreads();
    s[threadIdx.x] = v;
    __syncthreads();
    for (int w = blockDim.x / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    return s[0];
}
// float64 sum of losses[0..P) in a fixed order: thread t takes t, t + threads, .. ; then the tree
__device__ __forceinline__ double eval_loss_sum(double* s, const float* __restrict__ losses, int P) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < P; i += blockDim.x) acc += (double)losses[i];
    __syncthreads();
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int w = blockDim.x / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    return s[0];
}

// ---- detection: the scan -----------------------------------------------------------------------------------------------------------
// ONE block over the sorted keys (P <= 2^20: at most 1024 keys per thread and phase).  With neg_before[i] = negatives among the
// first i sorted clips (written to global memory by this block, read behind a barrier) every distinct value v -- a run of equal
// key >> 1, negatives first -- is handled by the thread that meets its first index g:
//     neg_below = neg_before[g], neg(v) / pos(v) from two binary searches for the ends of the run;
//     AUROC numerator += pos(v) * (2 * neg_below + neg(v));
//     threshold candidate v (utils.thresh_max_f1: the predictions prob >= v): tp = n_pos - pos_below, fp = n_neg - neg_below;
//     candidates with tp > 0 are compared by the float64 value the reference computes from these integers, operation for operation
//     (eval_f1_as_reference: IEEE division, product and sum round the same everywhere), ties to the lowest v (the lowest g).
// Then thread 0: thresh = the searched value (as the float it is) or the given one, the predictions are (double)prob > thresh
// (strict), their split in the sorted order is one more binary search, and the confusion counts follow from neg_before.
// Counters of labels outside {0, 1} and of probabilities outside [0, 1] / NaN come from the unsorted inputs.
__global__ __launch_bounds__(kEvalScanThreads) void eval_scan_kernel(const unsigned* __restrict__ keys, const float* __restrict__ probs,
                                                                     const float* __restrict__ labels, const float* __restrict__ losses,
                                                                     int P, int search, double thresh_in, int* __restrict__ neg_before,
                                                                     long long* __restrict__ rec) {
    EEG_DYN_SMEM(smf);
    long long* s = reinterpret_cast<long long*>(smf);                    // kEvalScanThreads words
    long long* s_tp = s + kEvalScanThreads;                              // the candidates of the threads: tp, F1, first index
    double* s_f1 = reinterpret_cast<double*>(s_tp + kEvalScanThreads);
    long long* s_idx = s_tp + 2 * kEvalScanThreads;
    const int tid = threadIdx.x, nt = blockDim.x;
    long long bad_l = 0, bad_p = 0;
    for (int i = tid; i < P; i += nt) {
        const float p = probs[i], y = labels[i];
        bad_p += !(p >= 0.f && p <= 1.f);
        bad_l += !(y == 0.f || y == 1.f);
    }
    bad_l = eval_block_sum(s, bad_l);
    bad_p = eval_block_sum(s, bad_p);
    const double loss_sum = eval_loss_sum(reinterpret_cast<double*>(s), losses, P);
    // negatives in front of every sorted index: thread t owns the indices [lo, hi)
    const int chunk = (P + nt - 1) / nt;
    const int lo = tid * chunk < P ? tid * chunk : P, hi = lo + chunk < P ? lo + chunk : P;
    long long cnt = 0;
    for (int i = lo; i < hi; ++i) cnt += (keys[i] & 1u) == 0u;
    __syncthreads();
    s[tid] = cnt;
    __syncthreads();
    if (tid == 0) {                                                      // exclusive prefix over the threads, in place
        long long run = 0;
        for (int t = 0; t < nt; ++t) { const long long c = s[t]; s[t] = run; run += c; }
        s_tp[0] = run;
    }
    __syncthreads();
    const long long n_neg = s_tp[0], n_pos = (long long)P - n_neg;
    int run = (int)s[tid];
    for (int i = lo; i < hi; ++i) { neg_before[i] = run; run += (keys[i] & 1u) == 0u; }
    if (tid == 0) neg_before[P] = (int)n_neg;
    __syncthreads();                                                     // (orders the block's global writes before the reads below)
    long long num = 0, best_tp = 0, best_idx = -1;
    double best_f1 = 0.0;
    for (int g = tid; g < P; g += nt) {
        const unsigned v = keys[g] >> 1;
        if (g > 0 && (keys[g - 1] >> 1) == v) continue;                  // not the first of its run
        const int m = eval_lower_bound(keys, g, P, (v << 1) | 1u), e = eval_lower_bound(keys, m, P, (v + 1u) << 1);
        const long long nb = neg_before[g], pb = (long long)g - nb;
        num += (long long)(e - m) * (2 * nb + (long long)(m - g));
        const long long tp = n_pos - pb;
        if (tp > 0) {
            const double f1 = eval_f1_as_reference(tp, n_neg - nb, n_pos);
            if (best_idx < 0 || f1 > best_f1) { best_tp = tp; best_f1 = f1; best_idx = g; }       // (g ascends: the first of equals stays)
        }
    }
    num = eval_block_sum(s, num);
    __syncthreads();
    s_tp[tid] = best_tp; s_f1[tid] = best_f1; s_idx[tid] = best_idx;
    __syncthreads();
    for (int w = nt / 2; w > 0; w >>= 1) {
        if (tid < w) {
            const long long tp = s_tp[tid + w], idx = s_idx[tid + w];
            const double f1 = s_f1[tid + w];
            if (idx >= 0 && (s_idx[tid] < 0 || f1 > s_f1[tid] || (f1 == s_f1[tid] && idx < s_idx[tid]))) {
                s_tp[tid] = tp; s_f1[tid] = f1; s_idx[tid] = idx;
            }
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const bool found = s_idx[0] >= 0;
    double thresh = thresh_in;
    if (search && found) thresh = (double)eval_u2f(keys[s_idx[0]] >> 1);
    int a = 0, b = P;                                                    // first sorted index with (double)prob > thresh
    while (a < b) {
        const int mid = a + ((b - a) >> 1);
        if ((double)eval_u2f(keys[mid] >> 1) > thresh) b = mid; else a = mid + 1;
    }
    const long long neg_le = neg_before[a], pos_le = (long long)a - neg_le;
    rec[kRecN] = P; rec[kRecPos] = n_pos; rec[kRecNeg] = n_neg; rec[kRecAurocNum] = num;
    rec[kRecThreshBits] = eval_d2ll(thresh);
    rec[kRecTp] = n_pos - pos_le; rec[kRecFp] = n_neg - neg_le; rec[kRecFn] = pos_le; rec[kRecTn] = neg_le;
    rec[kRecBadLabels] = bad_l; rec[kRecBadProbs] = bad_p; rec[kRecLossSumBits] = eval_d2ll(loss_sum);
    rec[kRecSearched] = search ? 1 : 0; rec[kRecFound] = found ? 1 : 0;
    rec[kRecBestTp] = found ? s_tp[0] : 0; rec[kRecBestF1Bits] = found ? eval_d2ll(s_f1[0]) : 0;
}

// ---- classification: the confusion matrix ---------------------------------------------------------------------------------------------
// ONE block: the prediction of a clip is the FIRST arg-max of its softmax row; rec[head + label * C + prediction] counts it (integer
// atomics: any order gives the same counts).  A label outside 0..C-1 and a row with a NaN or a value outside [0, 1] are counted as
// bad and left out of the matrix.
__global__ __launch_bounds__(kEvalScanThreads) void eval_confusion_kernel(const float* __restrict__ probs, const long long* __restrict__ labels,
                                                                          const float* __restrict__ losses, int P, int C,
                                                                          long long* __restrict__ rec) {
    EEG_DYN_SMEM(smf);
    long long* s = reinterpret_cast<long long*>(smf);
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int i = tid; i < kEvalRecordHead + C * C; i += nt) rec[i] = 0;
    __syncthreads();
    long long bad_l = 0, bad_p = 0;
    for (int i = tid; i < P; i += nt) {
        const float* r = probs + (size_t)i * C;
        int arg = 0;
        bool ok = true;
        for (int c = 0; c < C; ++c) {
            ok = ok && (r[c] >= 0.f && r[c] <= 1.f);
            if (r[c] > r[arg]) arg = c;
        }
        const long long y = labels[i];
        const bool y_ok = y >= 0 && y < (long long)C;
        bad_p += !ok;
        bad_l += !y_ok;
        if (ok && y_ok) atomic_add_u64(reinterpret_cast<unsigned long long*>(rec) + kEvalRecordHead + (int)y * C + arg, 1ull);
    }
    bad_l = eval_block_sum(s, bad_l);
    bad_p = eval_block_sum(s, bad_p);
    const double loss_sum = eval_loss_sum(reinterpret_cast<double*>(s), losses, P);
    if (tid != 0) return;
    rec[kRecN] = P; rec[kRecBadLabels] = bad_l; rec[kRecBadProbs] = bad_p; rec[kRecLossSumBits] = eval_d2ll(loss_sum);
}

// ---- ssl: per-clip masked MAE ------------------------------------------------------------------------------------------------------
// The SSL evaluation pass of train_ssl.py:232-280 on the device.  ssl_eval_scores_kernel is the twin of eval_scores_kernel behind the
// decoder of every step: ONE workgroup per batch slot, the slot -> pool position arithmetic and its bound as above (unsigned; a slot
// writes only if clip_w[b] != 0 AND 0 <= pos < P).  The clip's per4 16-byte pieces of pred and target are read once: thread t takes
// the pieces t, t + 256, ..; per element the terms of masked_terms (two roundings of the inverse transform, float32 d, mask = ys !=
// mask_val); the thread adds the float32 |d| of its masked-in elements in float64, in piece order, then a fixed LDS tree over the
// thread index.  Nothing in that order depends on B, the slot, the rank or the launch: a clip's sum has the same bits wherever it
// sits.  A masked-in element whose d is not finite is counted in bad and left out of the sum.  scores is (3, P) float64: abs_sum |
// count | bad.  keep (nullable, (P, per4 * 4)): the slot's pred is copied to keep[pos] by the threads that read it.
constexpr int kSslEvalThreads = 256;
constexpr long long kSslEvalMaxClipElems = 1ll << 24;   // EEG_SSL_EVAL_MAX_CLIP_ELEMS: count and bad of a clip stay exact in an int per thread
constexpr int kSslEvalRecordWords = 8;                  // EEG_SSL_EVAL_RECORD_WORDS
enum SslEvalRec { kSslRecN = 0, kSslRecBatches = 1, kSslRecLoss = 2, kSslRecPoolMae = 3, kSslRecAbsSum = 4, kSslRecCount = 5, kSslRecBad = 6,
                  kSslRecEmptyBatches = 7 };

// sum of the block's doubles, fixed order (tree over the thread index); s: blockDim.x words of LDS; every thread gets the sum
__device__ __forceinline__ double ssl_eval_block_sum(double* s, double v) {
    __syncthreads();
    s[threadIdx.x] = v;
    __syncthreads();
    for (int w = blockDim.x / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    return s[0];
}

__global__ __launch_bounds__(kSslEvalThreads) void ssl_eval_scores_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                          const float* __restrict__ clip_w, const long long* __restrict__ cursor,
                                                                          long long step, long long slot0, long long P, int per4, float mean,
                                                                          float std_, int scaled, float mask_val, double* __restrict__ scores,
                                                                          float* __restrict__ keep) {
    EEG_DYN_SMEM(smf);
    double* s = reinterpret_cast<double*>(smf);                          // kSslEvalThreads words
    const int b = blockIdx.x;
    if (clip_w[b] == 0.f) return;                                        // (the whole workgroup leaves: no barrier is left waiting)
    const unsigned long long pos = (unsigned long long)cursor[0] - (unsigned long long)step + (unsigned long long)slot0 + (unsigned long long)b;
    if (pos >= (unsigned long long)P) return;
    const size_t per = (size_t)per4 * 4;
    const float* p = pred + (size_t)b * per;
    const float* y = target + (size_t)b * per;
    float* k = keep != nullptr ? keep + (size_t)pos * per : nullptr;
    double sum = 0.0;
    int cnt = 0, bad = 0;
    auto term = [&](float pv, float yv) {
        float d, mk;
        masked_terms(pv, yv, mean, std_, scaled, mask_val, d, mk);
        if (mk != 0.f) {
            const float a = fabsf(d);
            ++cnt;
            if (a <= 3.402823466e+38f) sum += (double)a; else ++bad;     // (NaN and Inf fail the comparison)
        }
    };
    int i = threadIdx.x;
    for (; i + kSslEvalThreads < per4; i += 2 * kSslEvalThreads) {       // two 16-byte loads per operand in flight
        const f32x4 p0 = ld4(p + 4 * (size_t)i), y0 = ld4(y + 4 * (size_t)i);
        const f32x4 p1 = ld4(p + 4 * (size_t)(i + kSslEvalThreads)), y1 = ld4(y + 4 * (size_t)(i + kSslEvalThreads));
        if (k != nullptr) { st4(k + 4 * (size_t)i, p0); st4(k + 4 * (size_t)(i + kSslEvalThreads), p1); }
#pragma unroll
        for (int r = 0; r < 4; ++r) term(p0[r], y0[r]);
#pragma unroll
        for (int r = 0; r < 4; ++r) term(p1[r], y1[r]);
    }
    if (i < per4) {
        const f32x4 p0 = ld4(p + 4 * (size_t)i), y0 = ld4(y + 4 * (size_t)i);
        if (k != nullptr) st4(k + 4 * (size_t)i, p0);
#pragma unroll
        for (int r = 0; r < 4; ++r) term(p0[r], y0[r]);
    }
    sum = ssl_eval_block_sum(s, sum);
    const double c = ssl_eval_block_sum(s, (double)cnt), bd = ssl_eval_block_sum(s, (double)bad);   // (integers below 2^24: exact)
    if (threadIdx.x != 0) return;
    scores[pos] = sum;
    scores[(size_t)P + pos] = c;
    scores[2 * (size_t)P + pos] = bd;
}

// The pass's record from the (3, P) scores, ONE block, float64, fixed order.  loss is the reference's AverageMeter value over the
// consecutive groups g = [g*G, min((g+1)*G, P)) (the batches of a single process at batch size G): sum_g n_g * L_g / P with
// L_g = S_g / C_g, 0 where C_g == 0 (masked_mae_loss turns that 0/0 into 0 and the meter still counts the batch).  G < blockDim:
// thread t sums the groups t, t + blockDim, .. element by element, then the tree; else the block sums one group after the other
// (strided partial sums + the tree) and thread 0 adds n_g * L_g in group order.  Both orders depend on (P, G) alone.
__global__ __launch_bounds__(kSslEvalThreads) void ssl_eval_metrics_kernel(const double* __restrict__ scores, int P, int G, double* __restrict__ rec) {
    EEG_DYN_SMEM(smf);
    double* s = reinterpret_cast<double*>(smf);                          // kSslEvalThreads words
    const double* abs_sum = scores;
    const double* count = scores + P;
    const double* bad = scores + 2 * (size_t)P;
    const int tid = threadIdx.x, nt = blockDim.x;
    double ta = 0.0, tc = 0.0, tb = 0.0;
    for (int i = tid; i < P; i += nt) { ta += abs_sum[i]; tc += count[i]; tb += bad[i]; }
    ta = ssl_eval_block_sum(s, ta);
    tc = ssl_eval_block_sum(s, tc);
    tb = ssl_eval_block_sum(s, tb);
    const int ngroups = (P + G - 1) / G;                                 // (G <= P: the host clamps it)
    double acc = 0.0, empty = 0.0;
    auto add_group = [&](double sg, double cg, int n) {
        acc += (double)n * (cg > 0.0 ? sg / cg : 0.0);
        empty += cg > 0.0 ? 0.0 : 1.0;
    };
    if (G < nt) {
        for (int g = tid; g < ngroups; g += nt) {
            const int lo = g * G, hi = lo + G < P ? lo + G : P;
            double sg = 0.0, cg = 0.0;
            for (int i = lo; i < hi; ++i) { sg += abs_sum[i]; cg += count[i]; }
            add_group(sg, cg, hi - lo);
        }
        acc = ssl_eval_block_sum(s, acc);
        empty = ssl_eval_block_sum(s, empty);
    } else {
        for (int g = 0; g < ngroups; ++g) {
            const int lo = g * G, hi = lo + G < P ? lo + G : P;
            double sg = 0.0, cg = 0.0;
            for (int i = lo + tid; i < hi; i += nt) { sg += abs_sum[i]; cg += count[i]; }
            sg = ssl_eval_block_sum(s, sg);
            cg = ssl_eval_block_sum(s, cg);
            if (tid == 0) add_group(sg, cg, hi - lo);
        }
    }
    if (tid != 0) return;
    rec[kSslRecN] = (double)P; rec[kSslRecBatches] = (double)ngroups; rec[kSslRecLoss] = acc / (double)P;
    rec[kSslRecPoolMae] = tc > 0.0 ? ta / tc : 0.0;
    rec[kSslRecAbsSum] = ta; rec[kSslRecCount] = tc; rec[kSslRecBad] = tb; rec[kSslRecEmptyBatches] = empty;
}

}  // namespace eeg
