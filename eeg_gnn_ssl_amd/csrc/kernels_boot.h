// The clustered bootstrap of the evaluator's scores on the device.  A replicate r is a row of integer counts over G clusters
// (boot_counts_kernel: Philox draws, row 0 all ones); clip i of cluster groups[i] weighs counts[r, groups[i]], and every score of the
// replicate is the weighted form of the score eval_metrics computes.  The pool is sorted ONCE per call -- the bitonic network of
// kernels_eval.h on 64-bit words (key << 32 | clip index) -- and packed into one 32-bit word per sorted clip; then ONE workgroup per
// replicate streams those words, its counts row in LDS where it fits.  Integer arithmetic in int64; the two float64 words (average
// precision, the weighted loss sum) are summed in a fixed order: a record reproduces bit for bit.  Plain C++, vector stores; the
// only atomics are 64-bit integer adds (any order gives the same integers).
#pragma once
#include "common.h"
#include "kernels_eval.h"

namespace eeg {

constexpr int kBootMaxGroups = 1 << 20;          // EEG_BOOT_MAX_GROUPS: a cluster id fits the 20 low bits of a packed word
constexpr int kBootMaxReplicates = 65535;        // EEG_BOOT_MAX_REPLICATES
constexpr int kBootMaxClasses = 32;              // EEG_BOOT_MAX_CLASSES: a confusion cell (< 1024) above the cluster id never makes the skip word
constexpr int kBootMaxRecordWords = 64;          // EEG_BOOT_MAX_RECORD_WORDS: K of boot_records
constexpr unsigned kBootStream = 4u;             // counter word c3 of the draws (kEpochKeyStream is 3; see kernels_data.h)
constexpr int kBootThreads = 1024;               // threads of a replicate's workgroup = columns of the packed stream
constexpr int kBootScratchBytes = 4 * kBootThreads * 8;                                   // four int64 words per thread
constexpr int kBootLdsGroups = (int)((kMaxLdsBytes - kBootScratchBytes) / sizeof(int));   // 32768: the widest counts row kept in LDS
constexpr int kBootCountBins = 32768;            // clusters of one LDS histogram of boot_counts_kernel (two per 64-bit word: 128 KB)
constexpr int kBootCountThreads = 256;
constexpr unsigned long long kBootPadKey = ~0ull;
constexpr unsigned kBootSkipWord = 0xFFFFFFFFu;  // a packed word that names no clip (classification: a row left out of the matrix)

// words of a detection record (EEG_BOOT_DET_WORDS)
enum BootRec { kBootW = 0, kBootPos = 1, kBootNeg = 2, kBootAurocNum = 3, kBootTp = 4, kBootFp = 5, kBootFn = 6, kBootTn = 7, kBootApBits = 8,
               kBootLossBits = 9, kBootDetWords = 10 };

// ---- the draws ------------------------------------------------------------------------------------------------------------------------
// counts (n_boot + 1, G) int32.  Row 0: ones.  Row r >= 1: G draws; draw j is word j % 4 of Philox4x32-10 at the counter
// (lo(j / 4), hi(j / 4), r, kBootStream) under key seed (the layout of epoch_keys_kernel) and names cluster (word * G) >> 32.
// Block (r, part) owns the clusters [part * bins, (part + 1) * bins) of row r: it makes ALL draws of the row, counts those that fall
// into its range in LDS (two 32-bit counts per 64-bit word, a count is at most G <= 2^20: no carry crosses) and stores its range.
__global__ __launch_bounds__(kBootCountThreads) void boot_counts_kernel(unsigned long long seed, int G, int bins, int* __restrict__ counts) {
    EEG_DYN_SMEM(smf);
    unsigned long long* h = reinterpret_cast<unsigned long long*>(smf);
    const int r = blockIdx.x, b0 = (int)blockIdx.y * bins, b1 = b0 + bins < G ? b0 + bins : G;
    const int tid = threadIdx.x, nt = blockDim.x;
    int* row = counts + (size_t)r * G;
    if (r == 0) {
        for (int g = b0 + tid; g < b1; g += nt) row[g] = 1;
        return;
    }
    for (int i = tid; i < (bins + 1) / 2; i += nt) h[i] = 0ull;
    __syncthreads();
    const int quads = (G + 3) / 4;
    for (int q = tid; q < quads; q += nt) {
        unsigned w[4];
        philox4x32_10((unsigned)q, 0u, (unsigned)r, kBootStream, (unsigned)seed, (unsigned)(seed >> 32), w);   // (j / 4 < 2^18: its high word is 0)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (4 * q + u >= G) break;
            const int idx = (int)(((unsigned long long)w[u] * (unsigned long long)G) >> 32);
            if (idx >= b0 && idx < b1) atomic_add_u64(h + ((idx - b0) >> 1), 1ull << (32 * ((idx - b0) & 1)));
        }
    }
    __syncthreads();
    for (int l = tid; l < b1 - b0; l += nt) row[b0 + l] = (int)(unsigned)(h[l >> 1] >> (32 * (l & 1)));
}

// ---- the sort: eval_sort_* on 64-bit words -----------------------------------------------------------------------------------------------
// detection: word = eval_keys_kernel's key << 32 | clip index, the pad word behind the P clips
__global__ void boot_keys_kernel(const float* __restrict__ probs, const float* __restrict__ labels, int P, int npad,
                                 unsigned long long* __restrict__ keys) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npad) return;
    unsigned long long k = kBootPadKey;
    if (i < P) {
        const float p = probs[i];
        const unsigned bits = (p > 0.f && p <= 1.f) ? eval_f2u(p) : (p > 1.f ? 0x3F800000u : 0u);
        k = ((unsigned long long)((bits << 1) | (labels[i] == 1.f ? 1u : 0u)) << 32) | (unsigned)i;
    }
    keys[i] = k;
}
// classification: word = confusion cell (label * C + first arg-max, eval_confusion_kernel's rule) << 32 | clip index; a row with a
// label outside 0..C-1 or a value outside [0, 1] / NaN gets the pad word (left out of the matrix, as there)
__global__ void boot_cell_keys_kernel(const float* __restrict__ probs, const long long* __restrict__ labels, int P, int C, int npad,
                                      unsigned long long* __restrict__ keys) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npad) return;
    unsigned long long k = kBootPadKey;
    if (i < P) {
        const float* r = probs + (size_t)i * C;
        int arg = 0;
        bool ok = true;
        for (int c = 0; c < C; ++c) {
            ok = ok && (r[c] >= 0.f && r[c] <= 1.f);
            if (r[c] > r[arg]) arg = c;
        }
        const long long y = labels[i];
        if (ok && y >= 0 && y < (long long)C) k = ((unsigned long long)((int)y * C + arg) << 32) | (unsigned)i;
    }
    keys[i] = k;
}
__global__ __launch_bounds__(kEvalSortThreads) void boot_sort_tile_kernel(unsigned long long* __restrict__ keys, int npad, int k_first, int k_last) {
    EEG_DYN_SMEM(smf);
    unsigned long long* sm = reinterpret_cast<unsigned long long*>(smf);
    const int n = npad < kEvalSortTile ? npad : kEvalSortTile;
    const int base = blockIdx.x * kEvalSortTile;
    for (int t = threadIdx.x; t < n; t += kEvalSortThreads) sm[t] = keys[base + t];
    __syncthreads();
    for (int k = k_first; k <= k_last; k <<= 1) {
        for (int j = (k >> 1) < (n >> 1) ? (k >> 1) : (n >> 1); j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (n >> 1); t += kEvalSortThreads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned long long a = sm[i], b = sm[l];
                const bool asc = ((base + i) & k) == 0;
                if ((a > b) == asc) { sm[i] = b; sm[l] = a; }
            }
            __syncthreads();
        }
    }
    for (int t = threadIdx.x; t < n; t += kEvalSortThreads) keys[base + t] = sm[t];
}
__global__ __launch_bounds__(kEvalSortThreads) void boot_sort_step_kernel(unsigned long long* __restrict__ keys, int npad, int j, int k) {
    const int t0 = (blockIdx.x * kEvalSortThreads + threadIdx.x) * kEvalStepPairs;
    for (int u = 0; u < kEvalStepPairs; ++u) {
        const int t = t0 + u;
        if (t >= (npad >> 1)) return;
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const unsigned long long a = keys[i], b = keys[l];
        const bool asc = (i & k) == 0;
        if ((a > b) == asc) { keys[i] = b; keys[l] = a; }
    }
}

// ---- the packed stream ----------------------------------------------------------------------------------------------------------------
// Thread t of a replicate's workgroup owns the sorted clips [t * chunk, (t + 1) * chunk); the word of sorted clip s = t * chunk + i
// is stored at i * kBootThreads + t, so the threads of a wave read consecutive words at every i.  A cluster id outside 0..G-1 (the
// host layer refuses it) counts as cluster 0: nothing is ever read outside a counts row.
__device__ __forceinline__ int boot_cluster(const int* __restrict__ groups, unsigned i, int G) {
    const int c = groups != nullptr ? groups[i] : (int)i;
    return (unsigned)c < (unsigned)G ? c : 0;
}
__device__ __forceinline__ size_t boot_slot(int s, int chunk) { return (size_t)(s % chunk) * kBootThreads + (size_t)(s / chunk); }

// detection: cluster | label << 20 | run start << 21 (a run: equal probability, i.e. equal key >> 1); split[0] = the first sorted
// index whose (double)prob > thresh, P if none (the predictions are monotone in the sorted order: exactly one thread writes it)
__global__ void boot_pack_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ groups, int P, int G, int chunk, double thresh,
                                 unsigned* __restrict__ packed, int* __restrict__ split) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= P) return;
    const unsigned long long k = keys[s];
    const unsigned key = (unsigned)(k >> 32), prev = s > 0 ? (unsigned)(keys[s - 1] >> 32) : 0u;
    const bool start = s == 0 || (prev >> 1) != (key >> 1);
    packed[boot_slot(s, chunk)] = (unsigned)boot_cluster(groups, (unsigned)k, G) | ((key & 1u) << 20) | ((start ? 1u : 0u) << 21);
    const bool pred = (double)eval_u2f(key >> 1) > thresh, pred_prev = s > 0 && (double)eval_u2f(prev >> 1) > thresh;
    if (pred && !pred_prev) split[0] = s;
    if (s == P - 1 && !pred) split[0] = P;
}
// classification: cluster | cell << 20, the skip word for a row left out
__global__ void boot_pack_cells_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ groups, int P, int G, int chunk,
                                       unsigned* __restrict__ packed) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= P) return;
    const unsigned long long k = keys[s];
    packed[boot_slot(s, chunk)] = k == kBootPadKey ? kBootSkipWord : ((unsigned)boot_cluster(groups, (unsigned)k, G) | ((unsigned)(k >> 32) << 20));
}

// ---- one workgroup per replicate --------------------------------------------------------------------------------------------------------
// the block's counts row: in LDS (kLds, G <= kBootLdsGroups) behind the scratch words, else read from memory
template <bool kLds>
__device__ __forceinline__ const int* boot_counts_row(const int* __restrict__ row, int* cw, int G) {
    if (!kLds) return row;
    for (int g = threadIdx.x; g < G; g += blockDim.x) cw[g] = row[g];
    return cw;
}

// Detection.  With (pb, nb) the positive / negative weight in front of a run v and W+ / W- the totals:
//     AUROC numerator = sum_v posw(v) * (2 nb(v) + negw(v));   AP = sum_v posw(v) / W+ * tp(v) / (tp(v) + fp(v)),  tp = W+ - pb, fp = W- - nb.
// Inside a run the negatives sort in front of the positives, so a SEGMENT of a run's positives (the part of them in one thread's
// chunk) contributes seg * (nb(v) + neg weight in front of the segment) and seg * tp(v) / (tp(v) + fp(v)): a thread needs the weight
// in front of its chunk and the weight in front of the run that is open where its chunk begins.  Pass 1 sums the chunk (and where its
// last run starts); one scan over the threads gives the prefixes and, as a running maximum of thread indices, the thread that holds
// the start of the open run; pass 2 reads the chunk again and adds the segments.  Runs may span any number of chunks (a pool of one
// value: thread 0 holds the only start).  Totals below 2^31 (the host's limit): seg * (2 nb + negw) < 2^63.
template <bool kLds>
__global__ __launch_bounds__(kBootThreads) void boot_detection_kernel(const unsigned* __restrict__ packed, const int* __restrict__ split_p,
                                                                      const int* __restrict__ counts, const int* __restrict__ groups,
                                                                      const float* __restrict__ losses, int P, int G, int chunk,
                                                                      long long* __restrict__ out) {
    EEG_DYN_SMEM(smf);
    long long* s0 = reinterpret_cast<long long*>(smf);
    long long* s1 = s0 + kBootThreads;
    long long* s2 = s1 + kBootThreads;
    long long* s3 = s2 + kBootThreads;
    const int tid = threadIdx.x, nt = kBootThreads, r = blockIdx.x;
    const int* w_of = boot_counts_row<kLds>(counts + (size_t)r * G, reinterpret_cast<int*>(s3 + kBootThreads), G);
    __syncthreads();
    const int split = split_p[0];
    const long long lo = (long long)tid * chunk;
    const int n = lo >= P ? 0 : (P - lo < chunk ? (int)(P - lo) : chunk);
    // pass 1: the chunk's weights by label, the part of them in front of its last run start, the part behind the split
    long long cp = 0, cn = 0, lp = 0, ln = 0, tp = 0, fp = 0;
    bool has = false;
    for (int i = 0; i < n; ++i) {
        const unsigned u = packed[(size_t)i * nt + tid];
        const long long w = w_of[u & 0xFFFFFu];
        if ((u >> 21) & 1u) { has = true; lp = cp; ln = cn; }
        if ((u >> 20) & 1u) cp += w; else cn += w;
        if (lo + i >= split) { if ((u >> 20) & 1u) tp += w; else fp += w; }
    }
    s0[tid] = cp; s1[tid] = cn; s2[tid] = has ? tid : -1; s3[tid] = (lp << 32) | ln;
    __syncthreads();
    for (int off = 1; off < nt; off <<= 1) {                             // inclusive scans over the threads: two sums, one maximum
        long long a = 0, b = 0, c = -1;
        if (tid >= off) { a = s0[tid - off]; b = s1[tid - off]; c = s2[tid - off]; }
        __syncthreads();
        s0[tid] += a; s1[tid] += b; s2[tid] = c > s2[tid] ? c : s2[tid];
        __syncthreads();
    }
    const long long w_pos = s0[nt - 1], w_neg = s1[nt - 1];
    const long long bp = tid ? s0[tid - 1] : 0, bn = tid ? s1[tid - 1] : 0;
    const int holder = tid ? (int)s2[tid - 1] : -1;                      // the last thread in front of this one whose chunk has a run start
    long long sp = 0, sn = 0;                                            // the weights in front of the run open at the chunk's first clip
    if (holder >= 0) {
        const long long l = s3[holder];
        sp = (holder ? s0[holder - 1] : 0) + (l >> 32);
        sn = (holder ? s1[holder - 1] : 0) + (l & 0xFFFFFFFFll);
    }
    // pass 2: the segments
    long long rn = bn, rp = bp, seg = 0, num = 0;
    double ap = 0.0;
    auto flush = [&]() {
        if (seg > 0) {
            num += seg * (rn + sn);
            const long long tpv = w_pos - sp, fpv = w_neg - sn;
            ap += (double)seg * ((double)tpv / (double)(tpv + fpv));
            seg = 0;
        }
    };
    for (int i = 0; i < n; ++i) {
        const unsigned u = packed[(size_t)i * nt + tid];
        const long long w = w_of[u & 0xFFFFFu];
        if ((u >> 21) & 1u) { flush(); sp = rp; sn = rn; }
        if ((u >> 20) & 1u) { rp += w; seg += w; } else rn += w;
    }
    flush();
    // the weighted loss sum over the clips in pool order: thread t takes t, t + threads, ..; then the tree
    double ls = 0.0;
    if (losses != nullptr)
        for (int i = tid; i < P; i += nt) ls += (double)w_of[boot_cluster(groups, (unsigned)i, G)] * (double)losses[i];
    __syncthreads();
    double* d2 = reinterpret_cast<double*>(s2);
    double* d3 = reinterpret_cast<double*>(s3);
    s0[tid] = num; s1[tid] = (tp << 32) | fp; d2[tid] = ap; d3[tid] = ls;       // (tp, fp below 2^31 each: the halves never carry)
    __syncthreads();
    for (int w = nt / 2; w > 0; w >>= 1) {
        if (tid < w) { s0[tid] += s0[tid + w]; s1[tid] += s1[tid + w]; d2[tid] += d2[tid + w]; d3[tid] += d3[tid + w]; }
        __syncthreads();
    }
    if (tid != 0) return;
    long long* rec = out + (size_t)r * kBootDetWords;
    const long long tpw = s1[0] >> 32, fpw = s1[0] & 0xFFFFFFFFll;
    rec[kBootW] = w_pos + w_neg; rec[kBootPos] = w_pos; rec[kBootNeg] = w_neg; rec[kBootAurocNum] = s0[0];
    rec[kBootTp] = tpw; rec[kBootFp] = fpw; rec[kBootFn] = w_pos - tpw; rec[kBootTn] = w_neg - fpw;
    rec[kBootApBits] = eval_d2ll(w_pos > 0 ? d2[0] / (double)w_pos : __builtin_nan(""));
    rec[kBootLossBits] = losses != nullptr ? eval_d2ll(d3[0]) : 0;
}

// Classification: the clips sorted by confusion cell; a thread adds the weights of its chunk cell by cell and hands each sum to the
// workgroup's matrix in LDS when the cell changes (integer atomics: any order gives the same matrix).  cells = C * C.
template <bool kLds>
__global__ __launch_bounds__(kBootThreads) void boot_cells_kernel(const unsigned* __restrict__ packed, const int* __restrict__ counts, int P, int G,
                                                                  int cells, int chunk, long long* __restrict__ out) {
    EEG_DYN_SMEM(smf);
    unsigned long long* m = reinterpret_cast<unsigned long long*>(smf);   // kBootMaxClasses^2 words
    const int tid = threadIdx.x, nt = kBootThreads, r = blockIdx.x;
    for (int c = tid; c < cells; c += nt) m[c] = 0ull;
    const int* w_of = boot_counts_row<kLds>(counts + (size_t)r * G, reinterpret_cast<int*>(m + kBootMaxClasses * kBootMaxClasses), G);
    __syncthreads();
    const long long lo = (long long)tid * chunk;
    const int n = lo >= P ? 0 : (P - lo < chunk ? (int)(P - lo) : chunk);
    unsigned cur = 0;
    unsigned long long acc = 0;
    for (int i = 0; i < n; ++i) {
        const unsigned u = packed[(size_t)i * nt + tid];
        if (u == kBootSkipWord) continue;
        const unsigned cell = u >> 20;
        if (cell != cur) {
            if (acc != 0) atomic_add_u64(m + cur, acc);
            cur = cell;
            acc = 0;
        }
        acc += (unsigned long long)w_of[u & 0xFFFFFu];
    }
    if (acc != 0) atomic_add_u64(m + cur, acc);
    __syncthreads();
    for (int c = tid; c < cells; c += nt) out[(size_t)r * cells + c] = (long long)m[c];
}

// Records: out[r, k] = sum_g counts[r, g] * recs[g, k] in int64 (modulo 2^64).  Thread t of the first (threads / K) * K takes word
// k = t % K of the clusters t / K, t / K + threads / K, ..: consecutive threads read consecutive words; then K threads add the columns.
constexpr int kBootRecordThreads = 256;
__global__ __launch_bounds__(kBootRecordThreads) void boot_records_kernel(const long long* __restrict__ recs, const int* __restrict__ counts, int G, int K,
                                                                          long long* __restrict__ out) {
    EEG_DYN_SMEM(smf);
    unsigned long long* s = reinterpret_cast<unsigned long long*>(smf);   // kBootRecordThreads words
    const int tid = threadIdx.x, per = kBootRecordThreads / K, r = blockIdx.x;
    const int* row = counts + (size_t)r * G;
    unsigned long long acc = 0;
    if (tid < per * K) {
        const int k = tid % K;
        for (int g = tid / K; g < G; g += per) acc += (unsigned long long)(long long)row[g] * (unsigned long long)recs[(size_t)g * K + k];
    }
    s[tid] = acc;
    __syncthreads();
    if (tid >= K) return;
    unsigned long long sum = 0;
    for (int m = 0; m < per; ++m) sum += s[m * K + tid];
    out[(size_t)r * K + tid] = (long long)sum;
}

}  // namespace eeg
