// Whole recordings behind the detection head: the per-second probability timeline of every recording from the probabilities of its
// overlapping clips (scan_timeline_kernel), seizure events from the timeline (scan_events_kernel: smoothing, hysteresis, gap merge,
// minimum length) and event- and bin-level scores against annotated intervals (event_scores_kernel + event_scores_total_kernel: one
// small int64 record the host reads).  Plain C++ like kernels_eval.h: vector stores, integer records, every float sum in ascending
// index order, no atomics.  EVERY output element is written by EVERY launch (a poisoned buffer comes back fully defined), and every
// index derived from a table is clamped: whatever the tables hold, nothing is read or written outside the buffers the host sized.
//
// Units: a BIN is one step of `window` samples.  Recording r owns the bins bin_off[r] .. bin_off[r + 1] of the flat per-bin buffers
// (bin_off: int64 (R + 1), prefix sums of the recordings' whole steps) and the rows clip_off[r] .. clip_off[r + 1] of the clip table.
#pragma once
#include "common.h"
#include "kernels_eval.h"     // eval_block_sum: the block's fixed-order int64 sum

namespace eeg {

constexpr int kScanChunkBins = 2048;                              // EEG_SCAN_CHUNK_BINS: bins of a recording in LDS at a time
constexpr int kScanThreads = 256;
constexpr int kScanSeg = kScanChunkBins / kScanThreads;           // consecutive bins a thread owns within a chunk
constexpr int kScanMaxHalo = 64;                                  // bins staged on either side of a chunk for the smoothing window
constexpr int kScanMaxSmoothBins = 2 * kScanMaxHalo + 1;          // EEG_SCAN_MAX_SMOOTH_BINS
constexpr int kScanTile = kScanChunkBins + 2 * kScanMaxHalo;
constexpr int kScanRecordWords = 10;                              // EEG_SCAN_RECORD_WORDS
constexpr size_t kScanEventsLds = (size_t)kScanTile * (sizeof(float) + sizeof(int)) + kScanThreads * sizeof(int);
enum ScanRec { kScanNRef = 0, kScanNHyp = 1, kScanRefHit = 2, kScanHypHit = 3, kScanCovered = 4, kScanTp = 5, kScanFp = 6, kScanFn = 7,
               kScanTn = 8, kScanOverflowed = 9 };
static_assert(kScanSeg * kScanThreads == kScanChunkBins && kScanSeg <= 32, "a thread's bins of a chunk fit one bit mask");

__device__ __forceinline__ long long scan_clamp(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the bins [b0, b1) of recording r inside the flat buffers of `total` bins (bin_off clamped: b0 <= b1 <= total)
__device__ __forceinline__ void scan_bins_of(const long long* __restrict__ bin_off, int r, long long total, long long& b0, long long& b1) {
    b0 = scan_clamp(bin_off[r], 0, total);
    b1 = scan_clamp(bin_off[r + 1], b0, total);
}

// ---- the timeline -------------------------------------------------------------------------------------------------------------------
// One thread per bin g of the flat buffers: the recording is the last r with bin_off[r] <= g (binary search), the bin j = g - b0.  The
// rows of r start at ascending steps (the host refuses any other table), so the rows with start_step <= j < start_step + T are
// consecutive: two binary searches over the START STEPS READ FROM THE TABLE bound them, and each row between them is tested again
// before it counts (a table the host would have refused costs coverage, never an access).  mean: the float32 sum of the covering
// probabilities in ascending row order over float(cover); max: their maximum; an uncovered bin: value 0, cover 0.
__global__ void scan_timeline_kernel(const float* __restrict__ probs, long long P, const long long* __restrict__ table,
                                     const long long* __restrict__ clip_off, const long long* __restrict__ bin_off, int R, long long total,
                                     int T, int window, int agg, float* __restrict__ timeline, int* __restrict__ cover) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    int r = 0, hi_r = R;                                                 // last r in [0, R) with bin_off[r] <= g
    while (hi_r - r > 1) {
        const int mid = r + ((hi_r - r) >> 1);
        if (bin_off[mid] <= g) r = mid; else hi_r = mid;
    }
    long long b0, b1;
    scan_bins_of(bin_off, r, total, b0, b1);
    float sum = 0.f, mx = 0.f;
    int cnt = 0;
    if (g >= b0 && g < b1) {
        const long long j = g - b0;
        const long long c0 = scan_clamp(clip_off[r], 0, P), c1 = scan_clamp(clip_off[r + 1], c0, P);
        auto start_of = [&](long long row) { return table[4 * row + 1] / (long long)window; };
        auto first_above = [&](long long want) {                         // first row in [c0, c1) whose start step is > want
            long long lo = c0, hi = c1;
            while (lo < hi) {
                const long long mid = lo + ((hi - lo) >> 1);
                if (start_of(mid) > want) hi = mid; else lo = mid + 1;
            }
            return lo;
        };
        const long long lo = first_above(j - T), hi = first_above(j);
        for (long long row = lo; row < hi; ++row) {
            const long long s = start_of(row);
            if (s > j || j - s >= T) continue;
            const float p = probs[row];
            sum += p;
            mx = cnt == 0 ? p : fmaxf(mx, p);
            ++cnt;
        }
    }
    timeline[g] = cnt == 0 ? 0.f : (agg == 0 ? sum / (float)cnt : mx);
    cover[g] = cnt;
}

// ---- events -------------------------------------------------------------------------------------------------------------------------
// inclusive scan of one int per thread in thread order by an associative op(earlier, later), through s (blockDim.x ints of LDS).
// Returns the thread's inclusive value; until the next barrier s[t] holds thread t's (s[tid - 1]: the exclusive value, s[blockDim.x
// - 1]: the block's).  Every thread of the block calls it.
template <class Op>
__device__ __forceinline__ int scan_block_incl(int* s, int v, Op op) {
    const int tid = threadIdx.x, nt = blockDim.x;
    __syncthreads();
    s[tid] = v;
    __syncthreads();
    for (int d = 1; d < nt; d <<= 1) {
        const int a = tid >= d ? s[tid - d] : 0, b = s[tid];
        __syncthreads();
        if (tid >= d) s[tid] = op(a, b);
        __syncthreads();
    }
    return s[tid];
}

constexpr int kScanKeep = 0, kScanOff = 1, kScanOn = 2;                  // what a bin does to the state: keep it, or set it

// ONE workgroup per recording; its bins stream through LDS in chunks of kScanChunkBins (+ the smoothing halo), thread t owning the
// kScanSeg consecutive bins t * kScanSeg .. of a chunk.  Per bin j of recording r (S bins):
//   q_j     = the float32 sum, ascending, of timeline_i over the covered i in [j - h, j + h] and [0, S), over their number; an
//             uncovered j: 0 -> smoothed
//   map_j   = set-on if q_j >= th_on, set-off if q_j < th_off or j is uncovered, else keep;  state_j = map_j(state_{j-1}), state_{-1} off
// Composition of these maps is associative: a thread folds its bins, the block scans the folds (scan_block_incl), the chunk's fold is
// carried to the next chunk.  Runs of "on" merge into the event before them when at most merge_gap off bins lie between (a chain
// merges as a whole, because the gap is measured to the END of the event so far = the last on bin); so bin j STARTS an event iff it is
// on, j - 1 is off and the last on bin before it is more than merge_gap bins back (or there is none), and the event that ended before
// j is [previous start, last on bin + 1).  Both "last on bin before j" and "last start before j" are max-scans with a carry; an event
// is emitted where the next one starts (and, for the last, behind the recording's last bin), kept if it is at least min_bins long,
// at the index a sum-scan of the kept events gives.  events (R, E_max, 2) int32 (onset, offset exclusive) in order, zero rows behind
// them; event_count[r] the TRUE number of kept events: rows at or behind E_max are counted, never written.
__global__ __launch_bounds__(kScanThreads) void scan_events_kernel(const float* __restrict__ timeline, const int* __restrict__ cover,
                                                                   const long long* __restrict__ bin_off, long long total, int h, float th_on,
                                                                   float th_off, int merge_gap, int min_bins, int E_max,
                                                                   float* __restrict__ smoothed, int* __restrict__ events,
                                                                   int* __restrict__ event_count) {
    EEG_DYN_SMEM(smf);
    float* tl = smf;                                                     // [kScanTile] timeline of the chunk and its halo (0 where uncovered)
    int* cv = reinterpret_cast<int*>(tl + kScanTile);                    // [kScanTile] 1: covered and inside the recording
    int* s = cv + kScanTile;                                             // [kScanThreads] the scans
    const int r = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    long long b0, b1;
    scan_bins_of(bin_off, r, total, b0, b1);
    const int S = (int)(b1 - b0);                                        // (total < 2^31: the host checks)
    int* ev = events + (size_t)r * E_max * 2;
    int c_on = 0, c_last_on = -1, c_start = -1, c_kept = 0;              // carried from chunk to chunk; the same in every thread
    auto emit = [&](int idx, int a, int b) {
        if (idx < E_max) { ev[2 * idx] = a; ev[2 * idx + 1] = b; }
    };
    for (int base = 0; base < S; base += kScanChunkBins) {
        __syncthreads();                                                 // the previous chunk's tile has been read
        for (int i = tid; i < kScanTile; i += nt) {
            const int j = base - kScanMaxHalo + i;
            const bool in = j >= 0 && j < S && cover[b0 + j] > 0;
            cv[i] = in ? 1 : 0;
            tl[i] = in ? timeline[b0 + j] : 0.f;
        }
        __syncthreads();
        const int j0 = base + tid * kScanSeg, i0 = kScanMaxHalo + tid * kScanSeg;
        int maps[kScanSeg], fold = kScanKeep;
#pragma unroll
        for (int k = 0; k < kScanSeg; ++k) {
            maps[k] = kScanKeep;
            if (j0 + k >= S) continue;
            float q = 0.f;
            int m = kScanOff;
            if (cv[i0 + k]) {
                float sum = 0.f;
                int n = 0;
                for (int d = -h; d <= h; ++d) {
                    if (cv[i0 + k + d]) { sum += tl[i0 + k + d]; ++n; }
                }
                q = sum / (float)n;
                m = q >= th_on ? kScanOn : (q < th_off ? kScanOff : kScanKeep);
            }
            smoothed[b0 + j0 + k] = q;
            maps[k] = m;
            if (m != kScanKeep) fold = m;
        }
        // the state in front of the thread's bins, then of each of them
        scan_block_incl(s, fold, [](int a, int b) { return b != kScanKeep ? b : a; });
        const int before = tid > 0 ? s[tid - 1] : kScanKeep, whole = s[nt - 1];
        const int on_in = before != kScanKeep ? (before == kScanOn ? 1 : 0) : c_on;
        unsigned on = 0;
        int last_on = -1;
        {
            int st = on_in;
#pragma unroll
            for (int k = 0; k < kScanSeg; ++k) {
                if (maps[k] != kScanKeep) st = maps[k] == kScanOn ? 1 : 0;
                if (j0 + k < S && st) { on |= 1u << k; last_on = j0 + k; }
            }
        }
        c_on = whole != kScanKeep ? (whole == kScanOn ? 1 : 0) : c_on;
        auto imax = [](int a, int b) { return a > b ? a : b; };
        // the last on bin in front of the thread's bins
        scan_block_incl(s, last_on, imax);
        const int last_on_in = imax(tid > 0 ? s[tid - 1] : -1, c_last_on);
        c_last_on = imax(c_last_on, s[nt - 1]);
        // walk(f): f(j, prev_on) for every bin j of the thread that starts an event, prev_on the last on bin before it (-1: none)
        auto walk = [&](auto&& f) {
            int prev = last_on_in, was_on = on_in;
#pragma unroll
            for (int k = 0; k < kScanSeg; ++k) {
                const int is_on = (int)((on >> k) & 1u), j = j0 + k;
                if (is_on && !was_on && (prev < 0 || j - prev - 1 > merge_gap)) f(j, prev);
                if (is_on) prev = j;
                was_on = is_on;
            }
        };
        int last_start = -1;
        walk([&](int j, int) { last_start = j; });
        scan_block_incl(s, last_start, imax);
        const int start_in = imax(tid > 0 ? s[tid - 1] : -1, c_start);
        c_start = imax(c_start, s[nt - 1]);
        // the events that end in front of the thread's starts: count the kept ones, then write them at their index
        int kept = 0;
        {
            int ps = start_in;
            walk([&](int j, int prev) {
                if (ps >= 0 && prev + 1 - ps >= min_bins) ++kept;
                ps = j;
            });
        }
        scan_block_incl(s, kept, [](int a, int b) { return a + b; });
        {
            int ps = start_in, idx = c_kept + (tid > 0 ? s[tid - 1] : 0);
            walk([&](int j, int prev) {
                if (ps >= 0 && prev + 1 - ps >= min_bins) emit(idx++, ps, prev + 1);
                ps = j;
            });
        }
        c_kept += s[nt - 1];
    }
    if (c_start >= 0 && c_last_on + 1 - c_start >= min_bins) {           // the event still open behind the last bin
        if (tid == 0) emit(c_kept, c_start, c_last_on + 1);
        ++c_kept;
    }
    for (int i = (c_kept < E_max ? c_kept : E_max) * 2 + tid; i < E_max * 2; i += nt) ev[i] = 0;
    if (tid == 0) event_count[r] = c_kept;
}

// ---- scores -------------------------------------------------------------------------------------------------------------------------
// ONE workgroup per recording -> its kScanRecordWords int64 words in rec_records (R, words).  Detected events: the first
// min(event_count, E_max) rows of events[r] (n_hyp counts these; overflowed = 1 if event_count > E_max); reference events: the first
// ref_count[r] (clamped to A_max) rows of ref[r]; every interval is clamped into [0, S].  Two intervals overlap if they share a bin.
// A covered bin is positive inside a reference interval and predicted inside a detected event; uncovered bins count nowhere.
__global__ __launch_bounds__(kScanThreads) void event_scores_kernel(const int* __restrict__ events, const int* __restrict__ event_count, int E_max,
                                                                    const int* __restrict__ ref, const int* __restrict__ ref_count, int A_max,
                                                                    const int* __restrict__ cover, const long long* __restrict__ bin_off,
                                                                    long long total, long long* __restrict__ rec_records) {
    EEG_DYN_SMEM(smf);
    long long* s = reinterpret_cast<long long*>(smf);                    // kScanThreads words
    const int r = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    long long b0, b1;
    scan_bins_of(bin_off, r, total, b0, b1);
    const int S = (int)(b1 - b0);
    const int cnt = event_count[r];
    const int nh = cnt < 0 ? 0 : (cnt > E_max ? E_max : cnt);
    const int na = ref_count[r] < 0 ? 0 : (ref_count[r] > A_max ? A_max : ref_count[r]);
    const int* ev = events + (size_t)r * E_max * 2;
    const int* rf = ref + (size_t)r * A_max * 2;
    auto interval = [&](const int* p, int k, int& a, int& b) {
        a = (int)scan_clamp(p[2 * k], 0, S);
        b = (int)scan_clamp(p[2 * k + 1], a, S);
    };
    auto overlaps_any = [&](int a, int b, const int* other, int n) {
        for (int k = 0; k < n; ++k) {
            int c, d;
            interval(other, k, c, d);
            if ((a > c ? a : c) < (b < d ? b : d)) return true;
        }
        return false;
    };
    long long ref_hit = 0, hyp_hit = 0, covered = 0, tp = 0, fp = 0, fn = 0, tn = 0;
    for (int i = tid; i < na; i += nt) {
        int a, b;
        interval(rf, i, a, b);
        ref_hit += overlaps_any(a, b, ev, nh) ? 1 : 0;
    }
    for (int i = tid; i < nh; i += nt) {
        int a, b;
        interval(ev, i, a, b);
        hyp_hit += overlaps_any(a, b, rf, na) ? 1 : 0;
    }
    for (int j = tid; j < S; j += nt) {
        if (cover[b0 + j] <= 0) continue;
        const bool pos = overlaps_any(j, j + 1, rf, na), pred = overlaps_any(j, j + 1, ev, nh);
        ++covered;
        tp += pos && pred; fp += !pos && pred; fn += pos && !pred; tn += !pos && !pred;
    }
    ref_hit = eval_block_sum(s, ref_hit);
    hyp_hit = eval_block_sum(s, hyp_hit);
    covered = eval_block_sum(s, covered);
    tp = eval_block_sum(s, tp);
    fp = eval_block_sum(s, fp);
    fn = eval_block_sum(s, fn);
    tn = eval_block_sum(s, tn);
    if (tid != 0) return;
    long long* rec = rec_records + (size_t)r * kScanRecordWords;
    rec[kScanNRef] = na; rec[kScanNHyp] = nh; rec[kScanRefHit] = ref_hit; rec[kScanHypHit] = hyp_hit; rec[kScanCovered] = covered;
    rec[kScanTp] = tp; rec[kScanFp] = fp; rec[kScanFn] = fn; rec[kScanTn] = tn; rec[kScanOverflowed] = cnt > E_max ? 1 : 0;
}

// the record of the whole set: word by word the sum of the recordings' words, ONE block (thread t adds the recordings t, t + 256, ..)
__global__ __launch_bounds__(kScanThreads) void event_scores_total_kernel(const long long* __restrict__ rec_records, int R,
                                                                          long long* __restrict__ record) {
    EEG_DYN_SMEM(smf);
    long long* s = reinterpret_cast<long long*>(smf);
    for (int w = 0; w < kScanRecordWords; ++w) {
        long long v = 0;
        for (int r = threadIdx.x; r < R; r += blockDim.x) v += rec_records[(size_t)r * kScanRecordWords + w];
        v = eval_block_sum(s, v);
        if (threadIdx.x == 0) record[w] = v;
    }
}

}  // namespace eeg
