// Clips cut out of whole recordings that stay in HBM: the index arithmetic of the reference's three loaders at __getitem__ time, on
// the device.  Reference (host, per sample): `signal_array[:, start:end]` of computeSliceMatrix (data/dataloader_detection.py and
// dataloader_ssl.py:52-58: start = clip_idx * clip_len * 200; the SSL target is the head of another clip of the same recording,
// dataloader_ssl.py:303-310, 341) and the seizure window of dataloader_classification.py:44-85 (an arbitrary sample offset; whole
// 1-s steps are kept by the `while` loop and the clip is zero-padded to T steps afterwards).  Here the recordings lie channel-major
// in one signal buffer, a clip is a row (rec, x_start, x_samples, y_start) of an int64 table, and gather_records_kernel is the
// sibling of gather_clips_kernel (kernels_data.h): the same slot arithmetic over the sampler's perm and cursor, the same batch
// tensors behind it -- (B, N, Tx*W) raw signals, the (B, N, Ty*W) target, labels, lengths -- and the same cursor_advance_kernel
// behind it on the stream.
#pragma once
#include "common.h"
#include "kernels_data.h"

namespace eeg {

// signals: float32[signal_floats] (16-byte aligned, a whole number of 16-byte pieces); sample s of channel n of recording r lies at
// rec_table[r] = (offset, stride, samples): offset + n * stride + s.  clip_table[p] = (rec, x_start, x_samples, y_start).  The batch
// rows hold x_len = Tx * window and y_len = Ty * window floats (y_len = 0: no target); cx / cy = blocks per channel row.
struct RecordGather {
    const float* signals;
    long long signal_floats;
    const long long* rec_table;
    long long R;
    const long long* clip_table;
    float* x_out;
    float* y_out;
    unsigned N, window, x_len, y_len, cx, cy;
};

// hostile table entries are clamped to +-2^61 before any sum or difference of two of them is formed: none overflows
constexpr long long kRecordBig = 1LL << 61;
__device__ __forceinline__ long long record_clamp(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One launch per step.  blockIdx.x = batch slot b; blockIdx.y enumerates (channel n, stretch of kAugPerBlock 16-byte pieces of that
// channel's row) over the N x rows and then over the N y rows: a block lies in ONE channel row of ONE recording, so everything
// that decides addresses and paths is block-uniform.  Per block:
//   src  = gather_source(...) (the slot arithmetic of gather_clips), r = clamp(rec, 0, R-1)
//   keep = (clamp(x_samples, 0, x_len) / window) * window: whole steps only; the y row counts over all of y_len
//   out[b, n, i] = signals[offset + n*stride + start + i]  if i < keep (y: y_len) and 0 <= start + i < samples, else exactly 0.0f
// BOUNDS.  The samples of the row that may be read are those inside the recording row AND inside the signal buffer:
// [s_lo, s_hi); they map to the elements [i_lo, i_hi) of the output row.  Every load goes through a buffer descriptor over that
// stretch alone and its index is clamped into the stretch, whatever the tables hold; an empty stretch loads nothing.  The stores go
// through a descriptor over the one output row (a ragged last stretch is dropped by it).  Every element of the row is written.
// TWO SOURCE PATHS, block-uniform:
//   aligned   (offset + n*stride + start) % 4 == 0: the 16-byte pieces of the output row are 16-byte pieces of the signal buffer;
//             the stretch is widened to whole pieces -- still inside the buffer, which is a whole number of aligned pieces -- and a
//             piece that straddles i_lo or i_hi selects per element.  The launch shape of gather_clip_rows: kAugUnroll 16-byte loads
//             in flight per thread, no per-lane branch.
//   unaligned any other start (the classification recipe): nothing but 4-byte alignment is assumed.  The block reads its stretch as
//             dwords, consecutive lanes consecutive dwords (whole lines per wave instruction, 4 * kAugUnroll in flight per thread),
//             through LDS (`stage`, 16 bytes per piece of the stretch), and writes the same 16-byte pieces.
__device__ __forceinline__ void gather_record_rows(const RecordGather& g, const void* __restrict__ label_pool, void* __restrict__ label_out,
                                                   int label_bytes, long long* __restrict__ len_out, const long long* __restrict__ perm,
                                                   long long n_perm, long long P, const long long* __restrict__ cursor, long long slot0,
                                                   float* __restrict__ stage) {
    const unsigned b = blockIdx.x;
    const long long src = gather_source(perm, n_perm, P, cursor, slot0 + (long long)b);
    const long long* clip = g.clip_table + 4 * src;
    const long long r = record_clamp(clip[0], 0, g.R - 1);
    const long long keep = record_clamp(clip[2], 0, (long long)g.x_len) / g.window * g.window;
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        gather_label(label_pool, label_out, label_bytes, src, b);
        if (len_out != nullptr) len_out[b] = keep / g.window;
    }
    const unsigned nx = g.N * g.cx;
    const bool second = blockIdx.y >= nx;                               // block-uniform, like all that follows
    const unsigned idx = second ? blockIdx.y - nx : blockIdx.y, per = second ? g.cy : g.cx;
    const unsigned n = idx / per, chunk = idx % per;
    const unsigned row_len = second ? g.y_len : g.x_len;
    const long long limit = second ? (long long)g.y_len : keep;
    const long long start = record_clamp(clip[second ? 3 : 1], -kRecordBig, kRecordBig);
    const long long* rec = g.rec_table + 3 * r;
    const long long row_lo = (long long)((unsigned long long)rec[0] + (unsigned long long)n * (unsigned long long)rec[1]);
    const long long samples = record_clamp(rec[2], 0, kRecordBig);
    long long s_lo = 0, s_hi = 0;
    if (row_lo > -kRecordBig && row_lo < g.signal_floats) {
        s_lo = row_lo < 0 ? -row_lo : 0;
        s_hi = samples < g.signal_floats - row_lo ? samples : g.signal_floats - row_lo;
    }
    const long long i_lo = record_clamp(s_lo - start, 0, limit), i_hi = record_clamp(s_hi - start, 0, limit);
    const wbuf_t to = make_wbuf_n((second ? g.y_out : g.x_out) + ((size_t)b * g.N + n) * row_len, row_len * 4u);
    const unsigned e0 = chunk * (unsigned)kAugPerBlock + threadIdx.x;   // this thread's first piece of the row
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    if (i_lo >= i_hi) {                                                 // nothing of the row is there: zeros, no load
#pragma unroll
        for (int u = 0; u < kAugUnroll; ++u) wbuf_st4(to, 4u * (e0 + u * kAugThreads), 0, zero);
        return;
    }
    const long long first = row_lo + start;                            // the signal index of element 0 (|first| < 2^62)
    const unsigned lo = (unsigned)i_lo, hi = (unsigned)i_hi;            // 0 <= lo < hi <= row_len
    if ((first & 3) == 0) {
        const unsigned p_lo = lo / 4u, p_hi = (hi + 3u) / 4u;           // the pieces that hold an element of [lo, hi)
        const wbuf_t from = make_wbuf_n(g.signals + (first + 4ll * p_lo), (p_hi - p_lo) * 16u);
        f32x4 v[kAugUnroll];
#pragma unroll
        for (int u = 0; u < kAugUnroll; ++u) {
            const unsigned e = e0 + u * kAugThreads;
            v[u] = wbuf_ld4(from, 4u * ((e < p_lo ? p_lo : (e >= p_hi ? p_hi - 1u : e)) - p_lo), 0);
        }
#pragma unroll
        for (int u = 0; u < kAugUnroll; ++u) {
            const unsigned i = 4u * (e0 + u * kAugThreads);
            f32x4 w;
#pragma unroll
            for (unsigned j = 0; j < 4; ++j) w[j] = (i + j >= lo && i + j < hi) ? v[u][j] : 0.f;
            wbuf_st4(to, i, 0, w);
        }
        return;
    }
    const wbuf_t from = make_wbuf_n(g.signals + (first + (long long)lo), (hi - lo) * 4u);
    const unsigned i0 = chunk * (unsigned)(4 * kAugPerBlock);           // the first element of this block's stretch
    float d[4 * kAugUnroll];
#pragma unroll
    for (int k = 0; k < 4 * kAugUnroll; ++k) {
        const unsigned i = i0 + threadIdx.x + k * kAugThreads;
        d[k] = wbuf_ld(from, (i < lo ? lo : (i >= hi ? hi - 1u : i)) - lo, 0);
    }
#pragma unroll
    for (int k = 0; k < 4 * kAugUnroll; ++k) {
        const unsigned i = i0 + threadIdx.x + k * kAugThreads;
        stage[threadIdx.x + k * kAugThreads] = (i >= lo && i < hi) ? d[k] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kAugUnroll; ++u)
        wbuf_st4(to, 4u * (e0 + u * kAugThreads), 0, *reinterpret_cast<const f32x4*>(stage + 4u * (threadIdx.x + u * kAugThreads)));
}
constexpr size_t kRecordStageBytes = (size_t)kAugPerBlock * 16;

__global__ __launch_bounds__(kAugThreads) void gather_records_kernel(RecordGather g, const void* __restrict__ label_pool,
                                                                     void* __restrict__ label_out, int label_bytes,
                                                                     long long* __restrict__ len_out, const long long* __restrict__ perm,
                                                                     long long n_perm, long long P, const long long* __restrict__ cursor,
                                                                     long long slot0) {
    EEG_DYN_SMEM(stage);
    gather_record_rows(g, label_pool, label_out, label_bytes, len_out, perm, n_perm, P, cursor, slot0, stage);
}

// the gather of an epoch that keeps its short last batch: the same copy, plus the slots that count (gather_tail_scalars, kernels_data.h)
__global__ __launch_bounds__(kAugThreads) void gather_records_tail_kernel(RecordGather g, const void* __restrict__ label_pool,
                                                                          void* __restrict__ label_out, int label_bytes,
                                                                          long long* __restrict__ len_out, const long long* __restrict__ perm,
                                                                          long long n_perm, long long P, const long long* __restrict__ cursor,
                                                                          long long slot0, long long step, int world, float* __restrict__ clip_w,
                                                                          float* __restrict__ denom, long long* __restrict__ n_valid) {
    EEG_DYN_SMEM(stage);
    gather_record_rows(g, label_pool, label_out, label_bytes, len_out, perm, n_perm, P, cursor, slot0, stage);
    gather_tail_scalars(n_perm, cursor, slot0, step, world, clip_w, denom, n_valid);
}

}  // namespace eeg
