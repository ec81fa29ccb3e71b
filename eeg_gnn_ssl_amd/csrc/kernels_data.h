// Epochs from a device-resident data set: the DataLoader's shuffle and collate on the GPU.  Reference (host, per epoch and per
// batch): `DataLoader(dataset, shuffle=True, batch_size=...)` of data/dataloader_detection.py:505-523, dataloader_classification.py:
// 449-467 and dataloader_ssl.py:441-459 -- a RandomSampler permutation per epoch, then the default collate stacks the samples a
// batch names.  Here the samples (features, windows or raw signals; labels; lengths; the SSL target) stay in HBM as pools of P
// clips, the epoch's permutation is the stable argsort of P Philox keys (epoch_keys_kernel; the sort is the framework's, once per
// epoch) and every step copies its own clips out of the pools into the step's static batch tensors (gather_clips_kernel), finding
// them through a cursor that lives on the device: a captured step replays over a whole epoch with no host data traffic.
#pragma once
#include "common.h"
#include "kernels_feat.h"

namespace eeg {

// A wide pool and the batch tensor it is gathered into: rows of `pieces` 16-byte pieces (P rows in the pool, B in the batch), handled
// by `chunks` = ceil(pieces / kAugPerBlock) blocks per clip.  pieces = 0: absent.
struct GatherWide {
    const float* pool;
    float* out;
    unsigned pieces, chunks;
};

// The clip of batch slot `slot` = rank * B + b of this step: perm[(cursor + slot) mod n_perm], clamped into 0..P-1.  WHATEVER the cursor
// and the perm entry hold, the result names a clip of the pool: the wrap and the clamp are the kernel's bounds, not error paths (an
// epoch normally ends before the cursor reaches n_perm and a permutation has no entry outside 0..P-1).  slot < n_perm (the host
// refuses B * world > n_perm), so the common case -- a cursor inside 0..n_perm-1 -- takes no division.
__device__ __forceinline__ long long gather_source(const long long* __restrict__ perm, long long n_perm, long long P,
                                                   const long long* __restrict__ cursor, long long slot) {
    long long c = cursor[0];
    if ((unsigned long long)c >= (unsigned long long)n_perm) {
        c %= n_perm;
        if (c < 0) c += n_perm;
    }
    long long pos = c + slot;
    if (pos >= n_perm) pos -= n_perm;
    const long long s = perm[pos];
    return s < 0 ? 0 : (s >= P ? P - 1 : s);
}

// the label of clip `src` into batch slot b: 4 or 8 bytes (float / int64), copied as bits; 0: no label
__device__ __forceinline__ void gather_label(const void* __restrict__ label_pool, void* __restrict__ label_out, int label_bytes, long long src,
                                             unsigned b) {
    if (label_bytes == 8) static_cast<long long*>(label_out)[b] = static_cast<const long long*>(label_pool)[src];
    else if (label_bytes == 4) static_cast<unsigned*>(label_out)[b] = static_cast<const unsigned*>(label_pool)[src];
}

// One launch per step (the body of gather_clips_kernel and gather_clips_tail_kernel): blockIdx.x = clip b of the batch, blockIdx.y = a stretch of kAugPerBlock 16-byte pieces of that clip's row of
// the first wide tensor (blockIdx.y < w0.chunks) or of the second (the SSL target pool) -- the launch shape of
// augment_features_kernel / window_stream_kernel: kAugUnroll pieces in flight per thread, consecutive lanes hold consecutive pieces
// (whole-line loads and stores; rows are multiples of 16 bytes and 16-byte aligned, the host refuses anything else).  Source and
// destination are addressed through buffer descriptors over exactly ONE clip row each (block-uniform): a piece index past the row
// cannot reach a neighbouring clip whatever the index arithmetic does.  The block (b, 0) also copies the clip's scalars: a label of
// 4 or 8 bytes (float / int64, copied as bits) and an int64 length.  Nothing here writes the cursor: cursor_advance_kernel follows on
// the stream.
__device__ __forceinline__ void gather_clip_rows(const GatherWide& w0, const GatherWide& w1, const void* __restrict__ label_pool,
                                                 void* __restrict__ label_out, int label_bytes, const long long* __restrict__ len_pool,
                                                 long long* __restrict__ len_out, const long long* __restrict__ perm, long long n_perm,
                                                 long long P, const long long* __restrict__ cursor, long long slot0) {
    const unsigned b = blockIdx.x;
    const long long src = gather_source(perm, n_perm, P, cursor, slot0 + (long long)b);
    const bool second = blockIdx.y >= w0.chunks;                        // block-uniform
    const GatherWide w = second ? w1 : w0;
    const unsigned chunk = second ? blockIdx.y - w0.chunks : blockIdx.y;
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        gather_label(label_pool, label_out, label_bytes, src, b);
        if (len_out != nullptr) len_out[b] = len_pool[src];
    }
    const size_t row = (size_t)w.pieces * 4;                            // floats per clip row
    const wbuf_t from = make_wbuf_n(w.pool + (size_t)src * row, w.pieces * 16u);
    const wbuf_t to = make_wbuf_n(w.out + (size_t)b * row, w.pieces * 16u);
    const unsigned e0 = chunk * (unsigned)kAugPerBlock + threadIdx.x;
    f32x4 v[kAugUnroll];
    // No per-lane branch: a piece index past the row re-reads the row's last piece and its store is dropped by the destination
    // descriptor (make_wbuf_n: the bound of a ragged last stretch).  Behind a branch the compiler waits for each load before it
    // issues the next, and the four pieces would travel one after the other.
#pragma unroll
    for (int u = 0; u < kAugUnroll; ++u) {
        const unsigned e = e0 + u * kAugThreads;
        v[u] = wbuf_ld4(from, 4u * (e < w.pieces ? e : w.pieces - 1u), 0);
    }
#pragma unroll
    for (int u = 0; u < kAugUnroll; ++u) wbuf_st4(to, 4u * (e0 + u * kAugThreads), 0, v[u]);
}
__global__ __launch_bounds__(kAugThreads) void gather_clips_kernel(GatherWide w0, GatherWide w1, const void* __restrict__ label_pool,
                                                                   void* __restrict__ label_out, int label_bytes,
                                                                   const long long* __restrict__ len_pool, long long* __restrict__ len_out,
                                                                   const long long* __restrict__ perm, long long n_perm, long long P,
                                                                   const long long* __restrict__ cursor, long long slot0) {
    gather_clip_rows(w0, w1, label_pool, label_out, label_bytes, len_pool, len_out, perm, n_perm, P, cursor, slot0);
}

// The gather of an epoch that KEEPS its short last batch (the reference's DataLoader, drop_last=False): the same copy -- the wrap
// fills the slots behind the end of the epoch with real, finite clips -- plus which slots count.  With pos_b = cursor + slot0 + b
// (the cursor as it stands, not wrapped): clip_w[b] = 1 if 0 <= pos_b < n_perm else 0, written by block (b, 0); block (0, 0) also
// writes the GLOBAL count of the step, n_valid = clamp(n_perm - cursor, 0, step) with step = B * world clips, and the divisor of
// this rank's criterion, denom = max(n_valid, 1) / world: behind the summed all-reduce and its 1/world, sum_valid g / denom is the
// mean over the clips that are there.  A full batch gives clip_w = 1 and denom = B exactly.  The sums run in unsigned arithmetic:
// no cursor overflows them.  Plain stores, in front of cursor_advance_kernel on the stream.  (gather_tail_scalars: the tail of every
// gather whose blockIdx.x is the batch slot -- this kernel's and gather_records_tail_kernel's.)
__device__ __forceinline__ void gather_tail_scalars(long long n_perm, const long long* __restrict__ cursor, long long slot0, long long step,
                                                    int world, float* __restrict__ clip_w, float* __restrict__ denom,
                                                    long long* __restrict__ n_valid) {
    if (blockIdx.y != 0 || threadIdx.x != 0) return;
    const long long c = cursor[0];
    const unsigned long long pos = (unsigned long long)c + (unsigned long long)slot0 + blockIdx.x;
    clip_w[blockIdx.x] = pos < (unsigned long long)n_perm ? 1.f : 0.f;
    if (blockIdx.x == 0) {
        const long long nv = c >= n_perm ? 0 : (c <= n_perm - step ? step : n_perm - c);     // (step <= n_perm: the host refuses more)
        n_valid[0] = nv;
        denom[0] = (float)(nv > 1 ? nv : 1) / (float)world;
    }
}
__global__ __launch_bounds__(kAugThreads) void gather_clips_tail_kernel(GatherWide w0, GatherWide w1, const void* __restrict__ label_pool,
                                                                        void* __restrict__ label_out, int label_bytes,
                                                                        const long long* __restrict__ len_pool, long long* __restrict__ len_out,
                                                                        const long long* __restrict__ perm, long long n_perm, long long P,
                                                                        const long long* __restrict__ cursor, long long slot0, long long step,
                                                                        int world, float* __restrict__ clip_w, float* __restrict__ denom,
                                                                        long long* __restrict__ n_valid) {
    gather_clip_rows(w0, w1, label_pool, label_out, label_bytes, len_pool, len_out, perm, n_perm, P, cursor, slot0);
    gather_tail_scalars(n_perm, cursor, slot0, step, world, clip_w, denom, n_valid);
}

// cursor += step (B * world clips), behind the gather on the stream and in front of the next one: one thread of one wave (the launch
// shape of rng_take_kernel), plain C++
__global__ void cursor_advance_kernel(long long* __restrict__ cursor, long long step) {
    if (blockIdx.x == 0 && threadIdx.x == 0) cursor[0] = (long long)((unsigned long long)cursor[0] + (unsigned long long)step);
}

// The epoch's shuffle: key i = 63 bits of Philox4x32-10 (common.h, the generator of the dropout masks and the augmentation draws) at
// counter words (c0, c1, c2, c3) = (i low, i high, epoch, kEpochKeyStream) under key `seed`; the permutation is the stable argsort of
// the keys.  A function of (seed, epoch, i) alone: every rank of a data-parallel run, any batch size and a run resumed from a
// checkpoint draw the same epoch.
// kEpochKeyStream is counter word c3, under the user's seed AS GIVEN.  It is NOT a further value of the `stream_id` of
// ops.make_rng_state (0, 1: dropout of head and decoder, 2: augmentation): that one is mixed into the SEED on the host, and every
// draw of those generators runs at c2 = c3 = 0.  The keys are apart from all of them because c3 != 0 here, not because 0..2 are
// taken in this field; a further generator of the make_rng_state family takes stream_id 3 THERE, a further counter-domain draw a
// non-zero c3 other than this one HERE.
constexpr unsigned kEpochKeyStream = 3u;
__global__ __launch_bounds__(256) void epoch_keys_kernel(unsigned long long seed, unsigned epoch, long long P, long long* __restrict__ keys) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += (long long)gridDim.x * blockDim.x) {
        unsigned w[4];
        philox4x32_10((unsigned)i, (unsigned)((unsigned long long)i >> 32), epoch, kEpochKeyStream, (unsigned)seed, (unsigned)(seed >> 32), w);
        keys[i] = (long long)((((unsigned long long)w[1] << 32) | w[0]) >> 1);
    }
}

}  // namespace eeg
