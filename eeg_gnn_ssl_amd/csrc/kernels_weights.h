// Class imbalance on the device: the per-clip multipliers of a step's criterion (bce_logits_cw_kernel / ce_logits_cw_kernel of
// kernels_tail.h, cls_head_loss_cw_kernel of kernels_head.h) and their divisor, written into device memory at fixed addresses once per
// step -- nn.CrossEntropyLoss(weight=) / nn.BCEWithLogitsLoss(pos_weight=) and per-sample weights inside a captured step, in an
// epoch's short last batch and across ranks with no host synchronisation.
#pragma once
#include "common.h"
#include "kernels_eval.h"    // ssl_eval_block_sum: the block's fixed-order double sum

namespace eeg {

constexpr int kClipWeightThreads = 256;
enum WeightNorm { kWeightNormSum = 0, kWeightNormCount = 1 };

// the class of a label: the int64 itself (classification; outside 0..C-1: no class, weight 1 -- the criterion's NaN rule is what
// speaks for such a clip) or label >= 0.5 ? 1 : 0 for detection's float labels (taken to be 0 or 1; a NaN label is class 0)
__device__ __forceinline__ float class_weight_of(const void* __restrict__ labels, int label_bytes, long long i, const float* __restrict__ class_w,
                                                 int C) {
    if (class_w == nullptr) return 1.f;
    long long c;
    if (label_bytes == 8) c = static_cast<const long long*>(labels)[i];
    else c = static_cast<const float*>(labels)[i] >= 0.5f ? 1 : 0;
    return (c >= 0 && c < (long long)C) ? class_w[c] : 1.f;
}

// ONE workgroup per step.  Slot s of the step's `slots` clips carries u_s = valid_s * class_w[class(label_s)] * sample_w[src_s], each
// factor optional (nullptr: 1); this rank's slots slot0 .. slot0 + B - 1 are written to clip_u, and denom[0] = D / world with
//   norm sum:   D = sum_s u_s over ALL slots of the step (the reduction of nn.CrossEntropyLoss(weight=)); a zero sum gives D = 1
//               (loss 0, gradients 0, no 0/0);
//   norm count: D = max(n_valid, 1), the number of slots that are there (nn.BCEWithLogitsLoss(pos_weight=): a plain mean).
// D / world is the convention of the tail (gather_tail_scalars): behind the summed all-reduce and its 1/world the gradient is
// sum_s u_s g_s / D.  The quotient is formed in double and rounded to float once; for the count that is the float quotient
// (float)n / (float)world of gather_tail_scalars bit for bit (a double has more than 2 * 24 + 2 digits: the second rounding is
// innocuous), so all-ones weights reproduce the validity path.
// Two forms.  perm != nullptr (an epoch from device-resident pools): `labels` is the label POOL of P clips, slot s is the clip
// perm[..] at position c + s of the epoch, with c = cursor[0] - back the cursor as the step's gather saw it (the gather has advanced
// it by back = B * world since) -- position, clamp and validity are those of gather_source / gather_tail_scalars (kernels_data.h); a
// slot behind the end of the epoch has weight 0 and its (wrapped) clip is not looked at, so a step may be longer than the epoch.
// Every rank holds the pools and walks all slots: the same divisor bits everywhere, no communication.  perm == nullptr (a batch handed
// in): `labels` are the batch's own B labels, every slot counts, slots = B and world = 1: the divisor is the rank's own.
// The sum is fixed-order double (thread t adds the slots t, t + 256, ..., then the tree): bit-reproducible, no atomics; plain stores.
__global__ __launch_bounds__(kClipWeightThreads) void clip_weights_kernel(const void* __restrict__ labels, int label_bytes,
                                                                          const long long* __restrict__ perm, long long n_perm, long long P,
                                                                          const long long* __restrict__ cursor, long long back, int B,
                                                                          long long slot0, long long slots, int world,
                                                                          const float* __restrict__ class_w, int C,
                                                                          const float* __restrict__ sample_w, int norm,
                                                                          float* __restrict__ clip_u, float* __restrict__ denom) {
    EEG_DYN_SMEM(smf);
    double* s = reinterpret_cast<double*>(smf);                          // kClipWeightThreads words
    const bool pooled = perm != nullptr;
    const long long c = pooled ? (long long)((unsigned long long)cursor[0] - (unsigned long long)back) : 0;
    double sum = 0.0, count = 0.0;
    for (long long slot = threadIdx.x; slot < slots; slot += kClipWeightThreads) {
        float u = 0.f;
        // a slot that is there sits at position pos < n_perm of perm: where gather_source finds it (its wrap only moves the others)
        const unsigned long long pos = (unsigned long long)c + (unsigned long long)slot;
        const bool valid = !pooled || pos < (unsigned long long)n_perm;
        if (valid) {
            long long src = slot;
            if (pooled) {
                src = perm[pos];
                src = src < 0 ? 0 : (src >= P ? P - 1 : src);               // the gather's clamp: whatever perm holds names a clip of the pool
            }
            u = class_weight_of(labels, label_bytes, src, class_w, C) * (sample_w != nullptr ? sample_w[src] : 1.f);
            count += 1.0;
        }
        sum += (double)u;
        if (slot >= slot0 && slot < slot0 + B) clip_u[slot - slot0] = u;
    }
    sum = ssl_eval_block_sum(s, sum);
    count = ssl_eval_block_sum(s, count);
    if (threadIdx.x != 0) return;
    double d = norm == kWeightNormCount ? (count > 1.0 ? count : 1.0) : sum;
    if (d == 0.0) d = 1.0;
    denom[0] = (float)(d / (double)world);
}

}  // namespace eeg
