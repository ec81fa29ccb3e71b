// Occlusion maps (the interpretability method of the paper behind the model) on the device: for every clip, one group of channels is
// overwritten with a fill value over one window of steps and the map records how far the predicted probability drops.  An occlusion
// that starts at step t0 leaves every state before t0 untouched, so all variants of a window start from the unoccluded clip's state
// at t0 and run only T - t0 steps.  occlude_expand_kernel (one launch per window) builds what the layer operators need for the B * G
// variants of that window -- the time-major inputs, the initial states of all layers, the remaining lengths --, occlusion_scores_kernel
// (one launch per window, behind the head) turns the variants' logits into one (B, G) slice of the map.  Plain C++, vector stores.
#pragma once
#include "common.h"

namespace eeg {

constexpr int kOccMaxLayers = 4;       // EEG_OCCLUDE_MAX_LAYERS
constexpr int kOccMaxGroups = 64;      // EEG_OCCLUDE_MAX_GROUPS: a node's memberships are one 64-bit word
constexpr int kOccThreads = 256;
constexpr int kOccBlocksPerCu = 8;     // the grid is capped at this many blocks per compute unit; the units beyond it are grid-strided
constexpr int kOccMaxClasses = 1024;

// x (B, T, N, D) batch-major, hext[l] (T+1, B, N*H) of the unoccluded pass (slot t = the state in front of step t), groups (G, N) 0/1.
// Variant v = b * G + g of the window that starts at t0 and is w steps wide:
//   x_var[s, v, n, :]  = fill if s < w and groups[g, n] != 0, else x[b, t0 + s, n, :]        (T - t0, B*G, N, D)
//   h0_var[l, v, :]    = hext[l][t0, b, :]                                                   (L, B*G, N*H)
//   len_var[v]         = max(lengths[b] - t0, 1)   (lengths null: T - t0)                    (B*G)
// D4 = D / 4 and NH4 = N * H / 4: everything moves in 16-byte pieces.
struct OccludeExpand {
    const float* x;
    const float* hext[kOccMaxLayers];
    const int* groups;
    const long long* lengths;
    float* x_var;
    float* h0_var;
    long long* len_var;
    int B, T, N, D4, NH4, L, G, t0, w;
    int gper, nch;                     // groups per unit, units per (step, clip) = ceil(G / gper)
    float fill;
};

// The kernel is bound by the bytes it writes; its reads hit the same B clips G times.  A unit of work is one contiguous source row --
// the N * D4 pieces of x[b, t0 + s] or the NH4 pieces of hext[l][t0, b] -- and a stretch of gper consecutive groups: a thread loads
// its pieces of the row ONCE (two 16-byte loads in flight) and stores them to each of the unit's variants, whose rows lie N * D
// (N * H) floats apart.  The host splits G into stretches only as far as it takes to fill the capped grid, so the source is read
// between once and G times and the repeats come from L2.  Everything that decides addresses -- step, clip, layer, the stretch, whether
// the step lies inside the window -- is block-uniform; the one per-lane decision is the select between fill and the loaded piece.
// The group mask is read once per block: thread n folds column n of groups into bits[n] (bit g = node n belongs to group g).
__global__ __launch_bounds__(kOccThreads) void occlude_expand_kernel(OccludeExpand a) {
    EEG_DYN_SMEM(smf);
    unsigned long long* bits = reinterpret_cast<unsigned long long*>(smf);      // kMaxNodes words
    const int tid = threadIdx.x;
    if (tid < a.N) {
        unsigned long long m = 0;
        for (int g = 0; g < a.G; ++g) m |= (unsigned long long)(a.groups[g * a.N + tid] != 0) << g;
        bits[tid] = m;
    }
    __syncthreads();
    const int BG = a.B * a.G, steps = a.T - a.t0;
    if (blockIdx.x == 0) {
        for (int v = tid; v < BG; v += kOccThreads) {
            const long long len = a.lengths != nullptr ? a.lengths[v / a.G] : (long long)a.T;
            a.len_var[v] = len - a.t0 > 1 ? len - a.t0 : 1;
        }
    }
    const f32x4 fillv = {a.fill, a.fill, a.fill, a.fill};
    const int per_row = a.B * a.nch, x_units = steps * per_row, units = x_units + a.L * per_row;
    for (int u = blockIdx.x; u < units; u += gridDim.x) {
        const bool state = u >= x_units;
        const int q = state ? u - x_units : u;
        const int s = q / per_row, r = q - s * per_row;                         // s: the step behind t0, or the layer
        const int b = r / a.nch, c = r - b * a.nch;
        const int g0 = c * a.gper, g1 = g0 + a.gper < a.G ? g0 + a.gper : a.G;
        const int pieces = state ? a.NH4 : a.N * a.D4;
        const size_t row = 4 * (size_t)pieces;                                  // floats of one source / variant row
        const float* src = state ? a.hext[s] + ((size_t)a.t0 * a.B + b) * row : a.x + ((size_t)b * a.T + a.t0 + s) * row;
        float* dst = (state ? a.h0_var : a.x_var) + ((size_t)s * BG + (size_t)b * a.G) * row;
        const bool inside = !state && s < a.w;
        for (int i0 = tid; i0 < pieces; i0 += 2 * kOccThreads) {
            const int i1 = i0 + kOccThreads;
            const bool two = i1 < pieces;
            const f32x4 v0 = ld4(src + 4 * (size_t)i0);
            const f32x4 v1 = two ? ld4(src + 4 * (size_t)i1) : v0;
            const unsigned long long m0 = inside ? bits[i0 / a.D4] : 0ull, m1 = (inside && two) ? bits[i1 / a.D4] : 0ull;
            for (int g = g0; g < g1; ++g) {
                float* d = dst + (size_t)g * row;
                st4(d + 4 * (size_t)i0, ((m0 >> g) & 1ull) ? fillv : v0);
                if (two) st4(d + 4 * (size_t)i1, ((m1 >> g) & 1ull) ? fillv : v1);
            }
        }
    }
}

// the probability the map follows, in double from the float32 logits: the sigmoid of the one logit, or entry `cls` of the softmax row
__device__ __forceinline__ double occlusion_prob(const float* __restrict__ r, int C, int cls) {
    if (C == 1) return 1.0 / (1.0 + exp(-(double)r[0]));
    double mx = (double)r[0];
    for (int c = 1; c < C; ++c) mx = (double)r[c] > mx ? (double)r[c] : mx;
    double se = 0.0;
    for (int c = 0; c < C; ++c) se += exp((double)r[c] - mx);
    return exp((double)r[cls] - mx) / se;
}

// One thread per variant v = b * G + g of window k (start t0): maps[b, k, g] = p_b - p_v, exactly 0.0f where the window starts at or
// behind the clip's end (t0 >= lengths[b]; lengths null: never).  The class followed is target[b] clamped to 0..C-1, or (target null)
// the first arg-max of the baseline row.  Both probabilities are formed in double, so the cancellation in their difference costs
// nothing; the difference is rounded to float32 once.  first != 0 (window 0): the thread of group 0 also writes base_prob[b] and
// the class it followed (target_out nullable).
__global__ void occlusion_scores_kernel(const float* __restrict__ var_logits, const float* __restrict__ base_logits,
                                        const long long* __restrict__ lengths, const long long* __restrict__ target, int B, int G, int C,
                                        int Tw, int k, int t0, int first, float* __restrict__ maps, float* __restrict__ base_prob,
                                        long long* __restrict__ target_out) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= B * G) return;
    const int b = v / G, g = v - b * G;
    const float* base = base_logits + (size_t)b * C;
    int cls = 0;
    if (C > 1) {
        if (target != nullptr) {
            const long long t = target[b];
            cls = t < 0 ? 0 : (t >= (long long)C ? C - 1 : (int)t);
        } else {
            for (int c = 1; c < C; ++c)
                if (base[c] > base[cls]) cls = c;                               // (strict: the lowest index of equals stays)
        }
    }
    const double pb = occlusion_prob(base, C, cls);
    const bool live = lengths == nullptr || (long long)t0 < lengths[b];
    maps[((size_t)b * Tw + k) * G + g] = live ? (float)(pb - occlusion_prob(var_logits + (size_t)v * C, C, cls)) : 0.f;
    if (first && g == 0) {
        base_prob[b] = (float)pb;
        if (target_out != nullptr) target_out[b] = (long long)cls;
    }
}

}  // namespace eeg
