// Launch plans of the per-clip correlation Gram (kernels_graph.h: corr_gram_kernel<NQ, REM4, LEN>, corr_gram_rows_kernel<REM4, LEN>,
// corr_finish_kernel): the instance that takes a call, its grid, block and LDS bytes, the launch arguments derived from the shape,
// the workspace the partial Grams need, and every shape refusal.  Pure functions of the call (no global is read: dev knob 7 comes
// in through it); every selection rule of the family is stated here and nowhere else.  The entry points of api.cpp size the
// workspace and launch by the same plan.  No kernel bodies: this header compiles as plain host C++
// (tests/emu/gemm_plan_driver.cpp prints the plans, tests/golden/corr_plans_v1.json pins them).
#pragma once
#include "common.h"

namespace eeg {

constexpr int kGramTile = 256;                 // one 16x16 MFMA accumulator tile, C layout (r*64 + lane)
constexpr int kGramFloats = 3 * kGramTile;     // tiles (0,0), (0,1), (1,1) of the padded 32x32 Gram
constexpr int kRowChunk = 256;                 // floats of one node's row in a chunk of corr_gram_rows_kernel: one 1-KB wave-DMA
// LDS of corr_finish_kernel: the Gram G[32][33] and the adjacency A[32][33] (rows padded by one float against bank conflicts),
// then the row sums and the column sums of A, 32 floats each: 2*32*33 + 64 floats
constexpr size_t corr_finish_lds_bytes() { return (2 * kMaxNodes * (kMaxNodes + 1) + 2 * kMaxNodes) * sizeof(float); }

// CorrGramPlan::error / CorrRowsPlan::error, in the order the refusals are checked
constexpr int kCorrBadNodes = 1, kCorrBadDim = 2, kCorrEmpty = 3, kCorrStaging = 4, kCorrNoInstance = 5;
constexpr int kRowsBadNodes = 1, kRowsEmpty = 2, kRowsBadPiece = 3, kRowsPieceStride = 4, kRowsTwoGb = 5, kRowsRawSteps = 6, kRowsWindowSteps = 7;

// workgroups per clip that share a clip's `units` of work (time steps / row chunks): ~1024 workgroups in all (dev knob 7 overrides
// the target), every wave of a workgroup with at least one unit
inline long long corr_nsplit(int B, long long units, int knob_wgs) {
    long long ns = ceil_div(knob_wgs > 0 ? knob_wgs : 1024, B);
    const long long cap = (units + 3) / 4;
    if (ns > cap) ns = cap;
    return ns < 1 ? 1 : ns;
}

// X (B, T, N, D): grid (B, ns), a time step staged as one contiguous stream of whole 1-KB wave-DMAs
struct CorrGramPlan {
    int nq; bool rem4, len;         // corr_gram_kernel<nq, rem4, len>: 16-feature quads of a row, at most 20 nodes, variable lengths
    int ns, step_floats;
    int gx, gy, block;
    size_t lds, ws_floats;          // ws_floats depends on B, T and the knob alone (eeg_dcrnn_corr_graph_ws_floats knows no more)
    int error;
};
inline CorrGramPlan corr_gram_plan(int B, int T, int N, int D, bool has_len, int knob_wgs) {
    CorrGramPlan p{};
    p.error = (N < 1 || N > kMaxNodes) ? kCorrBadNodes : (D < 4 || D % 4 != 0) ? kCorrBadDim : (B < 1 || T < 1) ? kCorrEmpty : 0;
    if (B >= 1 && T >= 1) {
        p.ns = (int)corr_nsplit(B, T, knob_wgs);
        p.ws_floats = (size_t)B * p.ns * kGramFloats;
    }
    if (p.error) return p;
    p.step_floats = round_up(N * D, 256);
    p.lds = 4 * (size_t)(p.step_floats > kGramFloats ? p.step_floats : kGramFloats) * sizeof(float);
    if (p.lds > 64 * 1024) { p.error = kCorrStaging; return p; }
    p.nq = ceil_div(D, 16);
    if (p.nq > 8) { p.error = kCorrNoInstance; return p; }
    p.rem4 = N <= 20; p.len = has_len;
    p.gx = B; p.gy = p.ns; p.block = 256;
    return p;
}

// Wide channel rows: P pieces of Q floats per node, piece_stride floats apart (one piece: raw rows; >= N*Q apart: window tensors);
// grid (B, ns), chunks of kRowChunk floats per node.  has_len: `steps` = the steps of a full clip (raw rows: Q = steps * samples
// per step; window tensors: steps = P).
struct CorrRowsPlan {
    bool rem4, len;                 // corr_gram_rows_kernel<rem4, len>
    int ns, tile_floats;
    int unit;                       // samples per step of raw rows; 0: window tensors (a step = a piece), or no lengths
    unsigned ps;                    // piece stride handed to the kernel (0 for one piece)
    long long clip_floats;          // extent of a clip = what its buffer descriptor covers
    int gx, gy, block;
    size_t lds, ws_floats;          // ws_floats depends on B, P, Q and the knob alone
    int error;
};
inline CorrRowsPlan corr_rows_plan(int B, int N, int P, int Q, long long piece_stride, bool has_len, int steps, int knob_wgs) {
    CorrRowsPlan p{};
    if (B >= 1 && P >= 1 && Q >= 1) {
        const long long ns = corr_nsplit(B, (long long)P * ceil_div(Q, kRowChunk), knob_wgs);
        p.ns = (int)(ns > 65535 ? 65535 : ns);          // grid.y
        p.ws_floats = (size_t)B * p.ns * kGramFloats;
    }
    p.error = (N < 1 || N > kMaxNodes) ? kRowsBadNodes : (B < 1 || P < 1) ? kRowsEmpty : (Q < 4 || Q % 4 != 0) ? kRowsBadPiece : 0;
    if (p.error) return p;
    if (P > 1 && (piece_stride < (long long)N * Q || piece_stride % 4 != 0)) { p.error = kRowsPieceStride; return p; }
    p.clip_floats = (P > 1 ? (long long)(P - 1) * piece_stride : 0) + (long long)N * Q;
    if (p.clip_floats * 4 >= (1LL << 31)) { p.error = kRowsTwoGb; return p; }
    if (has_len && P == 1) {
        if (steps < 1 || Q % steps != 0 || (Q / steps) % 4 != 0) { p.error = kRowsRawSteps; return p; }
        p.unit = Q / steps;
    } else if (has_len && steps != P) {
        p.error = kRowsWindowSteps;
        return p;
    }
    p.tile_floats = N * kRowChunk > kGramFloats ? N * kRowChunk : kGramFloats;
    p.lds = 4 * (size_t)p.tile_floats * sizeof(float);            // <= 128 KB (N = 32)
    p.ps = P > 1 ? (unsigned)piece_stride : 0u;
    p.rem4 = N <= 20; p.len = has_len;
    p.gx = B; p.gy = p.ns; p.block = 256;
    return p;
}

}  // namespace eeg
