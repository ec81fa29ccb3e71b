// Launch plan of the hop diffusion (kernels_diffuse.h: diffuse_fwd_stream_kernel<19>, diffuse_adj_stream_kernel<19>,
// diffuse_adj_rows_kernel<19, 3 | 5> and the LDS/MFMA kernels diffuse_fwd_kernel / diffuse_adj_kernel): which kernel takes a call,
// with what grid, block, LDS bytes and column chunk.  A pure function of the call (no global is read: the dev knobs come in through
// it); every selection rule of the family is stated here and nowhere else.  diffuse_fwd / diffuse_adj of api.cpp execute the plan.
// No kernel bodies: this header compiles as plain host C++ (tests/emu/gemm_plan_driver.cpp prints the plans,
// tests/golden/diffuse_plans_v1.json pins them).
//
// The two directions differ in two places, kept as they were measured and shipped:
//   * the forward LDS kernel prefetches the next sample into kDiffPrefetch float4 per thread, so its column chunk is also bounded by
//     N * (fc / 4) <= 256 * kDiffPrefetch; the adjoint kernel has no such registers and no such bound;
//   * the adjoint streaming kernels address Z with 32-bit float4 offsets, so the adjoint streams only while S*N*M*F < 1.7e10; the
//     forward streaming rule has no such clause.
#pragma once
#include "common.h"

namespace eeg {

enum class DiffuseKind { None, StreamFwd, StreamAdj, RowsAdj, LdsFwd, LdsAdj };
constexpr int kDiffuseNoFit = 1, kDiffuseBatchMajorNeedsStream = 2;     // DiffusePlan::error

struct DiffuseCall {
    int p_batched, S, B, N, F, M;   // S samples of (N, F) rows, M hop matrices incl. the identity; per-clip graphs: S = T * B
    bool adjoint;
    int x_bt = 0;                   // forward: X is batch-major (B, S/B, N, F) (streaming kernel only)
    bool wants_copy = false;        // forward: the time-major copy of X is written too
    // dev knobs (include/eeg_dcrnn_dev.h; compile-time zeros in the product build)
    int fwd_wgs = 0;                // EEG_TUNE_DIFFUSE_FWD_WGS: workgroup target of the streaming forward (default 1024)
    int adj_wgs = 0;                // EEG_TUNE_DIFFUSE_ADJ_WGS: the same, adjoint (default 4096; 512 .. 4096 measured alike)
    int adj_lds = 0;                // EEG_TUNE_DIFFUSE_ADJ_LDS = 1: the LDS/MFMA adjoint also where the streaming one applies
    int adj_planes = 0;             // EEG_TUNE_DIFFUSE_ADJ_PLANES = 1: diffuse_adj_stream_kernel also where a rows instance exists
};
struct DiffusePlan {
    DiffuseKind kind;
    int mm;                         // RowsAdj: diffuse_adj_rows_kernel<19, mm>
    int gx, gy, block;
    size_t lds;                     // bytes of dynamic LDS
    int fc, nchunks;                // LDS kernels: one launch per column chunk [c0, c0 + fc) of the F-wide rows
    int error;
};

// The streaming kernels (no LDS) take the EEG montage with rows of at most 128 float4 and >= 4 samples per graph: launches with
// fewer (decoder steps) leave most of their lanes idle and are faster through the LDS/MFMA kernels.  The adjoint adds its knob and
// the bound of its 32-bit offsets (above).  The batch-major input option of eeg_dcrnn_layer_fwd exists where the forward streams.
inline bool diffuse_streams(const DiffuseCall& c) {
    if (c.adjoint && (c.adj_lds != 0 || !((double)c.S * c.N * c.M * c.F < 1.7e10))) return false;
    return c.N == 19 && c.F / 4 <= 128 && c.S / (c.p_batched ? c.B : 1) >= 4;
}
// grid (graphs, ny) and block of a streaming launch: a workgroup walks consecutive samples, block / (F/4) at a time
inline void diffuse_stream_launch(DiffusePlan& p, const DiffuseCall& c, int wgs) {
    const int F4 = c.F / 4, sB = c.p_batched ? c.B : 1, T = c.S / sB;
    int threads = 256;                        // few samples per graph: narrower workgroups
    while (threads > 64 && (threads / 2) / F4 >= T && (threads / 2) >= F4) threads /= 2;
    int ny = ceil_div(T, threads / F4);
    // forward: ~4 workgroups per CU in total, each walking >= 2 passes of consecutive samples: measured on MI355X (cfg2, F=100,
    // profiles/r02_b_diffuse_sweep.txt) 64 us against 75 us with 6 single-pass workgroups per CU and 68 / 85 us with 2 / 1
    // (fewer, longer sequential streams suit the DRAM pages better than more parallelism); prefetching the next
    // sample's rows ahead of the stores was slower (71 us)
    const int want = ceil_div(wgs, sB);
    if (ny > want) ny = want;
    if (ny < 1) ny = 1;
    p.gx = sB; p.gy = ny; p.block = threads; p.lds = 0;
}
// LDS of the LDS/MFMA kernels: Pl | tile [round_up(N, 4)][lds_stride(M * round_up(fc, 16))] (kernels_diffuse.h)
constexpr size_t diffuse_lds_bytes(int N, int M, int fc) {
    return ((size_t)(M - 1) * kPFloats + (size_t)round_up(N, 4) * lds_stride(M * round_up(fc, 16))) * sizeof(float);
}
// LDS kernels: rows wider than one tile (96 KB of LDS; forward: the prefetch registers) go in column chunks, one launch each
inline void diffuse_lds_launch(DiffusePlan& p, const DiffuseCall& c) {
    auto too_wide = [&](int fc) { return !c.adjoint && c.N * (fc / 4) > 256 * kDiffPrefetch; };
    int fc = c.F;
    while (fc > 16 && (diffuse_lds_bytes(c.N, c.M, fc) > 96 * 1024 || too_wide(fc))) fc = round_up(ceil_div(fc, 2), 16);
    p.lds = diffuse_lds_bytes(c.N, c.M, fc);
    if (p.lds > kMaxLdsBytes || too_wide(fc)) { p.error = kDiffuseNoFit; return; }
    p.fc = fc; p.nchunks = ceil_div(c.F, fc); p.block = 256;
    if (!c.adjoint && c.p_batched) {          // forward, per-clip graphs: workgroup (b, tg) keeps clip b's polynomials
        const int T = c.S / c.B;
        int tg = ceil_div(2048, c.B);
        if (tg > T) tg = T;
        p.gx = c.B; p.gy = tg < 1 ? 1 : tg;
    } else {
        p.gx = c.S < 2048 ? c.S : 2048; p.gy = 1;
    }
}

inline DiffusePlan diffuse_plan(const DiffuseCall& c) {
    DiffusePlan p{};
    if (!c.adjoint && c.M == 1 && !c.wants_copy) return p;      // max_diffusion_step = 0: no planes (a requested copy still runs)
    const bool streams = diffuse_streams(c);
    if (c.x_bt && !streams) { p.error = kDiffuseBatchMajorNeedsStream; return p; }
    if (!streams) {
        diffuse_lds_launch(p, c);
        if (p.error == 0) p.kind = c.adjoint ? DiffuseKind::LdsAdj : DiffuseKind::LdsFwd;
        return p;
    }
    if (!c.adjoint) {
        p.kind = DiffuseKind::StreamFwd;
        diffuse_stream_launch(p, c, c.fwd_wgs > 0 ? c.fwd_wgs : 1024);
        return p;
    }
    // Z walked in storage order (all hop slots of a node row together) where the hop count has an instantiation
    const bool rows = c.adj_planes == 0 && (c.M == 3 || c.M == 5);
    p.kind = rows ? DiffuseKind::RowsAdj : DiffuseKind::StreamAdj;
    p.mm = rows ? c.M : 0;
    diffuse_stream_launch(p, c, c.adj_wgs > 0 ? c.adj_wgs : 4096);
    return p;
}

}  // namespace eeg
