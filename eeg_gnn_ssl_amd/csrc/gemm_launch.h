// Launch plans of the hoisted GEMMs: which kernel takes an NN (C = [segments] @ pack + bias) or a TN (split-K partials of A^T dY)
// problem, with what template integers, grid, block, LDS bytes and row split.  Pure functions of the call (no global is read: CU
// count and dev knobs come in through it); every selection rule of the family is stated here and nowhere else.  The callers in
// api.cpp ask for a plan BEFORE they size workspaces and lay out operands; gemm_nn / gemm_tn there and the launchers of
// gemmq_inst.cpp execute it.  No kernel bodies and no operand types: this header compiles as plain host C++.
#pragma once
#include "common.h"
#include "nnq_order.h"

namespace eeg {

// dev knobs (include/eeg_dcrnn_dev.h; compile-time zeros in the product build)
struct GemmKnobs {
    int nn_staged = 0;      // EEG_TUNE_NN_STAGED = 1: register-staged NN kernel (no LDS-DMA, no quad kernel)
    int tn_staged = 0;      // EEG_TUNE_TN_STAGED = 1: register-staged TN kernel (no LDS-DMA, no quad kernel)
    int quad = 0;           // EEG_TUNE_QUAD: bit 0 = no quad NN kernel, bit 1 = no quad TN kernel, bits 2.. = rows per CU from which they run
    int tn_xcd = 0;         // EEG_TUNE_TN_XCD: 1 = no XCD placement in the DMA TN kernel, 2 = placement in the staged one
    int tn_wide_from = 0;   // EEG_TUNE_TN_WIDE_FROM: 8-wave / 128-column k-blocks for dY tiles of this width and up (0 = never)
    int tn_target = 0;      // EEG_TUNE_TN_TARGET: workgroup target of the split TN kernels
    int tnq_target = 0;     // EEG_TUNE_TNQ_TARGET: workgroup target of the quad TN kernel
    int tn_no_pair = 0;     // EEG_TUNE_TN_NO_PAIR = 1: the two h-part problems of a cell as two launches
};
enum GemmPlanError { kGemmOk = 0, kGemmNeedsRowMap, kGemmBadO };   // batch-major rows, but the kernel left has no row map / O > 192

// ---- LDS floats of the kernels, by their template integers (kernels_gemm.h, kernels_gemm_bf.h, kernels_gemm_q.h) -----------
constexpr size_t gemm_nn_lds_floats(int NCTW, int KC) { return 2 * (size_t)(128 * lds_stride(KC) + (KC / 4) * 2 * NCTW * 64); }   // gemm_nn_kernel
constexpr size_t gemm_nn_dma_lds_floats(int NCTW, int KC) { return 2 * (size_t)(128 * KC + (KC / 4) * 2 * NCTW * 64); }          // gemm_nn_dma_kernel
constexpr size_t gemm_nn_bf3_lds_bytes(int NTB) { return 2 * 3 * (size_t)NTB * 1024; }                                            // gemm_nn_bf3_kernel
constexpr int kNnrStages = 4;                           // gemm_nnr_kernel<NS = 4, 2>: 4 activation stages of 8 KB + 192 bias floats
constexpr size_t gemm_nnr_lds_floats(int NS) { return (size_t)NS * 128 * 16 + 192; }
constexpr size_t gemm_tn_lds_floats(int NCTW) {                                                                                   // gemm_tn_kernel
    const int OT = 2 * NCTW * 16, YS = OT + ((16 - (OT % 32)) + 32) % 32;
    return 2 * (size_t)(32 * 80 + 32 * YS);
}
constexpr size_t gemm_tn_dma_lds_floats(int KTW, int NCTW, int RC, int WK) {                                                       // gemm_tn_dma_kernel
    return 2 * (size_t)(RC * 16 * KTW * WK + RC * 2 * NCTW * 16);
}
constexpr int kTnqRc = 16;                              // row-chunk depth of gemm_tnq_kernel / gemm_tnq_pair_kernel
constexpr size_t gemm_tnq_lds_floats(int KT, int OT) { return 3 * (size_t)(kTnqRc * 32 * (KT + OT)); }

// fewest rows the persistent quad GEMMs are used for: below it the ramp of their 2-per-CU grid costs more than the split
// kernels' many small workgroups
inline int quad_min_rows(const GemmKnobs& k, int num_cus) { return ((k.quad >> 2) > 0 ? (k.quad >> 2) : 256) * num_cus; }

// ---- NN ---------------------------------------------------------------------------------------------------------------------
enum class NnKind { Quad, Dma, Staged, Bf3 };   // gemm_nnr_kernel<4, 2>, gemm_nn_dma_kernel<NCTW, KC, MINB>, gemm_nn_kernel<NCTW, KC>, gemm_nn_bf3_kernel<NTB>
struct NnCall {
    int nseg, F, R, nct_total, ldc, O;   // nseg segments of F columns, R rows; nct_total 16-column tiles of the fp32 packs
    bool batch_major = false;            // the rows of the segments are batch-major: only kernels with a row map can read them
    bool quad_pack = false;              // the caller holds the right-hand side in the quad order of gemm_nnr_kernel
    int bf3_nct = 0;                     // column tiles of the bf16 term pack the caller holds (opt-in, kernels_gemm_bf.h); 0 = none
    int num_cus = 0;
    GemmKnobs knobs;
};
struct NnPlan {
    NnKind kind;
    int nctw, kc, minb;     // Dma / Staged: NCTW, KC (Dma: MINB); Bf3: nctw = NTB
    int gx, gy, block;
    size_t lds;             // bytes of dynamic LDS
    int error;
};

// gemm_nnr_kernel applies to whole 192-column blocks (nct_total % 12 == 0), F % 4 == 0 with at most two tail chunks, 32-bit offsets
inline bool nnq_supported(int nseg, int F, int R, int nct_total, int ldc, int O) {
    if (nseg < 1 || nseg > kMaxM || F < 4 || F % 4 != 0 || R < 1) return false;
    if (nct_total < 12 || nct_total % 12 != 0 || O % 4 != 0 || ldc % 4 != 0 || O > 16 * nct_total) return false;
    if (make_nnq_order(nseg, F).ntail > 2) return false;
    // operands and results go through 2 GB buffer descriptors (platform.h make_wbuf): accesses beyond are dropped by the hardware
    return (double)R * F * 4.0 < 2147483648.0 && (double)R * ldc * 4.0 < 2147483648.0;
}
// floats of the quad pack of a (nseg * F) x (16 * nct) right-hand side
inline size_t nnq_pack_floats(int nseg, int F, int nct) { return (size_t)make_nnq_order(nseg, F).nch * nct * 256; }
// the LDS-DMA NN kernel (the default split kernel; it reads a row map): 16- or 20-deep K chunks that tile F, aligned result rows
inline bool nn_dma_applies(int F, int R, int ldc, const GemmKnobs& k) {
    return k.nn_staged == 0 && ldc % 4 == 0 && (double)R * F < 4.0e9 && (F % 16 == 0 || F % 20 == 0);
}

inline NnPlan gemm_nn_plan(const NnCall& c) {
    NnPlan p{NnKind::Staged, 0, 0, 2, ceil_div(c.R, 128), 0, 256, 0, kGemmOk};
    // opt-in three-term bf16 split: whole column blocks of 12, 10 or 8 tiles; a shape it does not cover plans as fp32 below
    const int ntb = c.bf3_nct % 12 == 0 ? 12 : c.bf3_nct % 10 == 0 ? 10 : c.bf3_nct % 8 == 0 ? 8 : 0;
    if (c.bf3_nct > 0 && ntb > 0 && c.F % 4 == 0 && c.ldc % 4 == 0 && c.O % 4 == 0 && (double)c.R * c.F < 4.0e9) {
        p.kind = NnKind::Bf3; p.nctw = ntb; p.gy = c.bf3_nct / ntb;
        p.lds = gemm_nn_bf3_lds_bytes(ntb);
        return p;
    }
    // the persistent quad kernel takes the launch when it covers the shape and every one of its 2-per-CU workgroups gets at
    // least two 128-row tiles
    if (c.quad_pack && (c.knobs.quad & 1) == 0 && c.knobs.nn_staged == 0 && c.R >= quad_min_rows(c.knobs, c.num_cus) &&
        nnq_supported(c.nseg, c.F, c.R, c.nct_total, c.ldc, c.O)) {
        p.kind = NnKind::Quad;
        const int tiles = ceil_div(ceil_div(c.R, 16), 8);              // at least one 128-row tile per workgroup
        p.gx = 2 * (c.num_cus > 0 ? c.num_cus : 256);
        if (p.gx > tiles) p.gx = tiles;
        if (p.gx < 1) p.gx = 1;
        p.gy = c.nct_total / 12;
        p.lds = gemm_nnr_lds_floats(kNnrStages) * sizeof(float);
        return p;
    }
    const bool dma = nn_dma_applies(c.F, c.R, c.ldc, c.knobs);
    // column block of 12, 10 or 8 tiles, whichever leaves the fewest padding tiles (20 tiles = dX at M = 5: 2 x 10 instead of
    // 2 x 12 with a sixth of the MFMAs on padding); with few row blocks (per-step decoder GEMMs) blocks of 4 fill more CUs
    const int pad6 = round_up(c.nct_total, 12) - c.nct_total, pad5 = round_up(c.nct_total, 10) - c.nct_total, pad4 = round_up(c.nct_total, 8) - c.nct_total;
    if (c.nct_total <= 4 || ceil_div(c.R, 128) * ceil_div(c.nct_total, 12) < 160) p.nctw = 2;
    else if (pad5 < pad6 && pad5 <= pad4 && c.F % 16 == 0 && dma) p.nctw = 5;
    else if (pad4 < pad6 && dma) p.nctw = 4;
    else p.nctw = 6;
    p.gy = ceil_div(c.nct_total, 2 * p.nctw);
    if (dma) {                                                          // LDS-DMA staging (default)
        p.kind = NnKind::Dma;
        p.kc = c.F % 16 == 0 ? 16 : 20;
        p.lds = gemm_nn_dma_lds_floats(p.nctw, p.kc) * sizeof(float);
        return p;
    }
    p.kc = c.F % 32 == 0 ? 32 : c.F % 20 == 0 ? 20 : c.F % 16 == 0 ? 16 : 4;
    p.lds = gemm_nn_lds_floats(p.nctw, p.kc) * sizeof(float);
    if (c.batch_major) p.error = kGemmNeedsRowMap;
    return p;
}

// ---- TN ---------------------------------------------------------------------------------------------------------------------
// partial[split][nseg*F][O] = sum over the rows of a split of A^T dY[:, ycol0 : ycol0 + O]; the caller's buffer holds
// plan.nsplit * nseg * F * O floats, asked from the same plan that is later executed
struct TnqPlan {
    int ok;                 // 0: the shape is not covered by gemm_tnq_kernel
    int KT, OT, planar;     // template instance
    int nkb, nsplit, rps;   // grid (k-blocks, row splits) and rows per split (multiple of 16)
};
// gemm_tnq_kernel<KT, OT, 16, BT, PLANAR, false>, gemm_tn_dma_kernel<2, NCTW, RC, WK> with WK = 2 / 4, gemm_tn_kernel<NCTW>
enum class TnKind { Quad, Dma, DmaWide, Staged };
struct TnCall {
    int nseg, F, R, O;
    bool batch_major = false;   // as NnCall
    bool offer_quad = false;    // the weight-gradient problems of a cell; the projection and dconv gradients keep the split kernels
    int num_cus = 0;
    GemmKnobs knobs;
};
struct TnPlan {
    TnKind kind;
    int nctw, rc, wk;       // Dma / DmaWide: NCTW, RC, WK; Staged: NCTW
    TnqPlan q;              // Quad: the template instance and the k-block count (launchers of gemmq_inst.cpp)
    int nsplit, rps;        // row splits and rows per split
    int gx, gy, block;
    size_t lds;             // bytes of dynamic LDS
    int remap;              // all k-blocks of a row split on ONE XCD (they read the same dY rows)
    int error;
};

// bt: the A segments are batch-major.  Covered: O in {64, 128, 192}, R % 16 == 0, and either 64-wide planes (any count,
// time-major) or O == 192 with any F % 4 == 0 (the x-part of a 64-unit cell)
inline TnqPlan tnq_plan(int nseg, int F, int R, int O, bool bt, int num_cus) {
    TnqPlan p{};
    if (nseg < 1 || nseg > kMaxM || F < 4 || F % 4 != 0 || R < 16 || R % 16 != 0) return p;
    if (O != 64 && O != 128 && O != 192) return p;
    if ((double)R * (F > 192 ? F : 192) * 4.0 >= 2147483648.0) return p;    // 2 GB descriptors on the segments and on dY (ldy <= 192)
    const int K = nseg * F;
    p.OT = O / 32;
    const bool planar_exact = F == 64 && !bt && (nseg % 3 == 0 || nseg % 2 == 0 || nseg == 1);
    if (planar_exact) {                                    // whole 64-wide planes per k-block, no padding plane
        p.planar = 1;
        p.KT = nseg % 3 == 0 ? 6 : (nseg % 2 == 0 ? 4 : 2);
        p.nkb = ceil_div(nseg, p.KT / 2);
    } else {
        // per-lane source pointers (any F % 4 == 0, batch-major or not; also 5 or 7 planes of 64, where whole-plane
        // blocks would multiply a padding plane: K = 320 is two exact blocks of 160 here).  k-block of 4 or 5 tiles per
        // wave slice (6 x 6 tiles + per-lane pointers spill): least padded K (= MFMA work), then the wider block
        if (bt && O != 192) return p;                      // (batch-major rows only occur on the x-part: 192 columns)
        int best = 5, bcost = 1 << 30, bnkb = 1;
        for (int kt = 5; kt >= 4; --kt) {
            const int nkb = ceil_div(K, 32 * kt), cost = nkb * 32 * kt;
            if (cost < bcost) { best = kt; bcost = cost; bnkb = nkb; }
        }
        p.KT = best; p.nkb = bnkb;
    }
    const int G = 2 * (num_cus > 0 ? num_cus : 256);
    int nsplit = G / p.nkb;
    if (nsplit < 1) nsplit = 1;
    int rps = round_up(ceil_div(R, nsplit), 16);
    if (rps < 64) rps = 64;
    p.rps = rps;
    p.nsplit = ceil_div(R, rps);
    p.ok = 1;
    return p;
}
// the LDS-DMA TN kernel (the default split kernel; it reads a row map)
inline bool tn_dma_applies(int F, int O, const GemmKnobs& k) { return k.tn_staged == 0 && O > 32 && O % 4 == 0 && F % 4 == 0; }
// k-block width of the DMA TN kernel.  128-wide blocks halve the re-reads of dY (PMC: 862 -> ~600 MB per launch) but measured
// SLOWER (gemm_tn 1.08-1.15 vs 0.92 ms/step, cfg2): the re-reads are served by the Infinity Cache, and the wider tile costs
// occupancy.  So the 8-wave kernel with its 128 columns stays behind a knob.
constexpr int kTnKbw = 64;

inline TnPlan gemm_tn_plan(const TnCall& c) {
    TnPlan p{TnKind::Staged, 0, 0, 2, TnqPlan{}, 0, 0, 0, 0, 256, 0, 0, kGemmOk};
    if (c.offer_quad && (c.knobs.quad & 2) == 0 && c.knobs.tn_staged == 0 && c.R >= quad_min_rows(c.knobs, c.num_cus))
        p.q = tnq_plan(c.nseg, c.F, c.R, c.O, c.batch_major, c.knobs.tnq_target > 0 ? c.knobs.tnq_target / 2 : c.num_cus);
    if (p.q.ok) {                                           // the persistent quad kernel: its own split
        p.kind = TnKind::Quad;
        p.nsplit = p.q.nsplit; p.rps = p.q.rps;
        p.gx = p.q.nkb; p.gy = p.q.nsplit;
        p.lds = gemm_tnq_lds_floats(p.q.KT, p.q.OT) * sizeof(float);
        return p;
    }
    const bool dma = tn_dma_applies(c.F, c.O, c.knobs);
    const bool wide = dma && c.knobs.tn_wide_from > 0 && c.O >= c.knobs.tn_wide_from;
    p.wk = wide ? 4 : 2;
    const int kbw = kTnKbw * p.wk / 2;
    p.gx = dma ? ceil_div(c.nseg * c.F, kbw) : c.nseg * ceil_div(c.F, 64);
    // ~3 workgroups per CU (wide: 2) per 400 k rows: measured, R = 291 840 rows (cfg2/3/4): 768 workgroups best (1152: +12 %,
    // 1536: +1..10 %); R = 583 680 (cfg5): 1536 best (768: +4 %, and +20 % on the h-gate shape with the XCD placement)
    const int target = (wide ? 512 : 768) * ceil_div(c.R, 400000);
    p.nsplit = ceil_div(c.knobs.tn_target > 0 ? c.knobs.tn_target : target, p.gx);
    p.rps = round_up(ceil_div(c.R, p.nsplit), 32);          // (whole 32-row stages: the DMA kernel needs them)
    if (p.rps < 128) p.rps = 128;
    p.nsplit = ceil_div(c.R, p.rps);
    if (p.nsplit >= 8) p.nsplit = round_up(p.nsplit, 8);    // multiple of 8: XCD-aware k-block placement (trailing splits may be empty)
    p.gy = p.nsplit;
    if (dma) {                                              // LDS-DMA staging (default)
        p.kind = wide ? TnKind::DmaWide : TnKind::Dma;
        // row-chunk depth: the 192-column tile stages 16 rows at a time (32 KB of LDS per workgroup -> 4 workgroups per CU
        // instead of 2 with 32-row stages: -3.5 % on that shape); the narrower tiles are better off with 32 rows (measured
        // both ways); 8-row stages are 15 % slower.  (Every caller has refused O > 192 before it plans.)
        p.nctw = c.O > 128 && c.O <= 192 ? 6 : c.O > 64 && c.O <= 128 ? 4 : 2;
        p.rc = p.nctw == 6 ? 16 : 32;
        p.block = 128 * p.wk;
        p.lds = gemm_tn_dma_lds_floats(2, p.nctw, p.rc, p.wk) * sizeof(float);
        // the placement: PMC traffic of the class 831 -> 432 MB per launch (1.93x -> 1.00x algorithmic) at unchanged time
        p.remap = (c.knobs.tn_xcd == 0 && p.nsplit % 8 == 0 && p.gx > 1) ? 1 : 0;
        return p;
    }
    p.nctw = c.O <= 32 ? 1 : c.O <= 64 ? 2 : c.O <= 128 ? 4 : 6;
    p.lds = gemm_tn_lds_floats(p.nctw) * sizeof(float);
    // in this register-staged kernel the placement measured slower in round 1 (1.19 vs 1.04 ms per step): a dev knob only
    p.remap = (c.knobs.tn_xcd == 2 && p.nsplit % 8 == 0 && p.gx > 1) ? 1 : 0;
    if (c.batch_major) p.error = kGemmNeedsRowMap;
    else if (c.O > 192) p.error = kGemmBadO;
    return p;
}

// The two h-part problems of a cell (gate: 2H columns, candidate: H) go out as ONE gemm_tnq_pair_kernel launch whose workgroups
// alternate between the two, where the quad kernel covers both with the same plan (same K, row splits and dY rows; only the
// column count differs) in one of the two instances the pair kernel is compiled for
inline bool tn_pair_applies(const TnPlan& g, const TnPlan& c, const GemmKnobs& k) {
    const TnqPlan &pg = g.q, &pc = c.q;
    if (k.tn_no_pair != 0 || !pg.ok || !pc.ok || pg.OT != 4 || pc.OT != 2 || pg.KT != pc.KT || pg.planar != pc.planar || pg.nkb != pc.nkb ||
        pg.nsplit != pc.nsplit || pg.rps != pc.rps) return false;
    return (pg.planar && pg.KT == 6) || (!pg.planar && pg.KT == 5);
}

}  // namespace eeg
