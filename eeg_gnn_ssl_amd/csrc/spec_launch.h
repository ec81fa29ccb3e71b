// Launch plans of the spectral form of the hoisted x-part (spec_common.h): which kernel takes a node mix, the x-part NN GEMM, the
// weight gradients of a cell and the input gradient of a layer, with what template integers, grid, block, LDS bytes and row split.
// Pure functions of the call (no global is read: CU count and dev knobs come in through it); every selection rule of the family
// is stated here and nowhere else, next to the LDS sizes and occupancy targets the rules size their launches by (the kernel
// headers kernels_spectral.h, kernels_gemm_g.h, kernels_gemm_f.h include this header and use the same functions).  The callers in
// api.cpp ask for a plan BEFORE they size workspaces and lay out operands; the launchers of spec_inst.cpp, declared at the end,
// execute it: a plan that carries an error never reaches them.  No kernel bodies: this header compiles as plain host C++
// (tests/emu/gemm_plan_driver.cpp prints the plans, tests/golden/spec_plans_v1.json pins them).
#pragma once
#include "common.h"
#include "nnq_order.h"
#include "spec_common.h"

namespace eeg {

// dev knobs (include/eeg_dcrnn_dev.h; compile-time zeros in the product build)
struct SpecKnobs {
    int nn_grouped = 0;     // EEG_TUNE_SPEC_NN_GROUPED = 1: the x-part NN on gemm_nng_kernel (no register-resident weights)
    int tn_separate = 0;    // EEG_TUNE_SPEC_TN_SEPARATE = 1: the weight gradients as the grouped launches (no fused kernel)
    int dx_passes = 0;      // EEG_TUNE_SPEC_DX_PASSES = 1: the input gradient as grouped GEMM + node mix (no fused kernel)
};
enum SpecPlanError { kSpecOk = 0, kSpecBadNct, kSpecNotCovered };   // no gemm_nng instance for this column count / shape outside the family

// the kernels reach these many floats through ONE 2-GB buffer descriptor (platform.h make_wbuf) or with 32-bit indices
inline bool spec_desc_reaches(double floats) { return floats * sizeof(float) < 2147483648.0; }

// Shapes the spectral path covers: 64 units (192-column pre-activations), Fin % 4 == 0, <= 32 nodes, every operand (N, Sp, Fin | 3H)
// within a descriptor; with need_dx additionally Fin == 64 (the input gradient of a layer above the first).
inline bool spec_supported(int T, int B, int N, int H, int Fin, int M, int need_dx) {
    if (T < 1 || B < 1 || N < 2 || N > kMaxNodes || H != 64 || Fin < 4 || Fin % 4 != 0 || M < 2 || M > kMaxM) return false;
    if (need_dx && Fin != 64) return false;
    if (Fin / 4 > 256 || make_nnq_order(1, Fin).ntail > 1) return false;
    return spec_desc_reaches((double)N * spec_rows(T * B) * (Fin > 192 ? Fin : 192));
}

// ---- LDS bytes and occupancy targets of the kernels, by their template integers --------------------------------------------------
constexpr size_t kSpecBasisLds = (2 * 32 * 32 + 32 + 256) * sizeof(double) + 32 * sizeof(int);                 // spectral_basis_kernel
__host__ __device__ constexpr size_t spec_mix_generic_lds_bytes(int N) { return (size_t)N * N * sizeof(float); }   // spec_mix_generic_kernel: U
// gemm_nng_kernel<NJ, MINW>: a ring of kNngStages stages, each 128 rows x 16 floats of activations + 4 NJ column tiles of weights
constexpr int kNngStages = 4;
__host__ __device__ constexpr size_t nng_lds_bytes(int NJ) { return (size_t)kNngStages * (128 * 16 + 4 * NJ * 256) * sizeof(float); }
// gemm_tnq_grouped_kernel<KT, OT, 16, PLANAR> / gemm_tnq_grouped_pair_kernel<KT, 16, PLANAR> (OT = 4): three stages of 16-row chunks
constexpr int kSpecTngRc = 16, kSpecTngOt = 6, kSpecTngPairOt = 4;
__host__ __device__ constexpr size_t spec_tng_lds_bytes(int KT, int OT) { return 3 * (size_t)(kSpecTngRc * 32 * (KT + OT)) * sizeof(float); }
// gemm_nnf_kernel<KQ, SWZ>: a ring of kNnfNS chunks of 64 rows (+ one zeroed 16-byte unit behind the last row)
#ifndef EEG_X_NNF_NS
#define EEG_X_NNF_NS 3
#endif
constexpr int kNnfNS = EEG_X_NNF_NS;
__host__ __device__ constexpr int nnf_stage_floats(int K) { return 64 * K + 4; }
__host__ __device__ constexpr size_t nnf_lds_bytes(int K) { return (size_t)kNnfNS * nnf_stage_floats(K) * sizeof(float); }
// gemm_tnf_kernel<FXT>: ring of tnf_ns() stages of kTnfRC rows, tnf_wgs_per_cu() workgroups per CU (__launch_bounds__ and the row split)
#ifndef EEG_X_TNF_RC
#define EEG_X_TNF_RC 8
#endif
#ifndef EEG_X_TNF_NS
#define EEG_X_TNF_NS 5
#endif
#ifndef EEG_X_TNF_MINW
#define EEG_X_TNF_MINW 2
#endif
// narrow inputs (FXT <= 2: 96 accumulator registers) run three workgroups per CU on a three-stage ring (measured: -3 % against 2 x 5)
#ifndef EEG_X_TNF_NS2
#define EEG_X_TNF_NS2 3
#endif
#ifndef EEG_X_TNF_MINW2
#define EEG_X_TNF_MINW2 3
#endif
constexpr int kTnfRC = EEG_X_TNF_RC;
__host__ __device__ constexpr int tnf_ns(int FXT) { return FXT <= 2 ? EEG_X_TNF_NS2 : EEG_X_TNF_NS; }
__host__ __device__ constexpr int tnf_wgs_per_cu(int FXT) { return FXT <= 2 ? EEG_X_TNF_MINW2 : EEG_X_TNF_MINW; }
// floats of one stage: Xh image (FXT pieces of 256 floats) | Hh (8 x 64) | RHh (8 x 64) | dYh (8 x 192)
__host__ __device__ constexpr int tnf_stage_floats(int FXT) { return (kTnfRC / 8) * (FXT * 256 + 512 + 512 + 1536); }
__host__ __device__ constexpr size_t tnf_lds_bytes(int FXT) { return (size_t)tnf_ns(FXT) * tnf_stage_floats(FXT) * sizeof(float); }
// gemm_dxf_kernel<NT>: kDxfRows samples per workgroup, ring of kDxfNS [rows x 192] images, N <= kDxfMaxN (accumulators: 8 N registers)
constexpr int kDxfMaxN = 20, kDxfNS = 3, kDxfRows = 32, kDxfStage = kDxfRows * 192;
__host__ __device__ constexpr size_t dxf_lds_bytes() { return (size_t)kDxfNS * kDxfStage * sizeof(float); }

// ---- node mixes -----------------------------------------------------------------------------------------------------------------
// to_nodes = 1: X (S, N, F) -> Xh (N, Sp, F) with U^T (pad rows zeroed); 0: Yh (N, Sp, F) -> Y (S, N, F) with U.  S = T * B
// time-major rows; node_rows: rows per frequency of the node-major side (its group stride; 0 = S rounded up to 16).
enum class SpecMixKind { Mfma, Valu19, Generic };   // spec_mix_mfma_kernel<DIR, KS>, spec_mix_in_kernel<19> / spec_mix_out_kernel<19>, spec_mix_generic_kernel
struct SpecMixPlan {
    SpecMixKind kind;
    int to_nodes, ks;       // Mfma: DIR = 1 - to_nodes, KS = 10 (N <= 20) or 16 k-steps of two nodes
    int S, Sp;              // rows of the sample-major side, rows per frequency of the node-major side
    int grid, block;
    size_t lds;             // bytes of dynamic LDS
};
inline SpecMixPlan spec_mix_plan(int to_nodes, int N, int T, int B, int F, int node_rows = 0) {
    SpecMixPlan p{SpecMixKind::Generic, to_nodes, 0, T * B, node_rows > 0 ? node_rows : spec_rows(T * B), 1, 256, 0};
    const int rows = to_nodes ? p.Sp : p.S, F4 = F / 4;
#ifndef EEG_X_MIX_VALU
    // the mixes on the matrix pipe where a row is whole 128-byte tiles (measured at cfg2: F = 64 from nodes 0.046 -> 0.037 ms; F = 100
    // to nodes 0.045 -> 0.070: a fourth tile with 4 of 32 columns and rows that straddle lines -- that one keeps the VALU form)
    if (N <= 32 && F % 32 == 0 && spec_desc_reaches((double)rows * F)) {
        p.kind = SpecMixKind::Mfma;
        p.ks = N <= 20 ? 10 : 16;
        p.grid = ceil_div(rows * (F / 32), 4);
        if (p.grid > 2048) p.grid = 2048;
        return p;
    }
#endif
    if (N == 19 && F4 <= 128) {                             // the EEG montage: one thread = one 16-byte column of one sample
        p.kind = SpecMixKind::Valu19;
        while (p.block > 64 && (p.block / 2) >= F4 && (p.block / 2) / F4 >= p.Sp) p.block /= 2;
        p.grid = ceil_div(rows, p.block / F4);
        if (p.grid > 1024) p.grid = 1024;                   // ~4 workgroups per CU, each walking consecutive passes (cf. diffuse_fwd)
        return p;
    }
    const size_t total = ((size_t)rows * N * F4 + 255) / 256;
    p.grid = (int)(total > 2048 ? 2048 : total);
    p.lds = spec_mix_generic_lds_bytes(N);
    return p;
}

// ---- grouped NN: C (G, Sp, 16 nct) = A (G, Sp, K) * W_i + gscale[i] * bias ------------------------------------------------------
// Regs: gemm_nnf_kernel<KQ, SWZ> (kernels_gemm_f.h: weights of a frequency in registers, SpecPack::sxr; 192 columns only);
// Grouped: gemm_nng_kernel<NJ, 2> (kernels_gemm_g.h: quad-ordered weights, SpecPack::sxq / sxtq; nct = 4 NJ)
enum class SpecNnKind { Regs, Grouped };
struct SpecNnPlan {
    SpecNnKind kind;
    int kq, swz, nj;        // Regs: KQ = ceil(K / 8), SWZ; Grouped: NJ
    int grid, block;
    size_t lds;             // bytes of dynamic LDS
    int error;
};
// KQ of the gemm_nnf_kernel instance for rows of K floats, 0 = none: K = 64 (16 sixteen-byte units, XOR-swizzled), else an ODD
// number of units per row (the plain row-major image is conflict-free) at the compiled depths
constexpr int nnf_kq(int K) {
    if (K < 4 || K % 4 != 0) return 0;
    if (K == 64) return 8;
    const int kq = ceil_div(K, 8);
    return ((K / 4) & 1) != 0 && (kq == 13 || kq == 9 || kq == 5 || kq == 2) ? kq : 0;
}
inline SpecNnPlan spec_nn_plan(int K, int Sp, int G, int nct, int num_cus, const SpecKnobs& k) {
    SpecNnPlan p{SpecNnKind::Grouped, 0, 0, nct / 4, 1, 256, 0, kSpecOk};
    const int cus = num_cus > 0 ? num_cus : 256;
    if (nct == 12 && k.nn_grouped == 0 && nnf_kq(K) > 0 && Sp >= 16 && G >= 1 && spec_desc_reaches((double)Sp * 192)) {
        p.kind = SpecNnKind::Regs;
        p.kq = nnf_kq(K); p.swz = K == 64;
        p.grid = G * ceil_div(Sp, 64) < 2 * cus ? G * ceil_div(Sp, 64) : 2 * cus;      // persistent: 2 per CU over the 64-row chunks
        p.lds = nnf_lds_bytes(K);
        return p;
    }
    // the knob, or no instantiation for this width: 3 column tiles per wave (the pre-activations) or 1 (dX of a layer above the first)
    if (nct != 12 && nct != 4) { p.error = kSpecBadNct; return p; }
    p.grid = ceil_div((Sp / 16) * G, 8) < 2 * cus ? ceil_div((Sp / 16) * G, 8) : 2 * cus;
    if (p.grid < 1) p.grid = 1;
    p.lds = nng_lds_bytes(p.nj);
    return p;
}

// ---- weight gradients of a cell: Xh^T dYh (Fin x 192), Hh^T dYh[:, 0:128], RHh^T dYh[:, 128:192], split-K partials -----------------
// fused: gemm_tnf_kernel<fxt> (kernels_gemm_f.h), the three problems in one pass over dYh with one row split; else
// gemm_tnq_grouped_kernel<KT, 6, 16, planar> for the x-part (grid nkb x G spg_x) and gemm_tnq_grouped_pair_kernel<2, 16, true> for the
// h-part pair (grid 1 x 2 G spg_h), each with its own split: the x-part's k-blocks count against the same 2-per-CU target.
// Partials: part_x [G * spg_x][Fin][192], part_g [G * spg_h][64][128], part_c [G * spg_h][64][64] (px / pg / pc floats); the fold
// (spec_common.h SpecFoldJob) takes spg_x / spg_h from here.
struct SpecTnPlan {
    int fused, fxt;
    int KT, planar, nkb;                    // the x-part's grouped instance
    int spg_x, rps_x, spg_h, rps_h;         // row splits per frequency and rows per split (multiples of 16); fused: the same pair twice
    int grid_x, grid_y, grid_h, block;      // fused / x-part: grid_x x grid_y; pair: 1 x grid_h
    size_t lds_x, lds_h;                    // bytes of dynamic LDS
    size_t px, pg, pc;
    int error;
};
// rows per split a multiple of 16 and at least 64, as many splits as the target allows
inline void spec_row_split(int Sp, int want, int& spg, int& rps) {
    rps = round_up(ceil_div(Sp, want < 1 ? 1 : want), 16);
    if (rps < 64) rps = 64;
    if (rps > Sp) rps = Sp;
    spg = ceil_div(Sp, rps);
}
inline SpecTnPlan spec_tn_plan(int Fin, int H, int Sp, int G, int num_cus, const SpecKnobs& k) {
    SpecTnPlan p{};
    p.block = 256;
    if (H != 64 || Fin < 4 || Fin % 4 != 0 || Sp < 16 || Sp % 16 != 0 || G < 1) { p.error = kSpecNotCovered; return p; }
    const int cus = num_cus > 0 ? num_cus : 256;
    // the fused kernel holds up to four 32-column tiles of Xh; a frequency's rows go through descriptors
    if (k.tn_separate == 0 && Fin <= 128 && spec_desc_reaches((double)Sp * 192)) {
        p.fused = 1;
        p.fxt = ceil_div(Fin, 32);
#ifdef EEG_X_TNF_TARGET1
        const int target = cus;
#else
        const int target = tnf_wgs_per_cu(p.fxt) * cus;     // every workgroup of the launch resident at once
#endif
        spec_row_split(Sp, target / G, p.spg_x, p.rps_x);
        p.spg_h = p.spg_x; p.rps_h = p.rps_x;
        p.grid_x = G * p.spg_x; p.grid_y = 1;
        p.lds_x = tnf_lds_bytes(p.fxt);
    } else {
        if (Fin == 64) {
            p.planar = 1; p.KT = 2; p.nkb = 1;
        } else {                                            // per-lane source pointers, k-blocks of 4 or 5 tiles per wave slice: least padded K
            int bcost = 1 << 30;
            for (int kt = 5; kt >= 4; --kt) {
                const int nkb = ceil_div(Fin, 32 * kt), cost = nkb * 32 * kt;
                if (cost < bcost) { p.KT = kt; bcost = cost; p.nkb = nkb; }
            }
        }
        spec_row_split(Sp, 2 * cus / (G * p.nkb), p.spg_x, p.rps_x);
        spec_row_split(Sp, 2 * cus / G, p.spg_h, p.rps_h);
        p.grid_x = p.nkb; p.grid_y = G * p.spg_x; p.grid_h = 2 * G * p.spg_h;
        p.lds_x = spec_tng_lds_bytes(p.KT, kSpecTngOt);
        p.lds_h = spec_tng_lds_bytes(2, kSpecTngPairOt);
    }
    p.px = (size_t)G * p.spg_x * Fin * 3 * H;
    p.pg = (size_t)G * p.spg_h * H * 2 * H;
    p.pc = (size_t)G * p.spg_h * H * H;
    return p;
}

// ---- input gradient of a layer: dX (S, N, Fin) = U [dYh_i Wt_i^T]_i ------------------------------------------------------------
// Fused: gemm_dxf_kernel<19> (the EEG montage: no branches in the fold) or <0> (N at run time), Fin = 64 and N <= kDxfMaxN; else two
// passes: the grouped NN over K = 192 into dXh (N, Sp, Fin) -- the only plan that needs that region (needs_dxh) -- and the node mix
// back.  (bwd_ws of api.cpp reserves the region whenever dX is asked for: eeg_dcrnn_layer_bwd_ws_floats is part of the ABI.  With
// needs_dxh = false it could be dropped.)
enum class SpecDxKind { Fused, TwoPass };
struct SpecDxPlan {
    SpecDxKind kind;
    int nt;                 // Fused: NT = 19 or 0
    int grid, block;
    size_t lds;             // bytes of dynamic LDS
    bool needs_dxh;
    SpecNnPlan nn;          // TwoPass
    SpecMixPlan mix;
    int error;
};
inline SpecDxPlan spec_dx_plan(int Fin, int N, int T, int B, int num_cus, const SpecKnobs& k) {
    SpecDxPlan p{};
    const int S = T * B, Sp = spec_rows(S);
    if (k.dx_passes == 0 && Fin == 64 && N >= 1 && N <= kDxfMaxN && S >= 1 && spec_desc_reaches((double)Sp * 192) &&
        spec_desc_reaches((double)S * N * 64)) {
        p.kind = SpecDxKind::Fused;
        p.nt = N == 19 ? 19 : 0;
        p.grid = ceil_div(Sp, kDxfRows); p.block = 256;
        p.lds = dxf_lds_bytes();
        return p;
    }
    p.kind = SpecDxKind::TwoPass;
    p.needs_dxh = true;
    SpecKnobs grouped = k;
    grouped.nn_grouped = 1;                                 // (the transposed packs exist in the quad order only: SpecPack::sxtq)
    p.nn = spec_nn_plan(192, Sp, N, round_up(Fin, 16) / 16, num_cus, grouped);
    p.mix = spec_mix_plan(0, N, T, B, Fin);
    p.error = p.nn.error;
    return p;
}

// ---- the launchers of spec_inst.cpp: the template switch and one launch per kernel signature; 0 = ok ----------------------------------
size_t spec_pack_floats(int Fin, int H, int M, int N);
int launch_spec_basis(const float* S, int N, float* basis, hipStream_t st);
int launch_spec_pack(const float* Wg, const float* Wc, const float* basis, int Fin, int H, int M, int N, float* spack, hipStream_t st);
// the fragment packs (and, with a basis, the per-frequency packs) of n_cells cells in ONE launch; spacks / basis nullable together
int launch_pack_cells(int n_cells, const float* const* Wg, const float* const* bg, const float* const* Wc, const float* const* bc,
                      const int* Fin, int H, int M, float* const* packs, const float* basis, int N, float* const* spacks, hipStream_t st);
// bm = 1: the sample-major side is the batch-major (B, T, N, F) model input
int launch_spec_mix(const SpecMixPlan& p, const float* in, const float* basis, int N, int T, int B, int F, int bm, float* out,
                    hipStream_t st, const char* tag);
// rows [S, Sp) of every group of a (N, Sp, F) node-major tensor <- 0, Sp any row count >= S (no launch when Sp == S)
int launch_spec_zero_rows(float* Xh, int N, int S, int Sp, int F, hipStream_t st);
inline int launch_spec_zero_pad(float* Xh, int N, int S, int F, hipStream_t st) { return launch_spec_zero_rows(Xh, N, S, spec_rows(S), F, st); }
// W: block 0 of the packs the plan's kind reads, wstride floats apart; a_gstride: floats between two groups of A (0 = Sp * K);
// bias (16 nct floats, nullable) + gscale (G floats): the tiles of group g start from gscale[g] * bias
int launch_spec_nn(const SpecNnPlan& p, const float* A, size_t a_gstride, int K, int Sp, int G, const float* W, size_t wstride, float* C,
                   hipStream_t st, const char* tag, const float* bias = nullptr, const float* gscale = nullptr);
// x_gstride / h_gstride: floats between two groups of Xh / Hh (0 = contiguous; RHh is contiguous)
int launch_tnf(const SpecTnPlan& p, const float* Xh, size_t x_gstride, int Fin, const float* Hh, size_t h_gstride, const float* RHh,
               const float* dY, int Sp, int G, float* part_x, float* part_g, float* part_c, hipStream_t st, const char* tag);
int launch_tng(const SpecTnPlan& p, const float* A, size_t a_gstride, int F, int Sp, int G, const float* dY, float* partial, hipStream_t st,
               const char* tag);
int launch_tng_pair(const SpecTnPlan& p, const float* Ah, size_t ah_gstride, const float* Arh, int Sp, int G, const float* dY, float* part_g,
                    float* part_c, hipStream_t st, const char* tag);
// Wtq = SpecPack::sxtq block 0
int launch_dxf(const SpecDxPlan& p, const float* dYh, int Sp, int S, int N, const float* Wtq, size_t wstride, const float* basis, float* dX,
               hipStream_t st, const char* tag);

}  // namespace eeg
