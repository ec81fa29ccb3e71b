// Instantiations of the kernels of the spectral form of the hoisted x-part, in their own translation unit, and the launchers that execute
// the plans of spec_launch.h (which kernel, grid, block, LDS: decided there, not here).
#include "kernels_gemm_g.h"
#include "kernels_gemm_f.h"
#include "kernels_spectral.h"
#include "pack_cell.h"
#include "spec_launch.h"
#include "prof.h"

namespace eeg {

// The packs of ALL cells of an encoder in one launch (their weights change with every optimisation step): blockIdx.y = job
// (a cell's fragment packs, kernels_pack.h, or its per-frequency packs above), blockIdx.x strides over the job's elements.
constexpr int kMaxPackJobs = 8;
struct PackJob {
    const float *Wg, *bg, *Wc, *bc, *basis;
    float* out;
    int spectral;          // 0: pack_cell_body (cp), 1: pack_spectral_body (sp)
    CellPack cp;
    SpecPack sp;
};
struct PackJobs { PackJob j[kMaxPackJobs]; };
__global__ void pack_cells_kernel(PackJobs jobs) {
    const PackJob& jb = jobs.j[blockIdx.y];
    if (jb.spectral) pack_spectral_body(jb.Wg, jb.Wc, jb.basis, jb.out, jb.sp, (int)blockIdx.x, (int)gridDim.x);
    else pack_cell_body(jb.Wg, jb.bg, jb.Wc, jb.bc, jb.out, jb.cp, (int)blockIdx.x, (int)gridDim.x);
}


size_t spec_pack_floats(int Fin, int H, int M, int N) { return make_spec_pack(Fin, H, M, N).total; }

int launch_spec_basis(const float* S, int N, float* basis, hipStream_t st) {
    EEG_SET_MAX_LDS(spectral_basis_kernel, kSpecBasisLds);
    EEG_LAUNCH_P("spec_basis", spectral_basis_kernel, dim3(1), dim3(256), kSpecBasisLds, st, S, N, basis);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

int launch_spec_pack(const float* Wg, const float* Wc, const float* basis, int Fin, int H, int M, int N, float* spack, hipStream_t st) {
    const SpecPack p = make_spec_pack(Fin, H, M, N);
    EEG_LAUNCH_P("pack_cell", pack_spectral_kernel, dim3(1024), dim3(256), 0, st, Wg, Wc, basis, spack, p);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

int launch_pack_cells(int n_cells, const float* const* Wg, const float* const* bg, const float* const* Wc, const float* const* bc,
                      const int* Fin, int H, int M, float* const* packs, const float* basis, int N, float* const* spacks, hipStream_t st) {
    PackJobs jobs{};
    int n = 0;
    for (int c = 0; c < n_cells; ++c) {
        if (n + (spacks != nullptr ? 2 : 1) > kMaxPackJobs) return 1;
        PackJob& a = jobs.j[n++];
        a.Wg = Wg[c]; a.bg = bg[c]; a.Wc = Wc[c]; a.bc = bc[c]; a.basis = nullptr; a.out = packs[c]; a.spectral = 0;
        a.cp = make_cell_pack(Fin[c], H, M);
        if (spacks != nullptr) {
            PackJob& b = jobs.j[n++];
            b.Wg = Wg[c]; b.bg = nullptr; b.Wc = Wc[c]; b.bc = nullptr; b.basis = basis; b.out = spacks[c]; b.spectral = 1;
            b.sp = make_spec_pack(Fin[c], H, M, N);
        }
    }
    EEG_LAUNCH_P("pack_cell", pack_cells_kernel, dim3(256, n), dim3(256), 0, st, jobs);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// The launchers below execute a plan of spec_launch.h: the template switch and one launch per kernel signature.
int launch_spec_mix(const SpecMixPlan& p, const float* in, const float* basis, int N, int T, int B, int F, int bm, float* out,
                    hipStream_t st, const char* tag) {
    const float* bias = nullptr;
    const dim3 grid(p.grid), block(p.block);
#define EEG_MIX_MFMA(DIR, KS) EEG_LAUNCH_P(tag, (spec_mix_mfma_kernel<DIR, KS>), grid, block, p.lds, st, in, basis, bias, N, p.S, p.Sp, F, bm, T, B, out)
    if (p.kind == SpecMixKind::Mfma) {
        if (p.ks == 10) { if (p.to_nodes) EEG_MIX_MFMA(0, 10); else EEG_MIX_MFMA(1, 10); }
        else { if (p.to_nodes) EEG_MIX_MFMA(0, 16); else EEG_MIX_MFMA(1, 16); }
    } else if (p.kind == SpecMixKind::Valu19) {
        if (p.to_nodes) EEG_LAUNCH_P(tag, spec_mix_in_kernel<19>, grid, block, p.lds, st, in, basis, p.S, p.Sp, F, bm, T, B, out);
        else EEG_LAUNCH_P(tag, spec_mix_out_kernel<19>, grid, block, p.lds, st, in, basis, bias, p.S, p.Sp, F, bm, T, B, out);
    } else {
        EEG_LAUNCH_P(tag, spec_mix_generic_kernel, grid, block, p.lds, st, in, basis, bias, N, p.S, p.Sp, F, bm, T, B, p.to_nodes, out);
    }
#undef EEG_MIX_MFMA
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

int launch_spec_zero_rows(float* Xh, int N, int S, int Sp, int F, hipStream_t st) {
    if (Sp <= S) return 0;
    EEG_LAUNCH_P("zero", spec_zero_pad_kernel, dim3(ceil_div(N * (Sp - S) * F, 256)), dim3(256), 0, st, Xh, N, S, Sp, F);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

namespace {
template <int KQ, bool SWZ>
void launch_nnf_one(const SpecNnPlan& p, const float* A, size_t ags, int K, int Sp, int G, const float* Wr, size_t wstride, float* C, hipStream_t st,
                    const char* tag, const float* bias, const float* gscale) {
    EEG_SET_MAX_LDS((gemm_nnf_kernel<KQ, SWZ>), p.lds);
    EEG_LAUNCH_P(tag, (gemm_nnf_kernel<KQ, SWZ>), dim3(p.grid), dim3(p.block), p.lds, st, A, (long long)ags, K, Sp, G, Wr, (unsigned)wstride, C, bias, gscale);
}
template <int NJ>
void launch_nng_one(const SpecNnPlan& p, const float* A, size_t ags, int F, int Sp, int G, const float* Wq, size_t wstride, float* C, hipStream_t st,
                    const char* tag, const float* bias, const float* gscale) {
    EEG_SET_MAX_LDS((gemm_nng_kernel<NJ, 2>), p.lds);
    EEG_LAUNCH_P(tag, (gemm_nng_kernel<NJ, 2>), dim3(p.grid), dim3(p.block), p.lds, st, A, (unsigned)ags, F, Sp, G, Wq, (unsigned)wstride, C, 64 * NJ, bias, gscale);
}
}  // namespace
int launch_spec_nn(const SpecNnPlan& p, const float* A, size_t a_gstride, int K, int Sp, int G, const float* W, size_t wstride, float* C,
                   hipStream_t st, const char* tag, const float* bias, const float* gscale) {
    const size_t ags = a_gstride != 0 ? a_gstride : (size_t)Sp * K;
#define EEG_NNF(KQ, SWZ) launch_nnf_one<KQ, SWZ>(p, A, ags, K, Sp, G, W, wstride, C, st, tag, bias, gscale)
    if (p.kind == SpecNnKind::Regs) {
        switch (p.kq) {
            case 8: EEG_NNF(8, true); break;
            case 13: EEG_NNF(13, false); break;
            case 9: EEG_NNF(9, false); break;
            case 5: EEG_NNF(5, false); break;
            case 2: EEG_NNF(2, false); break;
            default: return 1;
        }
    } else if (p.nj == 3) {
        launch_nng_one<3>(p, A, ags, K, Sp, G, W, wstride, C, st, tag, bias, gscale);
    } else if (p.nj == 1) {
        launch_nng_one<1>(p, A, ags, K, Sp, G, W, wstride, C, st, tag, bias, gscale);
    } else {
        return 1;
    }
#undef EEG_NNF
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

namespace {
template <int KT, bool PLANAR>
void launch_tng_one(const SpecTnPlan& p, const float* A, int F, int Sp, int G, const float* dY, float* partial, hipStream_t st, const char* tag,
                    long long skew) {
    constexpr int RC = kSpecTngRc, OT = kSpecTngOt;
    SegPtrs segs;
    for (int m = 0; m < kMaxM; ++m) segs.p[m] = m == 0 ? A : nullptr;
    EEG_SET_MAX_LDS((gemm_tnq_grouped_kernel<KT, OT, RC, PLANAR>), p.lds_x);
    EEG_LAUNCH_P(tag, (gemm_tnq_grouped_kernel<KT, OT, RC, PLANAR>), dim3(p.grid_x, p.grid_y), dim3(p.block), p.lds_x, st, segs, F, Sp, G, p.spg_x, dY,
                 192, 0, 192, partial, p.rps_x, skew);
}
template <int FXT>
void launch_tnf_one(const SpecTnPlan& p, const float* Xh, size_t xgs, int Fin, const float* Hh, size_t hgs, const float* RHh, const float* dY,
                    int Sp, float* part_x, float* part_g, float* part_c, hipStream_t st, const char* tag) {
    EEG_SET_MAX_LDS((gemm_tnf_kernel<FXT>), p.lds_x);
    EEG_LAUNCH_P(tag, (gemm_tnf_kernel<FXT>), dim3(p.grid_x, p.grid_y), dim3(p.block), p.lds_x, st, Xh, (long long)xgs, Fin, Hh, (long long)hgs, RHh, dY,
                 Sp, p.spg_x, p.rps_x, part_x, part_g, part_c);
}
}  // namespace

int launch_tng(const SpecTnPlan& p, const float* A, size_t a_gstride, int F, int Sp, int G, const float* dY, float* partial, hipStream_t st,
               const char* tag) {
    const long long skew = a_gstride != 0 ? (long long)a_gstride - (long long)Sp * F : 0;
    if (p.planar) launch_tng_one<2, true>(p, A, F, Sp, G, dY, partial, st, tag, skew);
    else if (p.KT == 4) launch_tng_one<4, false>(p, A, F, Sp, G, dY, partial, st, tag, skew);
    else launch_tng_one<5, false>(p, A, F, Sp, G, dY, partial, st, tag, skew);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// h-part pair (F = 64): part_g [G*spg][64][128] = Ah^T dY[:, 0:128], part_c [G*spg][64][64] = Arh^T dY[:, 128:192]; one launch
int launch_tng_pair(const SpecTnPlan& p, const float* Ah, size_t ah_gstride, const float* Arh, int Sp, int G, const float* dY, float* part_g,
                    float* part_c, hipStream_t st, const char* tag) {
    const long long skew = ah_gstride != 0 ? (long long)ah_gstride - (long long)Sp * 64 : 0;
    TnqJob ja, jb;
    for (int m = 0; m < kMaxM; ++m) { ja.segs.p[m] = m == 0 ? Ah : nullptr; jb.segs.p[m] = m == 0 ? Arh : nullptr; }
    ja.ycol0 = 0; ja.Ov = 128; ja.partial = part_g;
    jb.ycol0 = 128; jb.Ov = 64; jb.partial = part_c;
    EEG_SET_MAX_LDS((gemm_tnq_grouped_pair_kernel<2, kSpecTngRc, true>), p.lds_h);
    EEG_LAUNCH_P(tag, (gemm_tnq_grouped_pair_kernel<2, kSpecTngRc, true>), dim3(1, p.grid_h), dim3(p.block), p.lds_h, st, ja, jb, 64, Sp, G, p.spg_h, dY,
                 192, p.rps_h, skew, (long long)0);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

int launch_tnf(const SpecTnPlan& p, const float* Xh, size_t x_gstride, int Fin, const float* Hh, size_t h_gstride, const float* RHh,
               const float* dY, int Sp, int G, float* part_x, float* part_g, float* part_c, hipStream_t st, const char* tag) {
    const size_t xgs = x_gstride != 0 ? x_gstride : (size_t)Sp * Fin, hgs = h_gstride != 0 ? h_gstride : (size_t)Sp * 64;
    switch (p.fxt) {
        case 1: launch_tnf_one<1>(p, Xh, xgs, Fin, Hh, hgs, RHh, dY, Sp, part_x, part_g, part_c, st, tag); break;
        case 2: launch_tnf_one<2>(p, Xh, xgs, Fin, Hh, hgs, RHh, dY, Sp, part_x, part_g, part_c, st, tag); break;
        case 3: launch_tnf_one<3>(p, Xh, xgs, Fin, Hh, hgs, RHh, dY, Sp, part_x, part_g, part_c, st, tag); break;
        case 4: launch_tnf_one<4>(p, Xh, xgs, Fin, Hh, hgs, RHh, dY, Sp, part_x, part_g, part_c, st, tag); break;
        default: return 1;
    }
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

int launch_dxf(const SpecDxPlan& p, const float* dYh, int Sp, int S, int N, const float* Wtq, size_t wstride, const float* basis, float* dX,
               hipStream_t st, const char* tag) {
    if (p.nt == 19) {
        EEG_SET_MAX_LDS(gemm_dxf_kernel<19>, p.lds);
        EEG_LAUNCH_P(tag, gemm_dxf_kernel<19>, dim3(p.grid), dim3(p.block), p.lds, st, dYh, Sp, S, N, Wtq, (unsigned)wstride, basis, dX);
    } else {
        EEG_SET_MAX_LDS(gemm_dxf_kernel<0>, p.lds);
        EEG_LAUNCH_P(tag, gemm_dxf_kernel<0>, dim3(p.grid), dim3(p.block), p.lds, st, dYh, Sp, S, N, Wtq, (unsigned)wstride, basis, dX);
    }
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // namespace eeg
