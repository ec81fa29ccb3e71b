// Instantiations of the persistent quad GEMMs (kernels_gemm_q.h), in their own translation unit; they execute the plans of gemm_launch.h.
#include "kernels_gemm_q.h"
#include "gemmq_launch.h"
#include "prof.h"

namespace eeg {

int launch_nnq(const NnPlan& p, const SegPtrs& segs, int nseg, int F, int R, const float* Bq, int nct_total, const float* bias, float* C,
               int ldc, int O, int btT, int btB, int btN, hipStream_t st, const char* tag) {
    EEG_SET_MAX_LDS((gemm_nnr_kernel<kNnrStages, 2>), p.lds);
    EEG_LAUNCH_P(tag, (gemm_nnr_kernel<kNnrStages, 2>), dim3(p.gx, p.gy), dim3(p.block), p.lds, st, segs, nseg, F, R, Bq, nct_total, bias,
                 C, ldc, O, btT, btB, btN, 0);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

namespace {
template <int KT, int OT, bool BT, bool PLANAR>
int launch_tnq_one(const TnPlan& p, const SegPtrs& segs, int nseg, int F, int R, const float* dY, int ldy, int ycol0, int O,
                   float* partial, int btT, int btB, int btN, hipStream_t st, const char* tag) {
    EEG_SET_MAX_LDS((gemm_tnq_kernel<KT, OT, kTnqRc, BT, PLANAR, false>), p.lds);
    EEG_LAUNCH_P(tag, (gemm_tnq_kernel<KT, OT, kTnqRc, BT, PLANAR, false>), dim3(p.gx, p.gy), dim3(p.block), p.lds, st, segs, nseg, F, R, dY, ldy,
                 ycol0, O, partial, p.rps, btT, btB, btN, 0);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}
template <int KT, bool BT, bool PLANAR>
int launch_tnq_ot(const TnPlan& p, const SegPtrs& segs, int nseg, int F, int R, const float* dY, int ldy, int ycol0, int O,
                  float* partial, int btT, int btB, int btN, hipStream_t st, const char* tag) {
#define EEG_TNQ(OT) launch_tnq_one<KT, OT, BT, PLANAR>(p, segs, nseg, F, R, dY, ldy, ycol0, O, partial, btT, btB, btN, st, tag)
    if constexpr (!BT) {                                   // (batch-major segments: x-part only, 192 columns)
        if (p.q.OT == 2) return EEG_TNQ(2);
        if (p.q.OT == 4) return EEG_TNQ(4);
    }
    return p.q.OT == 6 ? EEG_TNQ(6) : 1;
#undef EEG_TNQ
}
}  // namespace

// hg (OT = 4) and hc (OT = 2) of one cell in one launch; the two plans agree in everything but OT (tn_pair_applies)
int launch_tnq_pair(const TnqPlan& pg, const TnqPlan& pc, const SegPtrs& sg, const SegPtrs& sc, int nseg, int F, int R, const float* dY, int ldy,
                    int ycol_g, int Og, float* part_g, int ycol_c, int Oc, float* part_c, hipStream_t st, const char* tag) {
    constexpr int RC = kTnqRc;
    TnqJob ja{sg, ycol_g, Og, part_g}, jb{sc, ycol_c, Oc, part_c};
#define EEG_PAIR(KT, PL)                                                                                                         \
    {                                                                                                                            \
        const size_t lds = gemm_tnq_lds_floats(KT, 4) * sizeof(float);                                                           \
        EEG_SET_MAX_LDS((gemm_tnq_pair_kernel<KT, RC, PL>), lds);                                                                \
        EEG_LAUNCH_P(tag, (gemm_tnq_pair_kernel<KT, RC, PL>), dim3(pg.nkb, 2 * pg.nsplit), dim3(256), lds, st, ja, jb, nseg, F, R, dY, ldy, \
                     pg.rps, 0);                                                                                                 \
        return hipGetLastError() == hipSuccess ? 0 : 2;                                                                          \
    }
    if (pg.planar && pg.KT == 6) EEG_PAIR(6, true)
    if (!pg.planar && pg.KT == 5) EEG_PAIR(5, false)
#undef EEG_PAIR
    return 1;
}

int launch_tnq(const TnPlan& p, const SegPtrs& segs, int nseg, int F, int R, const float* dY, int ldy, int ycol0, int O,
               float* partial, int btT, int btB, int btN, hipStream_t st, const char* tag) {
#define EEG_TNQ(KT, BT, PL) launch_tnq_ot<KT, BT, PL>(p, segs, nseg, F, R, dY, ldy, ycol0, O, partial, btT, btB, btN, st, tag)
    if (p.kind != TnKind::Quad) return 1;
    if (p.q.planar) {
        if (p.q.KT == 2) return EEG_TNQ(2, false, true);
        if (p.q.KT == 4) return EEG_TNQ(4, false, true);
        return EEG_TNQ(6, false, true);
    }
    const bool bt = btT > 0;
    if (p.q.KT == 4) return bt ? EEG_TNQ(4, true, false) : EEG_TNQ(4, false, false);
    return bt ? EEG_TNQ(5, true, false) : EEG_TNQ(5, false, false);
#undef EEG_TNQ
}

}  // namespace eeg
