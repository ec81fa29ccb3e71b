// Instantiations of the recurrent kernels for one hidden size (compile with -DEEG_SEQ_H=16|32|64).
#include "kernels_seq.h"
#include "prof.h"
#include "seq_launch.h"

#ifndef EEG_SEQ_H
#error "compile with -DEEG_SEQ_H=<hidden units>"
#endif
#define EEG_CAT2(a, b) a##b
#define EEG_CAT(a, b) EEG_CAT2(a, b)

namespace eeg {
namespace {

// one launch per kernel signature; grid, block and LDS bytes are the plan's
template <int H, int M, int NKS, bool PROBE>
int run_fwd1(const SeqPlan& p, const SeqFwdArgs& a, hipStream_t st) {
    EEG_SET_MAX_LDS((seq_fwd_kernel<H, M, NKS, PROBE>), p.lds);
    EEG_LAUNCH_P("seq_fwd", (seq_fwd_kernel<H, M, NKS, PROBE>), dim3(p.grid), dim3(p.block), p.lds, st, a.XW, a.h0, a.P, a.p_batched, a.bhg, a.bhc,
                 a.Hseq, a.Rs, a.Us, a.Cs, a.RHs, a.Hpl, a.RHpl, a.plane_stride, a.T, a.B, a.N, a.act, a.probe);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
template <int H, int M, int NKS, bool PROBE, bool SPEC>
int run_fwd2(const SeqPlan& p, const SeqFwdArgs& a, hipStream_t st) {
    EEG_SET_MAX_LDS((seq_fwd2_kernel<H, M, NKS, PROBE, SPEC>), p.lds);
    EEG_LAUNCH_P("seq_fwd", (seq_fwd2_kernel<H, M, NKS, PROBE, SPEC>), dim3(p.grid), dim3(p.block), p.lds, st, a.XW, a.h0, a.P, a.p_batched, a.bhg,
                 a.bhc, a.Hseq, a.Rs, a.Us, a.Cs, a.RHs, a.Hpl, a.RHpl, a.plane_stride, a.T, a.B, a.N, a.act, a.probe, a.spec_U, a.spec_Sp, a.spec_SpE);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
template <int H, int M, int NKS, bool PROBE>
int run_bwd1(const SeqPlan& p, const SeqBwdArgs& a, hipStream_t st) {
    EEG_SET_MAX_LDS((seq_bwd_kernel<H, M, NKS, PROBE>), p.lds);
    EEG_LAUNCH_P("seq_bwd", (seq_bwd_kernel<H, M, NKS, PROBE>), dim3(p.grid), dim3(p.block), p.lds, st, a.Hseq, a.h0, a.Rs, a.Us, a.Cs, a.dHseq,
                 a.d_at_end, a.d_at_len, a.lengths, a.P, a.p_batched, a.b1, a.b2, a.dXW, a.dh0, a.dbias_part, a.T, a.B, a.N, a.act, a.probe);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
template <int H, int M, int NKS, bool PROBE, bool SPEC>
int run_bwd2(const SeqPlan& p, const SeqBwdArgs& a, hipStream_t st) {
    EEG_SET_MAX_LDS((seq_bwd2_kernel<H, M, NKS, PROBE, SPEC>), p.lds);
    EEG_LAUNCH_P("seq_bwd", (seq_bwd2_kernel<H, M, NKS, PROBE, SPEC>), dim3(p.grid), dim3(p.block), p.lds, st, a.Hseq, a.h0, a.Rs, a.Us, a.Cs, a.dHseq,
                 a.d_at_end, a.d_at_len, a.lengths, a.P, a.p_batched, a.b1, a.b2, a.dXW, a.dh0, a.dbias_part, a.T, a.B, a.N, a.act, a.probe,
                 a.spec_U, a.dYh, a.spec_Sp);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// the plan's kind and probe flag name an instantiation that exists (seq_launch.h asks the same predicates)
template <int H, int M, int NKS>
int fwd_nks(const SeqPlan& p, const SeqFwdArgs& a, hipStream_t st) {
    if constexpr (seq_has_probe(H, M, NKS)) {
        if (p.probe && p.kind == SeqKind::OneWave) return run_fwd1<H, M, NKS, true>(p, a, st);
        if (p.probe && p.kind == SeqKind::TwoWave) return run_fwd2<H, M, NKS, true, false>(p, a, st);
        if (p.probe) return run_fwd2<H, M, NKS, true, true>(p, a, st);
    }
    if constexpr (seq_has_spec(H, M, NKS)) {
        if (p.kind == SeqKind::TwoWaveSpec) return run_fwd2<H, M, NKS, false, true>(p, a, st);
    }
    if constexpr (seq_has_two_wave(H, M, NKS)) {
        if (p.kind == SeqKind::TwoWave) return run_fwd2<H, M, NKS, false, false>(p, a, st);
    }
    return run_fwd1<H, M, NKS, false>(p, a, st);
}
template <int H, int M>
int fwd_one(const SeqPlan& p, const SeqFwdArgs& a, hipStream_t st) {
    return p.nks == 5 ? fwd_nks<H, M, 5>(p, a, st) : fwd_nks<H, M, 8>(p, a, st);
}
template <int H, int M, int NKS>
int bwd_nks(const SeqPlan& p, const SeqBwdArgs& a, hipStream_t st) {
    if constexpr (seq_has_probe(H, M, NKS)) {
        if (p.probe && p.kind == SeqKind::OneWave) return run_bwd1<H, M, NKS, true>(p, a, st);
        if (p.probe && p.kind == SeqKind::TwoWave) return run_bwd2<H, M, NKS, true, false>(p, a, st);
        if (p.probe) return run_bwd2<H, M, NKS, true, true>(p, a, st);
    }
    if constexpr (seq_has_spec(H, M, NKS)) {
        if (p.kind == SeqKind::TwoWaveSpec) return run_bwd2<H, M, NKS, false, true>(p, a, st);
    }
    if constexpr (seq_has_two_wave(H, M, NKS)) {
        if (p.kind == SeqKind::TwoWave) return run_bwd2<H, M, NKS, false, false>(p, a, st);
    }
    return run_bwd1<H, M, NKS, false>(p, a, st);
}
template <int H, int M>
int bwd_one(const SeqPlan& p, const SeqBwdArgs& a, hipStream_t st) {
    return p.nks == 5 ? bwd_nks<H, M, 5>(p, a, st) : bwd_nks<H, M, 8>(p, a, st);
}

}  // namespace

int EEG_CAT(launch_seq_fwd_h, EEG_SEQ_H)(int M, const SeqPlan& p, const SeqFwdArgs& a, hipStream_t st) {
    switch (M) {
        case 1: return fwd_one<EEG_SEQ_H, 1>(p, a, st);
        case 2: return fwd_one<EEG_SEQ_H, 2>(p, a, st);
        case 3: return fwd_one<EEG_SEQ_H, 3>(p, a, st);
        case 4: return fwd_one<EEG_SEQ_H, 4>(p, a, st);
        case 5: return fwd_one<EEG_SEQ_H, 5>(p, a, st);
        case 7: return fwd_one<EEG_SEQ_H, 7>(p, a, st);
        default: return 1;
    }
}
int EEG_CAT(launch_seq_bwd_h, EEG_SEQ_H)(int M, const SeqPlan& p, const SeqBwdArgs& a, hipStream_t st) {
    switch (M) {
        case 1: return bwd_one<EEG_SEQ_H, 1>(p, a, st);
        case 2: return bwd_one<EEG_SEQ_H, 2>(p, a, st);
        case 3: return bwd_one<EEG_SEQ_H, 3>(p, a, st);
        case 4: return bwd_one<EEG_SEQ_H, 4>(p, a, st);
        case 5: return bwd_one<EEG_SEQ_H, 5>(p, a, st);
        case 7: return bwd_one<EEG_SEQ_H, 7>(p, a, st);
        default: return 1;
    }
}

}  // namespace eeg
