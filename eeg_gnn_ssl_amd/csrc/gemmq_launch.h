// Launchers of the persistent quad GEMMs (kernels_gemm_q.h); the instantiations live in gemmq_inst.cpp.  Which call they take,
// with what grid and LDS, is the plan's business (gemm_launch.h).
#pragma once
#include "gemm_launch.h"
#include "kernels_gemm.h"

namespace eeg {

// NnKind::Quad: C[R x O] = [segments] @ quad pack + bias (gemm_nnr_kernel).  0 ok, 2 launch error.  bt*: batch-major segments (0 = time-major)
int launch_nnq(const NnPlan& p, const SegPtrs& segs, int nseg, int F, int R, const float* Bq, int nct_total, const float* bias, float* C,
               int ldc, int O, int btT, int btB, int btN, hipStream_t st, const char* tag);
// TnKind::Quad (gemm_tnq_kernel): p.q names the instance
int launch_tnq(const TnPlan& p, const SegPtrs& segs, int nseg, int F, int R, const float* dY, int ldy, int ycol0, int O,
               float* partial, int btT, int btB, int btN, hipStream_t st, const char* tag);
// hg + hc of one cell in one launch (gemm_tnq_pair_kernel) where tn_pair_applies; 1 = the pair has no instance
int launch_tnq_pair(const TnqPlan& pg, const TnqPlan& pc, const SegPtrs& sg, const SegPtrs& sc, int nseg, int F, int R, const float* dY, int ldy,
                    int ycol_g, int Og, float* part_g, int ycol_c, int Oc, float* part_c, hipStream_t st, const char* tag);

}  // namespace eeg
