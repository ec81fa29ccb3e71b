// C ABI of libeeg_dcrnn_hip.so (see include/eeg_dcrnn.h): argument checking + kernel orchestration.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include <string>
#include <vector>

#include "../../include/eeg_dcrnn.h"
#include "../../include/eeg_dcrnn_dev.h"
#include "../../include/eeg_dcrnn_prof.h"
#include "kernels_decoder.h"
#include "diffuse_launch.h"
#include "kernels_diffuse.h"
#include "kernels_eval.h"
#include "kernels_boot.h"
#include "kernels_moments.h"
#include "kernels_scan.h"
#include "kernels_resample.h"
#include "kernels_edf.h"
#include "kernels_occlude.h"
#include "kernels_data.h"
#include "kernels_records.h"
#include "kernels_feat.h"
#include "kernels_gemm.h"
#include "kernels_gemm_bf.h"
#include "corr_launch.h"
#include "kernels_graph.h"
#include "kernels_head.h"
#include "kernels_pack.h"
#include "spec_common.h"
#include "spec_launch.h"
#include "kernels_tail.h"
#include "kernels_weights.h"
#include "prof.h"
#include "seq_launch.h"
#include "gemmq_launch.h"

#include <string>
#include <vector>


namespace {

thread_local char g_err[512] = "";
// Development aids exist only in the dev build (make dev / the test emulator: -DEEG_DEV, declared in
// include/eeg_dcrnn_dev.h).  In the product build the knobs are compile-time zeros and there is no probe.
#if defined(EEG_DEV)
long long* g_seq_probe = nullptr;  // see eeg_dcrnn_set_seq_probe
int g_tune[EEG_TUNE_COUNT] = {0};               // see eeg_dcrnn_set_tuning
#else
constexpr int g_tune[EEG_TUNE_COUNT] = {0};
#endif

std::atomic<long long*> g_clock_samples{nullptr};   // eeg_dcrnn_prof_clock_samples (measurement hook, like the event recorder)
// the `probe` argument of the recurrent launches: the dev build's phase probe (which selects the probe instantiations), else the
// product's clock-sample buffer (4 x int64; dev builds leave it alone: a non-null probe means 32 slots per wave there).
// A launch that is being CAPTURED into a graph never gets the clock-sample buffer: the graph would keep the pointer and go on
// adding to it on every replay, after the buffer was disarmed and freed.
long long* seq_probe_arg(hipStream_t st) {
#if defined(EEG_DEV)
    (void)st;
    return g_seq_probe;
#else
    long long* p = g_clock_samples.load(std::memory_order_acquire);
    if (p != nullptr && eeg::platform_stream_is_capturing(st)) return nullptr;
    return p;
#endif
}

// a launch with this `probe` argument carries the dev build's armed phase probe (the product's clock-sample buffer is no such probe)
bool carries_phase_probe(const long long* probe) { return eeg::kDevBuild && probe != nullptr; }

int fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return 1;
}
int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("%s: launch failed: %s", what, hipGetErrorString(e));
    return 0;
}
inline hipStream_t S_(void* s) { return reinterpret_cast<hipStream_t>(s); }

using namespace eeg;

int check_dims(int N, int H, int Fin, int M) {
    if (N < 1 || N > kMaxNodes) return fail("num_nodes=%d unsupported (1..%d)", N, kMaxNodes);
    if (!seq_h_supported(H)) return fail("rnn_units=%d unsupported (16, 32 or 64)", H);
    if (Fin < 4 || Fin % 4 != 0) return fail("per-node input dim=%d unsupported (must be a positive multiple of 4)", Fin);
    if (!seq_m_supported(M)) return fail("num hop matrices M=%d unsupported (1,2,3,4,5,7)", M);
    // LDS of the one-wave BPTT kernel: the widest case (H=64, M=7) only fits montages of <= 20 nodes
    const size_t bwd = seq_bwd_lds_floats(H, M, seq_bwd_rows(H, M, seq_nks(N))) * sizeof(float);
    if (bwd > kMaxLdsBytes)
        return fail("rnn_units=%d with %d hop matrices and %d nodes needs %zu KB of LDS for the backward pass (160 available)",
                    H, M, N, bwd / 1024);
    return 0;
}

// CUs of the current device (the persistent GEMMs size their grids by it); queried once per process
int num_cus() { return platform_num_cus(); }

// ---- hoisted GEMMs -----------------------------------------------------------------------------
// The caller makes a plan (gemm_launch.h) from one of these calls, sizes its buffers and picks its operands by the plan, and the
// plan is executed here: the template switch and one launch per kernel signature.  The knobs are compile-time zeros in the
// product build.
GemmKnobs gemm_knobs() {
    return GemmKnobs{g_tune[EEG_TUNE_NN_STAGED], g_tune[EEG_TUNE_TN_STAGED], g_tune[EEG_TUNE_QUAD], g_tune[EEG_TUNE_TN_XCD],
                     g_tune[EEG_TUNE_TN_WIDE_FROM], g_tune[EEG_TUNE_TN_TARGET], g_tune[EEG_TUNE_TNQ_TARGET], g_tune[EEG_TUNE_TN_NO_PAIR]};
}
// the A segments of a GEMM are batch-major (B clips x T steps x N nodes): the kernels with a row map read them through it
struct BtMap { int T = 0, B = 0, N = 0; };
NnCall nn_call(int nseg, int F, int R, int nct_total, int ldc, int O, BtMap bt = BtMap(), bool quad_pack = false, int bf3_nct = 0) {
    return NnCall{nseg, F, R, nct_total, ldc, O, bt.T > 0, quad_pack, bf3_nct, num_cus(), gemm_knobs()};
}
TnCall tn_call(int nseg, int F, int R, int O, bool batch_major = false, bool offer_quad = false) {
    return TnCall{nseg, F, R, O, batch_major, offer_quad, num_cus(), gemm_knobs()};
}

// the right-hand side of an NN GEMM in the forms the caller holds: the fp32 pack, its quad order (kernels_pack.h: bxq / bxtq;
// NnCall::quad_pack) and the bf16 term pack (NnCall::bf3_nct)
struct NnRhs { const float* Bp; const float* Bq = nullptr; const unsigned short* W3 = nullptr; };
template <int NCTW, int KC>
int run_nn(const NnPlan& p, const NnCall& c, const SegPtrs& segs, const NnRhs& B, const float* bias, float* C, hipStream_t st, const char* tag) {
    EEG_SET_MAX_LDS((gemm_nn_kernel<NCTW, KC>), p.lds);
    EEG_LAUNCH_P(tag, (gemm_nn_kernel<NCTW, KC>), dim3(p.gx, p.gy), dim3(p.block), p.lds, st, segs, c.nseg, c.F, c.R, B.Bp, c.nct_total, bias, C, c.ldc, c.O);
    return check_launch("gemm_nn");
}
template <int NCTW, int KC, int MINB = 2>
int run_nn_dma(const NnPlan& p, const NnCall& c, const SegPtrs& segs, const NnRhs& B, const float* bias, float* C, hipStream_t st, const char* tag, BtMap bt) {
    EEG_SET_MAX_LDS((gemm_nn_dma_kernel<NCTW, KC, MINB>), p.lds);
    EEG_LAUNCH_P(tag, (gemm_nn_dma_kernel<NCTW, KC, MINB>), dim3(p.gx, p.gy), dim3(p.block), p.lds, st, segs, c.nseg, c.F, c.R, B.Bp, c.nct_total, bias, C, c.ldc, c.O, bt.T, bt.B, bt.N);
    return check_launch("gemm_nn_dma");
}
template <int NCTW>
int run_nn_chunk(const NnPlan& p, const NnCall& c, const SegPtrs& segs, const NnRhs& B, const float* bias, float* C, hipStream_t st, const char* tag, BtMap bt) {
    if (p.kind == NnKind::Dma) {
        if (p.kc == 16) return run_nn_dma<NCTW, 16>(p, c, segs, B, bias, C, st, tag, bt);
        return run_nn_dma<NCTW, 20>(p, c, segs, B, bias, C, st, tag, bt);
    }
    if (p.kc == 32) return run_nn<NCTW, 32>(p, c, segs, B, bias, C, st, tag);
    if (p.kc == 20) return run_nn<NCTW, 20>(p, c, segs, B, bias, C, st, tag);
    if (p.kc == 16) return run_nn<NCTW, 16>(p, c, segs, B, bias, C, st, tag);
    return run_nn<NCTW, 4>(p, c, segs, B, bias, C, st, tag);
}
template <int NTB>
int run_nn_bf3(const NnPlan& p, const NnCall& c, const SegPtrs& segs, const NnRhs& B, const float* bias, float* C, hipStream_t st, const char* tag, BtMap bt) {
    EEG_SET_MAX_LDS((gemm_nn_bf3_kernel<NTB>), p.lds);
    EEG_LAUNCH_P(tag, (gemm_nn_bf3_kernel<NTB>), dim3(p.gx, p.gy), dim3(p.block), p.lds, st, segs, c.nseg, c.F, c.R, B.W3, c.bf3_nct, bias, C, c.ldc, c.O, bt.T, bt.B, bt.N);
    return check_launch("gemm_nn_bf3");
}
// C[R x O] = [segments] @ B (nct_total col tiles) + bias
int gemm_nn(const NnPlan& p, const NnCall& c, const SegPtrs& segs, const NnRhs& B, const float* bias, float* C, hipStream_t st,
            const char* tag = "gemm_nn", BtMap bt = BtMap()) {
    if (p.error == kGemmNeedsRowMap) return fail("gemm_nn: a batch-major segment needs the LDS-DMA kernel (F=%d)", c.F);
    if (p.kind == NnKind::Quad) {
        if (launch_nnq(p, segs, c.nseg, c.F, c.R, B.Bq, c.nct_total, bias, C, c.ldc, c.O, bt.T, bt.B, bt.N, st, tag)) return fail("gemm_nnq: launch failed");
        return check_launch("gemm_nnq");
    }
    if (p.kind != NnKind::Bf3) {
        if (p.nctw == 2) return run_nn_chunk<2>(p, c, segs, B, bias, C, st, tag, bt);
        if (p.nctw == 5) return run_nn_dma<5, 16>(p, c, segs, B, bias, C, st, tag, bt);   // (planned for the DMA kernel with 16-deep chunks only)
        if (p.nctw == 4) return run_nn_chunk<4>(p, c, segs, B, bias, C, st, tag, bt);
        return run_nn_chunk<6>(p, c, segs, B, bias, C, st, tag, bt);
    }
    if (p.nctw == 12) return run_nn_bf3<12>(p, c, segs, B, bias, C, st, tag, bt);
    if (p.nctw == 10) return run_nn_bf3<10>(p, c, segs, B, bias, C, st, tag, bt);
    return run_nn_bf3<8>(p, c, segs, B, bias, C, st, tag, bt);
}
// the same for a caller that holds the fp32 pack only and time-major rows
int gemm_nn(const SegPtrs& segs, int nseg, int F, int R, const float* Bp, int nct_total, const float* bias, float* C, int ldc, int O, hipStream_t st) {
    const NnCall c = nn_call(nseg, F, R, nct_total, ldc, O);
    return gemm_nn(gemm_nn_plan(c), c, segs, NnRhs{Bp}, bias, C, st);
}

struct TnArgs { const float* dY; int ldy, ycol0; float* partial; };
template <int NCTW>
int run_tn(const TnPlan& p, const TnCall& c, const SegPtrs& segs, const TnArgs& a, hipStream_t st, const char* tag) {
    EEG_SET_MAX_LDS((gemm_tn_kernel<NCTW>), p.lds);
    EEG_LAUNCH_P(tag, (gemm_tn_kernel<NCTW>), dim3(p.gx, p.gy), dim3(p.block), p.lds, st, segs, c.nseg, c.F, c.R, a.dY, a.ldy, a.ycol0, c.O, a.partial, p.rps, p.remap);
    return check_launch("gemm_tn");
}
template <int KTW, int NCTW, int RC, int WK = 2>
int run_tn_dma(const TnPlan& p, const TnCall& c, const SegPtrs& segs, const TnArgs& a, hipStream_t st, const char* tag, BtMap bt) {
    EEG_SET_MAX_LDS((gemm_tn_dma_kernel<KTW, NCTW, RC, WK>), p.lds);
    EEG_LAUNCH_P(tag, (gemm_tn_dma_kernel<KTW, NCTW, RC, WK>), dim3(p.gx, p.gy), dim3(p.block), p.lds, st, segs, c.nseg, c.F, c.R, a.dY, a.ldy, a.ycol0, c.O, a.partial, p.rps, bt.T, bt.B, bt.N, p.remap);
    return check_launch("gemm_tn_dma");
}
// partial[nsplit][nseg*F][O] = per-split A^T dY[:, ycol0:ycol0+O]
int gemm_tn(const TnPlan& p, const TnCall& c, const SegPtrs& segs, const float* dY, int ldy, int ycol0, float* partial, hipStream_t st,
            const char* tag = "gemm_tn", BtMap bt = BtMap()) {
    if (p.error == kGemmNeedsRowMap) return fail("gemm_tn: a batch-major segment needs the LDS-DMA kernel (O=%d)", c.O);
    if (p.error == kGemmBadO) return fail("gemm_tn: O=%d unsupported", c.O);
    const TnArgs a{dY, ldy, ycol0, partial};
    if (p.kind == TnKind::Quad) {
        if (launch_tnq(p, segs, c.nseg, c.F, c.R, dY, ldy, ycol0, c.O, partial, bt.T, bt.B, bt.N, st, tag)) return fail("gemm_tnq: launch failed");
        return check_launch("gemm_tnq");
    }
    if (p.kind != TnKind::Staged) {
        const bool wide = p.kind == TnKind::DmaWide;
        if (p.nctw == 6) return wide ? run_tn_dma<2, 6, 16, 4>(p, c, segs, a, st, tag, bt) : run_tn_dma<2, 6, 16>(p, c, segs, a, st, tag, bt);
        if (p.nctw == 4) return wide ? run_tn_dma<2, 4, 32, 4>(p, c, segs, a, st, tag, bt) : run_tn_dma<2, 4, 32>(p, c, segs, a, st, tag, bt);
        return wide ? run_tn_dma<2, 2, 32, 4>(p, c, segs, a, st, tag, bt) : run_tn_dma<2, 2, 32>(p, c, segs, a, st, tag, bt);
    }
    if (p.nctw == 1) return run_tn<1>(p, c, segs, a, st, tag);
    if (p.nctw == 2) return run_tn<2>(p, c, segs, a, st, tag);
    if (p.nctw == 4) return run_tn<4>(p, c, segs, a, st, tag);
    return run_tn<6>(p, c, segs, a, st, tag);
}

// ---- hop diffusion ----------------------------------------------------------------------------
// diffuse_launch.h plans a call (kernel, grid, block, LDS, column chunk); it is executed here, one launch line per kernel signature.
DiffuseCall diffuse_call(bool adjoint, int p_batched, int S, int B, int N, int F, int M, int x_bt = 0, bool wants_copy = false) {
    return DiffuseCall{p_batched, S, B, N, F, M, adjoint, x_bt, wants_copy, g_tune[EEG_TUNE_DIFFUSE_FWD_WGS], g_tune[EEG_TUNE_DIFFUSE_ADJ_WGS],
                       g_tune[EEG_TUNE_DIFFUSE_ADJ_LDS], g_tune[EEG_TUNE_DIFFUSE_ADJ_PLANES]};
}
// x_bt: X is batch-major (B, S/B, N, F) and xcopy gets its time-major copy (streaming kernel only)
int diffuse_fwd(const float* X, const float* P, int p_batched, int S, int B, int N, int F, int M, float* planes,
                hipStream_t st, size_t plane_stride = 0, int x_bt = 0, float* xcopy = nullptr) {
    if (plane_stride == 0) plane_stride = (size_t)S * N * F;
    const DiffusePlan p = diffuse_plan(diffuse_call(false, p_batched, S, B, N, F, M, x_bt, xcopy != nullptr));
    if (p.error == kDiffuseBatchMajorNeedsStream) return fail("diffuse_fwd: batch-major input needs the streaming kernel");
    if (p.error == kDiffuseNoFit) return fail("diffuse_fwd: N=%d M=%d does not fit the LDS tile", N, M);
    switch (p.kind) {
        case DiffuseKind::None: return 0;
        case DiffuseKind::StreamFwd:
            EEG_LAUNCH_P("diffuse_fwd", diffuse_fwd_stream_kernel<19>, dim3(p.gx, p.gy), dim3(p.block), 0, st, X, P, p_batched, S, B, F, M, planes, plane_stride, x_bt, xcopy);
            return check_launch("diffuse_fwd");
        default:
            EEG_SET_MAX_LDS(diffuse_fwd_kernel, p.lds);
            for (int c0 = 0; c0 < F; c0 += p.fc) {
                EEG_LAUNCH_P("diffuse_fwd", diffuse_fwd_kernel, dim3(p.gx, p.gy), dim3(p.block), p.lds, st, X, P, p_batched, S, B, N, F, M, planes, plane_stride,
                             c0, F - c0 < p.fc ? F - c0 : p.fc);
                if (check_launch("diffuse_fwd")) return 1;
            }
            return 0;
    }
}
int diffuse_adj(const float* Z, const float* P, int p_batched, int S, int B, int N, int F, int M, float* dX,
                hipStream_t st, const float* add = nullptr) {
    const DiffusePlan p = diffuse_plan(diffuse_call(true, p_batched, S, B, N, F, M));
    if (p.error == kDiffuseNoFit) return fail("diffuse_adj: N=%d M=%d does not fit the LDS tile", N, M);
    const dim3 grid(p.gx, p.gy), block(p.block);
    switch (p.kind) {
        case DiffuseKind::RowsAdj:
            if (p.mm == 3) EEG_LAUNCH_P("diffuse_adj", (diffuse_adj_rows_kernel<19, 3>), grid, block, 0, st, Z, P, p_batched, S, B, F, add, dX);
            else EEG_LAUNCH_P("diffuse_adj", (diffuse_adj_rows_kernel<19, 5>), grid, block, 0, st, Z, P, p_batched, S, B, F, add, dX);
            return check_launch("diffuse_adj");
        case DiffuseKind::StreamAdj:
            EEG_LAUNCH_P("diffuse_adj", diffuse_adj_stream_kernel<19>, grid, block, 0, st, Z, P, p_batched, S, B, F, M, add, dX);
            return check_launch("diffuse_adj");
        default:
            EEG_SET_MAX_LDS(diffuse_adj_kernel, p.lds);
            for (int c0 = 0; c0 < F; c0 += p.fc) {
                EEG_LAUNCH_P("diffuse_adj", diffuse_adj_kernel, dim3(p.gx), block, p.lds, st, Z, P, p_batched, S, B, N, F, M, add, dX,
                             c0, F - c0 < p.fc ? F - c0 : p.fc);
                if (check_launch("diffuse_adj")) return 1;
            }
            return 0;
    }
}

// ---- per-clip correlation Gram ---------------------------------------------------------------
// corr_launch.h plans a call; these execute it: the template switch and one launch line per kernel signature
template <int NQ, bool REM4, bool LEN>
void run_corr_gram(const CorrGramPlan& p, const float* X, int T, int N, int D, float* ws, const long long* len, hipStream_t st) {
    EEG_SET_MAX_LDS((corr_gram_kernel<NQ, REM4, LEN>), p.lds);
    EEG_LAUNCH_P(LEN ? "corr_gram_len" : "corr_gram", (corr_gram_kernel<NQ, REM4, LEN>), dim3(p.gx, p.gy), dim3(p.block), p.lds, st, X, T, N, D, ws, p.step_floats, len);
}
template <int NQ>
void run_corr_gram(const CorrGramPlan& p, const float* X, int T, int N, int D, float* ws, const long long* len, hipStream_t st) {
    if (p.len) return p.rem4 ? run_corr_gram<NQ, true, true>(p, X, T, N, D, ws, len, st) : run_corr_gram<NQ, false, true>(p, X, T, N, D, ws, len, st);
    return p.rem4 ? run_corr_gram<NQ, true, false>(p, X, T, N, D, ws, len, st) : run_corr_gram<NQ, false, false>(p, X, T, N, D, ws, len, st);
}
int corr_finish(const float* ws, int B, int ns, int N, int top_k, float* adj, float* S1, float* S2, hipStream_t st) {
    EEG_LAUNCH_P("corr_finish", corr_finish_kernel, dim3(B), dim3(256), corr_finish_lds_bytes(), st, ws, ns, N, top_k, adj, S1, S2);
    return check_launch("corr_finish");
}
template <bool REM4, bool LEN>
void run_corr_gram_rows(const CorrRowsPlan& p, const float* X, int N, int P, int Q, float* ws, const long long* len, hipStream_t st) {
    EEG_SET_MAX_LDS((corr_gram_rows_kernel<REM4, LEN>), p.lds);
    EEG_LAUNCH_P(LEN ? "corr_gram_rows_len" : "corr_gram_rows", (corr_gram_rows_kernel<REM4, LEN>), dim3(p.gx, p.gy), dim3(p.block), p.lds, st, X, N, P, Q, p.ps,
                 (unsigned)p.clip_floats, ws, p.tile_floats, len, p.unit);
}

// The recurrent launches: the caller makes the plan (seq_launch.h) from one of these calls, lays its operands out by plan.kind,
// and the plan is executed here.  The knobs are compile-time zeros in the product build.
SeqCall seq_fwd_call(int H, int M, int N, int T, int B, size_t plane_stride, const long long* probe) {
    SeqCall c{H, M, N, T, B};
    c.plane_stride = plane_stride;
    c.knob_one_wave = g_tune[EEG_TUNE_SEQ_FWD_ONE_WAVE];
    c.knob_no_spec = g_tune[EEG_TUNE_SEQ_FWD_NO_SPEC];
    c.probe = carries_phase_probe(probe);
    return c;
}
SeqCall seq_bwd_call(int H, int M, int N, int T, int B, const long long* probe) {
    SeqCall c{H, M, N, T, B};
    c.knob_one_wave = g_tune[EEG_TUNE_SEQ_BWD_ONE_WAVE];
    c.knob_no_spec = g_tune[EEG_TUNE_SEQ_BWD_NO_SPEC];
    c.knob_stream = g_tune[EEG_TUNE_SEQ_STREAM];
    c.probe = carries_phase_probe(probe);
    return c;
}
int seq_plan_error(const char* what, const SeqPlan& p, int H, int M, int N) {
    if (p.error == kSeqNoKernel) return fail("%s: no kernel for H=%d M=%d", what, H, M);
    if (p.error == kSeqNoFit) return fail("%s: H=%d M=%d N=%d exceeds the LDS of a CU", what, H, M, N);
    return 0;
}
int seq_fwd(int H, int M, const SeqPlan& p, const SeqFwdArgs& a, hipStream_t st) {
    if (seq_plan_error("seq_fwd", p, H, M, a.N)) return 1;
    if (H == 16 ? launch_seq_fwd_h16(M, p, a, st) : H == 32 ? launch_seq_fwd_h32(M, p, a, st) : launch_seq_fwd_h64(M, p, a, st))
        return fail("seq_fwd: kernel launch failed (H=%d M=%d)", H, M);
    return 0;
}
int seq_bwd(int H, int M, const SeqPlan& p, const SeqBwdArgs& a, hipStream_t st) {
    if (seq_plan_error("seq_bwd", p, H, M, a.N)) return 1;
    if (p.kind == SeqKind::Stream) return launch_seq_bwd_stream(M, p, a, st) ? fail("seq_bwd: streamed kernel launch failed (M=%d)", M) : 0;
    if (H == 16 ? launch_seq_bwd_h16(M, p, a, st) : H == 32 ? launch_seq_bwd_h32(M, p, a, st) : launch_seq_bwd_h64(M, p, a, st))
        return fail("seq_bwd: kernel launch failed (H=%d M=%d)", H, M);
    return 0;
}

// The spectral form (spec_common.h): the caller makes the plans (spec_launch.h) from its dims, the CU count and these knobs
// (compile-time zeros in the product build), sizes its workspace by them, and the launchers of spec_inst.cpp execute them.
SpecKnobs spec_knobs() { return SpecKnobs{g_tune[EEG_TUNE_SPEC_NN_GROUPED], g_tune[EEG_TUNE_SPEC_TN_SEPARATE], g_tune[EEG_TUNE_SPEC_DX_PASSES]}; }
int spec_plan_error(const char* what, int error) {
    if (error == kSpecBadNct) return fail("%s: the grouped GEMM has no instance for this column count", what);
    if (error == kSpecNotCovered) return fail("%s: the spectral form does not cover this shape", what);
    return 0;
}
int spec_mix(int to_nodes, const float* in, const float* basis, int N, int T, int B, int F, int bm, float* out, hipStream_t st, const char* tag,
             int node_rows = 0) {
    return launch_spec_mix(spec_mix_plan(to_nodes, N, T, B, F, node_rows), in, basis, N, T, B, F, bm, out, st, tag) ? fail("spec_mix: launch failed") : 0;
}

struct BwdWs {
    size_t dxw, dbias, hplanes, rhplanes, partial, part_g, part_c, z, total;   // partial = x-part region; part_g / part_c follow it
    TnCall cx, chg, chc;       // the three weight-gradient TNs of the cell (x-part, h-part of the gate, of the candidate) ...
    TnPlan tx, thg, thc;       // ... and their plans: kernel, row split (-> the partial regions), grid
    bool pair;                 // the two h-part problems as one launch (tn_pair_applies)
    // spectral form (d->spectral): dyh = U^T dXW (N, Sp, 3H); hplanes / rhplanes = U^T h_{t-1}, U^T (r*h_{t-1}) (N, Sp, H); partial /
    // part_g / part_c = the grouped TNs' [N*spg][K][O]; z = dXh (N, Sp, Fin)
    size_t dyh;
    SpecTnPlan gs;             // the three problems in one pass or as the grouped launches, their row splits and partial sizes
};
BwdWs bwd_ws(const eeg_layer_dims* d, int need_dx) {
    BwdWs w;
    const size_t R = (size_t)d->T * d->B * d->N;
    const bool spec = d->spectral != nullptr;
    const size_t Rp = (size_t)d->N * spec_rows(d->T * d->B);
    size_t o = 0;
    w.dxw = o;      o += R * 3 * d->H;
    w.dbias = o;    o += round_up(d->B * 3 * d->H, 64);
    w.hplanes = o;  o += spec ? Rp * d->H : (size_t)(d->M - 1) * R * d->H;
    w.rhplanes = o; o += spec ? Rp * d->H : (size_t)(d->M - 1) * R * d->H;
    w.dyh = o;      o += spec ? Rp * 3 * d->H : 0;
    w.gs = spec ? spec_tn_plan(d->Fin, d->H, spec_rows(d->T * d->B), d->N, num_cus(), spec_knobs()) : SpecTnPlan{};
    w.cx = tn_call(d->M, d->Fin, (int)R, 3 * d->H, d->x_batch_major != 0, true);
    w.chg = tn_call(d->M, d->H, (int)R, 2 * d->H, false, true);
    w.chc = tn_call(d->M, d->H, (int)R, d->H, false, true);
    w.tx = gemm_tn_plan(w.cx);
    w.thg = gemm_tn_plan(w.chg);
    w.thc = gemm_tn_plan(w.chc);
    w.pair = tn_pair_applies(w.thg, w.thc, w.chg.knobs);
    size_t px = (size_t)w.tx.nsplit * d->M * d->Fin * 3 * d->H;
    size_t pg = (size_t)w.thg.nsplit * d->M * d->H * 2 * d->H;
    size_t pc = (size_t)w.thc.nsplit * d->M * d->H * d->H;
    if (spec) { px = w.gs.px; pg = w.gs.pg; pc = w.gs.pc; }
    w.partial = o;  o += (px + 63) / 64 * 64;      // one region per GEMM: the three are reduced by one launch
    w.part_g = o;   o += (pg + 63) / 64 * 64;
    w.part_c = o;   o += (pc + 63) / 64 * 64;
    // (spectral: dXh, read only by the two passes of a spec_dx_plan with needs_dxh; reserved whenever dX is asked for, because
    // eeg_dcrnn_layer_bwd_ws_floats is part of the ABI -- a bwd_ws that asked that plan first could drop it)
    w.z = o;        o += need_dx ? (spec ? Rp * d->Fin : R * d->M * d->Fin) : 0;
    w.total = o;
    return w;
}


// Hoisted weight gradients of one cell over all R = T*B*N rows (split-K GEMMs with fixed-order
// reduction): x-part [X | P_m X]^T [dR|dU|dC], h-part of the gate hops(h_{t-1})^T [dR|dU] and of the
// candidate hops(r*h_{t-1})^T dC.  accumulate = add into dWg/dWc (a cell shared by several layers).
// hpl_in / rpl_in: hop planes of h_{t-1} / r*h_{t-1} kept by the forward kernel (NULL: recomputed into hpl / rpl).
// x_stride / h_stride: floats between two hop planes of `planes` / of hpl_in, rpl_in.
int cell_weight_grads(const eeg_layer_dims* d, const float* X, const float* planes, size_t x_stride, const float* Hprev,
                      const float* RHs, const float* dXW, const float* P, const float* hpl_in, const float* rpl_in,
                      size_t h_stride, float* hpl_ws, float* rpl_ws, float* part, const BwdWs& w, bool accumulate,
                      float* dWg, float* dWc, hipStream_t st, BtMap bt = BtMap(), const float* bias_part = nullptr,
                      float* dbg = nullptr, float* dbc = nullptr) {
    const int S = d->T * d->B, R = S * d->N, H = d->H, M = d->M, Fin = d->Fin, N = d->N;
    const int acc = accumulate ? 8 : 0;
    SegPtrs sx;
    for (int m = 0; m < kMaxM; ++m) sx.p[m] = m == 0 ? X : (m < M ? planes + (size_t)(m - 1) * x_stride : nullptr);
    float* part_g = part + (w.part_g - w.partial);
    float* part_c = part + (w.part_c - w.partial);
    if (gemm_tn(w.tx, w.cx, sx, dXW, 3 * H, 0, part, st, "gemm_tn_x", bt)) return 1;
    //   h-part of the gate: hops(h_{t-1})^T [dR|dU]
    const float* hpl = hpl_in;
    size_t hs = h_stride;
    if (hpl == nullptr) {
        if (diffuse_fwd(Hprev, P, d->p_batched, S, d->B, N, H, M, hpl_ws, st)) return 1;
        hpl = hpl_ws;
        hs = (size_t)R * H;
    }
    SegPtrs sh;
    for (int m = 0; m < kMaxM; ++m) sh.p[m] = m == 0 ? Hprev : (m < M ? hpl + (size_t)(m - 1) * hs : nullptr);
    //   h-part of the candidate: hops(r*h_{t-1})^T dC
    const float* rpl = rpl_in;
    size_t rs = h_stride;
    if (rpl == nullptr) {
        if (diffuse_fwd(RHs, P, d->p_batched, S, d->B, N, H, M, rpl_ws, st)) return 1;
        rpl = rpl_ws;
        rs = (size_t)R * H;
    }
    SegPtrs sr;
    for (int m = 0; m < kMaxM; ++m) sr.p[m] = m == 0 ? RHs : (m < M ? rpl + (size_t)(m - 1) * rs : nullptr);
    // Round 5: where the pair applies (gemm_launch.h) the two h-part problems go out as ONE launch whose workgroups alternate
    // between the two -- the 64-column problem waits for its operands (0.61 of the MFMA peak alone), the 128-column one for the
    // matrix pipe (0.77): side by side on the two workgroup slots of a CU they take 0.366 instead of 0.390 ms per cfg2 step (role
    // `gemm_tn_h`)
    if (w.pair) {
        if (launch_tnq_pair(w.thg.q, w.thc.q, sh, sr, M, H, R, dXW, 3 * H, 0, 2 * H, part_g, 2 * H, H, part_c, st, "gemm_tn_h"))
            return fail("gemm_tnq_pair: launch failed");
    } else {
        if (gemm_tn(w.thg, w.chg, sh, dXW, 3 * H, 0, part_g, st, "gemm_tn_hg")) return 1;
        if (gemm_tn(w.thc, w.chc, sr, dXW, 3 * H, 2 * H, part_c, st, "gemm_tn_hc")) return 1;
    }
    //   one fixed-order reduction of the three sets of split-K partials into the reference's gradient layout
    ReduceJobs jobs;
    const int Ks[3] = {M * Fin, M * H, M * H}, Os[3] = {3 * H, 2 * H, H}, ns[3] = {w.tx.nsplit, w.thg.nsplit, w.thc.nsplit};
    const float* parts[3] = {part, part_g, part_c};
    int nblocks = 0;
    for (int j = 0; j < 3; ++j) {
        jobs.part[j] = parts[j]; jobs.nsplit[j] = ns[j]; jobs.K[j] = Ks[j]; jobs.O[j] = Os[j];
        jobs.nblocks[j] = ceil_div(Ks[j] * Os[j], 64);
        nblocks += jobs.nblocks[j];
    }
    // the cell's bias gradients (per-clip partials of the BPTT kernel -> dbg, dbc) as a fourth job of the same launch
    jobs.bias_part = bias_part; jobs.bias_B = d->B; jobs.dbg = dbg; jobs.dbc = dbc;
    if (bias_part != nullptr) nblocks += ceil_div(3 * H, 16);
    EEG_LAUNCH_P("reduce_unpack", reduce_unpack3_kernel, dim3(nblocks), dim3(256), 256 * sizeof(float4), st, jobs, acc, Fin, H, M, dWg, dWc);
    return check_launch("reduce_unpack");
}

// The same weight gradients in the eigenbasis of a shared symmetric support (spec_common.h): every hoisted contraction runs per
// graph frequency i over K = Fin (x-part) / K = H (h-parts) instead of M * Fin / M * H, and the fold dW_m = sum_i T_m(lam_i) dWt_i
// rides in the reduction launch.  Xh = U^T X (N, Sp, Fin; groups x_gs floats apart), dYh = U^T dXW (N, Sp, 3H), hh = U^T h_{t-1}
// (groups hh_gs floats apart, 0 = contiguous), rhh = U^T (r*h_{t-1}) (N, Sp, H); all rows time-major.
size_t xs_spec(const eeg_layer_dims* d) { return d->x_plane_stride > 0 ? (size_t)d->x_plane_stride : 0; }
int cell_weight_grads_spectral(const eeg_layer_dims* d, const float* Xh, size_t x_gs, const float* hh, size_t hh_gs, const float* rhh,
                               const float* dYh, float* part, const BwdWs& w, float* dWg, float* dWc, hipStream_t st,
                               const float* bias_part, float* dbg, float* dbc) {
    const int S = d->T * d->B, H = d->H, M = d->M, Fin = d->Fin, N = d->N, Sp = spec_rows(S);
    float* part_g = part + (w.part_g - w.partial);
    float* part_c = part + (w.part_c - w.partial);
    const SpecTnPlan& g = w.gs;
    if (spec_plan_error("weight gradients (spectral)", g.error)) return 1;
    if (g.fused) {
        if (launch_tnf(g, Xh, x_gs, Fin, hh, hh_gs, rhh, dYh, Sp, N, part, part_g, part_c, st, "gemm_tn_f")) return fail("gemm_tnf: launch failed");
    } else {
        if (launch_tng(g, Xh, x_gs, Fin, Sp, N, dYh, part, st, "gemm_tn_x")) return fail("gemm_tng: launch failed");
        if (launch_tng_pair(g, hh, hh_gs, rhh, Sp, N, dYh, part_g, part_c, st, "gemm_tn_h")) return fail("gemm_tng_pair: launch failed");
    }
    ReduceJobs jobs{};
    SpecFoldJobs sj{};
    sj.basis = d->spectral; sj.N = N;
    sj.j[0] = SpecFoldJob{part, g.spg_x, Fin, 3 * H, ceil_div(Fin * 3 * H, 64)};
    sj.j[1] = SpecFoldJob{part_g, g.spg_h, H, 2 * H, ceil_div(H * 2 * H, 64)};
    sj.j[2] = SpecFoldJob{part_c, g.spg_h, H, H, ceil_div(H * H, 64)};
    int nblocks = sj.j[0].nblocks + sj.j[1].nblocks + sj.j[2].nblocks;
    jobs.bias_part = bias_part; jobs.bias_B = d->B; jobs.dbg = dbg; jobs.dbc = dbc;
    if (bias_part != nullptr) nblocks += ceil_div(3 * H, 16);
    const int ns_max = N * (g.spg_x > g.spg_h ? g.spg_x : g.spg_h);
    const size_t fold_lds = spec_fold_lds_bytes(M, ns_max);
    EEG_SET_MAX_LDS(reduce_unpack3s_kernel, fold_lds);
    EEG_LAUNCH_P("reduce_unpack", reduce_unpack3s_kernel, dim3(nblocks), dim3(256), fold_lds, st, jobs, sj, 0, Fin, H, M, dWg, dWc);
    return check_launch("reduce_unpack (spectral)");
}

// out0[c] (c < split) / out1[c - split] = sum_r A[r][c]: two fixed-order stages.
int colsum_rows_per_chunk(int R) { int rpc = ceil_div(R, 512); return rpc < 64 ? 64 : rpc; }
size_t colsum_ws(int R, int C) { return (size_t)ceil_div(R, colsum_rows_per_chunk(R)) * C; }
int colsum(const float* A, int R, int C, int split, float* ws, float* out0, float* out1, hipStream_t st) {
    const int rpc = colsum_rows_per_chunk(R), nchunk = ceil_div(R, rpc);
    if (C % 4 == 0 && C <= 1024) {
        const int nrs = 256 / (C / 4);
        EEG_LAUNCH_P("reduce_bias", colsum_partial4_kernel, dim3(nchunk), dim3(256), (size_t)nrs * C * sizeof(float), st, A, R, C, rpc, ws);
    } else {
        EEG_LAUNCH_P("reduce_bias", colsum_partial_kernel, dim3(nchunk, ceil_div(C, 128)), dim3(256), 256 * sizeof(float), st, A, R, C, rpc, ws);
    }
    if (check_launch("colsum_partial")) return 1;
    EEG_LAUNCH_P("reduce_bias", colsum_final_kernel, dim3(ceil_div(C, 128)), dim3(128), 0, st, ws, nchunk, C, split, out0, out1);
    return check_launch("colsum_final");
}

// ---- decoder (model.py:112-204): buffer carving shared by forward and backward -------------------
struct DecLayout {
    // saved (forward -> backward)
    size_t xin, proj_pack, proj_bias, hd, saved_total;
    size_t planes[8], hext[8], rs[8], us[8], cs[8], rhs[8], hpl[8], rpl[8];
    // backward workspace
    size_t dxw[8], dbias[8], dotot, da, dhn, z, partial, projt_pack, colsum, bwd_total;
    TnCall cp;                 // the projection's weight gradient
    TnPlan tp;
    BwdWs lw[8];
    eeg_layer_dims ld[8];
};
size_t align64(size_t v) { return (v + 63) / 64 * 64; }
DecLayout dec_layout(const eeg_decoder_dims* d) {
    DecLayout y;
    const size_t state = (size_t)d->B * d->N * d->H, R = (size_t)d->T * d->B * d->N;
    const int nct_o = ceil_div(d->Dout, 16), nct_h = ceil_div(d->H, 16);
    size_t o = 0;
    y.xin = o;       o += align64(R * d->Dout);
    y.proj_pack = o; o += align64((size_t)(d->H / 4) * nct_o * 64);
    y.proj_bias = o; o += align64((size_t)nct_o * 16);
    for (int l = 0; l < d->L; ++l) {
        const int fin = l == 0 ? d->Dout : d->H;
        y.ld[l] = eeg_layer_dims{d->T, d->B, d->N, d->H, fin, d->M, d->act, d->p_batched, 0, 0, 0};
        y.planes[l] = o; if (l == 0) o += align64((size_t)(d->M - 1) * R * fin);   // layers >= 1: the hpl of the layer below
        y.hext[l] = o;   o += align64((size_t)(d->T + 1) * state);
        y.rs[l] = o;     o += align64((size_t)d->T * state);
        y.us[l] = o;     o += align64((size_t)d->T * state);
        y.cs[l] = o;     o += align64((size_t)d->T * state);
        y.rhs[l] = o;    o += align64((size_t)d->T * state);
        // hop planes of h_{t-1} (slots 0..T; slot t+1 = hops of this layer's output at step t = the next layer's
        // input planes) and of r*h_{t-1}: by-products of the forward kernel, A operands of the dW GEMMs
        y.hpl[l] = o;    o += align64((size_t)(d->M - 1) * (d->T + 1) * state);
        y.rpl[l] = o;    o += align64((size_t)(d->M - 1) * (d->T + 1) * state);
    }
    // dropout in front of the projection: the dropped top-layer outputs (T,B,N,H) (A operand of dW_p); without dropout they
    // ARE hext[L-1] slots 1..T
    y.hd = d->dropout_p > 0.f ? o : y.hext[d->L - 1] + state;
    if (d->dropout_p > 0.f) o += align64((size_t)d->T * state);
    y.saved_total = o;
    o = 0;
    size_t part = 0;
    for (int l = 0; l < d->L; ++l) {
        y.lw[l] = bwd_ws(&y.ld[l], 0);
        y.dxw[l] = o; o += align64(R * 3 * d->H);
        const size_t pl = y.lw[l].total - y.lw[l].partial;      // partial is the last region when need_dx = 0
        part = pl > part ? pl : part;
    }
    for (int l = 0; l < d->L; ++l) { y.dbias[l] = o; o += (size_t)d->T * d->B * 3 * d->H; }   // contiguous: shared layers reduce at once
    o = align64(o);
    y.dotot = o;  o += align64(R * d->Dout);
    y.da = o;     o += align64(state);
    y.dhn = o;    o += align64(2 * (size_t)d->L * state);
    y.z = o;      o += align64((size_t)d->B * d->N * d->M * (d->Dout > d->H ? d->Dout : d->H));
    y.cp = tn_call(1, d->Dout, (int)R, d->H);
    y.tp = gemm_tn_plan(y.cp);
    const size_t pp = (size_t)y.tp.nsplit * d->Dout * d->H;
    part = pp > part ? pp : part;
    y.partial = o; o += align64(part);
    y.projt_pack = o; o += align64((size_t)(d->Dout / 4) * nct_h * 64);
    const size_t c1 = colsum_ws((int)R, d->Dout), c2 = colsum_ws(d->L * d->T * d->B, 3 * d->H);
    y.colsum = o; o += align64(c1 > c2 ? c1 : c2);
    y.bwd_total = o;
    return y;
}
// nn.Dropout's own argument check (torch: "dropout probability has to be between 0 and 1, but got ...")
int check_dropout_p(const char* who, float p) {
    if (!(p >= 0.f && p <= 1.f)) return fail("%s: dropout probability has to be between 0 and 1, but got %g", who, p);
    return 0;
}
int check_decoder_dims(const eeg_decoder_dims* d) {
    if (d->L < 1 || d->L > 8) return fail("decoder: num_rnn_layers=%d unsupported (1..8)", d->L);
    if (d->T < 1 || d->B < 1) return fail("decoder: empty sequence/batch (T=%d, B=%d)", d->T, d->B);
    if (check_dropout_p("decoder", d->dropout_p)) return 1;
    if (check_dims(d->N, d->H, d->Dout, d->M)) return 1;
    return check_dims(d->N, d->H, d->H, d->M);
}
// The persistent decoder kernels: the caller asks dec_plan (dec_launch.h) with these dims and knobs (compile-time zeros in the product
// build) whether they take the decoder, and the launchers of dec_inst.cpp / decb_inst.cpp execute the plan.
DecCall dec_call(const eeg_decoder_dims* d) {
    return DecCall{d->T, d->B, d->N, d->H, d->Dout, d->M, d->L, g_tune[EEG_TUNE_DEC_FWD_PER_STEP], g_tune[EEG_TUNE_DEC_BWD_PER_STEP]};
}
int copy_floats(float* dst, const float* src, size_t n, hipStream_t st) {
    return platform_copy_floats(dst, src, n, st) ? 0 : fail("device copy failed");
}

}  // namespace

// ---- Fourier resampling of whole recordings (kernels_resample.h): the lengths and the FFT passes of eeg_dcrnn_resample ----
namespace {
constexpr int kRsMaxChunk = 1024;                                        // channels of one pass over the workspace (grid.y)
// the two chirp-z transforms of a (n_in -> n_out) resample: log2 of their FFT lengths; false: a length outside the limits
bool rs_lengths(int64_t n_in, int64_t n_out, int& lm1, int& lm2) {
    if (n_in < 2 || n_in > EEG_RESAMPLE_MAX_SAMPLES || n_out < 1 || n_out > EEG_RESAMPLE_MAX_SAMPLES) return false;
    lm1 = rs_log2_len(n_in + std::min(n_in, n_out) / 2);                 // n_in inputs, the min(n_in, n_out) / 2 + 1 bins that are kept
    lm2 = rs_log2_len(n_out / 2 + 1 + n_out - 1);
    return lm1 <= kRsMaxBits && lm2 <= kRsMaxBits;
}
// buf[c][0 .. 2^lm) for `channels` rows: the forward transform alone (filt null), or the circular convolution with the filter whose
// forward transform is filt (unscaled: 2^lm times the convolution)
template <int MODE>
int rs_pass(rs_c64* buf, long long stride, int channels, const rs_c64* filt, int lm, int lbits, int sbits, int gbits, hipStream_t st) {
    const size_t lds = rs_pass_lds(lbits, gbits);
    EEG_SET_MAX_LDS(rs_fft_pass_kernel<MODE>, kRsMaxLds);
    EEG_LAUNCH_P("resample_fft", rs_fft_pass_kernel<MODE>, dim3((unsigned)(1u << (lm - lbits - gbits)), (unsigned)channels), dim3(kRsThreads), lds, st,
                 buf, stride, filt, lm, lbits, sbits, gbits);
    return check_launch("resample_fft");
}
int rs_transform(rs_c64* buf, long long stride, int channels, const rs_c64* filt, int lm, hipStream_t st) {
    const RsPlan p = rs_plan(lm);
    int sb[kRsMaxPasses], gb[kRsMaxPasses], rest = lm;
    for (int i = 0; i < p.passes; ++i) {
        rest -= p.bits[i];
        sb[i] = rest;
        gb[i] = p.passes == 1 ? 0 : kRsPassTileBits - p.bits[i];
    }
    const int last = p.passes - 1;
    for (int i = 0; i < last; ++i)
        if (int rc = rs_pass<kRsFwd>(buf, stride, channels, nullptr, lm, p.bits[i], sb[i], gb[i], st)) return rc;
    if (filt == nullptr) return rs_pass<kRsFwd>(buf, stride, channels, nullptr, lm, p.bits[last], sb[last], gb[last], st);
    if (int rc = rs_pass<kRsBoth>(buf, stride, channels, filt, lm, p.bits[last], sb[last], gb[last], st)) return rc;
    for (int i = last - 1; i >= 0; --i)
        if (int rc = rs_pass<kRsInv>(buf, stride, channels, nullptr, lm, p.bits[i], sb[i], gb[i], st)) return rc;
    return 0;
}
}  // namespace

extern "C" {

const char* eeg_dcrnn_last_error(void) { return g_err; }
int eeg_dcrnn_abi_version(void) { return 5; }
int eeg_dcrnn_is_device_build(void) { return kPlatformIsDevice; }
#if defined(EEG_DEV)
int eeg_dcrnn_set_tuning(int key, int value) {
    if (key < 0 || key >= EEG_TUNE_COUNT) return fail("set_tuning: key %d out of range", key);
    g_tune[key] = value;
    return 0;
}
int eeg_dcrnn_set_seq_probe(int64_t* probe) {
    g_seq_probe = reinterpret_cast<long long*>(probe);
    return 0;
}
#endif
int eeg_dcrnn_prof_enable(int on) {
    eeg::prof_enable(on != 0);
    return 0;
}
int eeg_dcrnn_prof_report(char* buf, size_t cap) {
    if (buf == nullptr || cap == 0) return fail("prof_report: empty buffer");
    buf[0] = 0;
    const size_t need = eeg::prof_report(buf, cap);
    if (need != 0) return fail("prof_report: buffer too small (%zu needed)", need);
    return 0;
}
namespace {
// Every SIMD of the chip streams fp32 MFMAs (two accumulator chains per wave = the issue rate) for `ticks` of the chip-wide 100 MHz
// counter; the shader-clock cycles that pass during the SECOND half are summed over the workgroups: out[0] += cycles, out[1] += ticks.
__global__ __launch_bounds__(256) void clock_probe_kernel(long long ticks, long long* __restrict__ out) {
    const float a = 0.001f * (threadIdx.x & 63), b = 1.f + (threadIdx.x & 63);
    f32x4 p = {0.f, 0.f, 0.f, 0.f}, q = p;
    const long long r0 = realtime_now();
    long long r1 = r0, rh = 0, ch = 0;
    for (int i = 0; i < (1 << 20) && r1 - r0 < ticks; ++i) {
#pragma unroll
        for (int k = 0; k < 16; ++k) { p = mfma16(a, b, p); q = mfma16(b, a, q); }
        r1 = realtime_now();
        if (rh == 0 && r1 - r0 >= ticks / 2) { rh = r1; ch = cycle_now(); }
    }
    const long long c1 = cycle_now();
    if (p[0] + q[0] == 12345.f) out[2] = 1;                       // (keeps the MFMAs)
    if (threadIdx.x == 0 && rh != 0) {
        atomic_add_u64(reinterpret_cast<unsigned long long*>(out), (unsigned long long)(c1 - ch));
        atomic_add_u64(reinterpret_cast<unsigned long long*>(out) + 1, (unsigned long long)(r1 - rh));
    }
}
}  // namespace
int eeg_dcrnn_prof_clock_samples(int64_t* buf4) {
    g_clock_samples.store(reinterpret_cast<long long*>(buf4), std::memory_order_release);
    return 0;
}
int eeg_dcrnn_prof_clock_probe(int64_t* out2, void* stream) {
    if (out2 == nullptr) return fail("prof_clock_probe: null output");
    // 200 us of full-chip fp32-MFMA load; the caller zeroes out2 (3 x int64) first
    EEG_LAUNCH(clock_probe_kernel, dim3(platform_num_cus()), dim3(256), 0, S_(stream), (long long)20000, reinterpret_cast<long long*>(out2));
    return check_launch("clock_probe");
}
int eeg_dcrnn_supported(int N, int H, int Fin, int M) { return check_dims(N, H, Fin, M) == 0 ? 1 : 0; }
int eeg_dcrnn_zero(void* p, size_t bytes, void* stream) {
    if (bytes == 0) return 0;
    if (p == nullptr) return fail("zero: null pointer");
    if (reinterpret_cast<uintptr_t>(p) % 16 != 0)                       // (torch allocations are 256-byte aligned; views may not be)
        return hipMemsetAsync(p, 0, bytes, S_(stream)) == hipSuccess ? 0 : fail("zero: memset failed");
    const size_t n16 = bytes / 16;
    const int blocks = (int)(n16 / 256 < 1 ? 1 : (n16 / 256 > 1024 ? 1024 : n16 / 256));
    EEG_LAUNCH_P("zero", zero_kernel, dim3(blocks), dim3(256), 0, S_(stream), reinterpret_cast<float4*>(p), n16,
                 reinterpret_cast<unsigned char*>(p) + 16 * n16, (int)(bytes - 16 * n16));
    return check_launch("zero");
}

int eeg_dcrnn_hop_polys(const float* const* supports, int n_supports, int n_graphs, int N, int K, float* P_out,
                        void* stream) {
    if (n_supports < 1 || n_supports > 4) return fail("hop_polys: n_supports=%d unsupported (1..4)", n_supports);
    if (N < 1 || N > kMaxNodes) return fail("hop_polys: num_nodes=%d unsupported", N);
    if (K < 0) return fail("hop_polys: max_diffusion_step=%d unsupported (>= 0)", K);
    if (n_graphs < 1) return fail("hop_polys: no graphs (n_graphs=%d)", n_graphs);
    if (K == 0) return 0;                            // cell.py:80-81: no hop matrices beyond the identity, P_out is empty
    if (n_supports * K + 1 > kMaxM) return fail("hop_polys: %d supports x K=%d exceeds %d hop matrices", n_supports, K, kMaxM);
    SupPtrs sp;
    for (int i = 0; i < 4; ++i) sp.p[i] = i < n_supports ? supports[i] : nullptr;
    const size_t lds = 4 * kMaxNodes * kMaxNodes * sizeof(float);
    EEG_LAUNCH_P("hop_polys", hop_polys_kernel, dim3(n_graphs), dim3(round_up(N * N, 64)), lds, S_(stream), sp, n_supports, N, K, P_out);
    return check_launch("hop_polys");
}

size_t eeg_dcrnn_pack_floats(int Fin, int H, int M) { return make_cell_pack(Fin, H, M).total; }

int eeg_dcrnn_pack_cell(const float* Wg, const float* bg, const float* Wc, const float* bc, int Fin, int H, int M,
                        float* pack, void* stream) {
    if (!seq_h_supported(H)) return fail("pack_cell: rnn_units=%d unsupported", H);
    if (Fin < 4 || Fin % 4 != 0) return fail("pack_cell: input dim %d must be a positive multiple of 4", Fin);
    if (!seq_m_supported(M)) return fail("pack_cell: num hop matrices M=%d unsupported (1,2,3,4,5,7)", M);
    CellPack p = make_cell_pack(Fin, H, M);
    EEG_LAUNCH_P("pack_cell", pack_cell_kernel, dim3(512), dim3(256), 0, S_(stream), Wg, bg, Wc, bc, pack, p);
    return check_launch("pack_cell");
}
size_t eeg_dcrnn_pack3_halves(int Fin, int H, int M) { return pack3_supported(Fin, H, M) ? make_pack3(Fin, H, M).total : 0; }
int eeg_dcrnn_pack_cell_bf16x3(const float* Wg, const float* Wc, int Fin, int H, int M, uint16_t* pack3, void* stream) {
    if (!pack3_supported(Fin, H, M)) return fail("pack_cell_bf16x3: rnn_units=%d, input_dim=%d, %d hop matrices: the bf16 split exists for 64 units", H, Fin, M);
    if (Wg == nullptr || Wc == nullptr || pack3 == nullptr) return fail("pack_cell_bf16x3: null pointer");
    EEG_LAUNCH_P("pack_cell", pack_cell_bf3_kernel, dim3(512), dim3(256), 0, S_(stream), Wg, Wc, Fin, H, M, pack3);
    return check_launch("pack_cell_bf3");
}

int eeg_dcrnn_diffuse_fwd(const float* X, const float* P, int p_batched, int S, int B, int N, int F, int M,
                          float* planes, void* stream) {
    if (N < 1 || N > kMaxNodes || F < 4 || F % 4 != 0 || M < 1 || M > kMaxM) return fail("diffuse_fwd: bad dims N=%d F=%d M=%d", N, F, M);
    if (S < 1 || B < 1) return fail("diffuse_fwd: empty input (S=%d, B=%d)", S, B);
    return diffuse_fwd(X, P, p_batched, S, B, N, F, M, planes, S_(stream));
}
int eeg_dcrnn_diffuse_adj(const float* Z, const float* P, int p_batched, int S, int B, int N, int F, int M,
                          float* dX, void* stream) {
    if (N < 1 || N > kMaxNodes || F < 4 || F % 4 != 0 || M < 1 || M > kMaxM) return fail("diffuse_adj: bad dims N=%d F=%d M=%d", N, F, M);
    if (S < 1 || B < 1) return fail("diffuse_adj: empty input (S=%d, B=%d)", S, B);
    return diffuse_adj(Z, P, p_batched, S, B, N, F, M, dX, S_(stream));
}

// Size queries never fail and never fault: dims the compute entry would refuse (empty batch / sequence, zero widths) size to 0.
static bool layer_dims_positive(const eeg_layer_dims* d) {
    return d != nullptr && d->T >= 1 && d->B >= 1 && d->N >= 1 && d->H >= 1 && d->Fin >= 1 && d->M >= 1;
}
size_t eeg_dcrnn_layer_fwd_ws_floats(const eeg_layer_dims* d) {
    if (!layer_dims_positive(d)) return 0;
    const size_t xw = (size_t)d->T * d->B * d->N * 3 * d->H;
    return d->spectral != nullptr ? xw + (size_t)d->N * spec_rows(d->T * d->B) * 3 * d->H : xw;   // + Yh (N, Sp, 3H)
}

size_t eeg_dcrnn_spectral_basis_floats(int N) { return (N >= 1 && N <= kMaxNodes) ? (size_t)spec_basis_floats(N) : 0; }
size_t eeg_dcrnn_spectral_rows(size_t S) { return (S + 15) / 16 * 16; }
int eeg_dcrnn_spectral_basis(const float* support, int N, float* basis, void* stream) {
    if (N < 2 || N > kMaxNodes) return fail("spectral_basis: num_nodes=%d unsupported (2..%d)", N, kMaxNodes);
    if (support == nullptr || basis == nullptr) return fail("spectral_basis: null pointer");
    if (launch_spec_basis(support, N, basis, S_(stream))) return fail("spectral_basis: launch failed");
    return check_launch("spectral_basis");
}
size_t eeg_dcrnn_spectral_pack_floats(int Fin, int H, int M, int N) {
    return (Fin >= 4 && Fin % 4 == 0 && H == 64 && M >= 1 && M <= kMaxM && N >= 1 && N <= kMaxNodes) ? spec_pack_floats(Fin, H, M, N) : 0;
}
int eeg_dcrnn_pack_cell_spectral(const float* Wg, const float* Wc, const float* basis, int Fin, int H, int M, int N, float* spack,
                                 void* stream) {
    if (eeg_dcrnn_spectral_pack_floats(Fin, H, M, N) == 0)
        return fail("pack_cell_spectral: input_dim=%d rnn_units=%d hop matrices=%d nodes=%d: the spectral form exists for 64 units", Fin, H, M, N);
    if (Wg == nullptr || Wc == nullptr || basis == nullptr || spack == nullptr) return fail("pack_cell_spectral: null pointer");
    if (launch_spec_pack(Wg, Wc, basis, Fin, H, M, N, spack, S_(stream))) return fail("pack_cell_spectral: launch failed");
    return check_launch("pack_cell_spectral");
}
int eeg_dcrnn_pack_cells(int n_cells, const float* const* Wg, const float* const* bg, const float* const* Wc, const float* const* bc,
                         const int32_t* Fin, int H, int M, float* const* packs, const float* basis, int N, float* const* spacks,
                         void* stream) {
    if (n_cells < 1 || n_cells > 4) return fail("pack_cells: %d cells (1..4 per launch)", n_cells);
    if (Wg == nullptr || bg == nullptr || Wc == nullptr || bc == nullptr || Fin == nullptr || packs == nullptr) return fail("pack_cells: null pointer table");
    if (!seq_h_supported(H)) return fail("pack_cells: rnn_units=%d unsupported", H);
    if (!seq_m_supported(M)) return fail("pack_cells: num hop matrices M=%d unsupported (1,2,3,4,5,7)", M);
    if ((basis == nullptr) != (spacks == nullptr)) return fail("pack_cells: the per-frequency packs need the basis block and their output table");
    int fin[4];
    for (int c = 0; c < n_cells; ++c) {
        fin[c] = Fin[c];
        if (fin[c] < 4 || fin[c] % 4 != 0) return fail("pack_cells: input dim %d of cell %d must be a positive multiple of 4", fin[c], c);
        if (Wg[c] == nullptr || bg[c] == nullptr || Wc[c] == nullptr || bc[c] == nullptr || packs[c] == nullptr || (spacks != nullptr && spacks[c] == nullptr))
            return fail("pack_cells: null pointer in the tables of cell %d", c);
        if (spacks != nullptr && eeg_dcrnn_spectral_pack_floats(fin[c], H, M, N) == 0)
            return fail("pack_cells: input_dim=%d rnn_units=%d hop matrices=%d nodes=%d: the spectral form exists for 64 units", fin[c], H, M, N);
    }
    if (launch_pack_cells(n_cells, Wg, bg, Wc, bc, fin, H, M, packs, basis, N, spacks, S_(stream))) return fail("pack_cells: launch failed");
    return check_launch("pack_cells");
}
int eeg_dcrnn_spectral_ok(const eeg_layer_dims* d, int need_dx) {
    if (!layer_dims_positive(d) || d->p_batched) return 0;
    if (d->x_planes_ready && d->Fin != d->H) return 0;           // (a handed-over transformed input is the layer below's U^T h)
    if (check_dims(d->N, d->H, d->Fin, d->M)) return 0;
    return spec_supported(d->T, d->B, d->N, d->H, d->Fin, d->M, need_dx) ? 1 : 0;
}

int eeg_dcrnn_batch_major_ok(const eeg_layer_dims* d) {
    // the plan's own predicate, not a whole plan: a size query takes degenerate dims (Fin = 0) and plans no launch
    if (!diffuse_streams(diffuse_call(false, d->p_batched, d->T * d->B, d->B, d->N, d->Fin, d->M))) return 0;
    // 2: the GEMMs read the batch-major input through a row map (d->x_batch_major = 1, no copy); 1: only with the
    // time-major copy Xtm.  The rule is "the LDS-DMA kernel applies to both x-part GEMMs", NOT "both x-part plans succeed with a
    // row map": the quad kernels read a row map too, also where the DMA kernels do not apply, and Python keeps other tensors for
    // the backward by this answer.
    const int R = d->T * d->B * d->N;
    const GemmKnobs k = gemm_knobs();
    return (nn_dma_applies(d->Fin, R, 3 * d->H, k) && tn_dma_applies(d->Fin, 3 * d->H, k)) ? 2 : 1;
}

int eeg_dcrnn_layer_fwd(const eeg_layer_dims* d, const float* X, float* Xtm, const float* h0, const float* P,
                        const float* pack, float* planes, float* Hext, float* Rs, float* Us, float* Cs, float* RHs,
                        float* Hplanes, float* RHplanes, float* ws, void* stream) {
    if (check_dims(d->N, d->H, d->Fin, d->M)) return 1;
    if (d->T < 1 || d->B < 1) return fail("layer_fwd: empty sequence/batch (T=%d, B=%d)", d->T, d->B);
    const bool save = Rs != nullptr;
    if (save != (Us != nullptr) || save != (Cs != nullptr) || save != (RHs != nullptr))
        return fail("layer_fwd: Rs/Us/Cs/RHs must be all NULL or all non-NULL");
    hipStream_t st = S_(stream);
    const int S = d->T * d->B, R = S * d->N, H = d->H, M = d->M, Fin = d->Fin;
    const size_t state = (size_t)d->B * d->N * H;
    CellPack p = make_cell_pack(Fin, H, M);
    // slot 0 of Hext = initial state (h0 == NULL: the recurrent kernel clears it)
    if (h0 != nullptr && h0 != Hext && copy_floats(Hext, h0, state, st)) return 1;
    // 1. hoisted diffusion of the layer input: planes[m-1] = P_m X  (Xtm != NULL: X is batch-major and Xtm
    //    receives the time-major copy that everything after this point reads) -- unless the previous layer's
    //    recurrent kernel already left these planes behind (x_planes_ready)
    const size_t xs = d->x_plane_stride > 0 ? (size_t)d->x_plane_stride : (size_t)R * Fin;
    BtMap bt;
    if (d->x_batch_major) {
        if (Xtm != nullptr || d->x_planes_ready) return fail("layer_fwd: x_batch_major excludes Xtm and x_planes_ready");
        if (d->spectral == nullptr && eeg_dcrnn_batch_major_ok(d) != 2) return fail("layer_fwd: x_batch_major is not available for this shape (eeg_dcrnn_batch_major_ok)");
        bt.T = d->T; bt.B = d->B; bt.N = d->N;
    }
    float* XW = ws;
    if (d->spectral != nullptr) {
        // spectral form (shared symmetric support; spec_common.h): Xh = U^T X (node-major, time-major rows; kept in `planes` for the
        // backward, or handed over by the layer below: x_planes_ready), Yh_i = Xh_i Wt_i + csum_i * bias (grouped GEMM, K = Fin), and
        // the two-wave recurrent kernel takes Yh as it is (U Yh in its role B) and leaves U^T h / U^T (r*h) behind (Hplanes = Hh
        // (N, B + Sp, H), RHplanes = RHh (N, Sp, H)).  Where that kernel does not apply: XW = U Yh and the by-products as HBM passes.
        if (!eeg_dcrnn_spectral_ok(d, 0)) return fail("layer_fwd: the spectral form does not cover this shape (eeg_dcrnn_spectral_ok)");
        if (Xtm != nullptr || d->spack == nullptr) return fail("layer_fwd: spectral excludes Xtm and needs spack");
        if ((Hplanes != nullptr) != (RHplanes != nullptr)) return fail("layer_fwd: Hplanes/RHplanes must be both NULL or both non-NULL");
        const SpecPack sp = make_spec_pack(Fin, H, M, d->N);
        const int N = d->N, Sp = spec_rows(S), SpE = d->B + Sp;
        const size_t xgs = d->x_plane_stride > 0 ? (size_t)d->x_plane_stride : (size_t)Sp * Fin;
        float* Yh = ws + (size_t)R * 3 * H;
        if (!d->x_planes_ready && spec_mix(1, X, d->spectral, N, d->T, d->B, Fin, d->x_batch_major ? 1 : 0, planes, st, "spec_mix_x")) return 1;
        const SpecNnPlan nn = spec_nn_plan(Fin, Sp, N, sp.nct_x, num_cus(), spec_knobs());
        if (spec_plan_error("layer_fwd (spectral x-part)", nn.error)) return 1;
        const bool regs = nn.kind == SpecNnKind::Regs;       // the weights of a frequency row-major (sxr) or in the quad order (sxq)
        if (launch_spec_nn(nn, planes, xgs, Fin, Sp, N, d->spack + (regs ? sp.sxr : sp.sxq), regs ? sp.sxr_stride : sp.sxq_stride, Yh, st, "gemm_nn_xw",
                           pack + p.bias, d->spectral + spec_csum_offset(N))) return fail("gemm_nn (spectral): launch failed");
        SeqFwdArgs a{XW, h0 != nullptr ? Hext : nullptr, P, d->p_batched, pack + p.bhg, pack + p.bhc, Hext + state, Rs, Us, Cs, RHs, nullptr, nullptr,
                     (size_t)0, d->T, d->B, N, d->act, seq_probe_arg(st)};
        SeqCall call = seq_fwd_call(H, M, N, d->T, d->B, 0, a.probe);
        call.spectral = true; call.Sp = Sp; call.SpE = SpE;
        const SeqPlan plan = seq_fwd_plan(call);
        if (plan.kind == SeqKind::TwoWaveSpec) {   // the two-wave kernel in its SPEC instantiation: the mixes happen inside
            a.XW = Yh; a.Hpl = Hplanes; a.RHpl = RHplanes; a.spec_U = d->spectral; a.spec_Sp = Sp; a.spec_SpE = SpE;
            if (seq_fwd(H, M, plan, a, st)) return 1;
            if (Hplanes != nullptr) {
                if (launch_spec_zero_rows(Hplanes, N, (d->T + 1) * d->B, SpE, H, st)) return fail("spec_zero_rows: launch failed");
                if (launch_spec_zero_pad(RHplanes, N, S, H, st)) return fail("spec_zero_pad: launch failed");
            }
        } else {                                   // the mixes as separate passes
            if (spec_mix(0, Yh, d->spectral, N, d->T, d->B, 3 * H, 0, XW, st, "spec_mix_y")) return 1;
            if (seq_fwd(H, M, plan, a, st)) return 1;
            if (Hplanes != nullptr) {
                if (spec_mix(1, Hext, d->spectral, N, d->T + 1, d->B, H, 0, Hplanes, st, "spec_mix_h", SpE)) return 1;
                if (spec_mix(1, RHs, d->spectral, N, d->T, d->B, H, 0, RHplanes, st, "spec_mix_h")) return 1;
            }
        }
        return check_launch("layer_fwd (spectral)");
    } else if (d->x_planes_ready) {
        if (Xtm != nullptr) return fail("layer_fwd: x_planes_ready excludes a batch-major input");
    } else {
        if (diffuse_fwd(X, P, d->p_batched, S, d->B, d->N, Fin, M, planes, st, xs, d->x_batch_major ? 2 : (Xtm != nullptr ? 1 : 0), Xtm)) return 1;
        if (Xtm != nullptr) X = Xtm;
    }
    // 2. hoisted x-part GEMM: XW = [X | planes] @ Bx + [bg|bc]
    SegPtrs segs;
    for (int m = 0; m < kMaxM; ++m) segs.p[m] = m == 0 ? X : (m < M ? planes + (size_t)(m - 1) * xs : nullptr);
    const bool bf3 = d->pack3 != nullptr && pack3_supported(Fin, H, M);   // opt-in: three-term bf16 split (include/eeg_dcrnn.h, eeg_layer_dims.pack3)
    const Pack3 q = make_pack3(Fin, H, M);
    const NnCall cxw = nn_call(M, Fin, R, 3 * H / 16, 3 * H, 3 * H, bt, p.has_bxq, bf3 ? q.xw_nct : 0);
    if (gemm_nn(gemm_nn_plan(cxw), cxw, segs, NnRhs{pack + p.bx, pack + p.bxq, bf3 ? d->pack3 + q.xw : nullptr}, pack + p.bias, XW, st, "gemm_nn_xw", bt)) return 1;
    // 3. the recurrence
    if ((Hplanes != nullptr) != (RHplanes != nullptr)) return fail("layer_fwd: Hplanes/RHplanes must be both NULL or both non-NULL");
    SeqFwdArgs a{XW, h0 != nullptr ? Hext : nullptr, P, d->p_batched, pack + p.bhg, pack + p.bhc, Hext + state, Rs, Us, Cs, RHs, Hplanes, RHplanes,
                 (size_t)(d->T + 1) * state, d->T, d->B, d->N, d->act, seq_probe_arg(st)};
    return seq_fwd(H, M, seq_fwd_plan(seq_fwd_call(H, M, d->N, d->T, d->B, a.plane_stride, a.probe)), a, st);
}

size_t eeg_dcrnn_layer_bwd_ws_floats(const eeg_layer_dims* d, int need_dx) { return layer_dims_positive(d) ? bwd_ws(d, need_dx).total : 0; }

int eeg_dcrnn_layer_bwd(const eeg_layer_dims* d, const float* X, const float* P, const float* pack,
                        const float* planes, const float* Hext, const float* Rs, const float* Us, const float* Cs,
                        const float* RHs, const float* Hplanes, const float* RHplanes, const float* dHseq,
                        const float* d_at_end, const float* d_at_len,
                        const int64_t* lengths, float* dX, float* dh0, float* dWg, float* dbg, float* dWc,
                        float* dbc, float* ws, void* stream) {
    if (check_dims(d->N, d->H, d->Fin, d->M)) return 1;
    if (d->T < 1 || d->B < 1) return fail("layer_bwd: empty sequence/batch (T=%d, B=%d)", d->T, d->B);
    hipStream_t st = S_(stream);
    const int S = d->T * d->B, R = S * d->N, H = d->H, M = d->M, Fin = d->Fin, N = d->N;
    const size_t state = (size_t)d->B * N * H;
    CellPack p = make_cell_pack(Fin, H, M);
    BwdWs w = bwd_ws(d, dX != nullptr);
    float* dXW = ws + w.dxw;
    float* dbias = ws + w.dbias;
    // 1. BPTT through the recurrence: dXW = [dR|dU|dC] per step, dh0, per-clip bias partials
    SeqBwdArgs a{Hext + state, Hext, Rs, Us, Cs, dHseq, d_at_end, d_at_len,
                 reinterpret_cast<const long long*>(lengths), P, d->p_batched, pack + p.b1, pack + p.b2,
                 dXW, dh0, dbias, d->T, d->B, N, d->act, seq_probe_arg(st)};
    SeqCall call = seq_bwd_call(H, M, N, d->T, d->B, a.probe);
    call.spectral = d->spectral != nullptr; call.Sp = spec_rows(S); call.SpE = d->B + spec_rows(S);
    const SeqPlan plan = seq_bwd_plan(call);
    const bool dyh_done = plan.kind == SeqKind::TwoWaveSpec;   // spectral form: the two-wave BPTT kernel writes dYh = U^T dXW itself
    if (dyh_done) { a.spec_U = d->spectral; a.dYh = ws + w.dyh; a.spec_Sp = call.Sp; }
    if (seq_bwd(H, M, plan, a, st)) return 1;
    // 2. weight gradients (hoisted, split-K with fixed-order reduction); the bias sums ride in their reduction launch
    const size_t xs = d->x_plane_stride > 0 ? (size_t)d->x_plane_stride : (size_t)R * Fin;
    BtMap bt;
    if (d->x_batch_major) {
        if (d->spectral == nullptr && eeg_dcrnn_batch_major_ok(d) != 2) return fail("layer_bwd: x_batch_major is not available for this shape");
        bt.T = d->T; bt.B = d->B; bt.N = N;
    }
    if (d->spectral != nullptr) {
        // spectral form: dYh = U^T dXW (node-major, time-major rows; written by the two-wave BPTT kernel itself where it runs),
        // dWt_i = Xh_i^T dYh_i etc. folded into dW_m by the reduction, dX = U [dYh_i Wt_i^T]_i
        if (!eeg_dcrnn_spectral_ok(d, dX != nullptr)) return fail("layer_bwd: the spectral form does not cover this shape (eeg_dcrnn_spectral_ok)");
        if (d->spack == nullptr) return fail("layer_bwd: spectral needs spack");
        if ((Hplanes != nullptr) != (RHplanes != nullptr)) return fail("layer_bwd: Hplanes/RHplanes must be both NULL or both non-NULL");
        const SpecPack sp = make_spec_pack(Fin, H, M, N);
        const int Sp = spec_rows(S), SpE = d->B + Sp;
        float* dYh = ws + w.dyh;
        if (dyh_done) {
            if (launch_spec_zero_pad(dYh, N, S, 3 * H, st)) return fail("spec_zero_pad: launch failed");
        } else if (spec_mix(1, dXW, d->spectral, N, d->T, d->B, 3 * H, 0, dYh, st, "spec_mix_dy")) return 1;
        const float *hh = Hplanes, *rhh = RHplanes;
        size_t hh_gs = (size_t)SpE * H;
        if (hh == nullptr) {                        // no by-products from the forward: U^T h_{t-1}, U^T (r*h_{t-1}) here
            if (spec_mix(1, Hext, d->spectral, N, d->T, d->B, H, 0, ws + w.hplanes, st, "spec_mix_h")) return 1;
            if (spec_mix(1, RHs, d->spectral, N, d->T, d->B, H, 0, ws + w.rhplanes, st, "spec_mix_h")) return 1;
            hh = ws + w.hplanes; rhh = ws + w.rhplanes; hh_gs = 0;
        }
        if (cell_weight_grads_spectral(d, planes, xs_spec(d), hh, hh_gs, rhh, dYh, ws + w.partial, w, dWg, dWc, st, dbias, dbg, dbc)) return 1;
        if (dX != nullptr) {
            // one kernel (GEMM over K = 3H + the node mix back) where it applies, else the grouped GEMM and the mix as passes
            const SpecDxPlan dx = spec_dx_plan(Fin, N, d->T, d->B, num_cus(), spec_knobs());
            if (spec_plan_error("layer_bwd (spectral dX)", dx.error)) return 1;
            if (dx.kind == SpecDxKind::Fused) {
                if (launch_dxf(dx, dYh, Sp, S, N, d->spack + sp.sxtq, sp.sxtq_stride, d->spectral, dX, st, "gemm_dx_f")) return fail("gemm_dxf: launch failed");
            } else {
                float* dXh = ws + w.z;
                if (launch_spec_nn(dx.nn, dYh, 0, 3 * H, Sp, N, d->spack + sp.sxtq, sp.sxtq_stride, dXh, st, "gemm_nn_dx")) return fail("gemm_nng: launch failed");
                if (launch_spec_mix(dx.mix, dXh, d->spectral, N, d->T, d->B, Fin, 0, dX, st, "spec_mix_dx")) return fail("spec_mix: launch failed");
            }
        }
        return check_launch("layer_bwd (spectral)");
    }
    if (cell_weight_grads(d, X, planes, xs, Hext, RHs, dXW, P, Hplanes, RHplanes, (size_t)(d->T + 1) * state,
                          ws + w.hplanes, ws + w.rhplanes, ws + w.partial, w, false, dWg, dWc, st, bt, dbias, dbg, dbc)) return 1;
    // 3. gradient w.r.t. the layer input: Z = dXW @ Bx^T, dX = Z_0 + sum_m P_m^T Z_m
    if (dX != nullptr) {
        float* Z = ws + w.z;
        SegPtrs sd;
        for (int m = 0; m < kMaxM; ++m) sd.p[m] = m == 0 ? dXW : nullptr;
        const bool bf3 = d->pack3 != nullptr && pack3_supported(Fin, H, M);      // opt-in: three-term bf16 split
        const Pack3 q = make_pack3(Fin, H, M);
        const NnCall cdx = nn_call(1, 3 * H, R, round_up(M * Fin, 16) / 16, M * Fin, M * Fin, BtMap(), p.has_bxtq, bf3 ? q.dx_nct : 0);
        if (gemm_nn(gemm_nn_plan(cdx), cdx, sd, NnRhs{pack + p.bxt, pack + p.bxtq, bf3 ? d->pack3 + q.dx : nullptr}, nullptr, Z, st, "gemm_nn_dx")) return 1;
        if (diffuse_adj(Z, P, d->p_batched, S, d->B, N, Fin, M, dX, st)) return 1;
    }
    return 0;
}


/* ---- input featurisation -------------------------------------------------------------------------- */
// lengths == nullptr: the plain kernels (every window transformed); else their length-aware variants
static int fft_features(const float* raw, int B, int N, int T, int W, const int32_t* perm, const float* log_scale, float mean, float std_,
                        const int64_t* lengths, float pad_val, float* feat_raw, float* feat_std, void* stream) {
    const long long* len = reinterpret_cast<const long long*>(lengths);
    if (B < 1 || N < 1 || T < 1) return fail("fft_features: empty input (B=%d, N=%d, T=%d)", B, N, T);
    if (W < 4 || W % 4 != 0 || W / 4 + 1 > 64) return fail("fft_features: window=%d unsupported (multiple of 4, <= 252)", W);
    if (feat_raw == nullptr && feat_std == nullptr) return fail("fft_features: no output requested");
    if (feat_std != nullptr && !(std_ != 0.f)) return fail("fft_features: std must be non-zero");
    if (W == kFftWin) {                               // the reference's 200-sample steps: mixed-radix transform, 6 windows per wave
        const long long n_windows = (long long)B * N * T;
        const long long n_items = (n_windows + kFftPerWave - 1) / kFftPerWave;
        long long blocks = (n_items + 3) / 4;
        const long long cap = (long long)platform_num_cus() * kFftWgPerCu;  // workgroups of 4 waves per CU the kernel's registers allow, persistent
        if (blocks > cap) blocks = cap;
        const size_t lds = 4 * (size_t)kFftWaveDoubles * sizeof(double);
        if (len == nullptr) {
            EEG_SET_MAX_LDS(fft200_features_kernel<false>, lds);
            EEG_LAUNCH_P("fft_features", fft200_features_kernel<false>, dim3((unsigned)blocks), dim3(256), lds, S_(stream), raw, N, T, n_windows,
                         reinterpret_cast<const int*>(perm), log_scale, mean, 1.0f / std_, feat_raw, feat_std, len, 0.f);
        } else {
            EEG_SET_MAX_LDS(fft200_features_kernel<true>, lds);
            EEG_LAUNCH_P("fft_features_len", fft200_features_kernel<true>, dim3((unsigned)blocks), dim3(256), lds, S_(stream), raw, N, T, n_windows,
                         reinterpret_cast<const int*>(perm), log_scale, mean, 1.0f / std_, feat_raw, feat_std, len, pad_val);
        }
        return check_launch("fft_features");
    }
    int tchunk = T;                                   // ~8 waves per SIMD in total
    while (tchunk > 1 && (long long)B * N * ceil_div(T, tchunk) < 8192) tchunk = ceil_div(tchunk, 2);
    if (len == nullptr)
        EEG_LAUNCH_P("fft_features", fft_features_kernel<false>, dim3(B * N, ceil_div(T, tchunk)), dim3(64), (size_t)W * sizeof(double), S_(stream),
                     raw, N, T, W, tchunk, reinterpret_cast<const int*>(perm), log_scale, mean, 1.0f / std_, feat_raw, feat_std, len, 0.f);
    else
        EEG_LAUNCH_P("fft_features_len", fft_features_kernel<true>, dim3(B * N, ceil_div(T, tchunk)), dim3(64), (size_t)W * sizeof(double), S_(stream),
                     raw, N, T, W, tchunk, reinterpret_cast<const int*>(perm), log_scale, mean, 1.0f / std_, feat_raw, feat_std, len, pad_val);
    return check_launch("fft_features");
}

int eeg_dcrnn_fft_features(const float* raw, int B, int N, int T, int W, const int32_t* perm, const float* log_scale,
                           float mean, float std_, float* feat_raw, float* feat_std, void* stream) {
    return fft_features(raw, B, N, T, W, perm, log_scale, mean, std_, nullptr, 0.f, feat_raw, feat_std, stream);
}

int eeg_dcrnn_fft_features_len(const float* raw, int B, int N, int T, int W, const int32_t* perm, const float* log_scale, float mean,
                               float std_, const int64_t* lengths, float pad_val, float* feat_raw, float* feat_std, void* stream) {
    if (raw == nullptr || lengths == nullptr) return fail("fft_features_len: null input / lengths");
    return fft_features(raw, B, N, T, W, perm, log_scale, mean, std_, lengths, pad_val, feat_raw, feat_std, stream);
}

int eeg_dcrnn_fft_features_pair(const float* raw_x, const float* raw_y, int B, int N, int Tx, int Ty, int W, const int32_t* perm,
                                const float* log_scale, float mean, float std_, float* feat_raw_x, float* x_std, float* y_std,
                                void* stream) {
    if (raw_x == nullptr || raw_y == nullptr) return fail("fft_features_pair: null input (raw_x=%p, raw_y=%p)", (const void*)raw_x, (const void*)raw_y);
    if (B < 1 || N < 1 || Tx < 1 || Ty < 1) return fail("fft_features_pair: empty input (B=%d, N=%d, Tx=%d, Ty=%d)", B, N, Tx, Ty);
    if (W < 4 || W % 4 != 0 || W / 4 + 1 > 64) return fail("fft_features_pair: window=%d unsupported (multiple of 4, <= 252)", W);
    if (x_std == nullptr || y_std == nullptr)
        return fail("fft_features_pair: null output (x_std=%p, y_std=%p): the pair is the standardised input and target", (void*)x_std, (void*)y_std);
    if (!(std_ != 0.f)) return fail("fft_features_pair: std must be non-zero");
    if (W != kFftWin) {                               // no paired kernel for a window nobody trains with: the general kernel, once per half
        if (eeg_dcrnn_fft_features(raw_x, B, N, Tx, W, perm, log_scale, mean, std_, feat_raw_x, x_std, stream)) return 1;
        return eeg_dcrnn_fft_features(raw_y, B, N, Ty, W, perm, log_scale, mean, std_, nullptr, y_std, stream);
    }
    const FftHalf hx = {raw_x, Tx, (long long)B * N * Tx, feat_raw_x, x_std}, hy = {raw_y, Ty, (long long)B * N * Ty, nullptr, y_std};
    const long long n_items = (hx.n_windows + kFftPerWave - 1) / kFftPerWave + (hy.n_windows + kFftPerWave - 1) / kFftPerWave;
    long long blocks = (n_items + 3) / 4;
    const long long cap = (long long)platform_num_cus() * kFftWgPerCu;      // persistent, as the single-buffer launch
    if (blocks > cap) blocks = cap;
    const size_t lds = 4 * (size_t)kFftWaveDoubles * sizeof(double);
    EEG_SET_MAX_LDS(fft200_features_pair_kernel, lds);
    EEG_LAUNCH_P("fft_features_pair", fft200_features_pair_kernel, dim3((unsigned)blocks), dim3(256), lds, S_(stream), hx, hy, N,
                 reinterpret_cast<const int*>(perm), log_scale, mean, 1.0f / std_);
    return check_launch("fft_features_pair");
}

int eeg_dcrnn_augment_features(const float* x, const float* y, int B, int Tx, int Ty, int N, int D, const int32_t* perm, const float* shift,
                               float* x_out, float* y_out, void* stream) {
    if (x == nullptr || y == nullptr || perm == nullptr || shift == nullptr) return fail("augment_features: null input / perm / shift");
    if (x_out == nullptr || y_out == nullptr) return fail("augment_features: null output (x_out=%p, y_out=%p)", (void*)x_out, (void*)y_out);
    if (x_out == x || y_out == y) return fail("augment_features: in-place call (rows move between nodes: outputs must not alias inputs)");
    if (B < 1 || N < 1 || Tx < 1 || Ty < 1) return fail("augment_features: empty input (B=%d, N=%d, Tx=%d, Ty=%d)", B, N, Tx, Ty);
    if (D < 4 || D % 4 != 0) return fail("augment_features: feature dim=%d unsupported (positive multiple of 4)", D);
    if ((((uintptr_t)x | (uintptr_t)y | (uintptr_t)x_out | (uintptr_t)y_out) & 15) != 0) return fail("augment_features: tensors must be 16-byte aligned");
    const long long pieces = (long long)(Tx + Ty) * N * (D / 4);            // 16-byte pieces per clip
    const long long chunks = (pieces + kAugPerBlock - 1) / kAugPerBlock;
    if (chunks > 65535) return fail("augment_features: %lld values per clip exceed one launch (limit %lld)", 4 * pieces, 4LL * 65535 * kAugPerBlock);
    const dim3 grid((unsigned)B, (unsigned)chunks);
    if (D == 100)
        EEG_LAUNCH_P("augment_features", augment_features_kernel<25>, grid, dim3(kAugThreads), 0, S_(stream), x, y, N, Tx, Ty, D / 4,
                     reinterpret_cast<const int*>(perm), shift, x_out, y_out);
    else
        EEG_LAUNCH_P("augment_features", augment_features_kernel<0>, grid, dim3(kAugThreads), 0, S_(stream), x, y, N, Tx, Ty, D / 4,
                     reinterpret_cast<const int*>(perm), shift, x_out, y_out);
    return check_launch("augment_features");
}

/* ---- time-domain inputs: windows of the raw signals, multiplicative augmentation -------------------- */
// one launch of window_stream_kernel over x (and y when Ty > 0); `what` names the entry point in refusals
static int window_stream(const char* what, bool raw, const float* x, const float* y, int B, int Tx, int Ty, int N, int W, const int32_t* perm,
                         const float* a, const float* c, float mean, float std_, float* x_out, float* y_out, void* stream,
                         const int64_t* lengths = nullptr, float pad_val = 0.f) {
    if (B < 1 || N < 1 || Tx < 1 || Ty < 0) return fail("%s: empty input (B=%d, N=%d, Tx=%d, Ty=%d)", what, B, N, Tx, Ty);
    if (W < 4 || W % 4 != 0) return fail("%s: window=%d unsupported (positive multiple of 4)", what, W);
    if (x_out == x || (Ty > 0 && y_out == y)) return fail("%s: in-place call (rows move between nodes: outputs must not alias inputs)", what);
    if ((((uintptr_t)x | (uintptr_t)y | (uintptr_t)x_out | (uintptr_t)y_out) & 15) != 0) return fail("%s: tensors must be 16-byte aligned", what);
    const long long pieces = (long long)(Tx + Ty) * N * (W / 4);            // 16-byte pieces per clip
    const long long chunks = (pieces + kAugPerBlock - 1) / kAugPerBlock;
    if (chunks > 65535) return fail("%s: %lld values per clip exceed one launch (limit %lld)", what, 4 * pieces, 4LL * 65535 * kAugPerBlock);
    const dim3 grid((unsigned)B, (unsigned)chunks);
    const int* pm = reinterpret_cast<const int*>(perm);
    const long long* len = reinterpret_cast<const long long*>(lengths);
#define EEG_WSTREAM(RAW, D4C) \
    EEG_LAUNCH_P(what, (window_stream_kernel<RAW, D4C>), grid, dim3(kAugThreads), 0, S_(stream), x, y, N, Tx, Ty, W / 4, pm, a, c, mean, std_, x_out, y_out, \
                 len, 0.f)
#define EEG_WSTREAM_LEN(D4C)                                                                                                            \
    EEG_LAUNCH_P(what, (window_stream_kernel<true, D4C, true>), grid, dim3(kAugThreads), 0, S_(stream), x, y, N, Tx, Ty, W / 4, pm, a, c, mean, \
                 std_, x_out, y_out, len, pad_val)
    if (lengths != nullptr) {                         // raw signals of ONE clip per sample (the callers see to that): the padded variant
        if (W == 200) EEG_WSTREAM_LEN(50); else EEG_WSTREAM_LEN(0);
    } else if (raw) { if (W == 200) EEG_WSTREAM(true, 50); else EEG_WSTREAM(true, 0); }
    else { if (W == 200) EEG_WSTREAM(false, 50); else EEG_WSTREAM(false, 0); }
#undef EEG_WSTREAM_LEN
#undef EEG_WSTREAM
    return check_launch(what);
}

int eeg_dcrnn_window_features(const float* raw, int B, int N, int T, int W, const int32_t* perm, const float* scale, float mean, float std_,
                              float* x_std, void* stream) {
    if (raw == nullptr) return fail("window_features: null input");
    if (x_std == nullptr) return fail("window_features: null output");
    if (!(std_ != 0.f)) return fail("window_features: std must be non-zero");
    return window_stream("window_features", true, raw, nullptr, B, T, 0, N, W, perm, scale, nullptr, mean, std_, x_std, nullptr, stream);
}

int eeg_dcrnn_window_features_len(const float* raw, int B, int N, int T, int W, const int32_t* perm, const float* scale, float mean,
                                  float std_, const int64_t* lengths, float pad_val, float* x_std, void* stream) {
    if (raw == nullptr || lengths == nullptr) return fail("window_features_len: null input / lengths");
    if (x_std == nullptr) return fail("window_features_len: null output");
    if (!(std_ != 0.f)) return fail("window_features_len: std must be non-zero");
    return window_stream("window_features_len", true, raw, nullptr, B, T, 0, N, W, perm, scale, nullptr, mean, std_, x_std, nullptr, stream,
                         lengths, pad_val);
}

int eeg_dcrnn_window_features_pair(const float* raw_x, const float* raw_y, int B, int N, int Tx, int Ty, int W, const int32_t* perm,
                                   const float* scale, float mean, float std_, float* x_std, float* y_std, void* stream) {
    if (raw_x == nullptr || raw_y == nullptr)
        return fail("window_features_pair: null input (raw_x=%p, raw_y=%p)", (const void*)raw_x, (const void*)raw_y);
    if (x_std == nullptr || y_std == nullptr)
        return fail("window_features_pair: null output (x_std=%p, y_std=%p): the pair is the standardised input and target", (void*)x_std, (void*)y_std);
    if (Ty < 1) return fail("window_features_pair: empty input (B=%d, N=%d, Tx=%d, Ty=%d)", B, N, Tx, Ty);
    if (!(std_ != 0.f)) return fail("window_features_pair: std must be non-zero");
    return window_stream("window_features_pair", true, raw_x, raw_y, B, Tx, Ty, N, W, perm, scale, nullptr, mean, std_, x_std, y_std, stream);
}

int eeg_dcrnn_augment_windows(const float* x, const float* y, int B, int Tx, int Ty, int N, int D, const int32_t* perm, const float* a,
                              const float* c, float* x_out, float* y_out, void* stream) {
    if (x == nullptr || perm == nullptr || a == nullptr || c == nullptr) return fail("augment_windows: null input / perm / factors");
    if ((y == nullptr) != (Ty == 0)) return fail("augment_windows: target and Ty=%d disagree (no target: y = NULL and Ty = 0)", Ty);
    if (x_out == nullptr || (y != nullptr && y_out == nullptr)) return fail("augment_windows: null output (x_out=%p, y_out=%p)", (void*)x_out, (void*)y_out);
    return window_stream("augment_windows", false, x, y, B, Tx, Ty, N, D, perm, a, c, 0.f, 1.f, x_out, y_out, stream);
}

/* ---- epochs from a device-resident data set: shuffle keys, batch gather ------------------------------- */
int eeg_dcrnn_epoch_keys(uint64_t seed, int64_t epoch, int64_t P, int64_t* keys, void* stream) {
    if (keys == nullptr) return fail("epoch_keys: null output");
    if (P < 1) return fail("epoch_keys: P=%lld clips (P >= 1)", (long long)P);
    if (epoch < 0 || epoch > 0x7fffffffLL) return fail("epoch_keys: epoch=%lld outside 0..2^31-1", (long long)epoch);
    long long blocks = (P + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    EEG_LAUNCH_P("epoch_keys", epoch_keys_kernel, dim3((unsigned)blocks), dim3(256), 0, S_(stream), (unsigned long long)seed, (unsigned)epoch,
                 (long long)P, reinterpret_cast<long long*>(keys));
    return check_launch("epoch_keys");
}

// clip_w != nullptr: the validity gather (eeg_dcrnn_gather_clips_tail), else the plain one -- the same checks, the same two launches
static int gather_clips_launch(const float* x_pool, float* x_out, size_t x_row_bytes, const float* y_pool, float* y_out, size_t y_row_bytes,
                               const void* label_pool, void* label_out, int label_bytes, const int64_t* len_pool, int64_t* len_out,
                               const int64_t* perm, int64_t n_perm, int64_t P, int64_t* cursor, int B, int rank, int world, float* clip_w,
                               float* denom, int64_t* n_valid, void* stream) {
    if (x_pool == nullptr || x_out == nullptr) return fail("gather_clips: null x_pool / x_out");
    if (perm == nullptr || cursor == nullptr) return fail("gather_clips: null perm / cursor");
    if ((y_pool == nullptr) != (y_out == nullptr) || (y_pool == nullptr) != (y_row_bytes == 0))
        return fail("gather_clips: y_pool, y_out and y_row_bytes=%zu disagree (no second wide tensor: NULL, NULL, 0)", y_row_bytes);
    if ((label_pool == nullptr) != (label_out == nullptr) || (label_pool == nullptr) != (label_bytes == 0))
        return fail("gather_clips: label_pool, label_out and label_bytes=%d disagree (no label: NULL, NULL, 0)", label_bytes);
    if (label_bytes != 0 && label_bytes != 4 && label_bytes != 8) return fail("gather_clips: label_bytes=%d unsupported (4: float, 8: int64)", label_bytes);
    if ((len_pool == nullptr) != (len_out == nullptr)) return fail("gather_clips: len_pool and len_out disagree (no lengths: both NULL)");
    if (B < 1 || world < 1 || rank < 0 || rank >= world) return fail("gather_clips: B=%d, rank=%d, world=%d unsupported (B >= 1, 0 <= rank < world)", B, rank, world);
    if (P < 1 || n_perm < 1) return fail("gather_clips: P=%lld clips, n_perm=%lld entries (both >= 1)", (long long)P, (long long)n_perm);
    if ((long long)B * world > (long long)n_perm)
        return fail("gather_clips: B*world=%lld clips per step exceed the %lld entries of perm", (long long)B * world, (long long)n_perm);
    // a clip row of a wide tensor: whole 16-byte pieces, 16-byte aligned, inside one buffer descriptor and one launch
    constexpr size_t kMaxRow = (size_t)65535 * kAugPerBlock * 16;
    if (x_row_bytes < 16 || x_row_bytes % 16 != 0 || x_row_bytes > kMaxRow)
        return fail("gather_clips: x_row_bytes=%zu unsupported (a positive multiple of 16, at most %zu)", x_row_bytes, kMaxRow);
    if (y_row_bytes % 16 != 0 || y_row_bytes > kMaxRow)
        return fail("gather_clips: y_row_bytes=%zu unsupported (a multiple of 16, at most %zu)", y_row_bytes, kMaxRow);
    if ((((uintptr_t)x_pool | (uintptr_t)x_out | (uintptr_t)y_pool | (uintptr_t)y_out) & 15) != 0) return fail("gather_clips: wide tensors must be 16-byte aligned");
    if ((((uintptr_t)label_pool | (uintptr_t)label_out) & (uintptr_t)(label_bytes == 8 ? 7 : 3)) != 0 ||
        (((uintptr_t)len_pool | (uintptr_t)len_out | (uintptr_t)perm | (uintptr_t)cursor) & 7) != 0)
        return fail("gather_clips: labels / lengths / perm / cursor must be aligned to their element size");
    if (x_out == x_pool || (y_out != nullptr && y_out == y_pool)) return fail("gather_clips: in-place call (the batch tensors must not alias the pools)");
    GatherWide w0{x_pool, x_out, (unsigned)(x_row_bytes / 16), 0u}, w1{y_pool, y_out, (unsigned)(y_row_bytes / 16), 0u};
    w0.chunks = (w0.pieces + kAugPerBlock - 1) / kAugPerBlock;
    w1.chunks = (w1.pieces + kAugPerBlock - 1) / kAugPerBlock;
    if (w0.chunks + w1.chunks > 65535u) return fail("gather_clips: %zu + %zu bytes per clip exceed one launch", x_row_bytes, y_row_bytes);
    if (clip_w == nullptr) {
        EEG_LAUNCH_P("gather_clips", gather_clips_kernel, dim3((unsigned)B, w0.chunks + w1.chunks), dim3(kAugThreads), 0, S_(stream), w0, w1, label_pool,
                     label_out, label_bytes, reinterpret_cast<const long long*>(len_pool), reinterpret_cast<long long*>(len_out),
                     reinterpret_cast<const long long*>(perm), (long long)n_perm, (long long)P, reinterpret_cast<const long long*>(cursor),
                     (long long)rank * B);
    } else {
        EEG_LAUNCH_P("gather_clips", gather_clips_tail_kernel, dim3((unsigned)B, w0.chunks + w1.chunks), dim3(kAugThreads), 0, S_(stream), w0, w1,
                     label_pool, label_out, label_bytes, reinterpret_cast<const long long*>(len_pool), reinterpret_cast<long long*>(len_out),
                     reinterpret_cast<const long long*>(perm), (long long)n_perm, (long long)P, reinterpret_cast<const long long*>(cursor),
                     (long long)rank * B, (long long)B * world, world, clip_w, denom, reinterpret_cast<long long*>(n_valid));
    }
    if (int rc = check_launch("gather_clips")) return rc;
    EEG_LAUNCH_P("gather_clips_cursor", cursor_advance_kernel, dim3(1), dim3(64), 0, S_(stream), reinterpret_cast<long long*>(cursor), (long long)B * world);
    return check_launch("gather_clips_cursor");
}
int eeg_dcrnn_gather_clips(const float* x_pool, float* x_out, size_t x_row_bytes, const float* y_pool, float* y_out, size_t y_row_bytes,
                           const void* label_pool, void* label_out, int label_bytes, const int64_t* len_pool, int64_t* len_out,
                           const int64_t* perm, int64_t n_perm, int64_t P, int64_t* cursor, int B, int rank, int world, void* stream) {
    return gather_clips_launch(x_pool, x_out, x_row_bytes, y_pool, y_out, y_row_bytes, label_pool, label_out, label_bytes, len_pool, len_out, perm,
                               n_perm, P, cursor, B, rank, world, nullptr, nullptr, nullptr, stream);
}
int eeg_dcrnn_gather_clips_tail(const float* x_pool, float* x_out, size_t x_row_bytes, const float* y_pool, float* y_out, size_t y_row_bytes,
                                const void* label_pool, void* label_out, int label_bytes, const int64_t* len_pool, int64_t* len_out,
                                const int64_t* perm, int64_t n_perm, int64_t P, int64_t* cursor, int B, int rank, int world, float* clip_w,
                                float* denom, int64_t* n_valid, void* stream) {
    if (clip_w == nullptr || denom == nullptr || n_valid == nullptr) return fail("gather_clips_tail: null clip_w / denom / n_valid");
    if ((((uintptr_t)clip_w | (uintptr_t)denom) & 3) != 0 || ((uintptr_t)n_valid & 7) != 0)
        return fail("gather_clips_tail: clip_w / denom / n_valid must be aligned to their element size");
    return gather_clips_launch(x_pool, x_out, x_row_bytes, y_pool, y_out, y_row_bytes, label_pool, label_out, label_bytes, len_pool, len_out, perm,
                               n_perm, P, cursor, B, rank, world, clip_w, denom, n_valid, stream);
}

/* ---- clips cut out of device-resident recordings through a device clip table ------------------------- */
int eeg_dcrnn_gather_records(const float* signals, int64_t signal_floats, const int64_t* rec_table, int64_t R, const int64_t* clip_table, int64_t P,
                             const void* label_pool, void* label_out, int label_bytes, const int64_t* perm, int64_t n_perm, int64_t* cursor, int B,
                             int rank, int world, int N, int window, int64_t x_len, int64_t y_len, float* x_out, float* y_out, int64_t* len_out,
                             float* clip_w, float* denom, int64_t* n_valid, void* stream) {
    if (signals == nullptr || rec_table == nullptr || clip_table == nullptr) return fail("gather_records: null signals / rec_table / clip_table");
    if (x_out == nullptr) return fail("gather_records: null x_out");
    if (perm == nullptr || cursor == nullptr) return fail("gather_records: null perm / cursor");
    if ((y_out == nullptr) != (y_len == 0)) return fail("gather_records: y_out and y_len=%lld disagree (no target: NULL, 0)", (long long)y_len);
    if ((label_pool == nullptr) != (label_out == nullptr) || (label_pool == nullptr) != (label_bytes == 0))
        return fail("gather_records: label_pool, label_out and label_bytes=%d disagree (no label: NULL, NULL, 0)", label_bytes);
    if (label_bytes != 0 && label_bytes != 4 && label_bytes != 8) return fail("gather_records: label_bytes=%d unsupported (4: float, 8: int64)", label_bytes);
    if ((clip_w == nullptr) != (denom == nullptr) || (clip_w == nullptr) != (n_valid == nullptr))
        return fail("gather_records: clip_w, denom and n_valid come together (the plain form: all three NULL)");
    if (B < 1 || world < 1 || rank < 0 || rank >= world) return fail("gather_records: B=%d, rank=%d, world=%d unsupported (B >= 1, 0 <= rank < world)", B, rank, world);
    if (P < 1 || n_perm < 1 || R < 1) return fail("gather_records: P=%lld clips, n_perm=%lld entries, R=%lld recordings (all >= 1)", (long long)P, (long long)n_perm, (long long)R);
    if ((long long)B * world > (long long)n_perm)
        return fail("gather_records: B*world=%lld clips per step exceed the %lld entries of perm", (long long)B * world, (long long)n_perm);
    if (N < 1) return fail("gather_records: N=%d channels (N >= 1)", N);
    if (window < 4 || window % 4 != 0) return fail("gather_records: window=%d unsupported (a positive multiple of 4: rows of whole 16-byte pieces)", window);
    // a channel row of a batch tensor: whole steps, inside one buffer descriptor (its byte count is 32 bits wide)
    constexpr int64_t kMaxRow = (int64_t)1 << 28;
    if (x_len < window || x_len % window != 0 || x_len > kMaxRow)
        return fail("gather_records: x_len=%lld unsupported (a positive multiple of window=%d, at most %lld)", (long long)x_len, window, (long long)kMaxRow);
    if (y_len < 0 || y_len % window != 0 || y_len > kMaxRow)
        return fail("gather_records: y_len=%lld unsupported (a multiple of window=%d, at most %lld)", (long long)y_len, window, (long long)kMaxRow);
    if (signal_floats < 4 || signal_floats % 4 != 0 || signal_floats >= ((int64_t)1 << 60))
        return fail("gather_records: signal_floats=%lld unsupported (a positive multiple of 4: whole 16-byte pieces)", (long long)signal_floats);
    if ((((uintptr_t)signals | (uintptr_t)x_out | (uintptr_t)y_out) & 15) != 0) return fail("gather_records: signals, x_out and y_out must be 16-byte aligned");
    if ((((uintptr_t)label_pool | (uintptr_t)label_out) & (uintptr_t)(label_bytes == 8 ? 7 : 3)) != 0 ||
        (((uintptr_t)rec_table | (uintptr_t)clip_table | (uintptr_t)len_out | (uintptr_t)perm | (uintptr_t)cursor | (uintptr_t)n_valid) & 7) != 0 ||
        (((uintptr_t)clip_w | (uintptr_t)denom) & 3) != 0)
        return fail("gather_records: tables / labels / lengths / perm / cursor / clip_w / denom / n_valid must be aligned to their element size");
    const uintptr_t s0 = (uintptr_t)signals, s1 = s0 + (uintptr_t)signal_floats * 4;
    const uintptr_t x0 = (uintptr_t)x_out, x1 = x0 + (uintptr_t)B * N * (uintptr_t)x_len * 4;
    const uintptr_t y0 = (uintptr_t)y_out, y1 = y0 + (uintptr_t)B * N * (uintptr_t)y_len * 4;
    if ((x0 < s1 && s0 < x1) || (y_out != nullptr && y0 < s1 && s0 < y1)) return fail("gather_records: the batch tensors must not alias the signal buffer");
    RecordGather g{signals, (long long)signal_floats, reinterpret_cast<const long long*>(rec_table), (long long)R, reinterpret_cast<const long long*>(clip_table),
                   x_out, y_out, (unsigned)N, (unsigned)window, (unsigned)x_len, (unsigned)y_len, 0u, 0u};
    g.cx = (unsigned)((x_len / 4 + kAugPerBlock - 1) / kAugPerBlock);
    g.cy = (unsigned)((y_len / 4 + kAugPerBlock - 1) / kAugPerBlock);
    const long long blocks = (long long)N * ((long long)g.cx + g.cy);
    if (blocks > 65535) return fail("gather_records: N=%d rows of %lld + %lld floats exceed one launch", N, (long long)x_len, (long long)y_len);
    if (clip_w == nullptr) {
        EEG_LAUNCH_P("gather_records", gather_records_kernel, dim3((unsigned)B, (unsigned)blocks), dim3(kAugThreads), kRecordStageBytes, S_(stream), g, label_pool,
                     label_out, label_bytes, reinterpret_cast<long long*>(len_out), reinterpret_cast<const long long*>(perm), (long long)n_perm,
                     (long long)P, reinterpret_cast<const long long*>(cursor), (long long)rank * B);
    } else {
        EEG_LAUNCH_P("gather_records", gather_records_tail_kernel, dim3((unsigned)B, (unsigned)blocks), dim3(kAugThreads), kRecordStageBytes, S_(stream), g,
                     label_pool, label_out, label_bytes, reinterpret_cast<long long*>(len_out), reinterpret_cast<const long long*>(perm),
                     (long long)n_perm, (long long)P, reinterpret_cast<const long long*>(cursor), (long long)rank * B, (long long)B * world, world,
                     clip_w, denom, reinterpret_cast<long long*>(n_valid));
    }
    if (int rc = check_launch("gather_records")) return rc;
    EEG_LAUNCH_P("gather_records_cursor", cursor_advance_kernel, dim3(1), dim3(64), 0, S_(stream), reinterpret_cast<long long*>(cursor), (long long)B * world);
    return check_launch("gather_records_cursor");
}

/* ---- the evaluation pass: per-clip scores, scores of the pool ------------------------------------ */
static_assert(EEG_EVAL_MAX_CLIPS == kEvalMaxClips && EEG_EVAL_RECORD_HEAD == kEvalRecordHead, "include/eeg_dcrnn.h and kernels_eval.h disagree");
int eeg_dcrnn_eval_scores(const float* logits, const void* label_pool, int label_bytes, const float* clip_w, const int64_t* cursor, int B, int C,
                          int rank, int world, int64_t P, float* probs, float* losses, void* stream) {
    if (logits == nullptr || label_pool == nullptr || clip_w == nullptr || cursor == nullptr) return fail("eval_scores: null logits / label_pool / clip_w / cursor");
    if (probs == nullptr || losses == nullptr) return fail("eval_scores: null probs / losses");
    if (B < 1 || C < 1) return fail("eval_scores: empty batch (B=%d, C=%d)", B, C);
    if (P < 1 || P > EEG_EVAL_MAX_CLIPS) return fail("eval_scores: P=%lld clips unsupported (1..%d)", (long long)P, EEG_EVAL_MAX_CLIPS);
    if (world < 1 || rank < 0 || rank >= world) return fail("eval_scores: rank=%d of world=%d", rank, world);
    if (label_bytes != (C == 1 ? 4 : 8)) return fail("eval_scores: label_bytes=%d (float32 labels for C = 1, int64 classes for C > 1; C=%d)", label_bytes, C);
    if ((((uintptr_t)logits | (uintptr_t)clip_w | (uintptr_t)probs | (uintptr_t)losses) & 3) != 0 ||
        (((uintptr_t)cursor | (C == 1 ? 0 : (uintptr_t)label_pool)) & 7) != 0 || ((uintptr_t)label_pool & 3) != 0)
        return fail("eval_scores: pointers must be aligned to their element size");
    EEG_LAUNCH_P("eval_scores", eval_scores_kernel, dim3(ceil_div(B, 256)), dim3(256), 0, S_(stream), logits, label_pool, clip_w,
                 reinterpret_cast<const long long*>(cursor), (long long)B * world, (long long)rank * B, (long long)P, B, C, probs, losses);
    return check_launch("eval_scores");
}
static int eval_npad(int64_t P) {
    int n = 1;
    while (n < P) n <<= 1;
    return n;
}
size_t eeg_dcrnn_eval_metrics_ws_bytes(int64_t P, int C) {
    if (P < 1 || P > EEG_EVAL_MAX_CLIPS || C < 1) return 0;
    return C == 1 ? sizeof(unsigned) * (size_t)eval_npad(P) + sizeof(int) * ((size_t)eval_npad(P) + 1) : 0;
}
int eeg_dcrnn_eval_metrics(const float* probs, const void* labels, int label_bytes, const float* losses, int64_t P, int C, int search,
                           double thresh, void* ws, int64_t* record, void* stream) {
    if (probs == nullptr || labels == nullptr || losses == nullptr || record == nullptr) return fail("eval_metrics: null probs / labels / losses / record");
    if (C < 1 || C > 1024) return fail("eval_metrics: C=%d classes unsupported (1..1024)", C);
    if (P < 1 || P > EEG_EVAL_MAX_CLIPS) return fail("eval_metrics: P=%lld clips unsupported (1..%d)", (long long)P, EEG_EVAL_MAX_CLIPS);
    if (label_bytes != (C == 1 ? 4 : 8)) return fail("eval_metrics: label_bytes=%d (float32 labels for C = 1, int64 classes for C > 1; C=%d)", label_bytes, C);
    if ((((uintptr_t)probs | (uintptr_t)losses | (uintptr_t)labels | (uintptr_t)ws) & 3) != 0 || ((uintptr_t)record & 7) != 0 ||
        (C > 1 && ((uintptr_t)labels & 7) != 0))
        return fail("eval_metrics: pointers must be aligned to their element size");
    hipStream_t st = S_(stream);
    long long* rec = reinterpret_cast<long long*>(record);
    if (C > 1) {
        EEG_LAUNCH_P("eval_metrics", eval_confusion_kernel, dim3(1), dim3(kEvalScanThreads), kEvalScanThreads * sizeof(long long), st, probs,
                     static_cast<const long long*>(labels), losses, (int)P, C, rec);
        return check_launch("eval_confusion");
    }
    if (ws == nullptr) return fail("eval_metrics: null workspace (eeg_dcrnn_eval_metrics_ws_bytes)");
    if (!(thresh == thresh)) return fail("eval_metrics: the threshold is NaN");
    const int npad = eval_npad(P), tile = kEvalSortTile;
    unsigned* keys = static_cast<unsigned*>(ws);
    int* neg_before = reinterpret_cast<int*>(keys + npad);
    const float* lab = static_cast<const float*>(labels);
    EEG_LAUNCH_P("eval_metrics", eval_keys_kernel, dim3(ceil_div(npad, 256)), dim3(256), 0, st, probs, lab, (int)P, npad, keys);
    if (check_launch("eval_keys")) return 1;
    const int ntile = npad > tile ? npad / tile : 1;
    const size_t tile_lds = (size_t)tile * sizeof(unsigned);
    EEG_LAUNCH_P("eval_metrics", eval_sort_tile_kernel, dim3(ntile), dim3(kEvalSortThreads), tile_lds, st, keys, npad, 2, npad < tile ? npad : tile);
    if (check_launch("eval_sort_tile")) return 1;
    const int step_grid = ceil_div(npad / 2, kEvalSortThreads * kEvalStepPairs);
    for (int k = 2 * tile; k <= npad && k > 0; k <<= 1) {
        for (int j = k >> 1; j >= tile; j >>= 1) {
            EEG_LAUNCH_P("eval_metrics", eval_sort_step_kernel, dim3(step_grid), dim3(kEvalSortThreads), 0, st, keys, npad, j, k);
            if (check_launch("eval_sort_step")) return 1;
        }
        EEG_LAUNCH_P("eval_metrics", eval_sort_tile_kernel, dim3(ntile), dim3(kEvalSortThreads), tile_lds, st, keys, npad, k, k);
        if (check_launch("eval_sort_tile")) return 1;
    }
    EEG_LAUNCH_P("eval_metrics", eval_scan_kernel, dim3(1), dim3(kEvalScanThreads), 4 * kEvalScanThreads * sizeof(long long), st, keys, probs, lab,
                 losses, (int)P, search ? 1 : 0, thresh, neg_before, rec);
    return check_launch("eval_scan");
}

/* ---- the clustered bootstrap of the scores: counts, one record per replicate ---------------------- */
static_assert(EEG_BOOT_MAX_GROUPS == kBootMaxGroups && EEG_BOOT_MAX_REPLICATES == kBootMaxReplicates && EEG_BOOT_DET_WORDS == kBootDetWords &&
              EEG_BOOT_MAX_CLASSES == kBootMaxClasses && EEG_BOOT_MAX_RECORD_WORDS == kBootMaxRecordWords && EEG_BOOT_LDS_GROUPS == kBootLdsGroups,
              "include/eeg_dcrnn.h and kernels_boot.h disagree");
static int boot_chunk(int64_t P) { return (int)((P + kBootThreads - 1) / kBootThreads); }
// the arguments every bootstrap entry shares; max_cluster < 0: the entry has no clips (boot_counts, boot_records)
static int boot_shape(const char* what, int64_t G, int64_t n_boot, int64_t max_cluster) {
    if (G < 1 || G > EEG_BOOT_MAX_GROUPS) return fail("%s: G=%lld clusters unsupported (1..%d)", what, (long long)G, EEG_BOOT_MAX_GROUPS);
    if (n_boot < 1 || n_boot > EEG_BOOT_MAX_REPLICATES) return fail("%s: n_boot=%lld replicates unsupported (1..%d)", what, (long long)n_boot, EEG_BOOT_MAX_REPLICATES);
    if (max_cluster >= 0 && (max_cluster < 1 || G * max_cluster >= (1ll << 31)))
        return fail("%s: max_cluster=%lld clips in the largest of G=%lld clusters (>= 1, G * max_cluster < 2^31: a replicate's weight fits 31 bits)", what,
                    (long long)max_cluster, (long long)G);
    return 0;
}
int eeg_dcrnn_boot_counts(uint64_t seed, int64_t G, int64_t n_boot, int32_t* counts, void* stream) {
    if (counts == nullptr) return fail("boot_counts: null counts");
    if (boot_shape("boot_counts", G, n_boot, -1)) return 1;
    if (((uintptr_t)counts & 3) != 0) return fail("boot_counts: pointers must be aligned to their element size");
    const int bins = G < kBootCountBins ? (int)G : kBootCountBins;
    const size_t lds = (size_t)((bins + 1) / 2) * sizeof(unsigned long long);
    EEG_SET_MAX_LDS(boot_counts_kernel, lds);
    EEG_LAUNCH_P("boot_counts", boot_counts_kernel, dim3((unsigned)n_boot + 1, (unsigned)ceil_div((int)G, bins)), dim3(kBootCountThreads), lds, S_(stream),
                 (unsigned long long)seed, (int)G, bins, counts);
    return check_launch("boot_counts");
}
size_t eeg_dcrnn_boot_ws_bytes(int64_t P) {
    if (P < 1 || P > EEG_EVAL_MAX_CLIPS) return 0;
    return sizeof(unsigned long long) * (size_t)eval_npad(P) + sizeof(unsigned) * ((size_t)boot_chunk(P) * kBootThreads + 2);
}
// keys (npad 64-bit words, filled) -> sorted ascending: the network of eeg_dcrnn_eval_metrics
static int boot_sort(unsigned long long* keys, int npad, hipStream_t st) {
    const int tile = kEvalSortTile, ntile = npad > tile ? npad / tile : 1;
    const size_t tile_lds = (size_t)tile * sizeof(unsigned long long);
    EEG_LAUNCH_P("boot_sort_tile", boot_sort_tile_kernel, dim3(ntile), dim3(kEvalSortThreads), tile_lds, st, keys, npad, 2, npad < tile ? npad : tile);
    if (check_launch("boot_sort_tile")) return 1;
    const int step_grid = ceil_div(npad / 2, kEvalSortThreads * kEvalStepPairs);
    for (int k = 2 * tile; k <= npad && k > 0; k <<= 1) {
        for (int j = k >> 1; j >= tile; j >>= 1) {
            EEG_LAUNCH_P("boot_sort_step", boot_sort_step_kernel, dim3(step_grid), dim3(kEvalSortThreads), 0, st, keys, npad, j, k);
            if (check_launch("boot_sort_step")) return 1;
        }
        EEG_LAUNCH_P("boot_sort_tile", boot_sort_tile_kernel, dim3(ntile), dim3(kEvalSortThreads), tile_lds, st, keys, npad, k, k);
        if (check_launch("boot_sort_tile")) return 1;
    }
    return 0;
}
int eeg_dcrnn_boot_detection(const float* probs, const float* labels, const int32_t* groups, const float* losses, int64_t P, int64_t G,
                             int64_t max_cluster, const int32_t* counts, int64_t n_boot, double thresh, void* ws, int64_t* records, void* stream) {
    if (probs == nullptr || labels == nullptr || counts == nullptr || records == nullptr) return fail("boot_detection: null probs / labels / counts / records");
    if (ws == nullptr) return fail("boot_detection: null workspace (eeg_dcrnn_boot_ws_bytes)");
    if (P < 1 || P > EEG_EVAL_MAX_CLIPS) return fail("boot_detection: P=%lld clips unsupported (1..%d)", (long long)P, EEG_EVAL_MAX_CLIPS);
    if (boot_shape("boot_detection", G, n_boot, max_cluster)) return 1;
    if (groups == nullptr && G != P) return fail("boot_detection: groups is null (every clip its own cluster) and G=%lld is not P=%lld", (long long)G, (long long)P);
    if (!(thresh == thresh)) return fail("boot_detection: thresh is NaN");
    if ((((uintptr_t)probs | (uintptr_t)labels | (uintptr_t)groups | (uintptr_t)losses | (uintptr_t)counts) & 3) != 0 ||
        (((uintptr_t)ws | (uintptr_t)records) & 7) != 0)
        return fail("boot_detection: pointers must be aligned to their element size");
    hipStream_t st = S_(stream);
    const int npad = eval_npad(P), chunk = boot_chunk(P);
    unsigned long long* keys = static_cast<unsigned long long*>(ws);
    unsigned* packed = reinterpret_cast<unsigned*>(keys + npad);
    int* split = reinterpret_cast<int*>(packed + (size_t)chunk * kBootThreads);
    EEG_LAUNCH_P("boot_keys", boot_keys_kernel, dim3(ceil_div(npad, 256)), dim3(256), 0, st, probs, labels, (int)P, npad, keys);
    if (check_launch("boot_keys")) return 1;
    if (boot_sort(keys, npad, st)) return 1;
    EEG_LAUNCH_P("boot_pack", boot_pack_kernel, dim3(ceil_div((int)P, 256)), dim3(256), 0, st, keys, groups, (int)P, (int)G, chunk, thresh, packed, split);
    if (check_launch("boot_pack")) return 1;
    long long* rec = reinterpret_cast<long long*>(records);
    if (G <= kBootLdsGroups) {
        const size_t lds = kBootScratchBytes + (size_t)G * sizeof(int);
        EEG_SET_MAX_LDS(boot_detection_kernel<true>, lds);
        EEG_LAUNCH_P("boot_detection", boot_detection_kernel<true>, dim3((unsigned)n_boot + 1), dim3(kBootThreads), lds, st, packed, split, counts, groups,
                     losses, (int)P, (int)G, chunk, rec);
    } else {
        EEG_LAUNCH_P("boot_detection", boot_detection_kernel<false>, dim3((unsigned)n_boot + 1), dim3(kBootThreads), (size_t)kBootScratchBytes, st, packed,
                     split, counts, groups, losses, (int)P, (int)G, chunk, rec);
    }
    return check_launch("boot_detection");
}
int eeg_dcrnn_boot_classification(const float* probs, const int64_t* labels, const int32_t* groups, int64_t P, int C, int64_t G, int64_t max_cluster,
                                  const int32_t* counts, int64_t n_boot, void* ws, int64_t* records, void* stream) {
    if (probs == nullptr || labels == nullptr || counts == nullptr || records == nullptr) return fail("boot_classification: null probs / labels / counts / records");
    if (ws == nullptr) return fail("boot_classification: null workspace (eeg_dcrnn_boot_ws_bytes)");
    if (C < 2 || C > EEG_BOOT_MAX_CLASSES) return fail("boot_classification: C=%d classes unsupported (2..%d)", C, EEG_BOOT_MAX_CLASSES);
    if (P < 1 || P > EEG_EVAL_MAX_CLIPS) return fail("boot_classification: P=%lld clips unsupported (1..%d)", (long long)P, EEG_EVAL_MAX_CLIPS);
    if (boot_shape("boot_classification", G, n_boot, max_cluster)) return 1;
    if (groups == nullptr && G != P) return fail("boot_classification: groups is null (every clip its own cluster) and G=%lld is not P=%lld", (long long)G, (long long)P);
    if ((((uintptr_t)probs | (uintptr_t)groups | (uintptr_t)counts) & 3) != 0 || (((uintptr_t)labels | (uintptr_t)ws | (uintptr_t)records) & 7) != 0)
        return fail("boot_classification: pointers must be aligned to their element size");
    hipStream_t st = S_(stream);
    const int npad = eval_npad(P), chunk = boot_chunk(P), cells = C * C;
    unsigned long long* keys = static_cast<unsigned long long*>(ws);
    unsigned* packed = reinterpret_cast<unsigned*>(keys + npad);
    EEG_LAUNCH_P("boot_cell_keys", boot_cell_keys_kernel, dim3(ceil_div(npad, 256)), dim3(256), 0, st, probs, reinterpret_cast<const long long*>(labels), (int)P,
                 C, npad, keys);
    if (check_launch("boot_cell_keys")) return 1;
    if (boot_sort(keys, npad, st)) return 1;
    EEG_LAUNCH_P("boot_pack_cells", boot_pack_cells_kernel, dim3(ceil_div((int)P, 256)), dim3(256), 0, st, keys, groups, (int)P, (int)G, chunk, packed);
    if (check_launch("boot_pack_cells")) return 1;
    long long* rec = reinterpret_cast<long long*>(records);
    const size_t head = (size_t)kBootMaxClasses * kBootMaxClasses * sizeof(unsigned long long);
    if (G <= kBootLdsGroups) {
        const size_t lds = head + (size_t)G * sizeof(int);
        EEG_SET_MAX_LDS(boot_cells_kernel<true>, lds);
        EEG_LAUNCH_P("boot_classification", boot_cells_kernel<true>, dim3((unsigned)n_boot + 1), dim3(kBootThreads), lds, st, packed, counts, (int)P, (int)G,
                     cells, chunk, rec);
    } else {
        EEG_LAUNCH_P("boot_classification", boot_cells_kernel<false>, dim3((unsigned)n_boot + 1), dim3(kBootThreads), head, st, packed, counts, (int)P, (int)G,
                     cells, chunk, rec);
    }
    return check_launch("boot_classification");
}
int eeg_dcrnn_boot_records(const int64_t* rec_records, int64_t G, int K, const int32_t* counts, int64_t n_boot, int64_t* records, void* stream) {
    if (rec_records == nullptr || counts == nullptr || records == nullptr) return fail("boot_records: null rec_records / counts / records");
    if (K < 1 || K > EEG_BOOT_MAX_RECORD_WORDS) return fail("boot_records: K=%d words per record unsupported (1..%d)", K, EEG_BOOT_MAX_RECORD_WORDS);
    if (boot_shape("boot_records", G, n_boot, -1)) return 1;
    if (((uintptr_t)counts & 3) != 0 || (((uintptr_t)rec_records | (uintptr_t)records) & 7) != 0)
        return fail("boot_records: pointers must be aligned to their element size");
    EEG_LAUNCH_P("boot_records", boot_records_kernel, dim3((unsigned)n_boot + 1), dim3(kBootRecordThreads), kBootRecordThreads * sizeof(unsigned long long),
                 S_(stream), reinterpret_cast<const long long*>(rec_records), counts, (int)G, K, reinterpret_cast<long long*>(records));
    return check_launch("boot_records");
}

/* ---- the SSL evaluation pass: per-clip masked MAE, the pass's record ------------------------------ */
static_assert(EEG_SSL_EVAL_MAX_CLIP_ELEMS == kSslEvalMaxClipElems && EEG_SSL_EVAL_RECORD_WORDS == kSslEvalRecordWords,
              "include/eeg_dcrnn.h and kernels_eval.h disagree");
int eeg_dcrnn_ssl_eval_scores(const float* pred, const float* target, const float* clip_w, const int64_t* cursor, int B, int64_t clip_elems, int D,
                              int rank, int world, int64_t P, int scaled, float mean, float std_, float mask_val, double* scores, float* keep,
                              void* stream) {
    if (pred == nullptr || target == nullptr || clip_w == nullptr || cursor == nullptr) return fail("ssl_eval_scores: null pred / target / clip_w / cursor");
    if (scores == nullptr) return fail("ssl_eval_scores: null scores");
    if (B < 1) return fail("ssl_eval_scores: empty batch (B=%d)", B);
    if (D < 1 || D % 4 != 0) return fail("ssl_eval_scores: D=%d: the clips are read in 16-byte pieces, D must be a multiple of 4", D);
    if (clip_elems < D || clip_elems % D != 0) return fail("ssl_eval_scores: a clip of %lld elements is no whole number of rows of D=%d", (long long)clip_elems, D);
    if (clip_elems >= EEG_SSL_EVAL_MAX_CLIP_ELEMS)
        return fail("ssl_eval_scores: a clip of %lld elements unsupported (below %d)", (long long)clip_elems, EEG_SSL_EVAL_MAX_CLIP_ELEMS);
    if (P < 1 || P > EEG_EVAL_MAX_CLIPS) return fail("ssl_eval_scores: P=%lld clips unsupported (1..%d)", (long long)P, EEG_EVAL_MAX_CLIPS);
    if (world < 1 || rank < 0 || rank >= world) return fail("ssl_eval_scores: rank=%d of world=%d", rank, world);
    if ((((uintptr_t)pred | (uintptr_t)target | (uintptr_t)keep) & 15) != 0) return fail("ssl_eval_scores: pred, target and keep must be 16-byte aligned");
    if (((uintptr_t)clip_w & 3) != 0 || (((uintptr_t)cursor | (uintptr_t)scores) & 7) != 0)
        return fail("ssl_eval_scores: pointers must be aligned to their element size");
    EEG_LAUNCH_P("ssl_eval_scores", ssl_eval_scores_kernel, dim3(B), dim3(kSslEvalThreads), kSslEvalThreads * sizeof(double), S_(stream), pred, target,
                 clip_w, reinterpret_cast<const long long*>(cursor), (long long)B * world, (long long)rank * B, (long long)P, (int)(clip_elems / 4), mean,
                 std_, scaled ? 1 : 0, mask_val, scores, keep);
    return check_launch("ssl_eval_scores");
}
int eeg_dcrnn_ssl_eval_metrics(const double* scores, int64_t P, int64_t G, double* record, void* stream) {
    if (scores == nullptr || record == nullptr) return fail("ssl_eval_metrics: null scores / record");
    if (P < 1 || P > EEG_EVAL_MAX_CLIPS) return fail("ssl_eval_metrics: P=%lld clips unsupported (1..%d)", (long long)P, EEG_EVAL_MAX_CLIPS);
    if (G < 1) return fail("ssl_eval_metrics: groups of G=%lld clips", (long long)G);
    if ((((uintptr_t)scores | (uintptr_t)record) & 7) != 0) return fail("ssl_eval_metrics: pointers must be aligned to their element size");
    EEG_LAUNCH_P("ssl_eval_metrics", ssl_eval_metrics_kernel, dim3(1), dim3(kSslEvalThreads), kSslEvalThreads * sizeof(double), S_(stream), scores, (int)P,
                 (int)(G < P ? G : P), record);
    return check_launch("ssl_eval_metrics");
}

/* ---- the fit of the input scaler: per-clip moments of the un-standardised inputs, the pool's record ----- */
static_assert(EEG_MOMENTS_RECORD_WORDS == kMomRecordWords && EEG_MOMENTS_MAX_BATCH == kMomMaxBatch, "include/eeg_dcrnn.h and kernels_moments.h disagree");
// the checks the size query and the launch share; `what` names the entry point in refusals
static int moments_shape(const char* what, int B, int N, int T, int W, int kind) {
    if (B < 1 || N < 1 || T < 1) return fail("%s: empty input (B=%d, N=%d, T=%d)", what, B, N, T);
    if (B > kMomMaxBatch) return fail("%s: B=%d clips exceed one launch (limit %d)", what, B, kMomMaxBatch);
    if (kind != 0 && kind != 1) return fail("%s: kind=%d (0: log|FFT| features, 1: the values as given)", what, kind);
    if (W < 4 || W % 4 != 0) return fail("%s: window=%d unsupported (a positive multiple of 4)", what, W);
    if (kind == 0 && W / 4 + 1 > 64) return fail("%s: window=%d unsupported for kind=0 (multiple of 4, <= 252)", what, W);
    if ((long long)N * T * W >= kMomMaxClipElems) return fail("%s: a clip of %lld elements unsupported (below 2^31)", what, (long long)N * T * W);
    return 0;
}
size_t eeg_dcrnn_moments_ws_bytes(int B, int N, int T, int W, int kind) {
    if (moments_shape("moments_ws_bytes", B, N, T, W, kind)) return 0;
    return (size_t)B * (size_t)moments_chunks(N, T, W, kind) * 4 * sizeof(double);
}
int eeg_dcrnn_feature_moments(const float* raw, int B, int N, int T, int W, int kind, const int64_t* lengths, const float* clip_w,
                              const int64_t* cursor, int rank, int world, int64_t P, void* ws, double* scores, void* stream) {
    if (raw == nullptr) return fail("feature_moments: null raw");
    if (scores == nullptr || ws == nullptr) return fail("feature_moments: null scores / ws (eeg_dcrnn_moments_ws_bytes)");
    if (moments_shape("feature_moments", B, N, T, W, kind)) return 1;
    if (P < 1 || P > EEG_EVAL_MAX_CLIPS) return fail("feature_moments: P=%lld clips unsupported (1..%d)", (long long)P, EEG_EVAL_MAX_CLIPS);
    if (world < 1 || rank < 0 || rank >= world) return fail("feature_moments: rank=%d of world=%d", rank, world);
    if (((uintptr_t)raw & 15) != 0) return fail("feature_moments: raw must be 16-byte aligned");
    if (((uintptr_t)clip_w & 3) != 0 || (((uintptr_t)lengths | (uintptr_t)cursor | (uintptr_t)scores | (uintptr_t)ws) & 7) != 0)
        return fail("feature_moments: lengths / clip_w / cursor / scores / ws must be aligned to their element size");
    hipStream_t st = S_(stream);
    const long long* len = reinterpret_cast<const long long*>(lengths);
    const long long* cur = reinterpret_cast<const long long*>(cursor);
    const long long step = (long long)B * world, slot0 = (long long)rank * B;
    const int chunks = (int)moments_chunks(N, T, W, kind);
    double* part = static_cast<double*>(ws);
    const dim3 grid((unsigned)chunks, (unsigned)B);
    if (kind != 0) {
        EEG_LAUNCH_P("feature_moments", moments_values_kernel, grid, dim3(kMomThreads), kMomThreads * sizeof(double), st, raw, (unsigned)N,
                     (unsigned)(T * (W / 4)), (unsigned)(W / 4), T, len, clip_w, cur, step, slot0, (long long)P, part);
    } else if (W == kFftWin) {
        const size_t lds = 4 * (size_t)kFftWaveDoubles * sizeof(double);
        EEG_SET_MAX_LDS(moments_fft200_kernel, lds);
        EEG_LAUNCH_P("feature_moments", moments_fft200_kernel, grid, dim3(kMomThreads), lds, st, raw, N, T, len, clip_w, cur, step, slot0, (long long)P,
                     part);
    } else {
        const size_t lds = (size_t)std::max(4 * W, kMomThreads) * sizeof(double);
        EEG_LAUNCH_P("feature_moments", moments_dft_kernel, grid, dim3(kMomThreads), lds, st, raw, N, T, W, len, clip_w, cur, step, slot0, (long long)P,
                     part);
    }
    if (int rc = check_launch("feature_moments")) return rc;
    EEG_LAUNCH_P("feature_moments_fold", moments_fold_kernel, dim3(ceil_div(B, 256)), dim3(256), 0, st, part, chunks, clip_w, cur, step, slot0,
                 (long long)P, B, scores);
    return check_launch("feature_moments_fold");
}
int eeg_dcrnn_moments_record(const double* scores, int64_t P, double* record, void* stream) {
    if (scores == nullptr || record == nullptr) return fail("moments_record: null scores / record");
    if (P < 1 || P > EEG_EVAL_MAX_CLIPS) return fail("moments_record: P=%lld clips unsupported (1..%d)", (long long)P, EEG_EVAL_MAX_CLIPS);
    if ((((uintptr_t)scores | (uintptr_t)record) & 7) != 0) return fail("moments_record: pointers must be aligned to their element size");
    EEG_LAUNCH_P("moments_record", moments_record_kernel, dim3(1), dim3(kMomThreads), kMomThreads * sizeof(double), S_(stream), scores, (int)P, record);
    return check_launch("moments_record");
}

/* ---- whole recordings: the timeline of a scan, its events, their scores --------------------------- */
static_assert(EEG_SCAN_CHUNK_BINS == kScanChunkBins && EEG_SCAN_MAX_SMOOTH_BINS == kScanMaxSmoothBins && EEG_SCAN_RECORD_WORDS == kScanRecordWords,
              "include/eeg_dcrnn.h and kernels_scan.h disagree");
// the checks the three entry points share; `what` names the entry point in refusals
static int scan_shape(const char* what, int64_t R, int64_t total_bins) {
    if (R < 1 || R > EEG_SCAN_MAX_RECORDINGS) return fail("%s: R=%lld recordings unsupported (1..%d)", what, (long long)R, EEG_SCAN_MAX_RECORDINGS);
    if (total_bins < 1 || total_bins >= ((int64_t)1 << 31)) return fail("%s: total_bins=%lld unsupported (1..2^31-1)", what, (long long)total_bins);
    return 0;
}
int eeg_dcrnn_scan_timeline(const float* probs, int64_t P, const int64_t* clip_table, const int64_t* clip_off, const int64_t* bin_off, int64_t R,
                            int64_t total_bins, int x_steps, int window, int agg, float* timeline, int32_t* cover, void* stream) {
    if (probs == nullptr || clip_table == nullptr || clip_off == nullptr || bin_off == nullptr) return fail("scan_timeline: null probs / clip_table / clip_off / bin_off");
    if (timeline == nullptr || cover == nullptr) return fail("scan_timeline: null timeline / cover");
    if (scan_shape("scan_timeline", R, total_bins)) return 1;
    if (P < 1 || P > EEG_EVAL_MAX_CLIPS) return fail("scan_timeline: P=%lld clips unsupported (1..%d)", (long long)P, EEG_EVAL_MAX_CLIPS);
    if (x_steps < 1 || window < 1) return fail("scan_timeline: x_steps=%d, window=%d (both >= 1)", x_steps, window);
    if (agg != 0 && agg != 1) return fail("scan_timeline: agg=%d (0 = mean, 1 = max)", agg);
    if ((((uintptr_t)probs | (uintptr_t)timeline | (uintptr_t)cover) & 3) != 0 || (((uintptr_t)clip_table | (uintptr_t)clip_off | (uintptr_t)bin_off) & 7) != 0)
        return fail("scan_timeline: pointers must be aligned to their element size");
    EEG_LAUNCH_P("scan_timeline", scan_timeline_kernel, dim3((unsigned)((total_bins + 255) / 256)), dim3(256), 0, S_(stream), probs, (long long)P,
                 reinterpret_cast<const long long*>(clip_table), reinterpret_cast<const long long*>(clip_off), reinterpret_cast<const long long*>(bin_off),
                 (int)R, (long long)total_bins, x_steps, window, agg, timeline, cover);
    return check_launch("scan_timeline");
}
int eeg_dcrnn_scan_events(const float* timeline, const int32_t* cover, const int64_t* bin_off, int64_t R, int64_t total_bins, int smooth_bins,
                          float th_on, float th_off, int merge_gap, int min_bins, int E_max, float* smoothed, int32_t* events, int32_t* event_count,
                          void* stream) {
    if (timeline == nullptr || cover == nullptr || bin_off == nullptr) return fail("scan_events: null timeline / cover / bin_off");
    if (smoothed == nullptr || events == nullptr || event_count == nullptr) return fail("scan_events: null smoothed / events / event_count");
    if (scan_shape("scan_events", R, total_bins)) return 1;
    if (smooth_bins < 1 || smooth_bins % 2 == 0 || smooth_bins > kScanMaxSmoothBins)
        return fail("scan_events: smooth_bins=%d unsupported (odd, 1..%d)", smooth_bins, kScanMaxSmoothBins);
    if (!(th_on == th_on) || !(th_off == th_off)) return fail("scan_events: a threshold is NaN");
    if (th_off > th_on) return fail("scan_events: th_off=%g above th_on=%g", (double)th_off, (double)th_on);
    if (merge_gap < 0 || min_bins < 1) return fail("scan_events: merge_gap=%d (>= 0), min_bins=%d (>= 1)", merge_gap, min_bins);
    if (E_max < 1 || (long long)R * E_max >= (1ll << 30)) return fail("scan_events: E_max=%d events per recording unsupported (>= 1, R*E_max < 2^30)", E_max);
    if ((((uintptr_t)timeline | (uintptr_t)cover | (uintptr_t)smoothed | (uintptr_t)events | (uintptr_t)event_count) & 3) != 0 || ((uintptr_t)bin_off & 7) != 0)
        return fail("scan_events: pointers must be aligned to their element size");
    EEG_LAUNCH_P("scan_events", scan_events_kernel, dim3((unsigned)R), dim3(kScanThreads), kScanEventsLds, S_(stream), timeline, cover,
                 reinterpret_cast<const long long*>(bin_off), (long long)total_bins, (smooth_bins - 1) / 2, th_on, th_off, merge_gap, min_bins, E_max,
                 smoothed, events, event_count);
    return check_launch("scan_events");
}
int eeg_dcrnn_event_scores(const int32_t* events, const int32_t* event_count, int E_max, const int32_t* ref, const int32_t* ref_count, int A_max,
                           const int32_t* cover, const int64_t* bin_off, int64_t R, int64_t total_bins, int64_t* record, int64_t* rec_records,
                           void* stream) {
    if (events == nullptr || event_count == nullptr || ref == nullptr || ref_count == nullptr) return fail("event_scores: null events / event_count / ref / ref_count");
    if (cover == nullptr || bin_off == nullptr || record == nullptr || rec_records == nullptr) return fail("event_scores: null cover / bin_off / record / rec_records");
    if (scan_shape("event_scores", R, total_bins)) return 1;
    if (E_max < 1 || (long long)R * E_max >= (1ll << 30)) return fail("event_scores: E_max=%d events per recording unsupported (>= 1, R*E_max < 2^30)", E_max);
    if (A_max < 1 || (long long)R * A_max >= (1ll << 30)) return fail("event_scores: A_max=%d reference events per recording unsupported (>= 1, R*A_max < 2^30)", A_max);
    if ((((uintptr_t)events | (uintptr_t)event_count | (uintptr_t)ref | (uintptr_t)ref_count | (uintptr_t)cover) & 3) != 0 ||
        (((uintptr_t)bin_off | (uintptr_t)record | (uintptr_t)rec_records) & 7) != 0)
        return fail("event_scores: pointers must be aligned to their element size");
    hipStream_t st = S_(stream);
    long long* recs = reinterpret_cast<long long*>(rec_records);
    EEG_LAUNCH_P("event_scores", event_scores_kernel, dim3((unsigned)R), dim3(kScanThreads), kScanThreads * sizeof(long long), st, events, event_count, E_max,
                 ref, ref_count, A_max, cover, reinterpret_cast<const long long*>(bin_off), (long long)total_bins, recs);
    if (int rc = check_launch("event_scores")) return rc;
    EEG_LAUNCH_P("event_scores_total", event_scores_total_kernel, dim3(1), dim3(kScanThreads), kScanThreads * sizeof(long long), st, recs, (int)R,
                 reinterpret_cast<long long*>(record));
    return check_launch("event_scores_total");
}

/* ---- native-rate recordings to the model's rate: Fourier resampling of whole recordings -------------- */
static_assert(EEG_RESAMPLE_MAX_SAMPLES == (1ll << (kRsMaxBits - 1)), "include/eeg_dcrnn.h and kernels_resample.h disagree");
size_t eeg_dcrnn_resample_ws_bytes(int64_t n_in, int64_t n_out, int channels) {
    int lm1, lm2;
    if (channels < 1 || !rs_lengths(n_in, n_out, lm1, lm2)) return 0;
    const size_t m1 = (size_t)1 << lm1, m2 = (size_t)1 << lm2;
    return (m1 + m2 + (size_t)channels * std::max(m1, m2)) * sizeof(rs_c64);
}
int eeg_dcrnn_resample(const void* in, int in_f64, int channels, int64_t n_in, int64_t in_stride, int64_t n_out, float* out, int64_t out_stride,
                       void* ws, size_t ws_bytes, void* stream) {
    if (in == nullptr || out == nullptr || ws == nullptr) return fail("resample: null in / out / ws");
    if (in_f64 != 0 && in_f64 != 1) return fail("resample: in_f64=%d (0 = float32, 1 = float64)", in_f64);
    if (channels < 1) return fail("resample: channels=%d (>= 1)", channels);
    int lm1, lm2;
    if (n_in < 2 || n_in > EEG_RESAMPLE_MAX_SAMPLES) return fail("resample: n_in=%lld samples unsupported (2..%lld)", (long long)n_in, (long long)EEG_RESAMPLE_MAX_SAMPLES);
    if (n_out < 1 || n_out > EEG_RESAMPLE_MAX_SAMPLES) return fail("resample: n_out=%lld samples unsupported (1..%lld)", (long long)n_out, (long long)EEG_RESAMPLE_MAX_SAMPLES);
    if (!rs_lengths(n_in, n_out, lm1, lm2)) return fail("resample: n_in=%lld, n_out=%lld unsupported", (long long)n_in, (long long)n_out);
    if (in_stride < n_in) return fail("resample: in_stride=%lld below n_in=%lld", (long long)in_stride, (long long)n_in);
    if (out_stride < n_out) return fail("resample: out_stride=%lld below n_out=%lld", (long long)out_stride, (long long)n_out);
    if (((uintptr_t)in & (in_f64 ? 7 : 3)) != 0 || ((uintptr_t)out & 3) != 0) return fail("resample: in / out must be aligned to their element size");
    if (((uintptr_t)ws & 15) != 0) return fail("resample: ws must be 16-byte aligned");
    const size_t m1 = (size_t)1 << lm1, m2 = (size_t)1 << lm2, mb = std::max(m1, m2);
    const size_t one = (m1 + m2 + mb) * sizeof(rs_c64);
    if (ws_bytes < one) return fail("resample: ws_bytes=%zu below the %zu bytes of one channel (eeg_dcrnn_resample_ws_bytes(n_in, n_out, 1))", ws_bytes, one);
    const int chunk = (int)std::min<size_t>({(size_t)channels, (size_t)kRsMaxChunk, (ws_bytes / sizeof(rs_c64) - m1 - m2) / mb});
    hipStream_t st = S_(stream);
    rs_c64* h1 = reinterpret_cast<rs_c64*>(ws);
    rs_c64* h2 = h1 + m1;
    rs_c64* buf = h2 + m2;
    const long long Nx = n_in, num = n_out, N = std::min(Nx, num), K = num / 2 + 1;
    auto blocks = [](size_t n) { return (unsigned)((n + kRsThreads - 1) / kRsThreads); };
    // the spectra of the two chirp filters, shared by the channels
    EEG_LAUNCH_P("resample_filter", rs_filter_kernel, dim3(blocks(m1)), dim3(kRsThreads), 0, st, h1, (long long)m1, Nx, Nx, N / 2 + 1, +1);
    if (int rc = check_launch("resample_filter")) return rc;
    if (int rc = rs_transform(h1, 0, 1, nullptr, lm1, st)) return rc;
    EEG_LAUNCH_P("resample_filter", rs_filter_kernel, dim3(blocks(m2)), dim3(kRsThreads), 0, st, h2, (long long)m2, num, K, num, -1);
    if (int rc = check_launch("resample_filter")) return rc;
    if (int rc = rs_transform(h2, 0, 1, nullptr, lm2, st)) return rc;
    for (int c0 = 0; c0 < channels; c0 += chunk) {
        const int nc = std::min(chunk, channels - c0);
        if (in_f64)
            EEG_LAUNCH_P("resample_load", rs_load_kernel<double>, dim3(blocks(m1), (unsigned)nc), dim3(kRsThreads), 0, st,
                         static_cast<const double*>(in) + (size_t)c0 * in_stride, (long long)in_stride, Nx, buf, (long long)mb, (long long)m1);
        else
            EEG_LAUNCH_P("resample_load", rs_load_kernel<float>, dim3(blocks(m1), (unsigned)nc), dim3(kRsThreads), 0, st,
                         static_cast<const float*>(in) + (size_t)c0 * in_stride, (long long)in_stride, Nx, buf, (long long)mb, (long long)m1);
        if (int rc = check_launch("resample_load")) return rc;
        if (int rc = rs_transform(buf, (long long)mb, nc, h1, lm1, st)) return rc;
        EEG_LAUNCH_P("resample_bridge", rs_bridge_kernel, dim3(blocks(m2), (unsigned)nc), dim3(kRsThreads), 0, st, buf, (long long)mb, Nx, num,
                     1.0 / (double)m1, (long long)m2);
        if (int rc = check_launch("resample_bridge")) return rc;
        if (int rc = rs_transform(buf, (long long)mb, nc, h2, lm2, st)) return rc;
        EEG_LAUNCH_P("resample_store", rs_store_kernel, dim3(blocks((size_t)num), (unsigned)nc), dim3(kRsThreads), 0, st, buf, (long long)mb, num,
                     1.0 / ((double)m2 * (double)Nx), out + (size_t)c0 * out_stride, (long long)out_stride);
        if (int rc = check_launch("resample_store")) return rc;
    }
    return 0;
}

/* ---- EDF payload -> physical signals: the int16 samples of the selected signals, scaled in float64 (kernels_edf.h) ---------- */
static_assert(EEG_EDF_MAX_CHANNELS == kEdfMaxChannels && EEG_EDF_MAX_CHANNELS == kMaxNodes, "include/eeg_dcrnn.h and kernels_edf.h disagree");
int eeg_dcrnn_edf_decode(const void* payload, size_t payload_bytes, int64_t num_records, int64_t R, int64_t n, int channels, const int64_t* chan_off,
                         const double* gain, const double* offset, int out_f64, void* out, int64_t out_stride, void* stream) {
    if (payload == nullptr || chan_off == nullptr || gain == nullptr || offset == nullptr || out == nullptr)
        return fail("edf_decode: null payload / chan_off / gain / offset / out");
    if (((uintptr_t)payload & 1) != 0) return fail("edf_decode: payload must be 2-byte aligned (an odd address)");
    if (out_f64 != 0 && out_f64 != 1) return fail("edf_decode: out_f64=%d (0 = float32, 1 = float64)", out_f64);
    if (channels < 1 || channels > EEG_EDF_MAX_CHANNELS) return fail("edf_decode: channels=%d unsupported (1..%d)", channels, EEG_EDF_MAX_CHANNELS);
    if (num_records < 1) return fail("edf_decode: num_records=%lld (>= 1)", (long long)num_records);
    if (n < 1 || n > kEdfMaxN) return fail("edf_decode: n=%lld samples per record unsupported (1..%lld)", (long long)n, kEdfMaxN);
    if (R < n) return fail("edf_decode: R=%lld int16 per record below n=%lld", (long long)R, (long long)n);
    if (num_records > (int64_t)((1ull << 62) / (uint64_t)R) || (uint64_t)num_records * (uint64_t)R > (uint64_t)(payload_bytes / 2))
        return fail("edf_decode: payload_bytes=%zu below the 2 * num_records * R = 2 * %lld * %lld bytes of whole records", payload_bytes,
                    (long long)num_records, (long long)R);
    EdfChannels ch = {};
    for (int c = 0; c < channels; ++c) {
        if (chan_off[c] < 0 || chan_off[c] > R - n)
            return fail("edf_decode: chan_off[%d]=%lld + n=%lld outside a record of R=%lld", c, (long long)chan_off[c], (long long)n, (long long)R);
        ch.off[c] = chan_off[c];
        ch.gain[c] = gain[c];
        ch.offset[c] = offset[c];
    }
    const long long L = (long long)num_records * n;                      // <= num_records * R < 2^62
    if (out_stride < L) return fail("edf_decode: out_stride=%lld below the row length num_records * n = %lld", (long long)out_stride, L);
    if (((uintptr_t)out & (out_f64 ? 7 : 3)) != 0) return fail("edf_decode: out must be aligned to its element size");
    const long long tiles = (L + kEdfTile - 1) / kEdfTile;
    if (tiles > 0x7fffffffll) return fail("edf_decode: num_records * n = %lld samples per channel exceed the grid", L);
    hipStream_t st = S_(stream);
    const dim3 grid((unsigned)tiles, (unsigned)channels);
    if (out_f64)
        EEG_LAUNCH_P("edf_decode", edf_decode_kernel<double>, grid, dim3(kEdfThreads), 0, st, static_cast<const int16_t*>(payload), (long long)num_records,
                     (long long)R, (long long)n, ch, static_cast<double*>(out), (long long)out_stride);
    else
        EEG_LAUNCH_P("edf_decode", edf_decode_kernel<float>, grid, dim3(kEdfThreads), 0, st, static_cast<const int16_t*>(payload), (long long)num_records,
                     (long long)R, (long long)n, ch, static_cast<float*>(out), (long long)out_stride);
    return check_launch("edf_decode");
}

/* ---- occlusion maps: the variants of one window, their scores ------------------------------------- */
static_assert(EEG_OCCLUDE_MAX_LAYERS == kOccMaxLayers && EEG_OCCLUDE_MAX_GROUPS == kOccMaxGroups, "include/eeg_dcrnn.h and kernels_occlude.h disagree");
int eeg_dcrnn_occlude_expand(const float* x, const float* const* hext, int L, const int32_t* groups, const int64_t* lengths, int B, int T, int N, int D,
                             int H, int G, int t0, int w, float fill, float* x_var, float* h0_var, int64_t* len_var, void* stream) {
    if (x == nullptr || hext == nullptr || groups == nullptr) return fail("occlude_expand: null x / layer table / groups");
    if (x_var == nullptr || h0_var == nullptr || len_var == nullptr) return fail("occlude_expand: null x_var / h0_var / len_var");
    if (L < 1 || L > kOccMaxLayers) return fail("occlude_expand: %d layers (1..%d)", L, kOccMaxLayers);
    if (G < 1 || G > kOccMaxGroups) return fail("occlude_expand: G=%d groups (1..%d)", G, kOccMaxGroups);
    if (B < 1 || T < 1 || H < 1) return fail("occlude_expand: B=%d clips, T=%d steps, H=%d units", B, T, H);
    if (N < 1 || N > kMaxNodes) return fail("occlude_expand: num_nodes=%d unsupported (1..%d)", N, kMaxNodes);
    if (D < 4 || D % 4 != 0) return fail("occlude_expand: D=%d: the rows move in 16-byte pieces, D must be a positive multiple of 4", D);
    if (((long long)N * H) % 4 != 0) return fail("occlude_expand: N*H=%lld must be a multiple of 4", (long long)N * H);
    if (t0 < 0 || t0 >= T) return fail("occlude_expand: the window starts at t0=%d of T=%d steps", t0, T);
    if (w < 1) return fail("occlude_expand: a window of w=%d steps", w);
    if ((long long)(T + L) * B * G >= (1ll << 30) || (long long)N * D >= (1ll << 30) || (long long)N * H >= (1ll << 30))
        return fail("occlude_expand: B=%d, G=%d, T=%d, N=%d, D=%d, H=%d: too many rows for one launch", B, G, T, N, D, H);
    OccludeExpand a;
    uintptr_t al = (uintptr_t)x | (uintptr_t)x_var | (uintptr_t)h0_var;
    for (int l = 0; l < kOccMaxLayers; ++l) {
        a.hext[l] = l < L ? hext[l] : nullptr;
        if (l < L && hext[l] == nullptr) return fail("occlude_expand: null hext of layer %d", l);
        al |= (uintptr_t)a.hext[l];
    }
    if ((al & 15) != 0) return fail("occlude_expand: x, hext, x_var and h0_var must be 16-byte aligned");
    if (((uintptr_t)groups & 3) != 0 || (((uintptr_t)lengths | (uintptr_t)len_var) & 7) != 0)
        return fail("occlude_expand: pointers must be aligned to their element size");
    a.x = x; a.groups = reinterpret_cast<const int*>(groups); a.lengths = reinterpret_cast<const long long*>(lengths);
    a.x_var = x_var; a.h0_var = h0_var; a.len_var = reinterpret_cast<long long*>(len_var);
    a.B = B; a.T = T; a.N = N; a.D4 = D / 4; a.NH4 = N * H / 4; a.L = L; a.G = G; a.t0 = t0; a.w = w; a.fill = fill;
    // the stretches of groups: one per (row, clip) unless the capped grid would stay unfilled
    const int cap = kOccBlocksPerCu * platform_num_cus(), rows = (T - t0 + L) * B;
    const int want = std::min(G, std::max(1, ceil_div(cap, rows)));
    a.gper = ceil_div(G, want);
    a.nch = ceil_div(G, a.gper);
    const int units = rows * a.nch;
    EEG_LAUNCH_P("occlude_expand", occlude_expand_kernel, dim3(std::min(units, cap)), dim3(kOccThreads), kMaxNodes * sizeof(unsigned long long), S_(stream), a);
    return check_launch("occlude_expand");
}
int eeg_dcrnn_occlusion_scores(const float* var_logits, const float* base_logits, const int64_t* lengths, const int64_t* target, int B, int G, int C,
                               int Tw, int k, int t0, float* maps, float* base_prob, int64_t* target_out, void* stream) {
    if (var_logits == nullptr || base_logits == nullptr) return fail("occlusion_scores: null variant / baseline logits");
    if (maps == nullptr || base_prob == nullptr) return fail("occlusion_scores: null maps / base_prob");
    if (B < 1 || (long long)B * G >= (1ll << 30)) return fail("occlusion_scores: B=%d clips of G=%d groups", B, G);
    if (G < 1 || G > kOccMaxGroups) return fail("occlusion_scores: G=%d groups (1..%d)", G, kOccMaxGroups);
    if (C < 1 || C > kOccMaxClasses) return fail("occlusion_scores: C=%d classes unsupported (1..%d)", C, kOccMaxClasses);
    if (Tw < 1 || k < 0 || k >= Tw) return fail("occlusion_scores: window k=%d of Tw=%d", k, Tw);
    if (t0 < 0) return fail("occlusion_scores: the window starts at t0=%d", t0);
    if ((((uintptr_t)var_logits | (uintptr_t)base_logits | (uintptr_t)maps | (uintptr_t)base_prob) & 3) != 0 ||
        (((uintptr_t)lengths | (uintptr_t)target | (uintptr_t)target_out) & 7) != 0)
        return fail("occlusion_scores: pointers must be aligned to their element size");
    EEG_LAUNCH_P("occlusion_scores", occlusion_scores_kernel, dim3(ceil_div(B * G, 256)), dim3(256), 0, S_(stream), var_logits, base_logits,
                 reinterpret_cast<const long long*>(lengths), reinterpret_cast<const long long*>(target), B, G, C, Tw, k, t0, k == 0 ? 1 : 0, maps,
                 base_prob, reinterpret_cast<long long*>(target_out));
    return check_launch("occlusion_scores");
}

/* ---- per-clip correlation graph -> supports --------------------------------------------------- */
int eeg_dcrnn_augment_draw(const uint64_t* rng_used, int B, int N, const int32_t* swap_perm, int32_t* flags, int32_t* perm,
                           float* log_scale, const float* S_plain, const float* S_reflected, int n_supports, float* S_out, void* stream) {
    if (rng_used == nullptr || swap_perm == nullptr || flags == nullptr || perm == nullptr || log_scale == nullptr)
        return fail("augment_draw: null generator pair / swap table / output");
    if (B < 1 || N < 1 || N > kMaxNodes) return fail("augment_draw: B=%d clips, num_nodes=%d unsupported (B >= 1, 1 <= N <= %d)", B, N, kMaxNodes);
    if (S_out != nullptr && (S_plain == nullptr || S_reflected == nullptr || n_supports < 1))
        return fail("augment_draw: per-clip supports need the plain and the reflected set (n_supports=%d)", n_supports);
    EEG_LAUNCH_P("augment_draw", augment_draw_kernel, dim3(B), dim3(128), 0, S_(stream), reinterpret_cast<const unsigned long long*>(rng_used), N,
                 reinterpret_cast<const int*>(swap_perm), reinterpret_cast<int*>(flags), reinterpret_cast<int*>(perm), log_scale, S_plain,
                 S_reflected, n_supports, S_out);
    return check_launch("augment_draw");
}

// corr_launch.h plans a call (instance, grid, LDS, workspace, refusals); the entry points size the workspace and launch by the same plan
size_t eeg_dcrnn_corr_graph_ws_floats(int B, int T) { return corr_gram_plan(B, T, 1, 4, false, g_tune[EEG_TUNE_GRAM_WGS]).ws_floats; }
static int corr_graph(const float* X, int B, int T, int N, int D, int top_k, const int64_t* lengths, float* adj, float* S1, float* S2,
                      float* ws, void* stream) {
    const long long* len = reinterpret_cast<const long long*>(lengths);
    const CorrGramPlan p = corr_gram_plan(B, T, N, D, len != nullptr, g_tune[EEG_TUNE_GRAM_WGS]);
    if (p.error == kCorrBadNodes) return fail("corr_graph: num_nodes=%d unsupported (1..%d)", N, kMaxNodes);
    if (p.error == kCorrBadDim) return fail("corr_graph: feature dim=%d unsupported (positive multiple of 4)", D);
    if (p.error == kCorrEmpty) return fail("corr_graph: empty batch/clip (B=%d, T=%d)", B, T);
    if (top_k < 0 || top_k >= N) return fail("corr_graph: top_k=%d unsupported (0..%d)", top_k, N - 1);
    if (p.error == kCorrStaging) return fail("corr_graph: N*D=%d too large for the per-wave staging buffers", N * D);
    if (p.error == kCorrNoInstance) return fail("corr_graph: feature dim=%d unsupported (<= 128)", D);
    hipStream_t st = S_(stream);
    switch (p.nq) {
        case 1: run_corr_gram<1>(p, X, T, N, D, ws, len, st); break;
        case 2: run_corr_gram<2>(p, X, T, N, D, ws, len, st); break;
        case 3: run_corr_gram<3>(p, X, T, N, D, ws, len, st); break;
        case 4: run_corr_gram<4>(p, X, T, N, D, ws, len, st); break;
        case 5: run_corr_gram<5>(p, X, T, N, D, ws, len, st); break;
        case 6: run_corr_gram<6>(p, X, T, N, D, ws, len, st); break;
        case 7: run_corr_gram<7>(p, X, T, N, D, ws, len, st); break;
        default: run_corr_gram<8>(p, X, T, N, D, ws, len, st); break;
    }
    if (check_launch("corr_gram")) return 1;
    return corr_finish(ws, B, p.ns, N, top_k, adj, S1, S2, st);
}
int eeg_dcrnn_corr_graph(const float* X, int B, int T, int N, int D, int top_k, float* adj, float* S1, float* S2,
                         float* ws, void* stream) {
    return corr_graph(X, B, T, N, D, top_k, nullptr, adj, S1, S2, ws, stream);
}
int eeg_dcrnn_corr_graph_len(const float* X, int B, int T, int N, int D, int top_k, const int64_t* lengths, float* adj, float* S1, float* S2,
                             float* ws, void* stream) {
    if (X == nullptr || ws == nullptr || lengths == nullptr) return fail("corr_graph_len: null input / workspace / lengths");
    if (S1 == nullptr || S2 == nullptr) return fail("corr_graph_len: null output (S1=%p, S2=%p)", (void*)S1, (void*)S2);
    return corr_graph(X, B, T, N, D, top_k, lengths, adj, S1, S2, ws, stream);
}

size_t eeg_dcrnn_corr_graph_rows_ws_floats(int B, int P, int Q) { return corr_rows_plan(B, 1, P, Q, 0, false, 0, g_tune[EEG_TUNE_GRAM_WGS]).ws_floats; }
// lengths != nullptr: `steps` = the steps of a full clip (raw rows: Q = steps * samples per step; window tensors: steps = P)
static int corr_graph_rows(const float* X, int B, int N, int P, int Q, long long piece_stride, int top_k, const int64_t* lengths, int steps,
                           float* adj, float* S1, float* S2, float* ws, void* stream) {
    const long long* len = reinterpret_cast<const long long*>(lengths);
    if (X == nullptr || ws == nullptr) return fail("corr_graph_rows: null input / workspace");
    if (S1 == nullptr || S2 == nullptr) return fail("corr_graph_rows: null output (S1=%p, S2=%p)", (void*)S1, (void*)S2);
    const CorrRowsPlan p = corr_rows_plan(B, N, P, Q, piece_stride, len != nullptr, steps, g_tune[EEG_TUNE_GRAM_WGS]);
    if (p.error == kRowsBadNodes) return fail("corr_graph_rows: num_nodes=%d unsupported (1..%d)", N, kMaxNodes);
    if (p.error == kRowsEmpty) return fail("corr_graph_rows: empty batch/clip (B=%d, pieces=%d)", B, P);
    if (p.error == kRowsBadPiece) return fail("corr_graph_rows: row piece of %d floats unsupported (positive multiple of 4)", Q);
    if (top_k < 0 || top_k >= N) return fail("corr_graph_rows: top_k=%d unsupported (0..%d)", top_k, N - 1);
    if (((uintptr_t)X & 15) != 0) return fail("corr_graph_rows: clips must be 16-byte aligned");
    if (p.error == kRowsPieceStride) return fail("corr_graph_rows: piece stride %lld unsupported (multiple of 4, >= N*Q = %d)", piece_stride, N * Q);
    if (p.error == kRowsTwoGb) return fail("corr_graph_rows: a clip of %lld bytes exceeds the 2 GB one descriptor covers", p.clip_floats * 4);
    if (p.error == kRowsRawSteps) return fail("corr_graph_rows_len: rows of %d floats are not %d steps of a multiple of 4 samples", Q, steps);
    if (p.error == kRowsWindowSteps) return fail("corr_graph_rows_len: steps=%d for a window tensor of %d pieces (a step is a piece)", steps, P);
    hipStream_t st = S_(stream);
    if (p.len) p.rem4 ? run_corr_gram_rows<true, true>(p, X, N, P, Q, ws, len, st) : run_corr_gram_rows<false, true>(p, X, N, P, Q, ws, len, st);
    else p.rem4 ? run_corr_gram_rows<true, false>(p, X, N, P, Q, ws, len, st) : run_corr_gram_rows<false, false>(p, X, N, P, Q, ws, len, st);
    if (check_launch("corr_gram_rows")) return 1;
    return corr_finish(ws, B, p.ns, N, top_k, adj, S1, S2, st);
}
int eeg_dcrnn_corr_graph_rows(const float* X, int B, int N, int P, int Q, long long piece_stride, int top_k, float* adj, float* S1, float* S2,
                              float* ws, void* stream) {
    return corr_graph_rows(X, B, N, P, Q, piece_stride, top_k, nullptr, 0, adj, S1, S2, ws, stream);
}
int eeg_dcrnn_corr_graph_rows_len(const float* X, int B, int N, int P, int Q, long long piece_stride, int top_k, const int64_t* lengths,
                                  int steps, float* adj, float* S1, float* S2, float* ws, void* stream) {
    if (lengths == nullptr) return fail("corr_graph_rows_len: null lengths");
    return corr_graph_rows(X, B, N, P, Q, piece_stride, top_k, lengths, steps, adj, S1, S2, ws, stream);
}

/* ---- decoder ---------------------------------------------------------------------------------- */
static bool dec_dims_positive(const eeg_decoder_dims* d) {
    return d != nullptr && d->T >= 1 && d->B >= 1 && d->N >= 1 && d->H >= 1 && d->Dout >= 1 && d->M >= 1 && d->L >= 1;
}
size_t eeg_dcrnn_decoder_saved_floats(const eeg_decoder_dims* d) { return dec_dims_positive(d) ? dec_layout(d).saved_total : 0; }
size_t eeg_dcrnn_decoder_fwd_ws_floats(const eeg_decoder_dims* d) { return dec_dims_positive(d) ? (size_t)d->B * d->N * 3 * d->H : 0; }
size_t eeg_dcrnn_decoder_bwd_ws_floats(const eeg_decoder_dims* d) { return dec_dims_positive(d) ? dec_layout(d).bwd_total : 0; }

int eeg_dcrnn_decoder_is_persistent(const eeg_decoder_dims* d) {
    if (check_decoder_dims(d)) return 0;
    return dec_plan(dec_call(d)).covered ? 1 : 0;
}

int eeg_dcrnn_decoder_fwd(const eeg_decoder_dims* d, const float* targets, const int32_t* teacher, const float* h0,
                          const float* P, const float* const* packs, const float* Wp, const float* bp,
                          const uint64_t* rng_used, float* out, float* saved, float* ws, void* stream) {
    if (check_decoder_dims(d)) return 1;
    ProfPrefix tag("dec_");
    hipStream_t st = S_(stream);
    const DecLayout y = dec_layout(d);
    const DropCfg drop = make_drop_cfg(d->dropout_p);
    const unsigned long long* used = reinterpret_cast<const unsigned long long*>(rng_used);
    if (drop.on && rng_used == nullptr) return fail("decoder_fwd: dropout_p > 0 needs the {seed, offset} pair of eeg_dcrnn_rng_take");
    const bool tf_dev = d->teacher_on_device != 0 && teacher != nullptr;
    if (tf_dev && targets == nullptr) return fail("decoder_fwd: teacher flags on the device need the target sequence");
    const int B = d->B, N = d->N, H = d->H, M = d->M, Dout = d->Dout, L = d->L, RB = B * N;
    const size_t state = (size_t)RB * H, xstep = (size_t)RB * Dout;
    const int nct_o = ceil_div(Dout, 16);
    float* xin = saved + y.xin;
    float* ppack = saved + y.proj_pack;
    float* pbias = saved + y.proj_bias;
    EEG_LAUNCH_P("pack_cell", pack_linear_kernel, dim3(64), dim3(256), 0, st, Wp, Dout, H, 1, ppack);
    if (check_launch("pack_linear")) return 1;
    if (hipMemsetAsync(pbias, 0, (size_t)nct_o * 16 * sizeof(float), st) != hipSuccess) return fail("decoder_fwd: memset failed");
    if (copy_floats(pbias, bp, Dout, st)) return 1;
    if (hipMemsetAsync(xin, 0, xstep * sizeof(float), st) != hipSuccess) return fail("decoder_fwd: memset failed");   // GO symbol
    for (int l = 0; l < L; ++l)
        if (copy_floats(saved + y.hext[l], h0 + (size_t)l * state, state, st)) return 1;
    // ---- persistent path: ONE launch for all T steps, layers and the projection (kernels_decoder.h); where it does not
    //      apply (dec_plan: hidden size, montage > 20 nodes, LDS, ...) the per-step launches below run
    const DecPlan plan = dec_plan(dec_call(d));
    if (plan.fwd_persistent) {
        DecFwdArgs a;
        for (int l = 0; l < L; ++l) {
            const CellPack p = make_cell_pack(l == 0 ? Dout : H, H, M);
            a.l[l] = DecLayerPtrs{packs[l] + p.bxq, packs[l] + p.bias, packs[l] + p.bhg, packs[l] + p.bhc,
                                  saved + y.hext[l], saved + y.rs[l], saved + y.us[l], saved + y.cs[l], saved + y.rhs[l],
                                  saved + y.hpl[l], saved + y.rpl[l]};
        }
        for (int l = L; l < 4; ++l) a.l[l] = a.l[0];
        a.P = P; a.targets = targets; a.ppack = ppack; a.pbias = pbias;
        a.out = out; a.xin = xin; a.planes0 = saved + y.planes[0];
        a.planes0_stride = (size_t)d->T * RB * Dout;
        a.hplane_stride = (size_t)(d->T + 1) * state;
        a.teacher_mask = 0;
        a.teacher_dev = tf_dev ? reinterpret_cast<const int*>(teacher) : nullptr;
        for (int t = 0; t < d->T && !tf_dev; ++t)
            if (teacher != nullptr && teacher[t] != 0) a.teacher_mask |= 1ull << t;
        a.p_batched = d->p_batched; a.T = d->T; a.B = B; a.N = N; a.Dout = Dout; a.L = L; a.act = d->act;
        a.drop = drop; a.rng_used = used; a.hd = saved + y.hd; a.probe = seq_probe_arg(st);
        return launch_dec_fwd_persist(plan, a, st) ? fail("decoder_fwd: persistent kernel launch failed") : 0;
    }
    if (tf_dev) return fail("decoder_fwd: teacher_on_device needs the persistent decoder kernel, which does not cover this shape "
                            "(H=%d, N=%d, L=%d, T=%d, Dout=%d, M=%d): pass the flags as a host array", H, N, L, d->T, Dout, M);
    float* XW = ws;
    for (int t = 0; t < d->T; ++t) {
        for (int l = 0; l < L; ++l) {
            const int Fin = l == 0 ? Dout : H;
            const size_t Rall = (size_t)d->T * RB, hstride = (size_t)(d->T + 1) * state;
            const float* X = l == 0 ? xin + (size_t)t * xstep : saved + y.hext[l - 1] + (size_t)(t + 1) * state;
            // input hop planes: layer 0 diffuses its input; above, the layer below has just left them behind
            float* planes = l == 0 ? saved + y.planes[0] + (size_t)t * RB * Fin : saved + y.hpl[l - 1] + (size_t)(t + 1) * state;
            const size_t xs = l == 0 ? Rall * Fin : hstride;
            const CellPack p = make_cell_pack(Fin, H, M);
            const float* pack = packs[l];
            if (l == 0 && diffuse_fwd(X, P, d->p_batched, B, B, N, Fin, M, planes, st, xs)) return 1;
            SegPtrs segs;
            for (int m = 0; m < kMaxM; ++m) segs.p[m] = m == 0 ? X : (m < M ? planes + (size_t)(m - 1) * xs : nullptr);
            if (gemm_nn(segs, M, Fin, RB, pack + p.bx, 3 * H / 16, pack + p.bias, XW, 3 * H, 3 * H, st)) return 1;
            float* Hext = saved + y.hext[l];
            SeqFwdArgs a{XW, Hext + (size_t)t * state, P, d->p_batched, pack + p.bhg, pack + p.bhc,
                         Hext + (size_t)(t + 1) * state, saved + y.rs[l] + (size_t)t * state,
                         saved + y.us[l] + (size_t)t * state, saved + y.cs[l] + (size_t)t * state,
                         saved + y.rhs[l] + (size_t)t * state, saved + y.hpl[l] + (size_t)t * state,
                         saved + y.rpl[l] + (size_t)t * state, hstride, 1, B, N, d->act, nullptr};
            if (seq_fwd(H, M, seq_fwd_plan(seq_fwd_call(H, M, N, 1, B, hstride, nullptr)), a, st)) return 1;
        }
        // projection (model.py:188-191): out_t = drop(h_top) W_p^T + b_p
        if (drop.on) {
            EEG_LAUNCH_P("dropout_apply", dropout_apply_kernel, dim3(ceil_div((int)(state / 4), 256)), dim3(256), 0, st,
                         saved + y.hext[L - 1] + (size_t)(t + 1) * state, saved + y.hd + (size_t)t * state, state, (size_t)t * state, used, drop);
            if (check_launch("dropout_apply")) return 1;
        }
        SegPtrs sp;
        for (int m = 0; m < kMaxM; ++m) sp.p[m] = m == 0 ? saved + y.hd + (size_t)t * state : nullptr;
        if (gemm_nn(sp, 1, H, RB, ppack, nct_o, pbias, out + (size_t)t * xstep, Dout, Dout, st)) return 1;
        if (t + 1 < d->T) {   // next decoder input: the projection, or the target under teacher forcing (model.py:194-200)
            const bool tf = teacher != nullptr && teacher[t] != 0;
            if (copy_floats(xin + (size_t)(t + 1) * xstep, tf ? targets + (size_t)t * xstep : out + (size_t)t * xstep, xstep, st)) return 1;
        }
    }
    return 0;
}

int eeg_dcrnn_decoder_bwd(const eeg_decoder_dims* d, const int32_t* teacher, const float* P, const float* const* packs,
                          const float* Wp, const float* saved, const float* dOut, const uint64_t* rng_used, float* dh0,
                          float* const* dWg, float* const* dbg, float* const* dWc, float* const* dbc, float* dWp, float* dbp,
                          float* ws, void* stream) {
    if (check_decoder_dims(d)) return 1;
    ProfPrefix tag("dec_");
    hipStream_t st = S_(stream);
    const DecLayout y = dec_layout(d);
    const DropCfg drop = make_drop_cfg(d->dropout_p);
    const unsigned long long* used = reinterpret_cast<const unsigned long long*>(rng_used);
    if (drop.on && rng_used == nullptr) return fail("decoder_bwd: dropout_p > 0 needs the rng_used pair of the forward call");
    const bool tf_dev = d->teacher_on_device != 0 && teacher != nullptr;
    const int B = d->B, N = d->N, H = d->H, M = d->M, Dout = d->Dout, L = d->L, RB = B * N, T = d->T;
    const size_t state = (size_t)RB * H, xstep = (size_t)RB * Dout, Rall = (size_t)T * RB;
    const int nct_h = ceil_div(H, 16);
    float* tpack = ws + y.projt_pack;
    EEG_LAUNCH_P("pack_cell", pack_linear_kernel, dim3(64), dim3(256), 0, st, Wp, Dout, H, 0, tpack);
    if (check_launch("pack_linear")) return 1;
    float* dOtot = ws + y.dotot;
    float* dA = ws + y.da;
    float* Z = ws + y.z;
    // out_t is step t+1's input (host flags; with device flags the persistent kernel derives the same mask itself)
    auto feeds_back = [&](int t) { return t + 1 < T && !(!tf_dev && teacher != nullptr && teacher[t] != 0); };
    // ---- persistent path: ONE launch walks the T steps backwards (kernels_decoder.h); it leaves dXW of every
    //      (layer, step), dOtot and dh0 -- the hoisted parameter gradients below are common to both paths
    const DecPlan plan = dec_plan(dec_call(d));
    if (plan.bwd_persistent) {
        DecBwdArgs a;
        for (int l = 0; l < L; ++l) {
            const CellPack p = make_cell_pack(l == 0 ? Dout : H, H, M);
            a.l[l] = DecBwdLayerPtrs{packs[l] + p.c1, packs[l] + p.c2, saved + y.hext[l], saved + y.rs[l],
                                     saved + y.us[l], saved + y.cs[l], ws + y.dxw[l]};
        }
        for (int l = L; l < 4; ++l) a.l[l] = a.l[0];
        a.P = P; a.tpack = tpack; a.dOut = dOut; a.dOtot = dOtot; a.dh0 = dh0;
        a.dbias0 = ws + y.dbias[0]; a.dbias1 = ws + y.dbias[L > 1 ? 1 : 0];
        a.feeds_mask = 0;
        a.teacher_dev = tf_dev ? reinterpret_cast<const int*>(teacher) : nullptr;
        for (int t = 0; t < T; ++t)
            if (feeds_back(t)) a.feeds_mask |= 1ull << t;
        a.p_batched = d->p_batched; a.T = T; a.B = B; a.N = N; a.Dout = Dout; a.L = L; a.act = d->act;
        a.drop = drop; a.rng_used = used; a.probe = seq_probe_arg(st);
        if (launch_dec_bwd_persist(plan, a, st)) return fail("decoder_bwd: persistent kernel launch failed");
    }
    if (tf_dev && !plan.bwd_persistent) return fail("decoder_bwd: teacher_on_device needs the persistent decoder kernel, which does not cover "
                                           "this shape (H=%d, N=%d, L=%d, T=%d, Dout=%d, M=%d)", H, N, L, T, Dout, M);
    for (int t = plan.bwd_persistent ? -1 : T - 1; t >= 0; --t) {
        // total gradient of out_t: the loss term, plus (autoregressive feedback) dx of layer 0 at step t+1, which
        // the adjoint diffusion of that step has already added into dOtot[t]
        const float* dO = feeds_back(t) ? dOtot + (size_t)t * xstep : dOut + (size_t)t * xstep;
        if (!feeds_back(t) && copy_floats(dOtot + (size_t)t * xstep, dO, xstep, st)) return 1;   // dense copy for the hoisted GEMM
        SegPtrs sp;
        for (int m = 0; m < kMaxM; ++m) sp.p[m] = m == 0 ? dOtot + (size_t)t * xstep : nullptr;
        if (gemm_nn(sp, 1, Dout, RB, tpack, nct_h, nullptr, dA, H, H, st)) return 1;               // d drop(h_top) = dO W_p
        if (drop.on) {                                                                              // d h_top = mask * that
            EEG_LAUNCH_P("dropout_apply", dropout_apply_kernel, dim3(ceil_div((int)(state / 4), 256)), dim3(256), 0, st, dA, dA, state, (size_t)t * state, used, drop);
            if (check_launch("dropout_apply")) return 1;
        }
        for (int l = L - 1; l >= 0; --l) {
            const int Fin = l == 0 ? Dout : H;
            const CellPack p = make_cell_pack(Fin, H, M);
            const float* pack = packs[l];
            const float* Hext = saved + y.hext[l];
            float* dXW = ws + y.dxw[l] + (size_t)t * RB * 3 * H;
            float* dhn_in = ws + y.dhn + ((size_t)((t + 1) & 1) * L + l) * state;
            float* dhn_out = ws + y.dhn + ((size_t)(t & 1) * L + l) * state;
            SeqBwdArgs a{Hext + (size_t)(t + 1) * state, Hext + (size_t)t * state, saved + y.rs[l] + (size_t)t * state,
                         saved + y.us[l] + (size_t)t * state, saved + y.cs[l] + (size_t)t * state, dA,
                         t == T - 1 ? nullptr : dhn_in, nullptr, nullptr, P, d->p_batched, pack + p.b1, pack + p.b2,
                         dXW, t == 0 ? dh0 + (size_t)l * state : dhn_out, ws + y.dbias[l] + (size_t)t * B * 3 * H,
                         1, B, N, d->act, nullptr};
            if (seq_bwd(H, M, seq_bwd_plan(seq_bwd_call(H, M, N, 1, B, nullptr)), a, st)) return 1;
            const bool need_dx = l > 0 || (t > 0 && feeds_back(t - 1));
            if (need_dx) {
                SegPtrs sd;
                for (int m = 0; m < kMaxM; ++m) sd.p[m] = m == 0 ? dXW : nullptr;
                if (gemm_nn(sd, 1, 3 * H, RB, pack + p.bxt, round_up(M * Fin, 16) / 16, nullptr, Z, M * Fin, M * Fin, st)) return 1;
                if (l > 0) {
                    if (diffuse_adj(Z, P, d->p_batched, B, B, N, Fin, M, dA, st)) return 1;         // -> layer below's h_t
                } else {
                    if (diffuse_adj(Z, P, d->p_batched, B, B, N, Fin, M, dOtot + (size_t)(t - 1) * xstep, st,
                                    dOut + (size_t)(t - 1) * xstep)) return 1;
                }
            }
        }
    }
    // hoisted parameter gradients over all T steps
    for (int l = 0; l < L; ++l) {
        const bool first_use = l <= 1;                    // layers >= 1 share one cell (model.py:126-143)
        const float* X = l == 0 ? saved + y.xin : saved + y.hext[l - 1] + state;
        const size_t hstride = (size_t)(T + 1) * state;
        const float* xpl = l == 0 ? saved + y.planes[0] : saved + y.hpl[l - 1] + state;
        if (cell_weight_grads(&y.ld[l], X, xpl, l == 0 ? Rall * Dout : hstride, saved + y.hext[l], saved + y.rhs[l],
                              ws + y.dxw[l], P, saved + y.hpl[l], saved + y.rpl[l], hstride, nullptr, nullptr,
                              ws + y.partial, y.lw[l], !first_use, dWg[l], dWc[l], st)) return 1;
    }
    if (plan.bwd_persistent) {   // per-clip sums over steps and nodes (layers >= 1 share a cell: already added up)
        if (colsum(ws + y.dbias[0], B, 3 * H, 2 * H, ws + y.colsum, dbg[0], dbc[0], st)) return 1;
        if (L > 1 && colsum(ws + y.dbias[1], B, 3 * H, 2 * H, ws + y.colsum, dbg[1], dbc[1], st)) return 1;
    } else {
        if (colsum(ws + y.dbias[0], T * B, 3 * H, 2 * H, ws + y.colsum, dbg[0], dbc[0], st)) return 1;
        if (L > 1 && colsum(ws + y.dbias[1], (L - 1) * T * B, 3 * H, 2 * H, ws + y.colsum, dbg[1], dbc[1], st)) return 1;
    }
    // projection: dW_p (Dout x H) = sum_rows dOtot^T h_top ;  db_p = column sums of dOtot
    SegPtrs so;
    for (int m = 0; m < kMaxM; ++m) so.p[m] = m == 0 ? dOtot : nullptr;
    if (gemm_tn(y.tp, y.cp, so, saved + y.hd, H, 0, ws + y.partial, st)) return 1;   // (hd = h_top without dropout)
    EEG_LAUNCH_P("reduce_unpack", reduce_unpack_kernel, dim3(ceil_div(Dout * H, 64)), dim3(256), 256 * sizeof(float4), st, ws + y.partial, y.tp.nsplit, Dout, H, 3, Dout, H, 1, dWp, dWp);
    if (check_launch("reduce_unpack(proj)")) return 1;
    return colsum(dOtot, (int)Rall, Dout, Dout, ws + y.colsum, dbp, nullptr, st);
}

int eeg_dcrnn_gather_last(const float* Htop, const int64_t* lengths, int T, int B, int NH, float* last, void* stream) {
    if (T < 1 || B < 1 || NH < 1) return fail("gather_last: empty input (T=%d, B=%d, N*H=%d)", T, B, NH);
    EEG_LAUNCH_P("gather_last", gather_last_kernel, dim3(ceil_div(B * NH, 256)), dim3(256), 0, S_(stream), Htop,
               reinterpret_cast<const long long*>(lengths), T, B, NH, last);
    return check_launch("gather_last");
}
int eeg_dcrnn_dropout_mask(const uint64_t* rng_used, size_t n, float dropout_p, float* mask, void* stream) {
    if (check_dropout_p("dropout_mask", dropout_p)) return 1;
    const DropCfg drop = make_drop_cfg(dropout_p);
    if (drop.on && rng_used == nullptr) return fail("dropout_mask: dropout_p > 0 needs the rng_used pair of a forward call");
    if (n == 0) return 0;
    EEG_LAUNCH_P("dropout_mask", dropout_mask_kernel, dim3(256), dim3(256), 0, S_(stream), reinterpret_cast<const unsigned long long*>(rng_used), n, drop, mask);
    return check_launch("dropout_mask");
}
int eeg_dcrnn_rng_take(uint64_t* rng_state, uint64_t groups, uint64_t* rng_used, void* stream) {
    if (rng_state == nullptr || rng_used == nullptr) return fail("rng_take: null state / output");
    EEG_LAUNCH_P("rng_take", rng_take_kernel, dim3(1), dim3(64), 0, S_(stream), reinterpret_cast<unsigned long long*>(rng_state),
                 reinterpret_cast<unsigned long long*>(rng_used), (unsigned long long)groups);
    return check_launch("rng_take");
}
int eeg_dcrnn_teacher_flags(uint64_t* rng_state, int64_t* samples_seen, int64_t increment, double cl_decay_steps, int T,
                            int32_t* flags, void* stream) {
    if (rng_state == nullptr || samples_seen == nullptr || flags == nullptr) return fail("teacher_flags: null state / counter / output");
    if (T < 1 || T > 64) return fail("teacher_flags: T=%d unsupported (1..64)", T);
    if (!(cl_decay_steps > 0.0)) return fail("teacher_flags: cl_decay_steps must be positive");
    EEG_LAUNCH_P("teacher_flags", teacher_flags_kernel, dim3(1), dim3(64), 0, S_(stream), reinterpret_cast<unsigned long long*>(rng_state),
                 reinterpret_cast<long long*>(samples_seen), (long long)increment, cl_decay_steps, T, reinterpret_cast<int*>(flags));
    return check_launch("teacher_flags");
}
int eeg_dcrnn_teacher_flags_dev(uint64_t* rng_state, int64_t* samples_seen, const int64_t* increment, double cl_decay_steps, int T,
                                int32_t* flags, void* stream) {
    if (rng_state == nullptr || samples_seen == nullptr || flags == nullptr) return fail("teacher_flags_dev: null state / counter / output");
    if (increment == nullptr) return fail("teacher_flags_dev: null increment (a device int64[1])");
    if (T < 1 || T > 64) return fail("teacher_flags_dev: T=%d unsupported (1..64)", T);
    if (!(cl_decay_steps > 0.0)) return fail("teacher_flags_dev: cl_decay_steps must be positive");
    EEG_LAUNCH_P("teacher_flags", teacher_flags_dev_kernel, dim3(1), dim3(64), 0, S_(stream), reinterpret_cast<unsigned long long*>(rng_state),
                 reinterpret_cast<long long*>(samples_seen), reinterpret_cast<const long long*>(increment), cl_decay_steps, T,
                 reinterpret_cast<int*>(flags));
    return check_launch("teacher_flags_dev");
}
int eeg_dcrnn_cls_head_fwd(const float* z, const float* W, const float* bias, int B, int N, int H, int C, float dropout_p,
                           const uint64_t* rng_used, float* logits, int32_t* arg, void* stream) {
    if (N > 64) return fail("cls_head: num_nodes=%d unsupported (<= 64)", N);
    if (H % 4 != 0) return fail("cls_head: rnn_units=%d must be a multiple of 4", H);
    if (check_dropout_p("cls_head", dropout_p)) return 1;
    const DropCfg drop = make_drop_cfg(dropout_p);
    if (drop.on && rng_used == nullptr) return fail("cls_head: dropout_p > 0 needs the {seed, offset} pair of eeg_dcrnn_rng_take");
    // LDS: [N][C] node logits + [N][H] masked relu(z) rows
    const size_t head_lds = (size_t)N * (C + H) * sizeof(float);
    if (B < 1 || C < 1 || head_lds > kMaxLdsBytes) return fail("cls_head: B=%d, N=%d x (classes=%d + rnn_units=%d) floats do not fit the %zu-byte LDS", B, N, C, H, (size_t)kMaxLdsBytes);
    EEG_SET_MAX_LDS(cls_head_fwd_kernel, head_lds);
    EEG_LAUNCH_P("cls_head_fwd", cls_head_fwd_kernel, dim3(B), dim3(64), head_lds, S_(stream), z, W, bias, B, N, H, C, drop,
                 reinterpret_cast<const unsigned long long*>(rng_used), logits, arg);
    return check_launch("cls_head_fwd");
}
int eeg_dcrnn_cls_head_bwd(const float* z, const float* W, const float* dlogits, const int32_t* arg, int B, int N,
                           int H, int C, float dropout_p, const uint64_t* rng_used, float* dz, float* dW, float* dbias, void* stream) {
    if (check_dropout_p("cls_head_bwd", dropout_p)) return 1;
    const DropCfg drop = make_drop_cfg(dropout_p);
    if (drop.on && rng_used == nullptr) return fail("cls_head_bwd: dropout_p > 0 needs the rng_used pair of the forward call");
    if (B < 1 || N < 1 || H < 1 || C < 1) return fail("cls_head_bwd: empty input (B=%d, N=%d, H=%d, C=%d)", B, N, H, C);
    const unsigned long long* used = reinterpret_cast<const unsigned long long*>(rng_used);
    EEG_LAUNCH_P("cls_head_bwd_dz", cls_head_bwd_dz_kernel, dim3(ceil_div(B * N * H, 256)), dim3(256), 0, S_(stream), z, W, dlogits, arg, B, N, H, C, drop, used, dz);
    if (check_launch("cls_head_bwd_dz")) return 1;
    EEG_LAUNCH_P("cls_head_bwd_w", cls_head_bwd_w_kernel, dim3(ceil_div(C * H + C, 16)), dim3(256), 256 * sizeof(float), S_(stream), z, dlogits, arg, B, N, H, C, drop, used, dW, dbias);
    return check_launch("cls_head_bwd_w");
}

size_t eeg_dcrnn_cls_head_loss_ws_floats(int B, int H, int C) {
    return (B >= 1 && H >= 1 && C >= 1) ? (size_t)ceil_div(B, 4) * ((size_t)C * H + C + 1) : 0;
}
// clip_w != nullptr: the weighted head (eeg_dcrnn_cls_head_loss_w; multiply: eeg_dcrnn_cls_head_loss_cw), else the plain one -- the same
// checks and launch shapes
static int cls_head_loss_launch(const float* z, const float* W, const float* bias, const void* targets, int kind, int B, int N, int H, int C,
                                float dropout_p, const uint64_t* rng_used, const float* clip_w, const float* denom, bool multiply, float* logits,
                                int32_t* arg, float* dlogits, float* dz, float* dW, float* dbias, float* loss, float* ws, void* stream) {
    if (B < 1 || N < 1 || H < 1 || C < 1) return fail("cls_head_loss: empty input (B=%d, N=%d, H=%d, C=%d)", B, N, H, C);
    if (N > 64) return fail("cls_head_loss: num_nodes=%d unsupported (<= 64)", N);
    if (H % 4 != 0) return fail("cls_head_loss: rnn_units=%d must be a multiple of 4", H);
    if (kind != 0 && kind != 1) return fail("cls_head_loss: kind=%d (0 = BCE-with-logits, 1 = cross-entropy)", kind);
    if (kind == 0 && C != 1) return fail("cls_head_loss: BCE-with-logits takes one logit per clip (num_classes=%d)", C);
    if (check_dropout_p("cls_head_loss", dropout_p)) return 1;
    const DropCfg drop = make_drop_cfg(dropout_p);
    if (drop.on && rng_used == nullptr) return fail("cls_head_loss: dropout_p > 0 needs the {seed, offset} pair of eeg_dcrnn_rng_take");
    if (z == nullptr || W == nullptr || bias == nullptr || targets == nullptr || logits == nullptr || arg == nullptr || dlogits == nullptr ||
        dz == nullptr || dW == nullptr || dbias == nullptr || loss == nullptr || ws == nullptr)
        return fail("cls_head_loss: null pointer");
    const int O = C * H + C, nblk = ceil_div(B, 4);
    const size_t lds = (size_t)(4 * cls_tail_wave_floats(N, H, C) + 4 * (O + 1)) * sizeof(float);
    if (lds > kMaxLdsBytes) return fail("cls_head_loss: N=%d x (classes=%d + rnn_units=%d) floats of four clips do not fit the %zu-byte LDS", N, C, H, (size_t)kMaxLdsBytes);
    if (clip_w != nullptr && multiply) {
        EEG_SET_MAX_LDS(cls_head_loss_cw_kernel, lds);
        EEG_LAUNCH_P("cls_head_loss", cls_head_loss_cw_kernel, dim3(nblk), dim3(256), lds, S_(stream), z, W, bias, targets, kind, B, N, H, C, drop,
                     reinterpret_cast<const unsigned long long*>(rng_used), clip_w, denom, logits, reinterpret_cast<int*>(arg), dlogits, dz, ws);
        if (check_launch("cls_head_loss_cw")) return 1;
        EEG_LAUNCH_P("cls_head_loss", cls_head_loss_w_finish_kernel, dim3(1), dim3(256), 0, S_(stream), ws, nblk, denom, H, C, dW, dbias, loss);
        return check_launch("cls_head_loss_cw_finish");
    }
    if (clip_w != nullptr) {
        EEG_SET_MAX_LDS(cls_head_loss_w_kernel, lds);
        EEG_LAUNCH_P("cls_head_loss", cls_head_loss_w_kernel, dim3(nblk), dim3(256), lds, S_(stream), z, W, bias, targets, kind, B, N, H, C, drop,
                     reinterpret_cast<const unsigned long long*>(rng_used), clip_w, denom, logits, reinterpret_cast<int*>(arg), dlogits, dz, ws);
        if (check_launch("cls_head_loss_w")) return 1;
        EEG_LAUNCH_P("cls_head_loss", cls_head_loss_w_finish_kernel, dim3(1), dim3(256), 0, S_(stream), ws, nblk, denom, H, C, dW, dbias, loss);
        return check_launch("cls_head_loss_w_finish");
    }
    EEG_SET_MAX_LDS(cls_head_loss_kernel, lds);
    EEG_LAUNCH_P("cls_head_loss", cls_head_loss_kernel, dim3(nblk), dim3(256), lds, S_(stream), z, W, bias, targets, kind, B, N, H, C, drop,
                 reinterpret_cast<const unsigned long long*>(rng_used), logits, reinterpret_cast<int*>(arg), dlogits, dz, ws);
    if (check_launch("cls_head_loss")) return 1;
    EEG_LAUNCH_P("cls_head_loss", cls_head_loss_finish_kernel, dim3(1), dim3(256), 0, S_(stream), ws, nblk, B, H, C, dW, dbias, loss);
    return check_launch("cls_head_loss_finish");
}
int eeg_dcrnn_cls_head_loss(const float* z, const float* W, const float* bias, const void* targets, int kind, int B, int N, int H, int C,
                            float dropout_p, const uint64_t* rng_used, float* logits, int32_t* arg, float* dlogits, float* dz,
                            float* dW, float* dbias, float* loss, float* ws, void* stream) {
    return cls_head_loss_launch(z, W, bias, targets, kind, B, N, H, C, dropout_p, rng_used, nullptr, nullptr, false, logits, arg, dlogits, dz, dW,
                                dbias, loss, ws, stream);
}
int eeg_dcrnn_cls_head_loss_w(const float* z, const float* W, const float* bias, const void* targets, int kind, int B, int N, int H, int C,
                              float dropout_p, const uint64_t* rng_used, const float* clip_w, const float* denom, float* logits, int32_t* arg,
                              float* dlogits, float* dz, float* dW, float* dbias, float* loss, float* ws, void* stream) {
    if (clip_w == nullptr || denom == nullptr) return fail("cls_head_loss_w: null clip_w / denom");
    return cls_head_loss_launch(z, W, bias, targets, kind, B, N, H, C, dropout_p, rng_used, clip_w, denom, false, logits, arg, dlogits, dz, dW,
                                dbias, loss, ws, stream);
}
int eeg_dcrnn_cls_head_loss_cw(const float* z, const float* W, const float* bias, const void* targets, int kind, int B, int N, int H, int C,
                               float dropout_p, const uint64_t* rng_used, const float* clip_u, const float* denom, float* logits, int32_t* arg,
                               float* dlogits, float* dz, float* dW, float* dbias, float* loss, float* ws, void* stream) {
    if (clip_u == nullptr || denom == nullptr) return fail("cls_head_loss_cw: null clip_u / denom");
    return cls_head_loss_launch(z, W, bias, targets, kind, B, N, H, C, dropout_p, rng_used, clip_u, denom, true, logits, arg, dlogits, dz, dW,
                                dbias, loss, ws, stream);
}
size_t eeg_dcrnn_dconv_fwd_ws_floats(int B, int N, int F, int M, int O) {
    if (B < 1 || N < 1 || F < 1 || M < 1 || O < 1) return 0;
    return (size_t)(M - 1) * B * N * F + (size_t)F * M * O;
}
int eeg_dcrnn_dconv_fwd(const float* X, const float* P, int p_batched, int B, int N, int F, int M,
                        const float* W, const float* bias, int O, float* out, float* ws, void* stream) {
    if (N < 1 || N > kMaxNodes || F < 4 || F % 4 != 0 || M < 1 || M > kMaxM) return fail("dconv_fwd: bad dims N=%d F=%d M=%d", N, F, M);
    if (B < 1) return fail("dconv_fwd: empty batch (B=%d)", B);
    if (O % 16 != 0) return fail("dconv_fwd: output_dim=%d must be a multiple of 16", O);
    hipStream_t st = S_(stream);
    float* planes = ws;
    float* pack = ws + (size_t)(M - 1) * B * N * F;
    if (diffuse_fwd(X, P, p_batched, B, B, N, F, M, planes, st)) return 1;
    EEG_LAUNCH_P("pack_dense", pack_dense_kernel, dim3(256), dim3(256), 0, st, W, F, M, O, pack);
    if (check_launch("pack_dense")) return 1;
    SegPtrs segs;
    for (int m = 0; m < kMaxM; ++m) segs.p[m] = m == 0 ? X : (m < M ? planes + (size_t)(m - 1) * B * N * F : nullptr);
    return gemm_nn(segs, M, F, B * N, pack, O / 16, bias, out, O, O, st);
}
size_t eeg_dcrnn_dconv_bwd_ws_floats(int B, int N, int F, int M, int O) {
    if (B < 1 || N < 1 || F < 1 || M < 1 || O < 1) return 0;
    const int R = B * N;
    const int nsplit = gemm_tn_plan(tn_call(M, F, R, O)).nsplit;
    return (size_t)(M - 1) * R * F + align64((size_t)nsplit * M * F * O) + align64((size_t)(O / 4) * (round_up(M * F, 16) / 16) * 64)
           + (size_t)R * M * F + align64(colsum_ws(R, O));
}
int eeg_dcrnn_dconv_bwd(const float* X, const float* P, int p_batched, int B, int N, int F, int M, const float* W, int O,
                        const float* dOut, float* dX, float* dW, float* dbias, float* ws, void* stream) {
    if (N < 1 || N > kMaxNodes || F < 4 || F % 4 != 0 || M < 1 || M > kMaxM) return fail("dconv_bwd: bad dims N=%d F=%d M=%d", N, F, M);
    if (B < 1) return fail("dconv_bwd: empty batch (B=%d)", B);
    if (O % 16 != 0 || O > 192) return fail("dconv_bwd: output_dim=%d must be a multiple of 16 (<= 192)", O);
    hipStream_t st = S_(stream);
    const int R = B * N;
    const TnCall cw = tn_call(M, F, R, O);
    const TnPlan tw = gemm_tn_plan(cw);
    const int nsplit = tw.nsplit;
    float* planes = ws;
    float* part = planes + (size_t)(M - 1) * R * F;
    float* tpack = part + align64((size_t)nsplit * M * F * O);
    float* Z = tpack + align64((size_t)(O / 4) * (round_up(M * F, 16) / 16) * 64);
    float* cws = Z + (size_t)R * M * F;
    // dW[f*M+m][o] = sum_rows (P_m X)[row][f] dOut[row][o]: the hop planes are re-formed here (nothing is kept by the forward)
    if (dW != nullptr) {
        if (diffuse_fwd(X, P, p_batched, B, B, N, F, M, planes, st)) return 1;
        SegPtrs sx;
        for (int m = 0; m < kMaxM; ++m) sx.p[m] = m == 0 ? X : (m < M ? planes + (size_t)(m - 1) * R * F : nullptr);
        if (gemm_tn(tw, cw, sx, dOut, O, 0, part, st)) return 1;
        EEG_LAUNCH_P("reduce_unpack", reduce_unpack_kernel, dim3(ceil_div(M * F * O, 64)), dim3(256), 256 * sizeof(float4), st, part, nsplit, M * F, O, 4, F, 0, M, dW, dW);
        if (check_launch("reduce_unpack(dconv)")) return 1;
    }
    if (dbias != nullptr && colsum(dOut, R, O, O, cws, dbias, nullptr, st)) return 1;
    // dX = Z_0 + sum_m P_m^T Z_m with Z = dOut W^T (R x M*F, hop-major)
    if (dX != nullptr) {
        EEG_LAUNCH_P("pack_dense", pack_dense_t_kernel, dim3(256), dim3(256), 0, st, W, F, M, O, tpack);
        if (check_launch("pack_dense_t")) return 1;
        SegPtrs sd;
        for (int m = 0; m < kMaxM; ++m) sd.p[m] = m == 0 ? dOut : nullptr;
        if (gemm_nn(sd, 1, O, R, tpack, round_up(M * F, 16) / 16, nullptr, Z, M * F, M * F, st)) return 1;
        if (diffuse_adj(Z, P, p_batched, B, B, N, F, M, dX, st)) return 1;
    }
    return 0;
}
int eeg_dcrnn_bce_logits(const float* logits, const float* y, int B, float* loss, float* dlogits, void* stream) {
    if (B < 1) return fail("bce_logits: empty batch");
    EEG_LAUNCH_P("loss_bce", bce_logits_kernel, dim3(1), dim3(256), 256 * sizeof(float), S_(stream), logits, y, B, loss, dlogits);
    return check_launch("bce_logits");
}
int eeg_dcrnn_ce_logits(const float* logits, const int64_t* y, int B, int C, float* loss, float* dlogits, void* stream) {
    if (B < 1 || C < 1) return fail("ce_logits: empty batch");
    EEG_LAUNCH_P("loss_ce", ce_logits_kernel, dim3(1), dim3(256), 256 * sizeof(float), S_(stream), logits,
                 reinterpret_cast<const long long*>(y), B, C, loss, dlogits);
    return check_launch("ce_logits");
}
int eeg_dcrnn_bce_logits_w(const float* logits, const float* y, int B, const float* clip_w, const float* denom, float* loss, float* dlogits,
                           void* stream) {
    if (B < 1) return fail("bce_logits_w: empty batch");
    if (clip_w == nullptr || denom == nullptr) return fail("bce_logits_w: null clip_w / denom");
    EEG_LAUNCH_P("loss_bce", bce_logits_w_kernel, dim3(1), dim3(256), 256 * sizeof(float), S_(stream), logits, y, B, clip_w, denom, loss, dlogits);
    return check_launch("bce_logits_w");
}
int eeg_dcrnn_ce_logits_w(const float* logits, const int64_t* y, int B, int C, const float* clip_w, const float* denom, float* loss,
                          float* dlogits, void* stream) {
    if (B < 1 || C < 1) return fail("ce_logits_w: empty batch");
    if (clip_w == nullptr || denom == nullptr) return fail("ce_logits_w: null clip_w / denom");
    EEG_LAUNCH_P("loss_ce", ce_logits_w_kernel, dim3(1), dim3(256), 256 * sizeof(float), S_(stream), logits,
                 reinterpret_cast<const long long*>(y), B, C, clip_w, denom, loss, dlogits);
    return check_launch("ce_logits_w");
}
int eeg_dcrnn_bce_logits_cw(const float* logits, const float* y, int B, const float* clip_u, const float* denom, float* loss, float* dlogits,
                            void* stream) {
    if (B < 1) return fail("bce_logits_cw: empty batch");
    if (logits == nullptr || y == nullptr || loss == nullptr || dlogits == nullptr) return fail("bce_logits_cw: null logits / y / loss / dlogits");
    if (clip_u == nullptr || denom == nullptr) return fail("bce_logits_cw: null clip_u / denom");
    EEG_LAUNCH_P("loss_bce", bce_logits_cw_kernel, dim3(1), dim3(256), 256 * sizeof(float), S_(stream), logits, y, B, clip_u, denom, loss, dlogits);
    return check_launch("bce_logits_cw");
}
int eeg_dcrnn_ce_logits_cw(const float* logits, const int64_t* y, int B, int C, const float* clip_u, const float* denom, float* loss,
                           float* dlogits, void* stream) {
    if (B < 1 || C < 1) return fail("ce_logits_cw: empty batch");
    if (logits == nullptr || y == nullptr || loss == nullptr || dlogits == nullptr) return fail("ce_logits_cw: null logits / y / loss / dlogits");
    if (clip_u == nullptr || denom == nullptr) return fail("ce_logits_cw: null clip_u / denom");
    EEG_LAUNCH_P("loss_ce", ce_logits_cw_kernel, dim3(1), dim3(256), 256 * sizeof(float), S_(stream), logits,
                 reinterpret_cast<const long long*>(y), B, C, clip_u, denom, loss, dlogits);
    return check_launch("ce_logits_cw");
}
/* ---- the step's per-clip multipliers and their divisor (class / sample weights), written on the device ---- */
int eeg_dcrnn_clip_weights(const void* labels, int label_bytes, const int64_t* perm, int64_t n_perm, int64_t P, const int64_t* cursor, int64_t back,
                           int B, int rank, int world, const float* class_w, int C, const float* sample_w, int norm, float* clip_u, float* denom,
                           void* stream) {
    if (labels == nullptr || clip_u == nullptr || denom == nullptr) return fail("clip_weights: null labels / clip_u / denom");
    if (label_bytes != 4 && label_bytes != 8) return fail("clip_weights: label_bytes=%d unsupported (4: float 0/1 labels, 8: int64 classes)", label_bytes);
    if (B < 1 || world < 1 || rank < 0 || rank >= world) return fail("clip_weights: B=%d, rank=%d, world=%d unsupported (B >= 1, 0 <= rank < world)", B, rank, world);
    if (norm != kWeightNormSum && norm != kWeightNormCount) return fail("clip_weights: norm=%d (0 = sum of the weights, 1 = count of the clips)", norm);
    if ((class_w == nullptr) != (C == 0) || C < 0) return fail("clip_weights: class_w and C=%d disagree (no class weights: NULL and 0)", C);
    if (class_w != nullptr && label_bytes == 4 && C != 2) return fail("clip_weights: float labels are 0 / 1: C=%d class weights (2)", C);
    if ((((uintptr_t)labels) & (uintptr_t)(label_bytes == 8 ? 7 : 3)) != 0 || (((uintptr_t)perm | (uintptr_t)cursor) & 7) != 0 ||
        (((uintptr_t)class_w | (uintptr_t)sample_w | (uintptr_t)clip_u | (uintptr_t)denom) & 3) != 0)
        return fail("clip_weights: labels / perm / cursor / class_w / sample_w / clip_u / denom must be aligned to their element size");
    long long slots = B;
    if (perm != nullptr) {       // the sampler form: the label pool through perm and the cursor
        if (cursor == nullptr) return fail("clip_weights: perm without cursor");
        if (P < 1 || n_perm < 1) return fail("clip_weights: P=%lld clips, n_perm=%lld entries (both >= 1)", (long long)P, (long long)n_perm);
        slots = (long long)B * world;
        if (back != 0 && back != slots) return fail("clip_weights: back=%lld (0: ahead of the gather, B*world=%lld: behind it)", (long long)back, slots);
    } else {                     // the batch form: the batch's own labels, the rank's own divisor
        if (cursor != nullptr || sample_w != nullptr || back != 0) return fail("clip_weights: cursor / sample_w / back belong to the sampler form (perm is NULL)");
        rank = 0;
        world = 1;
    }
    EEG_LAUNCH_P("clip_weights", clip_weights_kernel, dim3(1), dim3(kClipWeightThreads), kClipWeightThreads * sizeof(double), S_(stream), labels, label_bytes,
                 reinterpret_cast<const long long*>(perm), (long long)n_perm, (long long)P, reinterpret_cast<const long long*>(cursor), (long long)back, B,
                 (long long)rank * B, slots, world, class_w, C, sample_w, norm, clip_u, denom);
    return check_launch("clip_weights");
}
size_t eeg_dcrnn_masked_loss_ws_floats(void) { return 2 * kLossBlocks + 64; }
int eeg_dcrnn_masked_loss(const float* pred, const float* y, size_t n, int use_scaler, float mean, float std_,
                          float mask_val, int kind, float* loss, float* dpred, float* ws, void* stream) {
    if (n < 1) return fail("masked_loss: empty tensors");
    if (kind != 0 && kind != 1) return fail("masked_loss: kind=%d unsupported (0 = MAE, 1 = RMSE)", kind);
    hipStream_t st = S_(stream);
    int nblk = (int)((n + 256 * 8 - 1) / (256 * 8));
    if (nblk > kLossBlocks) nblk = kLossBlocks;
    // 16-byte accesses need 16-byte aligned tensors (torch allocations are; views with an odd offset are not)
    if (((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(dpred)) & 15) != 0)
        return fail("masked_loss: tensors must be 16-byte aligned");
    EEG_LAUNCH_P("loss_masked", masked_loss_partial_kernel, dim3(nblk), dim3(256), 512 * sizeof(float), st, pred, y, n, mean, std_, use_scaler, mask_val, kind, ws);
    if (check_launch("masked_loss_partial")) return 1;
    EEG_LAUNCH_P("loss_masked", masked_loss_finish_kernel, dim3(1), dim3(256), 512 * sizeof(float), st, ws, nblk, kind, loss);
    if (check_launch("masked_loss_finish")) return 1;
    if (dpred != nullptr) {
        EEG_LAUNCH_P("loss_masked", masked_loss_grad_kernel, dim3(nblk * 2), dim3(256), 0, st, pred, y, n, mean, std_, use_scaler, mask_val, kind, ws, dpred);
        if (check_launch("masked_loss_grad")) return 1;
    }
    return 0;
}
int eeg_dcrnn_masked_loss_w(const float* pred, const float* y, size_t n, int B, const float* clip_w, const float* denom, int use_scaler,
                            float mean, float std_, float mask_val, int kind, float* loss, float* dpred, float* ws, void* stream) {
    if (n < 1) return fail("masked_loss_w: empty tensors");
    if (kind != 0 && kind != 1) return fail("masked_loss_w: kind=%d unsupported (0 = MAE, 1 = RMSE)", kind);
    if (B < 1 || n % (size_t)B != 0) return fail("masked_loss_w: n=%zu elements are not B=%d clips of equal size", n, B);
    if (clip_w == nullptr || denom == nullptr) return fail("masked_loss_w: null clip_w / denom");
    hipStream_t st = S_(stream);
    int nblk = (int)((n + 256 * 8 - 1) / (256 * 8));
    if (nblk > kLossBlocks) nblk = kLossBlocks;
    if (((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(dpred)) & 15) != 0)
        return fail("masked_loss_w: tensors must be 16-byte aligned");
    const ClipWeights cw{clip_w, n / (size_t)B};
    EEG_LAUNCH_P("loss_masked", masked_loss_w_partial_kernel, dim3(nblk), dim3(256), 512 * sizeof(float), st, pred, y, n, mean, std_, use_scaler, mask_val, kind, ws, cw);
    if (check_launch("masked_loss_w_partial")) return 1;
    EEG_LAUNCH_P("loss_masked", masked_loss_w_finish_kernel, dim3(1), dim3(256), 768 * sizeof(float), st, ws, nblk, kind, loss, B, clip_w, denom);
    if (check_launch("masked_loss_w_finish")) return 1;
    if (dpred != nullptr) {
        EEG_LAUNCH_P("loss_masked", masked_loss_w_grad_kernel, dim3(nblk * 2), dim3(256), 0, st, pred, y, n, mean, std_, use_scaler, mask_val, kind, ws, dpred, cw);
        if (check_launch("masked_loss_w_grad")) return 1;
    }
    return 0;
}
size_t eeg_dcrnn_clip_adam_ws_floats(void) { return 64; }
static int clip_adam_launch(float* params, float* grads, float* exp_avg, float* exp_avg_sq, size_t n, float max_norm, float lr,
                            float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale, float* ws,
                            float* norm_out, int32_t* step_dev, const float* lr_dev, void* stream) {
    const int nparts = 64;
    if (n < 1) return fail("clip_adam: empty parameter buffer");
    EEG_LAUNCH_P("grad_sqnorm", sqnorm_partial_kernel, dim3(nparts), dim3(256), 256 * sizeof(float), S_(stream), grads, n, ws, reinterpret_cast<int*>(step_dev));
    if (check_launch("grad_sqnorm")) return 1;
    // torch.optim.Adam forms `1 - beta ** step` and its square root as Python (fp64) scalars
    const float bc1 = step_dev ? 1.f : (float)(1.0 - pow((double)beta1, (double)step));
    const float bc2s = step_dev ? 1.f : (float)sqrt(1.0 - pow((double)beta2, (double)step));
    int blocks = (int)((n + 1023) / 1024);
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;
    EEG_LAUNCH_P("clip_adam", clip_adam_kernel, dim3(blocks), dim3(256), 0, S_(stream), params, grads, exp_avg, exp_avg_sq, n,
                 ws, nparts, max_norm, lr, beta1, beta2, eps, weight_decay, bc1, bc2s, grad_scale, norm_out,
                 reinterpret_cast<const int*>(step_dev), lr_dev);
    return check_launch("clip_adam");
}
int eeg_dcrnn_clip_adam(float* params, float* grads, float* exp_avg, float* exp_avg_sq, size_t n, float max_norm,
                        float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                        float grad_scale, float* ws, float* norm_out, void* stream) {
    if (step < 1) return fail("clip_adam: step must be >= 1");
    return clip_adam_launch(params, grads, exp_avg, exp_avg_sq, n, max_norm, lr, beta1, beta2, eps, weight_decay, step, grad_scale, ws,
                            norm_out, nullptr, nullptr, stream);
}
int eeg_dcrnn_clip_adam_dev(float* params, float* grads, float* exp_avg, float* exp_avg_sq, size_t n, float max_norm,
                            const float* lr_dev, float beta1, float beta2, float eps, float weight_decay, int32_t* step_dev,
                            float grad_scale, float* ws, float* norm_out, void* stream) {
    if (lr_dev == nullptr || step_dev == nullptr) return fail("clip_adam_dev: null learning-rate / step-counter pointer");
    return clip_adam_launch(params, grads, exp_avg, exp_avg_sq, n, max_norm, 0.f, beta1, beta2, eps, weight_decay, 0, grad_scale, ws,
                            norm_out, step_dev, lr_dev, stream);
}

}  // extern "C"
