// Launch plan of the persistent decoder kernels (kernels_decoder.h: dec_fwd_persist_kernel<64, M>, dec_bwd_persist_kernel<64, M, DT, CX0>):
// the operands of the two kernels, the LDS geometry they and the plan share, and dec_plan -- whether a decoder is covered and, if so,
// with what template integers, grid, block and LDS bytes.  A pure function of the call (no global is read: the dev knobs come in
// through it); every selection rule of the family is stated here and nowhere else.  The callers in api.cpp ask for the plan BEFORE
// they lay out operands; the launchers of dec_inst.cpp / decb_inst.cpp, declared at the end, execute it and are never handed a
// decoder that is not covered.  No kernel bodies: this header compiles as plain host C++ (tests/emu/gemm_plan_driver.cpp prints
// the plans, tests/golden/dec_plans_v1.json pins them).
#pragma once
#include "common.h"
#include "nnq_order.h"

namespace eeg {

// ---- kernel operands ------------------------------------------------------------------------------------------------------------
struct DecLayerPtrs {
    const float *bxq, *bias, *bhg, *bhc;                      // weight packs of the layer's cell (kernels_pack.h; bxq: the x-part in quad order)
    float *hext, *rs, *us, *cs, *rhs, *hpl, *rpl;             // saved for the backward (decoder `saved` layout)
};
struct DecFwdArgs {
    DecLayerPtrs l[4];
    const float* P;
    const float* targets;         // (T,B,N,Dout), read where teacher_mask says so (may be NULL when the mask is 0)
    const float *ppack, *pbias;   // projection: fragment pack (K = H, nct_o column tiles) and zero-padded bias
    float *out, *xin, *planes0;   // (T,B,N,Dout) predictions, step inputs, and the hop planes of the step inputs (M-1 planes)
    size_t planes0_stride;        // floats between two planes of planes0
    size_t hplane_stride;         // floats between two planes of hpl / rpl = (T+1)*B*N*H
    unsigned long long teacher_mask;   // bit t: step t+1 is fed targets[t] instead of out[t] (model.py:194-200)
    const int* teacher_dev;            // nullable DEVICE int32[T]: when set, the flags are read from it at launch instead (a captured
                                       // graph then replays with whatever eeg_dcrnn_teacher_flags drew in front of it)
    int p_batched, T, B, N, Dout, L, act;
    // nn.Dropout in front of the projection (model.py:191, training): the projection reads drop(h_top_t) = mask * h_top_t; the
    // recurrence keeps h_top_t.  Element ((t*B + b)*N + n)*H + h of the (T,B,N,H) top outputs takes word e % 4 of Philox counter
    // rng_used[1] + e / 4 under key rng_used[0] (common.h).  hd (T,B,N,H): the dropped rows, the A operand of dW_p in the backward.
    DropCfg drop;
    const unsigned long long* rng_used;
    float* hd;
    long long* probe;             // phase cycles (development builds with -DEEG_DEC_PROBE: tools/dec_probe.py), else unused
};
struct DecBwdLayerPtrs {
    const float *c1, *c2;                            // weight packs [hidden | input] (kernels_pack.h)
    const float *hext, *rs, *us, *cs;                // saved by the forward
    float* dxw;                                      // (T,B,N,3H) out
};
struct DecBwdArgs {
    DecBwdLayerPtrs l[4];
    const float* P;
    const float* tpack;           // projection, transposed role: K = Dout, H/16 column tiles
    const float* dOut;            // (T,B,N,Dout) loss gradient
    float* dOtot;                 // (T,B,N,Dout) total gradient of out_t (loss + feedback)
    float* dh0;                   // (L,B,N,H)
    float *dbias0, *dbias1;       // (B,3H) per-clip bias-gradient sums [r|u|c] over steps and nodes: layer 0, layers >= 1 (one shared cell)
    unsigned long long feeds_mask;     // bit t: out_t is the input of step t+1 (no teacher forcing there, t+1 < T)
    const int* teacher_dev;            // nullable DEVICE int32[T] teacher-forcing flags: when set, feeds_mask is derived from it at launch
    int p_batched, T, B, N, Dout, L, act;
    DropCfg drop;                      // dropout in front of the projection (DecFwdArgs): d h_top = mask * (dO W_p), mask recomputed
    const unsigned long long* rng_used;
    long long* probe;                  // phase cycles (development builds with -DEEG_DEC_PROBE), else unused
};

// ---- LDS geometry of the kernels (they carve their dynamic LDS by the same functions) ---------------------------------------------
// 16-deep chunks of a quad-packed x-part (nnq_order.h) padded to whole groups of 4: the weight ring of gemm_stream_nnq
__host__ __device__ inline int nnq_padded_chunks(int nseg, int F) { return round_up(make_nnq_order(nseg, F).nch, 4); }
// LDS floats of dec_fwd_persist_kernel<64, M>
__host__ __device__ constexpr size_t dec_fwd_lds_floats(int M, int L, int Dout) {
    const int H = 64, KAP = M * H, XS = lds_stride_q(M * round_up(Dout, 16));
    return (size_t)(M - 1) * kPFloats + (size_t)L * kDecRows * KAP + (size_t)kDecRows * (XS > KAP ? XS : KAP)
           + (size_t)kDecRows * 64       // + the dropped copy of the top state the projection reads (swizzled [rows][64])
           + 4 * (size_t)nnq_padded_chunks(M, Dout);   // + the piece-column table of the layer-0 x-part (gemm_stream_nnq)
}
// LDS floats of dec_bwd_persist_kernel<64, M, DT, CX0>
__host__ __device__ constexpr size_t dec_bwd_lds_floats(int M, int L, int Dout) {
    const int H = 64, FS = lds_stride_q(round_up(Dout, 16));
    return (size_t)(M - 1) * kPFloats + (size_t)kDecRows * (M * H + M * 2 * H) + 2 * (size_t)kDecRows * FS
           + (size_t)L * 4 * 2 * 256;
}

// ---- the plan -------------------------------------------------------------------------------------------------------------------
struct DecCall {
    int T, B, N, H, Dout, M, L;
    // dev knobs (include/eeg_dcrnn_dev.h; compile-time zeros in the product build)
    int knob_fwd_per_step = 0;      // EEG_TUNE_DEC_FWD_PER_STEP = 1: the forward as T x L per-step launches
    int knob_bwd_per_step = 0;      // EEG_TUNE_DEC_BWD_PER_STEP = 1: the backward likewise
};
struct DecPlan {
    bool covered;                   // the shape rule alone (eeg_dcrnn_decoder_is_persistent): forward and backward pair up over `saved`
    bool fwd_persistent, bwd_persistent;    // covered, and the direction's knob is 0; else that direction runs per step
    int M, dt, cx0;                 // dec_fwd_persist_kernel<64, M>, dec_bwd_persist_kernel<64, M, dt, cx0>
    int grid, block;
    size_t lds_fwd, lds_bwd;        // bytes of dynamic LDS
};

constexpr int kDecMaxGrid = 256;    // one workgroup per clip up to one per CU; more clips are walked by the resident workgroups
// k-steps per weight group of the backward's projection transpose: 5 where Dout / 4 is a multiple of 5, else 4; 0: neither divides
constexpr int dec_dt(int Dout) { return (Dout / 4) % 5 == 0 ? 5 : ((Dout / 4) % 4 == 0 ? 4 : 0); }
// column tiles of layer 0's c1 / c2 packs: 12 up to 128 outputs, 16 up to 192, 20 up to 256
constexpr int dec_cx0(int Dout) { return cell_pack_cx_cols(Dout, 64) / 16; }
// The compiled instances: the forward per hop count M, the backward per (M, DT in {4, 5}, CX0) -- the wide packs (CX0 > 12) up to
// M = 5 only: the LDS tiles of M = 7 do not fit at any such width.  decb_inst.cpp instantiates by this predicate.
constexpr bool dec_has_instance(int M, int cx0) { return (M >= 1 && M <= 5 && (cx0 == 12 || cx0 == 16 || cx0 == 20)) || (M == 7 && cx0 == 12); }

// Covered: 64 units, at most 20 nodes, 4 layers, 64 steps (the flag masks are 64 bits) and 256 outputs with Dout / 4 a multiple of 4
// or 5, a compiled instance, and both kernels within the LDS of a CU -- past 128 outputs that decides: M = 5 with two layers fits up
// to 200 outputs, M = 5 with three layers does not (table in DESIGN.md 4.4).  The clip count is no rule.
inline DecPlan dec_plan(const DecCall& c) {
    DecPlan p{};
    p.M = c.M; p.dt = dec_dt(c.Dout); p.cx0 = dec_cx0(c.Dout);
    p.grid = c.B < kDecMaxGrid ? c.B : kDecMaxGrid; p.block = 256;
    if (c.H != 64 || c.N > kDecRows || c.L < 1 || c.L > 4 || c.T < 1 || c.T > 64 || c.Dout > 256 || p.dt == 0 || !dec_has_instance(c.M, p.cx0)) return p;
    p.lds_fwd = dec_fwd_lds_floats(c.M, c.L, c.Dout) * sizeof(float);
    p.lds_bwd = dec_bwd_lds_floats(c.M, c.L, c.Dout) * sizeof(float);
    p.covered = p.lds_fwd <= kMaxLdsBytes && p.lds_bwd <= kMaxLdsBytes;
    p.fwd_persistent = p.covered && c.knob_fwd_per_step == 0;
    p.bwd_persistent = p.covered && c.knob_bwd_per_step == 0;
    return p;
}

// the launchers of dec_inst.cpp / decb_inst.cpp execute the plan of a covered decoder: the template switch and the launch; 0 ok, 1 launch error
int launch_dec_fwd_persist(const DecPlan& p, const DecFwdArgs& a, hipStream_t st);
int launch_dec_bwd_persist(const DecPlan& p, const DecBwdArgs& a, hipStream_t st);

}  // namespace eeg
