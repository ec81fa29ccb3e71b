// Host-side launch interface of the templated recurrent kernels: operands, the launch plan that selects among them, and the entry
// points of the instantiation units.  The (H, M) instantiations are compiled in separate translation units (seq_inst.cpp, one per
// H; seqs_inst.cpp) to keep build times parallel.
#pragma once
#include "kernels_seq.h"   // the family's geometry and existence predicates

namespace eeg {

// Kernel operands only; which kernel takes them is the plan's business (below).
struct SeqFwdArgs {
    // h0 == nullptr: zero initial state; the kernel then clears the (B,N,H) slot in FRONT of Hseq (Hext slot 0)
    const float *XW, *h0, *P;
    int p_batched;
    const float *bhg, *bhc;
    float *Hseq, *Rs, *Us, *Cs, *RHs;
    float *Hpl, *RHpl;      // optional by-product: hop planes P_m h_{t-1} / P_m (r*h_{t-1}), plane m at + (m-1)*plane_stride
    size_t plane_stride;
    int T, B, N, act;
    long long* probe;
    // SeqKind::TwoWaveSpec only (spectral form, spec_common.h): XW = the pre-activations in the eigenbasis, Yh (N, spec_Sp, 3H) node-major
    // with the bias inside; Hpl = Hh (N, spec_SpE, H) <- U^T h_slot (row slot*B + b, slots 0..T) and RHpl = RHh (N, spec_Sp, H) <-
    // U^T (r*h_{t-1}) (both nullable) instead of hop planes; plane_stride = 0
    const float* spec_U = nullptr;
    int spec_Sp = 0, spec_SpE = 0;
};
struct SeqBwdArgs {
    const float *Hseq, *h0, *Rs, *Us, *Cs, *dHseq, *d_at_end, *d_at_len;
    const long long* lengths;
    const float* P;
    int p_batched;
    const float *b1, *b2;
    float *dXW, *dh0, *dbias_part;
    int T, B, N, act;
    long long* probe;
    // SeqKind::TwoWaveSpec only: the kernel writes dYh = U^T dXW (node-major (N, spec_Sp, 3H); row of (t, b) = t*B + b) INSTEAD of dXW
    const float* spec_U = nullptr;
    float* dYh = nullptr;
    int spec_Sp = 0;
};

// ---- launch plans: which recurrent kernel takes a call, with what geometry ------------------------------------------------
// Pure functions of the call (no global is read); every selection rule of the family is stated here and nowhere else.  The
// instantiation units execute a plan, the callers in api.cpp ask for it BEFORE they lay out operands (SPEC or not, dYh or dXW).
enum class SeqKind { OneWave, TwoWave, TwoWaveSpec, Stream };   // seq_*_kernel, seq_*2_kernel, its SPEC form, seq_bwd_stream_kernel
enum SeqPlanError { kSeqOk = 0, kSeqNoKernel, kSeqNoFit };      // nothing compiled for (H, M) / the LDS of a CU is exceeded
struct SeqPlan {
    SeqKind kind;
    bool probe;             // the dev build's cycle-probe instantiation of `kind`
    int nks, block, grid;
    size_t lds;             // bytes of dynamic LDS
    int error;
};
struct SeqCall {
    int H, M, N, T, B;
    size_t plane_stride = 0;    // forward: floats between the hop planes the kernel leaves behind
    bool spectral = false;      // the caller can take the SPEC form: a spectral layer with Sp / SpE transformed rows (spec_common.h)
    int Sp = 0, SpE = 0;
    // dev knobs (include/eeg_dcrnn_dev.h; compile-time zeros in the product build)
    int knob_one_wave = 0;      // EEG_TUNE_SEQ_FWD_ONE_WAVE / _BWD_ONE_WAVE = 1: no two-wave kernel (backward: no streamed one either)
    int knob_no_spec = 0;       // EEG_TUNE_SEQ_FWD_NO_SPEC / _BWD_NO_SPEC = 1: the general-path kernels under the spectral form
    int knob_stream = 0;        // EEG_TUNE_SEQ_STREAM: 1 = the streamed kernel wherever it exists, 2 = never
    bool probe = false;         // dev build: the launch carries the armed phase probe
};

constexpr bool seq_h_supported(int H) { return H == 16 || H == 32 || H == 64; }
constexpr bool seq_m_supported(int M) { return M == 1 || M == 2 || M == 3 || M == 4 || M == 5 || M == 7; }
// the kernels reach these many floats through ONE buffer descriptor (32-bit offsets): under 2 GB
inline bool seq_desc_reaches(double floats) { return floats * sizeof(float) < 2147483648.0; }
// The SPEC form of a two-wave kernel: 16 to 20 nodes, dXW / Yh / dYh (3H wide) and Hh each within a descriptor; with the probe
// armed, only where the SPEC probe instantiation exists.
inline bool seq_spec_applies(const SeqCall& c, int nks) {
    return seq_has_spec(c.H, c.M, nks) && c.spectral && c.knob_no_spec == 0 && c.N >= 16 && seq_desc_reaches((double)c.T * c.B * c.N * 3 * c.H) &&
           seq_desc_reaches((double)c.N * c.Sp * 3 * c.H) && seq_desc_reaches((double)c.N * c.SpE * c.H) && (!c.probe || seq_has_probe(c.H, c.M, nks));
}
// the probe instantiation of the chosen kind where it exists; the one-wave one only when the knob asked for one wave
inline bool seq_probe_applies(const SeqCall& c, const SeqPlan& p) {
    return c.probe && seq_has_probe(c.H, c.M, p.nks) && (p.kind != SeqKind::OneWave || c.knob_one_wave != 0);
}
constexpr int kSeqMaxGrid = 256;   // one workgroup per CU; larger batches are walked by the resident workgroups
constexpr int kStreamGrid = 512;   // streamed weights: two workgroups per CU

inline SeqPlan seq_fwd_plan(const SeqCall& c) {
    SeqPlan p{SeqKind::OneWave, false, seq_nks(c.N), 256, c.B < kSeqMaxGrid ? c.B : kSeqMaxGrid, 0, kSeqOk};
    if (!seq_h_supported(c.H) || !seq_m_supported(c.M)) { p.error = kSeqNoKernel; return p; }
    p.lds = seq_fwd_lds_floats(c.H, c.M) * sizeof(float);
    if (p.lds > kMaxLdsBytes) { p.error = kSeqNoFit; return p; }
    // two waves per SIMD: its stores and the hop planes it leaves behind go through descriptors
    if (seq_has_two_wave(c.H, c.M, p.nks) && c.knob_one_wave == 0 && seq_desc_reaches((double)c.T * c.B * c.N * c.H) &&
        seq_desc_reaches((double)(c.M - 1) * c.plane_stride)) {
        p.kind = seq_spec_applies(c, p.nks) ? SeqKind::TwoWaveSpec : SeqKind::TwoWave;
        p.block = 512;
        p.lds = seq_fwd2_lds_floats(c.H, c.M, p.kind == SeqKind::TwoWaveSpec) * sizeof(float);
    }
    p.probe = seq_probe_applies(c, p);
    return p;
}
inline SeqPlan seq_bwd_plan(const SeqCall& c) {
    SeqPlan p{SeqKind::OneWave, false, seq_nks(c.N), 256, c.B < kSeqMaxGrid ? c.B : kSeqMaxGrid, 0, kSeqOk};
    if (!seq_h_supported(c.H) || !seq_m_supported(c.M)) { p.error = kSeqNoKernel; return p; }
    const bool dxw_reached = seq_desc_reaches((double)c.T * c.B * c.N * 3 * c.H);
    // BPTT with more clips than 1.5 x the CUs at hop counts the two-wave kernel does not cover: two streamed-weight workgroups
    // per CU (kernels_seq_stream.h), where two of them fit the LDS; else the rules below apply as if it had not been wanted
    const size_t lds_stream = seq_stream_bwd_lds_floats(c.M) * sizeof(float);
    if (c.knob_one_wave == 0 && !c.probe && seq_has_stream(c.H, c.M) && c.N <= kDecRows && c.knob_stream != 2 &&
        (c.knob_stream == 1 || (c.M >= 4 && c.B >= 384)) && 2 * lds_stream <= kMaxLdsBytes && dxw_reached) {
        p.kind = SeqKind::Stream;
        p.grid = c.B < kStreamGrid ? c.B : kStreamGrid;
        p.lds = lds_stream;
        return p;
    }
    if (seq_has_two_wave(c.H, c.M, p.nks) && c.knob_one_wave == 0 && dxw_reached) {
        p.kind = seq_spec_applies(c, p.nks) ? SeqKind::TwoWaveSpec : SeqKind::TwoWave;
        p.block = 512;
        p.lds = seq_bwd2_lds_floats(c.H, c.M) * sizeof(float);
    } else {
        p.lds = seq_bwd_lds_floats(c.H, c.M, seq_bwd_rows(c.H, c.M, p.nks)) * sizeof(float);
        if (p.lds > kMaxLdsBytes) p.error = kSeqNoFit;
    }
    p.probe = seq_probe_applies(c, p);
    return p;
}

// the instantiation units execute a plan without an error: 0 ok, 1 launch error
int launch_seq_fwd_h16(int M, const SeqPlan& p, const SeqFwdArgs& a, hipStream_t st);
int launch_seq_fwd_h32(int M, const SeqPlan& p, const SeqFwdArgs& a, hipStream_t st);
int launch_seq_fwd_h64(int M, const SeqPlan& p, const SeqFwdArgs& a, hipStream_t st);
int launch_seq_bwd_h16(int M, const SeqPlan& p, const SeqBwdArgs& a, hipStream_t st);
int launch_seq_bwd_h32(int M, const SeqPlan& p, const SeqBwdArgs& a, hipStream_t st);
int launch_seq_bwd_h64(int M, const SeqPlan& p, const SeqBwdArgs& a, hipStream_t st);
int launch_seq_bwd_stream(int M, const SeqPlan& p, const SeqBwdArgs& a, hipStream_t st);   // SeqKind::Stream

}  // namespace eeg
