// TEST INFRASTRUCTURE: prints the launch plans of csrc/gemm_launch.h, csrc/spec_launch.h, csrc/seq_launch.h, csrc/dec_launch.h,
// csrc/diffuse_launch.h and csrc/corr_launch.h for the calls read from stdin, one line each (see tests/test_gemm_plans.py,
// tests/test_spec_plans.py, tests/test_seq_kernels.py, tests/test_dec_plans.py, tests/test_diffuse_corr_plans.py).  Host code only:
// gemm_launch.h, spec_launch.h, dec_launch.h, diffuse_launch.h and corr_launch.h must compile without kernel bodies; seq_launch.h
// brings kernels_seq.h along, which is host code under platform_emu.h.
//   nn   nseg F R nct_total ldc O batch_major quad_pack bf3_nct num_cus KNOBS  ->  kind t1 t2 t3 gx gy block lds error
//   tn   nseg F R O batch_major offer_quad num_cus KNOBS                       ->  kind t1 t2 t3 nsplit rps gx gy block lds remap error
//   pair M H R num_cus KNOBS   (the two h-part problems of a cell)             ->  1 / 0: one paired launch or not
// KNOBS = keys 0 1 2 4 14 15 16 19 of include/eeg_dcrnn_dev.h.  t1..t3 are the template integers of the kind; a plan with an
// error prints zeros for what never reaches a launch.
// The spectral family (SKNOBS = keys 20 23 17) prints each launch as `kernel symbol ; grid.x grid.y block lds`, the symbol as the
// event recorder spells it, launches and trailing fields joined by " ; "; a plan with an error prints `error <code>`:
//   sup  T B N H Fin M need_dx            ->  1 / 0: spec_supported
//   mix  to_nodes N T B F node_rows       ->  launch
//   snn  K Sp G nct num_cus SKNOBS        ->  launch
//   stn  Fin H Sp G num_cus SKNOBS        ->  launch (fused) or x-part launch ; pair launch, then spg_x rps_x spg_h rps_h px pg pc
//   sdx  Fin N T B num_cus SKNOBS         ->  launch (fused) or grouped NN launch ; mix launch, then needs_dxh
// The recurrent family: every field of SeqCall in its order, dev knobs and the probe flag included (has_* asks the predicates of
// kernels_seq.h the plans are built on):
//   sfwd H M N T B plane_stride spectral Sp SpE one_wave no_spec stream probe   ->  kind probe nks block grid lds error
//   sbwd (the same fields)                                                      ->  kind probe nks block grid lds error
//   shas H M N                                          ->  nks two_wave spec probe stream h_supported m_supported dev_build
// The persistent decoder: every field of DecCall in its order; a direction that does not run persistently prints `per_step` in
// place of its launch:
//   dec  T B N H Dout M L knob_fwd knob_bwd   ->  covered ; fwd: kernel symbol ; grid 1 block lds ; bwd: likewise
// The hop diffusion: every field of DiffuseCall in its order, the direction being the op (DKNOBS = keys 5 6 9 18).  `none`: no launch
// (one hop matrix, no copy); the LDS kernels go out once per column chunk: `x<launches> <columns per chunk>` behind the launch:
//   dfwd p_batched S B N F M x_bt wants_copy DKNOBS   ->  none | launch | launch ; x<count> fc | error <code>
//   dadj (the same fields)                            ->  likewise
// The correlation Gram (knob = key 7): the Gram launch, the finish launch and the floats of workspace between them:
//   gram  B T N D has_len knob                        ->  launch ; corr_finish_kernel ; B 1 256 lds ; ws_floats | error <code>
//   grows B N P Q piece_stride has_len steps knob     ->  likewise
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "corr_launch.h"
#include "dec_launch.h"
#include "diffuse_launch.h"
#include "gemm_launch.h"
#include "spec_launch.h"
#include "seq_launch.h"
using namespace eeg;

static bool knobs(GemmKnobs& k) {
    return scanf("%d %d %d %d %d %d %d %d", &k.nn_staged, &k.tn_staged, &k.quad, &k.tn_xcd, &k.tn_wide_from, &k.tn_target, &k.tnq_target, &k.tn_no_pair) == 8;
}
void nn_line(const NnCall& c, char* out) {
    const NnPlan p = gemm_nn_plan(c);
    if (p.error) { sprintf(out, "0 0 0 0 0 0 0 0 %d", p.error); return; }
    const int t[4][3] = {{kNnrStages, 2, 0}, {p.nctw, p.kc, p.minb}, {p.nctw, p.kc, 0}, {p.nctw, 0, 0}};   // Quad, Dma, Staged, Bf3
    const int* k = t[(int)p.kind];
    sprintf(out, "%d %d %d %d %d %d %d %zu 0", (int)p.kind, k[0], k[1], k[2], p.gx, p.gy, p.block, p.lds);
}
void tn_line(const TnCall& c, char* out) {
    const TnPlan p = gemm_tn_plan(c);
    if (p.error) { sprintf(out, "0 0 0 0 %d %d 0 0 0 0 0 %d", p.nsplit, p.rps, p.error); return; }
    const int t[4][3] = {{p.q.KT, p.q.OT, p.q.planar}, {p.nctw, p.rc, p.wk}, {p.nctw, p.rc, p.wk}, {p.nctw, 0, 0}};   // Quad, Dma, DmaWide, Staged
    const int* k = t[(int)p.kind];
    sprintf(out, "%d %d %d %d %d %d %d %d %d %zu %d 0", (int)p.kind, k[0], k[1], k[2], p.nsplit, p.rps, p.gx, p.gy, p.block, p.lds, p.remap);
}
int pair_line(int M, int H, int R, int num_cus, const GemmKnobs& k) {
    const TnCall g{M, H, R, 2 * H, false, true, num_cus, k}, c{M, H, R, H, false, true, num_cus, k};
    return tn_pair_applies(gemm_tn_plan(g), gemm_tn_plan(c), k) ? 1 : 0;
}

static bool sknobs(SpecKnobs& k) { return scanf("%d %d %d", &k.nn_grouped, &k.tn_separate, &k.dx_passes) == 3; }
static int launch(char* out, const char* symbol, int gx, int gy, int block, size_t lds) { return sprintf(out, "%s ; %d %d %d %zu", symbol, gx, gy, block, lds); }
int mix_launch(const SpecMixPlan& p, char* out) {
    char sym[64];
    if (p.kind == SpecMixKind::Mfma) sprintf(sym, "spec_mix_mfma_kernel<%d, %d>", 1 - p.to_nodes, p.ks);
    else sprintf(sym, p.kind == SpecMixKind::Valu19 ? (p.to_nodes ? "spec_mix_in_kernel<19>" : "spec_mix_out_kernel<19>") : "spec_mix_generic_kernel");
    return launch(out, sym, p.grid, 1, p.block, p.lds);
}
int snn_launch(const SpecNnPlan& p, char* out) {
    char sym[64];
    if (p.error) return sprintf(out, "error %d", p.error);
    if (p.kind == SpecNnKind::Regs) sprintf(sym, "gemm_nnf_kernel<%d, %s>", p.kq, p.swz ? "true" : "false");
    else sprintf(sym, "gemm_nng_kernel<%d, 2>", p.nj);
    return launch(out, sym, p.grid, 1, p.block, p.lds);
}
void stn_line(const SpecTnPlan& p, char* out) {
    char sym[64];
    if (p.error) { sprintf(out, "error %d", p.error); return; }
    if (p.fused) {
        sprintf(sym, "gemm_tnf_kernel<%d>", p.fxt);
        out += launch(out, sym, p.grid_x, p.grid_y, p.block, p.lds_x);
    } else {
        sprintf(sym, "gemm_tnq_grouped_kernel<%d, %d, %d, %s>", p.KT, kSpecTngOt, kSpecTngRc, p.planar ? "true" : "false");
        out += launch(out, sym, p.grid_x, p.grid_y, p.block, p.lds_x);
        out += sprintf(out, " ; ");
        sprintf(sym, "gemm_tnq_grouped_pair_kernel<2, %d, true>", kSpecTngRc);
        out += launch(out, sym, 1, p.grid_h, p.block, p.lds_h);
    }
    sprintf(out, " ; %d %d %d %d %zu %zu %zu", p.spg_x, p.rps_x, p.spg_h, p.rps_h, p.px, p.pg, p.pc);
}
void sdx_line(const SpecDxPlan& p, char* out) {
    if (p.error) { sprintf(out, "error %d", p.error); return; }
    if (p.kind == SpecDxKind::Fused) {
        out += launch(out, p.nt == 19 ? "gemm_dxf_kernel<19>" : "gemm_dxf_kernel<0>", p.grid, 1, p.block, p.lds);
    } else {
        out += snn_launch(p.nn, out);
        out += sprintf(out, " ; ");
        out += mix_launch(p.mix, out);
    }
    sprintf(out, " ; %d", p.needs_dxh ? 1 : 0);
}
// one spectral line; false: not a spectral op.  A malformed line ends the run (exit 2).
static bool spec_line(const char* op, char* out) {
    int a[7];
    SpecKnobs k;
    if (!strcmp(op, "sup")) {
        if (scanf("%d %d %d %d %d %d %d", &a[0], &a[1], &a[2], &a[3], &a[4], &a[5], &a[6]) != 7) exit(2);
        sprintf(out, "%d", spec_supported(a[0], a[1], a[2], a[3], a[4], a[5], a[6]) ? 1 : 0);
    } else if (!strcmp(op, "mix")) {
        if (scanf("%d %d %d %d %d %d", &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]) != 6) exit(2);
        mix_launch(spec_mix_plan(a[0], a[1], a[2], a[3], a[4], a[5]), out);
    } else if (!strcmp(op, "snn")) {
        if (scanf("%d %d %d %d %d", &a[0], &a[1], &a[2], &a[3], &a[4]) != 5 || !sknobs(k)) exit(2);
        snn_launch(spec_nn_plan(a[0], a[1], a[2], a[3], a[4], k), out);
    } else if (!strcmp(op, "stn")) {
        if (scanf("%d %d %d %d %d", &a[0], &a[1], &a[2], &a[3], &a[4]) != 5 || !sknobs(k)) exit(2);
        stn_line(spec_tn_plan(a[0], a[1], a[2], a[3], a[4], k), out);
    } else if (!strcmp(op, "sdx")) {
        if (scanf("%d %d %d %d %d", &a[0], &a[1], &a[2], &a[3], &a[4]) != 5 || !sknobs(k)) exit(2);
        sdx_line(spec_dx_plan(a[0], a[1], a[2], a[3], a[4], k), out);
    } else {
        return false;
    }
    return true;
}

// one recurrent-family line; false: not such an op
static bool seq_line(const char* op, char* out) {
    if (!strcmp(op, "shas")) {
        int H, M, N;
        if (scanf("%d %d %d", &H, &M, &N) != 3) exit(2);
        const int nks = seq_nks(N);
        sprintf(out, "%d %d %d %d %d %d %d %d", nks, seq_has_two_wave(H, M, nks) ? 1 : 0, seq_has_spec(H, M, nks) ? 1 : 0, seq_has_probe(H, M, nks) ? 1 : 0,
                seq_has_stream(H, M) ? 1 : 0, seq_h_supported(H) ? 1 : 0, seq_m_supported(M) ? 1 : 0, kDevBuild ? 1 : 0);
        return true;
    }
    if (strcmp(op, "sfwd") && strcmp(op, "sbwd")) return false;
    SeqCall c{};
    int spectral, probe;
    if (scanf("%d %d %d %d %d %zu %d %d %d %d %d %d %d", &c.H, &c.M, &c.N, &c.T, &c.B, &c.plane_stride, &spectral, &c.Sp, &c.SpE, &c.knob_one_wave,
              &c.knob_no_spec, &c.knob_stream, &probe) != 13) exit(2);
    c.spectral = spectral != 0; c.probe = probe != 0;
    const SeqPlan p = op[1] == 'f' ? seq_fwd_plan(c) : seq_bwd_plan(c);
    sprintf(out, "%d %d %d %d %d %zu %d", (int)p.kind, p.probe ? 1 : 0, p.nks, p.block, p.grid, p.lds, p.error);
    return true;
}

// one persistent-decoder line; false: not such an op
static bool dec_line(const char* op, char* out) {
    if (strcmp(op, "dec")) return false;
    DecCall c{};
    if (scanf("%d %d %d %d %d %d %d %d %d", &c.T, &c.B, &c.N, &c.H, &c.Dout, &c.M, &c.L, &c.knob_fwd_per_step, &c.knob_bwd_per_step) != 9) exit(2);
    const DecPlan p = dec_plan(c);
    char sym[64];
    out += sprintf(out, "%d ; fwd: ", p.covered ? 1 : 0);
    sprintf(sym, "dec_fwd_persist_kernel<64, %d>", p.M);
    out += p.fwd_persistent ? launch(out, sym, p.grid, 1, p.block, p.lds_fwd) : sprintf(out, "per_step");
    out += sprintf(out, " ; bwd: ");
    sprintf(sym, "dec_bwd_persist_kernel<64, %d, %d, %d>", p.M, p.dt, p.cx0);
    out += p.bwd_persistent ? launch(out, sym, p.grid, 1, p.block, p.lds_bwd) : sprintf(out, "per_step");
    return true;
}

// one hop-diffusion line; false: not such an op
static bool diffuse_line(const char* op, char* out) {
    if (strcmp(op, "dfwd") && strcmp(op, "dadj")) return false;
    DiffuseCall c{};
    int copy;
    if (scanf("%d %d %d %d %d %d %d %d %d %d %d %d", &c.p_batched, &c.S, &c.B, &c.N, &c.F, &c.M, &c.x_bt, &copy, &c.fwd_wgs, &c.adj_wgs, &c.adj_lds,
              &c.adj_planes) != 12) exit(2);
    c.adjoint = op[1] == 'a'; c.wants_copy = copy != 0;
    const DiffusePlan p = diffuse_plan(c);
    char sym[64];
    if (p.error) { sprintf(out, "error %d", p.error); return true; }
    switch (p.kind) {
        case DiffuseKind::None: sprintf(out, "none"); return true;
        case DiffuseKind::StreamFwd: launch(out, "diffuse_fwd_stream_kernel<19>", p.gx, p.gy, p.block, p.lds); return true;
        case DiffuseKind::StreamAdj: launch(out, "diffuse_adj_stream_kernel<19>", p.gx, p.gy, p.block, p.lds); return true;
        case DiffuseKind::RowsAdj: sprintf(sym, "diffuse_adj_rows_kernel<19, %d>", p.mm); launch(out, sym, p.gx, p.gy, p.block, p.lds); return true;
        default: break;
    }
    out += launch(out, p.kind == DiffuseKind::LdsFwd ? "diffuse_fwd_kernel" : "diffuse_adj_kernel", p.gx, p.gy, p.block, p.lds);
    sprintf(out, " ; x%d %d", p.nchunks, p.fc);
    return true;
}

// one correlation-Gram line; false: not such an op
static bool corr_line(const char* op, char* out) {
    char sym[64];
    int B, T, N, D, P, Q, has_len, steps, knob, error, gy;
    size_t lds, ws;
    if (!strcmp(op, "gram")) {
        if (scanf("%d %d %d %d %d %d", &B, &T, &N, &D, &has_len, &knob) != 6) exit(2);
        const CorrGramPlan p = corr_gram_plan(B, T, N, D, has_len != 0, knob);
        sprintf(sym, "corr_gram_kernel<%d, %s, %s>", p.nq, p.rem4 ? "true" : "false", p.len ? "true" : "false");
        error = p.error; gy = p.gy; lds = p.lds; ws = p.ws_floats;
    } else if (!strcmp(op, "grows")) {
        long long piece_stride;
        if (scanf("%d %d %d %d %lld %d %d %d", &B, &N, &P, &Q, &piece_stride, &has_len, &steps, &knob) != 8) exit(2);
        const CorrRowsPlan p = corr_rows_plan(B, N, P, Q, piece_stride, has_len != 0, steps, knob);
        sprintf(sym, "corr_gram_rows_kernel<%s, %s>", p.rem4 ? "true" : "false", p.len ? "true" : "false");
        error = p.error; gy = p.gy; lds = p.lds; ws = p.ws_floats;
    } else {
        return false;
    }
    if (error) { sprintf(out, "error %d", error); return true; }
    out += launch(out, sym, B, gy, 256, lds);
    out += sprintf(out, " ; ");
    out += launch(out, "corr_finish_kernel", B, 1, 256, corr_finish_lds_bytes());
    sprintf(out, " ; %zu", ws);
    return true;
}

int main() {
    char op[8], out[512];
    while (scanf("%7s", op) == 1) {
        int bm, quad;
        if (spec_line(op, out) || seq_line(op, out) || dec_line(op, out) || diffuse_line(op, out) || corr_line(op, out)) {
        } else if (!strcmp(op, "nn")) {
            NnCall c{};
            if (scanf("%d %d %d %d %d %d %d %d %d %d", &c.nseg, &c.F, &c.R, &c.nct_total, &c.ldc, &c.O, &bm, &quad, &c.bf3_nct, &c.num_cus) != 10 || !knobs(c.knobs)) return 2;
            c.batch_major = bm != 0; c.quad_pack = quad != 0;
            nn_line(c, out);
        } else if (!strcmp(op, "tn")) {
            TnCall c{};
            if (scanf("%d %d %d %d %d %d %d", &c.nseg, &c.F, &c.R, &c.O, &bm, &quad, &c.num_cus) != 7 || !knobs(c.knobs)) return 2;
            c.batch_major = bm != 0; c.offer_quad = quad != 0;
            tn_line(c, out);
        } else {
            int M, H, R, cus;
            GemmKnobs k;
            if (strcmp(op, "pair") || scanf("%d %d %d %d", &M, &H, &R, &cus) != 4 || !knobs(k)) return 2;
            sprintf(out, "%d", pair_line(M, H, R, cus, k));
        }
        puts(out);
    }
    return 0;
}
