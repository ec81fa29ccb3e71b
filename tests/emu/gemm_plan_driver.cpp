// TEST INFRASTRUCTURE: prints the launch plans of csrc/gemm_launch.h for the calls read from stdin, one line each (see
// tests/test_gemm_plans.py).  Host code only: the header must compile without kernel bodies.
//   nn   nseg F R nct_total ldc O batch_major quad_pack bf3_nct num_cus KNOBS  ->  kind t1 t2 t3 gx gy block lds error
//   tn   nseg F R O batch_major offer_quad num_cus KNOBS                       ->  kind t1 t2 t3 nsplit rps gx gy block lds remap error
//   pair M H R num_cus KNOBS   (the two h-part problems of a cell)             ->  1 / 0: one paired launch or not
// KNOBS = keys 0 1 2 4 14 15 16 19 of include/eeg_dcrnn_dev.h.  t1..t3 are the template integers of the kind; a plan with an
// error prints zeros for what never reaches a launch.
#include <cstdio>
#include <cstring>

#include "gemm_launch.h"
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

int main() {
    char op[8], out[256];
    while (scanf("%7s", op) == 1) {
        int bm, quad;
        if (!strcmp(op, "nn")) {
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
