// Instantiations of the persistent decoder backward kernel (kernels_decoder.h), in their own translation unit.
#include "kernels_decoder.h"
#include "prof.h"
#include "seq_launch.h"

namespace eeg {
namespace {
constexpr int kCxNarrow = cell_pack_cx_cols(64, 64) / 16;
template <int M, int DT, int CX0>
int launch_one(const DecBwdArgs& a, size_t lds, hipStream_t st) {
    EEG_SET_MAX_LDS((dec_bwd_persist_kernel<64, M, DT, CX0>), lds);
    EEG_LAUNCH_P("bwd_persist", (dec_bwd_persist_kernel<64, M, DT, CX0>), dim3(a.B < 256 ? a.B : 256), dim3(256), lds, st, a);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}
template <int M, int CX0>
int launch_cx(int dt, const DecBwdArgs& a, size_t lds, hipStream_t st) {
    return dt == 5 ? launch_one<M, 5, CX0>(a, lds, st) : launch_one<M, 4, CX0>(a, lds, st);
}
template <int M>
int launch_m(int dt, const DecBwdArgs& a, size_t lds, hipStream_t st) { return launch_cx<M, kCxNarrow>(dt, a, lds, st); }
// more than 128 outputs: the wide instantiations, by the column tiles of layer 0's c1 / c2 packs (16 up to 192 outputs, 20 up to 256)
template <int M>
int launch_w(int dt, const DecBwdArgs& a, size_t lds, hipStream_t st) {
    if (a.Dout <= 128) return launch_m<M>(dt, a, lds, st);
    const int cx0 = cell_pack_cx_cols(a.Dout, 64) / 16;
    if (cx0 == 16) return launch_cx<M, 16>(dt, a, lds, st);
    if (cx0 == 20) return launch_cx<M, 20>(dt, a, lds, st);
    return 1;
}
}  // namespace

// 0 ok, 1 unsupported M or width, 2 launch error.  dt = k-steps per weight group of the projection transpose (5 or 4;
// (Dout/4) % dt == 0).  Wide outputs (Dout > 128) exist for M <= 5: the LDS tiles of M = 7 do not fit at any such width.
int launch_dec_bwd_persist(int M, int dt, const DecBwdArgs& a, size_t lds, hipStream_t st) {
    switch (M) {
        case 1: return launch_w<1>(dt, a, lds, st);
        case 2: return launch_w<2>(dt, a, lds, st);
        case 3: return launch_w<3>(dt, a, lds, st);
        case 4: return launch_w<4>(dt, a, lds, st);
        case 5: return launch_w<5>(dt, a, lds, st);
        case 7: return a.Dout <= 128 ? launch_m<7>(dt, a, lds, st) : 1;
        default: return 1;
    }
}
}  // namespace eeg
