// Instantiations of the streamed-weight BPTT kernel (kernels_seq_stream.h), in their own translation unit.
#include "kernels_seq_stream.h"
#include "prof.h"
#include "seq_launch.h"

namespace eeg {
namespace {
template <int M>
int bwd_one(const SeqPlan& p, const SeqBwdArgs& a, hipStream_t st) {
    EEG_SET_MAX_LDS((seq_bwd_stream_kernel<64, M>), p.lds);
    EEG_LAUNCH_P("seq_bwd", (seq_bwd_stream_kernel<64, M>), dim3(p.grid), dim3(p.block), p.lds, st, a.Hseq, a.h0, a.Rs, a.Us, a.Cs, a.dHseq,
                 a.d_at_end, a.d_at_len, a.lengths, a.P, a.p_batched, a.b1, a.b2, a.dXW, a.dh0, a.dbias_part, a.T, a.B, a.N, a.act);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
}  // namespace

// executes a SeqKind::Stream plan (seq_has_stream: 64 units, M <= 5).  0 ok, 1 launch error
int launch_seq_bwd_stream(int M, const SeqPlan& p, const SeqBwdArgs& a, hipStream_t st) {
    switch (M) {
        case 1: return bwd_one<1>(p, a, st);
        case 2: return bwd_one<2>(p, a, st);
        case 3: return bwd_one<3>(p, a, st);
        case 4: return bwd_one<4>(p, a, st);
        case 5: return bwd_one<5>(p, a, st);
        default: return 1;
    }
}
}  // namespace eeg
