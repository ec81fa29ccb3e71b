// Instantiations of the persistent decoder backward kernel (kernels_decoder.h), in their own translation unit: the launcher
// executes a plan of dec_launch.h (which instance, grid, block, LDS: decided there, not here).
#include "kernels_decoder.h"
#include "prof.h"

namespace eeg {
namespace {
template <int M, int DT, int CX0>
int launch_one(const DecPlan& p, const DecBwdArgs& a, hipStream_t st) {
    EEG_SET_MAX_LDS((dec_bwd_persist_kernel<64, M, DT, CX0>), p.lds_bwd);
    EEG_LAUNCH_P("bwd_persist", (dec_bwd_persist_kernel<64, M, DT, CX0>), dim3(p.grid), dim3(p.block), p.lds_bwd, st, a);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
// one dispatch over (M, dt, cx0); what is compiled is what dec_has_instance says, the predicate the plan covers a decoder by
template <int M, int CX0>
int launch_cx(const DecPlan& p, const DecBwdArgs& a, hipStream_t st) {
    if constexpr (dec_has_instance(M, CX0)) return p.dt == 5 ? launch_one<M, 5, CX0>(p, a, st) : launch_one<M, 4, CX0>(p, a, st);
    return 1;
}
template <int M>
int launch_m(const DecPlan& p, const DecBwdArgs& a, hipStream_t st) {
    return p.cx0 == 12 ? launch_cx<M, 12>(p, a, st) : p.cx0 == 16 ? launch_cx<M, 16>(p, a, st) : launch_cx<M, 20>(p, a, st);
}
}  // namespace

int launch_dec_bwd_persist(const DecPlan& p, const DecBwdArgs& a, hipStream_t st) {
    switch (p.M) {
        case 1: return launch_m<1>(p, a, st);
        case 2: return launch_m<2>(p, a, st);
        case 3: return launch_m<3>(p, a, st);
        case 4: return launch_m<4>(p, a, st);
        case 5: return launch_m<5>(p, a, st);
        case 7: return launch_m<7>(p, a, st);
        default: return 1;
    }
}
}  // namespace eeg
