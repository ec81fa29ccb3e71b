// Instantiations of the persistent decoder forward kernel (kernels_decoder.h), in their own translation unit: the launcher
// executes a plan of dec_launch.h (which instance, grid, block, LDS: decided there, not here).
#include "kernels_decoder.h"
#include "prof.h"

namespace eeg {
namespace {
template <int M>
int launch_m(const DecPlan& p, const DecFwdArgs& a, hipStream_t st) {
    EEG_SET_MAX_LDS((dec_fwd_persist_kernel<64, M>), p.lds_fwd);
    EEG_LAUNCH_P("fwd_persist", (dec_fwd_persist_kernel<64, M>), dim3(p.grid), dim3(p.block), p.lds_fwd, st, a);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
}  // namespace

int launch_dec_fwd_persist(const DecPlan& p, const DecFwdArgs& a, hipStream_t st) {
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
