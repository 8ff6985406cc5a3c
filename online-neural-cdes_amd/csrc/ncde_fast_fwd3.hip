// ncde_fwd_fast_bf3<.., NLT = 3, ..> of both register-resident shape sets: see ncde_fast_fwd3.h.
#include "ncde_fast_fwd3.h"
#include "ncde_fast_kernels.h"

namespace {
template <int H, int HH, int C, int HP>
NcdeKernel fwd3_pick(int interp, int method) {
    return pick_pair(interp, method, [](auto I, auto M) -> NcdeKernel { return ncde_fwd_fast_bf3<H, HH, C, 4, I, M, 0, 3, HP>; });
}
}  // namespace

NcdeKernel ncde_fast_fwd3(int hidden, int interp, int method, int hp) {
    if (hidden == 32) return hp ? fwd3_pick<32, 32, 20, 1>(interp, method) : fwd3_pick<32, 32, 20, 0>(interp, method);
    if (hidden == 64) return hp ? fwd3_pick<64, 64, 4, 1>(interp, method) : fwd3_pick<64, 64, 4, 0>(interp, method);
    return nullptr;
}
