// Small channel counts on the register-resident kernel set (round 6): (H, HH) = (32, 32) with C = NCDE_FAST_C in
// {4, 8, 12}.  A model with few channels -- CharacterTrajectories has 4, and the reference's DEFAULT widths are hidden_hidden_dim = 15,
// num_layers = 3 (src/ncde/ncde.py:47-48) -- used to be zero-padded to the C = 20 instantiations and paid for 10 output tiles per wave
// where 2 carry data: (4, 32, 15, 3) cost what (20, 32, 32, 3) costs, a tenth of the flops (profiles/r05_shape_sweep_perf.txt).
// The kernel templates are those of ncde_fast_kernels.h; this file is compiled once per channel count (Makefile).
#ifndef NCDE_FAST_C
#error "compile with -DNCDE_FAST_C=4 | 8 | 12"
#endif
#include "ncde_fast_c.h"
#include "ncde_fast_kernels.h"
#include "ncde_host.h"

namespace {
constexpr int FC = NCDE_FAST_C;
template <int HP>
NcdeKernel c_fwd_pick(int interp, int method) {
    return pick_pair(interp, method, [](auto I, auto M) -> NcdeKernel { return ncde_fwd_fast_bf3<32, 32, FC, 4, I, M, 0, 0, HP>; });
}
template <int NL, int DISC>
NcdeKernel c_adj_pick(int interp, int method, int hp) {
    return pick_pair(interp, method, [hp](auto I, auto M) -> NcdeKernel {
        return hp == 2 ? ncde_adj_fast3<NL, FC, I, M, 0, DISC, 2> : ncde_adj_fast3<NL, FC, I, M, 0, DISC, 0>;
    });
}
// f(Int<n_layers>) for the layer counts of this unit
template <class R, class F>
R for_layers(int n_layers, R none, F f) {
    switch (n_layers) {
        case 1: return f(Int<1>{});
        case 2: return f(Int<2>{});
        case 3: return f(Int<3>{});
        case 4: return f(Int<4>{});
        default: return none;
    }
}
}  // namespace

#define NCDE_CAT_(a, b, c) a##b##c
#define NCDE_CAT(a, b, c) NCDE_CAT_(a, b, c)
#define NCDE_CFN(name) NCDE_CAT(ncde_fast_c, NCDE_FAST_C, name)

NcdeKernel NCDE_CFN(_fwd)(int interp, int method, int hp) { return hp ? c_fwd_pick<1>(interp, method) : c_fwd_pick<0>(interp, method); }
size_t NCDE_CFN(_adj_lds)(int n_layers, int interp, int hp) {
    return for_layers(n_layers, (size_t)-1, [&](auto NL) { return adj3_lds_bytes<NL, FC>(interp, hp); });
}
NcdeKernel NCDE_CFN(_adj)(int n_layers, int interp, int method, int hp, bool discrete) {
    if (hp != 0 && hp != 2) return nullptr;
    if (NCDE_CFN(_adj_lds)(n_layers, interp, hp) > (size_t)kLdsLimit) return nullptr;
    return for_layers(n_layers, NcdeKernel(nullptr), [&](auto NL) { return discrete ? c_adj_pick<NL, 1>(interp, method, hp) : c_adj_pick<NL, 0>(interp, method, hp); });
}
