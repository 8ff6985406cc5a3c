// ncde_adj_fast3 (ncde_fast_kernels.h: the specialised chain + gradient-wave adjoint of H = HH = 32, C = 20) for the layer counts besides
// BASELINE's nl = 3: the reference's hyper-parameter range is num_layers in [1, 4] (experiments/configurations/configurations.json5:36)
// and a model one layer away used to fall to the batch-tiled family (2.3 - 3 x the time: profiles/r04_shape_sweep_perf.txt).
#include "ncde_fast_nl.h"
#include "ncde_fast_kernels.h"
#include "ncde_host.h"

namespace {
// (no cubic instantiations at four layers)
template <int NL, int DISC>
NcdeKernel nl_pick(int interp, int method, int hp) {
    return pick_pair<(NL < 4)>(interp, method, [hp](auto I, auto M) -> NcdeKernel {
        return hp == 2 ? ncde_adj_fast3<NL, 20, I, M, 0, DISC, 2> : ncde_adj_fast3<NL, 20, I, M, 0, DISC, 0>;
    });
}
// f(Int<n_layers>) for the layer counts of this unit
template <class R, class F>
R for_layers(int n_layers, R none, F f) {
    switch (n_layers) {
        case 1: return f(Int<1>{});
        case 2: return f(Int<2>{});
        case 4: return f(Int<4>{});
        default: return none;
    }
}
}  // namespace

NcdeKernel ncde_fast_adj3_nl(int n_layers, int interp, int method, int hp, bool discrete) {
    if (hp != 0 && hp != 2) return nullptr;
    if (ncde_fast_adj3_nl_lds(n_layers, interp, hp) > (size_t)kLdsLimit) return nullptr;
    return for_layers(n_layers, NcdeKernel(nullptr), [&](auto NL) { return discrete ? nl_pick<NL, 1>(interp, method, hp) : nl_pick<NL, 0>(interp, method, hp); });
}
size_t ncde_fast_adj3_nl_lds(int n_layers, int interp, int hp) {
    return for_layers(n_layers, (size_t)-1, [&](auto NL) { return adj3_lds_bytes<NL, 20>(interp, hp); });
}
