// Host-side pieces shared by ncde_abi.hip and the kernel families: the internal chain-dump flag, the LDS opt-in, the parameter-gradient
// Layout of a problem, the KArgs fields common to every family (fill_kargs) and the launch of the partials reduce (K4).
#pragma once
#include <mutex>
#include <map>
#include <utility>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "ncde_common.h"

struct ReduceSegs {
    int n;
    int off[2 * NCDE_MAX_LAYERS + 6];
    int len[2 * NCDE_MAX_LAYERS + 6];
    float* dst[2 * NCDE_MAX_LAYERS + 6];
};
extern "C" __global__ void ncde_reduce_partials(const float* gpart, int n_part, int theta_size, ReduceSegs segs);

constexpr int kLdsLimit = 160 * 1024;

// ncde_abi.hip: `text` becomes the calling thread's ncde_last_error_string(); returns `code` (for entry points of other units)
int ncde_fail_text(int code, const char* text);

// Internal flag (not in include/ncde_hip.h): the development adjoint kernels of the (32, 32, 20) set (ncde_adj_fast / ncde_adj_fast2,
// cubic + midpoint only) also write the per-stage chain values of workgroup 0 to the tail of the workspace, and every split-GEMM
// choice of that set falls back to split-bf16.  A problem that carries it is never zero-padded onto a kernel set.
constexpr uint32_t kFlagChainDump = 0x200u;
// NCDE_FLAG_DENSE_CHANNELS is BOTH development bits (0x100 | 0x200: no bit of `flags` was free, and an instrumented chain dump never
// existed).  ncde_dev_flags: the flags with that request taken out -- what every test of a development bit looks at.
inline bool ncde_dense_channels(uint32_t flags) { return (flags & NCDE_FLAG_DENSE_CHANNELS) == NCDE_FLAG_DENSE_CHANNELS; }
inline uint32_t ncde_dev_flags(uint32_t flags) { return ncde_dense_channels(flags) ? flags & ~NCDE_FLAG_DENSE_CHANNELS : flags; }

// Development switches are environment variables ONLY in builds with -DNCDE_DEV_KNOBS; the shipped library is stateless and
// reads nothing but its arguments.
inline const char* ncde_dev_env(const char* name) {
#ifdef NCDE_DEV_KNOBS
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

// Raise a kernel's dynamic-LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize) only when a launch needs more than what was
// already granted for this (device, kernel) -- not a hipFuncSetAttribute call in front of every launch.  (Granting a flat 160 KB
// would fail for kernels that also hold static __shared__ arrays.)
inline hipError_t ncde_lds_optin(const void* fn, size_t bytes) {
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, size_t> granted;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    std::lock_guard<std::mutex> lk(mu);
    size_t& have = granted[{dev, fn}];
    if (bytes <= have) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) have = bytes;
    return e;
}
// The one layer structure the shape-specialised kernel sets (register-resident, H = 64 in-sweep adjoint, fused dopri5, and the
// zero-padding onto them) understand -- the reference's: layer 0, then ONE other layer shared by every further position, and no
// aliasing between the two (neither the matrices nor the biases).  Their adjoints keep one gradient accumulator for layer 0 and
// one for the shared layer and STORE each to its offset of the partial: with layer 1 tied back to layer 0 (make_layout gives the two
// one offset) the second store would overwrite the first.  Widths are each caller's own check.
inline bool ncde_one_shared_inner_layer(const NcdeProblem* p) {
    for (int l = 2; l < p->n_layers; ++l)
        if (p->layer_W[l] != p->layer_W[1] || p->layer_b[l] != p->layer_b[1]) return false;
    return p->n_layers < 2 || (p->layer_W[1] != p->layer_W[0] && p->layer_b[1] != p->layer_b[0]);
}
inline int hru4(int x) { return (x + 3) & ~3; }
inline int hru16(int x) { return (x + 15) & ~15; }

struct Layout {
    int Hp, Cp, Dp, HS, DS, L;
    int theta_size;
    int gW_off[NCDE_MAX_LAYERS], gb_off[NCDE_MAX_LAYERS], gWo_off, gbo_off;
    int gWg_off, gbg_off, gWr_off, gbr_off;
    int d0, rows;          // field input width, head rows (low-rank field: rows of M_h = H * R)
    int rank, rows_g;      // low-rank field: R and the rows of M_o = R * C; every other field: 0 and rows
    bool variant;          // gated field or evaluate / derivative input (generic family only)
    int dlast;
    int n_wg;
    size_t lds_fwd, lds_adj;
    int gacc_in_lds;
};

// rank R of the low-rank field (NCDE_FLAG_FIELD_RANK in the top byte of flags); 0 for every other kind, whatever that byte holds
inline int ncde_field_rank(const NcdeProblem* p) { return p->field_kind == NCDE_FIELD_LOWRANK ? (int)(p->flags >> 24) : 0; }

inline Layout make_layout(const NcdeProblem* p) {
    Layout y{};
    y.L = p->n_layers;
    y.Hp = hru16(p->hidden);
    y.Cp = hru4(p->channels);
    y.variant = p->field_kind != NCDE_FIELD_ORIGINAL || p->field_input != NCDE_INPUT_MATMUL;
    y.d0 = p->field_input == NCDE_INPUT_MATMUL ? p->hidden : p->hidden + p->channels;
    y.rows = p->field_input == NCDE_INPUT_MATMUL ? p->hidden * p->channels : p->hidden;
    y.rank = ncde_field_rank(p);
    y.rows_g = y.rows;
    if (p->field_kind == NCDE_FIELD_LOWRANK) { y.rows = p->hidden * y.rank; y.rows_g = y.rank * p->channels; }
    y.Dp = std::max(y.Hp, hru16(y.d0));
    for (int l = 0; l < y.L; ++l) y.Dp = std::max(y.Dp, hru16(p->layer_out[l]));
    y.HS = y.Hp * 16;
    y.DS = y.Dp * 16;
    y.dlast = y.L ? p->layer_out[y.L - 1] : p->hidden;
    int off = 0;
    for (int l = 0; l < y.L; ++l) {
        int prevW = -1, prevB = -1;
        for (int q = 0; q < l; ++q) {
            if (p->layer_W[q] == p->layer_W[l]) prevW = q;
            if (p->layer_b[q] == p->layer_b[l]) prevB = q;
        }
        if (prevW >= 0) y.gW_off[l] = y.gW_off[prevW];
        else { y.gW_off[l] = off; off += p->layer_out[l] * p->layer_in[l]; }
        if (prevB >= 0) y.gb_off[l] = y.gb_off[prevB];
        else { y.gb_off[l] = off; off += p->layer_out[l]; }
    }
    y.gWo_off = off; off += y.rows * y.dlast;
    y.gbo_off = off; off += y.rows;
    y.gWg_off = y.gbg_off = y.gWr_off = y.gbr_off = 0;
    if (p->field_kind != NCDE_FIELD_ORIGINAL) {
        y.gWg_off = off; off += y.rows_g * y.dlast;
        y.gbg_off = off; off += y.rows_g;
    }
    if (p->field_kind == NCDE_FIELD_GRU) {
        y.gWr_off = off; off += y.d0 * y.d0;
        y.gbr_off = off; off += y.d0;
    }
    y.theta_size = off;
    y.n_wg = (p->batch + NCDE_TILE - 1) / NCDE_TILE;
    y.lds_fwd = sizeof(float) * (size_t)(5 * y.HS + 2 * y.DS + y.Cp * 16);
    size_t adj = sizeof(float) * (size_t)(10 * y.HS + ((y.L > 0 ? y.L : 1) + 4) * y.DS + y.Cp * 16 + 4 * 16 * 17);
    y.gacc_in_lds = adj + sizeof(float) * (size_t)y.theta_size <= (size_t)kLdsLimit;
    y.lds_adj = adj + (y.gacc_in_lds ? sizeof(float) * (size_t)y.theta_size : 0);
    return y;
}


// fills the dims / pointers / gradient offsets common to every kernel family
inline void fill_kargs(const NcdeProblem* p, const Layout& y, KArgs* a) {
    memset(a, 0, sizeof(*a));
    a->B = p->batch; a->T = p->n_knots; a->C = p->channels; a->H = p->hidden;
    a->interp = p->interp; a->method = p->method; a->output = p->output; a->n_layers = p->n_layers;
    a->n_pieces = p->n_knots - 1;
    a->n_out = p->output == NCDE_OUT_TIMES ? p->n_t_out : (p->output == NCDE_OUT_KNOTS ? p->n_knots : 2);
    if (p->output == NCDE_OUT_TIMES) {
        a->plan = (const int*)p->time_plan;
        a->n_steps_fwd = p->n_steps_fwd;
        a->n_steps_adj = p->n_steps_adj;
    }
    for (int l = 0; l < p->n_layers; ++l) {
        a->din[l] = p->layer_in[l]; a->dout[l] = p->layer_out[l];
        a->W[l] = p->layer_W[l]; a->b[l] = p->layer_b[l];
        a->gW_off[l] = y.gW_off[l]; a->gb_off[l] = y.gb_off[l];
    }
    a->Wo = p->Wo; a->bo = p->bo; a->coeffs = p->coeffs;
    a->cs_b = p->coeffs_stride_b; a->cs_t = p->coeffs_stride_t;
    a->z0 = p->z0;
    a->gWo_off = y.gWo_off; a->gbo_off = y.gbo_off; a->theta_size = y.theta_size;
    a->field_kind = p->field_kind; a->field_input = p->field_input; a->d0 = y.d0; a->rows = y.rows;
    a->Wg = p->Wg; a->bg = p->bg; a->Wr = p->Wr; a->br = p->br;
    a->gWg_off = y.gWg_off; a->gbg_off = y.gbg_off; a->gWr_off = y.gWr_off; a->gbr_off = y.gbr_off;
    a->gacc_in_lds = y.gacc_in_lds;
    a->rank = y.rank; a->rows_g = y.rows_g;
    a->dense_channels = ncde_dense_channels(p->flags);
    // internal (zero-padded problems, see KArgs): reserved_ = (real hidden size << 12) | real channel count, 0 = not padded
    a->Hr = p->reserved_ ? (p->reserved_ >> 12) : p->hidden;
    a->Cc = p->reserved_ ? (p->reserved_ & 0xFFF) : p->channels;
}

// The parameter tensors of a problem as segments of the flat gradient layout, in the layout's order: per layer W then b (a tensor tied
// to an earlier layer only at its first occurrence), Wo, bo, then Wg, bg (every field but the original) and Wr, br (GRU).  The one
// list behind the partials reduce (K4) and the dopri5 adjoint's mixed error norm, which sums its segments in this order.
enum SegPolicy {
    kSegsNoDst,       // every segment, no destinations; `g` may be NULL (dopri5 forward: its norm has no parameter part to scatter)
    kSegsSkipNull,    // a NULL destination = the tensor is not among the adjoint's parameters: it gets no segment
    kSegsRefuseNull,  // a NULL destination is an error: the list is not built
};
inline bool build_segs(const NcdeProblem* p, const Layout& y, const NcdeGrads* g, SegPolicy policy, ReduceSegs* s) {
    const NcdeGrads none{};
    if (policy == kSegsNoDst) g = &none;
    bool ok = true;
    int n = 0;
    auto add = [&](int off, int len, float* dst) {
        if (!dst && policy == kSegsRefuseNull) ok = false;
        if (!dst && policy != kSegsNoDst) return;
        s->off[n] = off; s->len[n] = len; s->dst[n] = dst; ++n;
    };
    for (int l = 0; l < p->n_layers; ++l) {
        bool firstW = true, firstB = true;
        for (int q = 0; q < l; ++q) {
            if (p->layer_W[q] == p->layer_W[l]) firstW = false;
            if (p->layer_b[q] == p->layer_b[l]) firstB = false;
        }
        if (firstW) add(y.gW_off[l], p->layer_out[l] * p->layer_in[l], g->grad_layer_W[l]);
        if (firstB) add(y.gb_off[l], p->layer_out[l], g->grad_layer_b[l]);
    }
    add(y.gWo_off, y.rows * y.dlast, g->grad_Wo);
    add(y.gbo_off, y.rows, g->grad_bo);
    if (p->field_kind != NCDE_FIELD_ORIGINAL) {
        add(y.gWg_off, y.rows_g * y.dlast, g->grad_Wg);
        add(y.gbg_off, y.rows_g, g->grad_bg);
    }
    if (p->field_kind == NCDE_FIELD_GRU) {
        add(y.gWr_off, y.d0 * y.d0, g->grad_Wr);
        add(y.gbr_off, y.d0, g->grad_br);
    }
    s->n = n;
    return ok;
}

// K4: sum the per-workgroup partials and scatter into the caller's buffers (every tensor needs one). 0 = ok, else NcdeStatus.
inline int launch_reduce_partials(const NcdeProblem* p, const Layout& y, const NcdeGrads* g, const float* gpart, int n_part,
                                  hipStream_t st) {
    ReduceSegs segs{};
    if (!build_segs(p, y, g, kSegsRefuseNull, &segs)) return NCDE_ERR_INVALID;
    hipLaunchKernelGGL(ncde_reduce_partials, dim3((y.theta_size + 255) / 256), dim3(256), 0, st, gpart, n_part, y.theta_size, segs);
    return hipGetLastError() == hipSuccess ? NCDE_OK : NCDE_ERR_HIP;
}
