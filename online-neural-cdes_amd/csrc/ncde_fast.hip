// Host side of the register-resident family (kernel templates: ncde_fast_kernels.h): the instantiations of this unit's own set --
// (32, 32, 20) at three layers, the fp32-input forward, the V1 / V2 adjoints, the instrumented variants -- and, for the whole family,
// the table of shapes, the reported names, the plan of a pass (ncde_fast_plan) and THE launch routine (ncde_fast_launch).
// The -D knobs of tools/build_variants.sh reach the kernels through this unit.
#include "ncde_fast.h"
#include "ncde_fast4.h"
#include "ncde_fast64.h"
#include "ncde_fast_nl.h"
#include "ncde_fast_c.h"
#include "ncde_fast_fwd3.h"
#include "ncde_fast_plan.h"
#include "ncde_fast_kernels.h"
#include "ncde_host.h"

namespace {

// ------------------------------------------------------------------------------------------------
// dispatch tables
// ------------------------------------------------------------------------------------------------
template <int H, int HH, int C, int NW>
NcdeKernel pick_fwd(int interp, int method) {
    return pick_pair(interp, method, [](auto I, auto M) -> NcdeKernel { return ncde_fwd_fast<H, HH, C, NW, I, M>; });
}

template <int H, int HH, int C, int NW, int HP>
NcdeKernel pick_fwd_split(int interp, int method, int n_layers) {
    // (the unrolled three-layer instantiations live in ncde_fast_fwd3.hip: the one unit built with MFMA results in VGPRs)
    if (n_layers == 3 && NW == 4 && ((H == 32 && HH == 32 && C == 20) || (H == 64 && HH == 64 && C == 4))) return ncde_fast_fwd3(H, interp, method, HP);
    return pick_pair(interp, method, [](auto I, auto M) -> NcdeKernel { return ncde_fwd_fast_bf3<H, HH, C, NW, I, M, 0, 0, HP>; });
}
template <int H, int HH, int C, int NW>
NcdeKernel pick_fwd_bf3(int interp, int method, int n_layers, int hp) {
    return hp ? pick_fwd_split<H, HH, C, NW, 1>(interp, method, n_layers) : pick_fwd_split<H, HH, C, NW, 0>(interp, method, n_layers);
}

template <int H, int HH, int C, int NL, int NW>
NcdeKernel pick_adj(int interp, int method) {
    return pick_pair(interp, method, [](auto I, auto M) -> NcdeKernel { return ncde_adj_fast<H, HH, C, NL, NW, I, M>; });
}

template <int H, int HH, int C, int NL>
NcdeKernel pick_adj2(int interp, int method) {
    return pick_pair(interp, method, [](auto I, auto M) -> NcdeKernel { return ncde_adj_fast2<H, HH, C, NL, I, M>; });
}

// The all-split-fp16 instantiations (HP = 1) exist in development builds only (-DNCDE_DEV_KNOBS): the shipped
// library neither contains them nor honours NCDE_FLAG_ADJOINT_SPLIT_FP16.
#ifdef NCDE_DEV_KNOBS
#define NCDE_ADJ3_HP1(NL_, C_, I_, M_, P_, D_) ncde_adj_fast3<NL_, C_, I_, M_, P_, D_, 1>
#define NCDE_ADJ3_HP1_AVAILABLE 1
#else
#define NCDE_ADJ3_HP1(NL_, C_, I_, M_, P_, D_) static_cast<NcdeKernel>(nullptr)
#define NCDE_ADJ3_HP1_AVAILABLE 0
#endif

template <int NL, int C, int DISC>
NcdeKernel pick_adj3(int interp, int method, int hp) {
    return pick_pair(interp, method, [hp](auto I, auto M) -> NcdeKernel {
        return hp == 2 ? ncde_adj_fast3<NL, C, I, M, 0, DISC, 2> : (hp == 1 ? NCDE_ADJ3_HP1(NL, C, I, M, 0, DISC) : ncde_adj_fast3<NL, C, I, M, 0, DISC>);
    });
}

// One row per kernel set that has a forward of its own.  Only (32, 32, 20) also has adjoints: ncde_adj_fast / fast2 / fast3 / fast4 for
// kAdjLayers layers here, ncde_adj_fast3 for the other layer counts in ncde_fast_nl.hip, the PLAN = 1 instances in ncde_fast_plan.hip.
struct FastEntry {
    int H, HH, C;
    NcdeKernel (*fwd)(int interp, int method);                            // fp32-input MFMA (NCDE_FLAG_FP32_MFMA)
    NcdeKernel (*fwd_split)(int interp, int method, int n_layers, int hp);   // split GEMMs: hp 1 = split-fp16 (default), 0 = split-bf16
    bool adjoint;
};
const FastEntry kFast[] = {
    {32, 32, 20, pick_fwd<32, 32, 20, 4>, pick_fwd_bf3<32, 32, 20, 4>, true},       // BASELINE cfg2 / cfg3
    // BASELINE cfg4 (adjoint: ncde_fast64.hip -- the per-wave LDS images of ncde_adj_fast3 do not fit at HH = 64)
    {64, 64, 4, pick_fwd<64, 64, 4, 4>, pick_fwd_bf3<64, 64, 4, 4>, false},
    // round 5: the forward alone for up to 40 channels at H, HH <= 32 (its 160 + 80 registers of output-layer operands fit the one
    // wave per SIMD the forward runs at; the adjoint's chain / gradient waves, two per SIMD, have no room for them): inference and the
    // forward half of a training step of such shapes leave the batch-tiled family.  Default time axis only.
    {32, 32, 40, pick_fwd<32, 32, 40, 4>, pick_fwd_bf3<32, 32, 40, 4>, false},
};
constexpr int kAdjLayers = 3;

const FastEntry* find_entry(const NcdeProblem* p) {
    // structure the fast family understands: layer 0 is H->HH, every further layer is ONE shared HH->HH
    if (p->n_layers < 1 || !ncde_one_shared_inner_layer(p)) return nullptr;
    const int HH = p->layer_out[0];
    for (int l = 1; l < p->n_layers; ++l)
        if (p->layer_out[l] != HH || p->layer_in[l] != HH) return nullptr;
    for (const FastEntry& e : kFast)
        if (e.H == p->hidden && e.HH == HH && e.C == p->channels) return &e;
    return nullptr;
}

// (H, HH) = (32, 32) with C = 4 / 8 / 12 (round 6, ncde_fast_c.hip): the same kernel templates instantiated for few channels, every
// layer count 1 .. 4, forward + continuous adjoint + exact discrete backward; default time axis, default / split-bf16 arithmetic
int c_set(const NcdeProblem* p) {
    if (p->hidden != 32 || p->n_layers < 1 || p->n_layers > 4 || p->layer_out[0] != 32 || p->layer_in[0] != 32) return 0;
    if (p->channels != 4 && p->channels != 8 && p->channels != 12) return 0;
    if (p->field_kind != NCDE_FIELD_ORIGINAL || p->field_input != NCDE_INPUT_MATMUL || p->output == NCDE_OUT_TIMES) return 0;
    for (int l = 1; l < p->n_layers; ++l)
        if (p->layer_out[l] != 32 || p->layer_in[l] != 32) return 0;
    if (!ncde_one_shared_inner_layer(p)) return 0;
    if (ncde_dev_flags(p->flags) & (NCDE_FLAG_FP32_MFMA | NCDE_FLAG_ADJOINT_V1 | NCDE_FLAG_ADJOINT_V2 | NCDE_FLAG_ADJOINT_V4 | NCDE_FLAG_ADJOINT_SPLIT_FP16 |
                    NCDE_FLAG_DEBUG_PROFILE | kFlagChainDump)) return 0;
    return p->channels;
}
NcdeKernel c_fwd(int C, int interp, int method, int hp) {
    return C == 4 ? ncde_fast_c4_fwd(interp, method, hp) : (C == 8 ? ncde_fast_c8_fwd(interp, method, hp) : ncde_fast_c12_fwd(interp, method, hp));
}
NcdeKernel c_adj(int C, int nl, int interp, int method, int hp, bool disc) {
    return C == 4 ? ncde_fast_c4_adj(nl, interp, method, hp, disc) : (C == 8 ? ncde_fast_c8_adj(nl, interp, method, hp, disc) : ncde_fast_c12_adj(nl, interp, method, hp, disc));
}
size_t c_adj_lds(int C, int nl, int interp, int hp) {
    return C == 4 ? ncde_fast_c4_adj_lds(nl, interp, hp) : (C == 8 ? ncde_fast_c8_adj_lds(nl, interp, hp) : ncde_fast_c12_adj_lds(nl, interp, hp));
}

// ---- reported names: the one place ---------------------------------------------------------------------------------------------
// shape index: the rows of kFast, then the few-channel sets
int shape_index(int H, int C) { return H == 64 ? 1 : (C == 20 ? 0 : (C == 40 ? 2 : 2 + C / 4)); }
#define NCDE_FWD_NAME(H, C, ARITH, SUFFIX) "ncde_fwd_fast_bf3<H" #H ",HH" #H ",C" #C ",NW4," ARITH SUFFIX ">"
#define NCDE_FWD_NAMES(H, C)                                                                                            \
    {{"ncde_fwd_fast<H" #H ",HH" #H ",C" #C ",NW4>", nullptr}, {NCDE_FWD_NAME(H, C, "bf16x3", ""), NCDE_FWD_NAME(H, C, "bf16x3", ",time plan")}, \
     {NCDE_FWD_NAME(H, C, "fp16x2", ""), NCDE_FWD_NAME(H, C, "fp16x2", ",time plan")}}
// [shape][0 fp32-input MFMA, 1 split-bf16, 2 split-fp16][time plan]
const char* const kFwdNames[6][3][2] = {NCDE_FWD_NAMES(32, 20), NCDE_FWD_NAMES(64, 4), NCDE_FWD_NAMES(32, 40),
                                        NCDE_FWD_NAMES(32, 4), NCDE_FWD_NAMES(32, 8), NCDE_FWD_NAMES(32, 12)};
#define NCDE_ADJ3_NAME(C, NL, ARITH, SUFFIX) "ncde_adj_fast3<H32,HH32,C" #C ",NL" #NL ",chain+grad," ARITH SUFFIX ">"
#define NCDE_ADJ3_ARITH(C, NL, ARITH) {NCDE_ADJ3_NAME(C, NL, ARITH, ""), NCDE_ADJ3_NAME(C, NL, ARITH, ",discrete"), NCDE_ADJ3_NAME(C, NL, ARITH, ",time plan")}
#define NCDE_ADJ3_LAYERS(C, NL) {NCDE_ADJ3_ARITH(C, NL, "bf16x3"), NCDE_ADJ3_ARITH(C, NL, "fp16x2"), NCDE_ADJ3_ARITH(C, NL, "fwd-side fp16x2 + bf16x3")}
#define NCDE_ADJ3_NAMES(C) {NCDE_ADJ3_LAYERS(C, 1), NCDE_ADJ3_LAYERS(C, 2), NCDE_ADJ3_LAYERS(C, 3), NCDE_ADJ3_LAYERS(C, 4)}
// [shape (2: none)][n_layers - 1][hp][0 continuous, 1 discrete, 2 time plan]
const char* const kAdj3Names[6][4][3][3] = {NCDE_ADJ3_NAMES(20), {}, {}, NCDE_ADJ3_NAMES(4), NCDE_ADJ3_NAMES(8), NCDE_ADJ3_NAMES(12)};

// The HP template argument of the split-GEMM kernels -- the one place that reads it off the flags.  Forward: 1 = split-fp16 (default),
// 0 = split-bf16 (NCDE_FLAG_SPLIT_BF16; NCDE_FLAG_FP32_MFMA runs the fp32-input kernel, which has no HP).  ncde_adj_fast3: 2 = the
// forward-side GEMMs of the chain waves split-fp16 (default), 0 = all split-bf16, 1 = everything split-fp16 (NCDE_FLAG_ADJOINT_SPLIT_FP16,
// experimental: DESIGN.md section 5.4c; development builds, and the entry's own layer count, only).  A kernel with hp != 0 reports
// range faults and is followed by the hp = 0 instance on the faulted workgroups.
int fast_hp(uint32_t flags, int pass, bool own_layers) {
    if (flags & NCDE_FLAG_SPLIT_BF16) return 0;
    if (pass == 0) return (flags & NCDE_FLAG_FP32_MFMA) ? 0 : 1;
    if (!own_layers) return (flags & NCDE_FLAG_FP32_MFMA) ? 0 : 2;
    if (flags & kFlagChainDump) return 0;
    return (NCDE_ADJ3_HP1_AVAILABLE != 0 && (flags & NCDE_FLAG_ADJOINT_SPLIT_FP16)) ? 1 : 2;
}

constexpr uint32_t kDevVariantFlags = NCDE_FLAG_ADJOINT_V1 | NCDE_FLAG_ADJOINT_V2 | NCDE_FLAG_ADJOINT_V4 | NCDE_FLAG_DEBUG_PROFILE | kFlagChainDump;

// forward: the few-channel sets, the PLAN = 1 instances (general time axis), else the entry's own
void plan_forward(const NcdeProblem* p, const Layout& y, int cset, const FastEntry* e, FastPlan* P) {
    const uint32_t f = ncde_dev_flags(p->flags);      // (NCDE_FLAG_DENSE_CHANNELS reaches the kernels through KArgs, not through the plan)
    const bool planned = p->output == NCDE_OUT_TIMES, fp32 = (f & NCDE_FLAG_FP32_MFMA) != 0, prof = (f & NCDE_FLAG_DEBUG_PROFILE) != 0;
    const int hp = fast_hp(f, 0, true), shape = cset ? shape_index(32, cset) : (e ? shape_index(e->H, e->C) : 0);
    auto pick = [&](int h) -> NcdeKernel {
        if (cset) return c_fwd(cset, p->interp, p->method, h);
        if (planned) return ncde_fast_plan_fwd(e->H == 32 ? 0 : 1, p->interp, p->method, h);
        return e->fwd_split(p->interp, p->method, p->n_layers, h);
    };
    if (!cset) {
        if (!e) return;
        // (the plan-walking instances: split GEMMs of the two BASELINE shapes; the forward-only C = 40 set has none)
        if (planned && ((f & (kDevVariantFlags | NCDE_FLAG_FP32_MFMA)) || e->C == 40)) return;
    }
    P->main = {fp32 ? e->fwd(p->interp, p->method) : pick(hp), 256, 0};
    if ((cset || planned) && !P->main.fn) return;
    P->ok = true;
    P->name = kFwdNames[shape][fp32 ? 0 : 1 + hp][planned];
    if (hp) P->redo = {pick(0), 256, 0};
    if (prof) {      // phase-cycle counters -> head of the workspace [n_wg][NW][4] u64; instrumented: (32, 32, 20), linear, rk4 only
        P->main.fn = nullptr;
        P->redo.fn = nullptr;
        P->tail_off = 0;
        if (e->H == 32 && e->C == 20 && p->interp == NCDE_INTERP_LINEAR && p->method == NCDE_RK4_38)
            P->main.fn = fp32 ? ncde_fwd_fast<32, 32, 20, 4, NCDE_INTERP_LINEAR, NCDE_RK4_38, 1>
                              : (p->n_layers != 3 ? ncde_fwd_fast_bf3<32, 32, 20, 4, NCDE_INTERP_LINEAR, NCDE_RK4_38, 1>
                                                  : (hp ? ncde_fwd_fast_bf3<32, 32, 20, 4, NCDE_INTERP_LINEAR, NCDE_RK4_38, 1, 3, 1>
                                                        : ncde_fwd_fast_bf3<32, 32, 20, 4, NCDE_INTERP_LINEAR, NCDE_RK4_38, 1, 3>));
    }
    ncde_fast_plan_workspace(P, 256 + (prof ? (int64_t)y.n_wg * 8 * 4 * 8 : 0), hp != 0);
}

// adjoint / exact discrete backward of the (32, 32, C) sets (H = 64: ncde_fast64_plan)
void plan_adjoint(const NcdeProblem* p, const Layout& y, int pass, int cset, const FastEntry* e, FastPlan* P) {
    const uint32_t f = ncde_dev_flags(p->flags);      // (NCDE_FLAG_DENSE_CHANNELS reaches the kernels through KArgs, not through the plan)
    const bool disc = pass == 2, planned = p->output == NCDE_OUT_TIMES;
    const bool prof = (f & NCDE_FLAG_DEBUG_PROFILE) != 0, dump = (f & kFlagChainDump) != 0;
    const int interp = p->interp, method = p->method, nl = p->n_layers;
    if (!cset && (!e || !e->adjoint)) return;
    const bool own_layers = !cset && !planned && nl == kAdjLayers;
    int hp = fast_hp(f, pass, own_layers);
    if (!own_layers) {
        // ncde_adj_fast3 alone, hp 2 / 0: few channels (ncde_fast_c.hip), the general time axis (ncde_fast_plan.hip: continuous adjoint,
        // kAdjLayers layers), another layer count (ncde_fast_nl.hip).  No development variants.
        if (!cset && ((f & kDevVariantFlags) || (planned && (disc || (f & NCDE_FLAG_FP32_MFMA))))) return;
        auto inst = [&](int h) -> FastLaunch {
            if (cset) return {c_adj(cset, nl, interp, method, h, disc), 512, c_adj_lds(cset, nl, interp, h)};
            if (planned) return {ncde_fast_plan_adj3(nl, interp, method, h), 512, ncde_fast_plan_adj3_lds(nl, interp, method, h)};
            return {ncde_fast_adj3_nl(nl, interp, method, h, disc), 512, ncde_fast_adj3_nl_lds(nl, interp, h)};
        };
        P->main = inst(hp);
        if (hp) P->redo = inst(0);
        if (!P->main.fn || (hp && !P->redo.fn)) return;
        P->name = kAdj3Names[shape_index(32, p->channels)][nl - 1][hp][planned ? 2 : disc];
    } else {
        // the entry's own layer count: ncde_adj_fast3 (default; always for the discrete backward), the single-role ncde_adj_fast
        // (NCDE_FLAG_ADJOINT_V1), ncde_adj_fast2 with an fp32 chain (NCDE_FLAG_ADJOINT_V2), the decoupled-chain ncde_adj_fast4
        // (NCDE_FLAG_ADJOINT_V4: selectable, measured slower -- DESIGN.md section 5.4b), and their instrumented variants
        const bool v1 = !disc && (f & NCDE_FLAG_ADJOINT_V1), v3 = disc || (!v1 && !(f & NCDE_FLAG_ADJOINT_V2));
        const bool lin_rk4 = interp == NCDE_INTERP_LINEAR && method == NCDE_RK4_38, cub_mid = interp == NCDE_INTERP_CUBIC && method == NCDE_MIDPOINT;
        NcdeKernel k4 = nullptr;
        if ((f & NCDE_FLAG_ADJOINT_V4) && !(f & (NCDE_FLAG_ADJOINT_V1 | NCDE_FLAG_ADJOINT_V2 | kFlagChainDump)) && !(disc && prof))
            k4 = ncde_fast4_pick(nl, p->channels, interp, method, disc, prof);
        if (k4) {
            hp = 0;
            P->main = {k4, 512, ncde_fast4_lds_bytes(nl, p->channels, interp)};
            P->name = disc ? "ncde_adj_fast4<H32,HH32,C20,NL3,y-waves+cotangent-waves(bf16x3),discrete>" : "ncde_adj_fast4<H32,HH32,C20,NL3,y-waves+cotangent-waves(bf16x3)>";
        } else {
            if (!v3) hp = 0;
            P->main.fn = disc ? pick_adj3<3, 20, 1>(interp, method, hp)
                              : (v1 ? pick_adj<32, 32, 20, 3, 4>(interp, method) : (v3 ? pick_adj3<3, 20, 0>(interp, method, hp) : pick_adj2<32, 32, 20, 3>(interp, method)));
            P->main.block = v1 ? 256 : 512;
            // (with the chain dump the LDS size is still the one of the kernel the other flags select)
            P->main.lds = v1 ? adj_lds_bytes<32, 32, 20, 3, 4>(interp) : (v3 ? adj3_lds_bytes<3, 20>(interp, hp) : adj2_lds_bytes<32, 32, 20, 3>(interp));
            P->name = v3 ? kAdj3Names[0][nl - 1][hp][disc] : (v1 ? "ncde_adj_fast<H32,HH32,C20,NL3,NW4>" : "ncde_adj_fast2<H32,HH32,C20,NL3,chain+grad>");
            if (hp && !prof) P->redo = {disc ? pick_adj3<3, 20, 1>(interp, method, 0) : pick_adj3<3, 20, 0>(interp, method, 0), 512, adj3_lds_bytes<3, 20>(interp, 0)};
            if (dump)      // per-stage chain values of workgroup 0 -> development tail: cubic + midpoint, continuous adjoint only
                P->main.fn = (disc || !cub_mid) ? nullptr
                             : (v1 ? ncde_adj_fast<32, 32, 20, 3, 4, NCDE_INTERP_CUBIC, NCDE_MIDPOINT, 2> : ncde_adj_fast2<32, 32, 20, 3, NCDE_INTERP_CUBIC, NCDE_MIDPOINT, 2>);
            if (prof)      // phase-cycle counters -> development tail [n_wg][NW][6] u64: linear + rk4, continuous adjoint only
                P->main.fn = (disc || dump || !lin_rk4) ? nullptr
                             : (v3 ? (hp == 2 ? ncde_adj_fast3<3, 20, NCDE_INTERP_LINEAR, NCDE_RK4_38, 1, 0, 2>
                                              : (hp == 1 ? NCDE_ADJ3_HP1(3, 20, NCDE_INTERP_LINEAR, NCDE_RK4_38, 1, 0) : ncde_adj_fast3<3, 20, NCDE_INTERP_LINEAR, NCDE_RK4_38, 1>))
                                   : (v1 ? ncde_adj_fast<32, 32, 20, 3, 4, NCDE_INTERP_LINEAR, NCDE_RK4_38, 1> : ncde_adj_fast2<32, 32, 20, 3, NCDE_INTERP_LINEAR, NCDE_RK4_38, 1>));
        }
    }
    P->ok = true;
    P->reduce = true;
    const int64_t partials = (int64_t)sizeof(float) * (int64_t)y.n_wg * (int64_t)y.theta_size + 256;
    if (prof || dump) P->tail_off = partials;
    ncde_fast_plan_workspace(P, partials + (prof ? (int64_t)y.n_wg * 8 * 6 * 8 + 256 : 0) + (dump ? (int64_t)p->n_knots * 4 * 5 * 64 * 4 + 256 : 0), hp != 0);
}

}  // namespace

FastPlan ncde_fast_plan(const NcdeProblem* p, int pass) {
    FastPlan P{};
    P.fault_off = P.tail_off = -1;
    // (a piecewise-quintic control never runs here: the dX/dt staging of these kernels knows the linear and cubic rows only)
    if (pass < 0 || pass > 2 || p->interp == NCDE_INTERP_QUINTIC) return P;
    const Layout y = make_layout(p);
    P.grid = y.n_wg;
    if (pass >= 1 && ncde_fast64_plan(p, pass, y, &P)) return P;      // H = HH = 64, C <= 4: the in-sweep adjoint of ncde_fast64.hip
    const int cset = c_set(p);
    const FastEntry* e = cset ? nullptr : find_entry(p);
    if (pass == 0) plan_forward(p, y, cset, e, &P);
    else plan_adjoint(p, y, pass, cset, e, &P);
    if (!P.ok) P.name = nullptr;
    return P;
}

// THE launch of a register-resident kernel: main kernel (LDS opt-in), the re-execution of range-faulted workgroups where the plan has
// one (normally no workgroup: each exits at once), then the reduce of the per-workgroup gradient partials.
int ncde_fast_launch(const NcdeProblem* p, int pass, float* out, float* stages, const float* src, const float* grad_out,
                     const NcdeGrads* g, void* ws, size_t ws_bytes, hipStream_t st, bool main_kernel_only) {
    const FastPlan P = ncde_fast_plan(p, pass);
    if (!P.ok || !P.main.fn) return NCDE_ERR_UNSUPPORTED;
    if ((int64_t)ws_bytes < P.ws_bytes) return NCDE_ERR_WORKSPACE;
    const Layout y = make_layout(p);
    KArgs a;
    fill_kargs(p, y, &a);
    if (pass == 0) {
        a.out = out;
        a.stages = stages;
    } else {
        a.grad_out = grad_out; a.grad_z0 = g->grad_z0;
        if (pass == 2) { a.stages = const_cast<float*>(src); a.discrete = 1; }
        else a.z_out = src;
        a.gpart = (float*)ws;
    }
    if (P.fault_off >= 0) a.fault = reinterpret_cast<int*>(static_cast<char*>(ws) + P.fault_off);
    if (P.tail_off >= 0) (pass == 0 ? a.gpart : a.out) = reinterpret_cast<float*>(static_cast<char*>(ws) + P.tail_off);
    for (const FastLaunch* l : {&P.main, &P.redo}) {
        if (!l->fn) break;
        if (l->lds && ncde_lds_optin((const void*)l->fn, l->lds) != hipSuccess) return NCDE_ERR_HIP;
        hipLaunchKernelGGL(l->fn, dim3(P.grid), dim3(l->block), l->lds, st, a);
        if (hipGetLastError() != hipSuccess) return NCDE_ERR_HIP;
        a.only_faulted = 1;
    }
    if (!P.reduce || main_kernel_only) return NCDE_OK;
    return launch_reduce_partials(p, y, g, (const float*)ws, P.grid, st);
}
