// The time-axis walk and the Butcher bookkeeping of the 16-sample-tile families (ncde_generic.hip, ncde_variant.hip,
// ncde_lowrank.hip), stated ONCE: which step and stage descriptor comes next (default integer grid or a host-built time plan), what one
// LDS element [unit][sample] does after a stage (forward: StageCombine and the output emit; reverse: the continuous adjoint's two
// StageCombine updates and its reset at an output, or the exact discrete backward's StageTranspose, output cotangents and next seed),
// the initial cotangent, and the stage record.  This text is the contract of DESIGN.md section 3: the fp32 operation order of
// torchdiffeq's steps, their exact transpose and the per-interval reverse solves.
//
// Everything here is per thread and per element: NO barrier and NO loop over steps or stages.  The kernels keep their own loops and
// their own __syncthreads() placement, which differs between them; what sits in the middle of a stage (the field and its VJP) is theirs.
#pragma once
#include "ncde_common.h"

// ---- tile dimensions -----------------------------------------------------------------------------------------------------------------
// Hp / Cp: H, C rounded up to the MFMA tile (16 / 4); Dp: the widest activation (H, every layer, and `extra_width`: the variant
// family's field input d0); HS / DS: floats of one [Hp][16] / [Dp][16] array
struct TileDims {
    int Hp, Cp, Dp, HS, DS;
};
__device__ __forceinline__ TileDims tile_dims(const KArgs& a, int extra_width = 0) {
    TileDims t;
    t.Hp = ru16(a.H);
    t.Cp = ru4(a.C);
    t.Dp = max(t.Hp, ru16(extra_width));
    for (int l = 0; l < a.n_layers; ++l) t.Dp = max(t.Dp, ru16(a.dout[l]));
    t.HS = t.Hp * 16;
    t.DS = t.Dp * 16;
    return t;
}

// ---- stage record of the exact discrete backward: a.stages[idx][B][H] <-> U[h][s] for the tile's 16 samples ----------------------------
__device__ __forceinline__ void stage_record_store(const KArgs& a, int idx, int b0, const float* U, int tid, int nthreads) {
    const int H = a.H;
    float* rec = a.stages + ((long long)idx * a.B + b0) * H;
    for (int e = tid; e < 16 * H; e += nthreads) {
        const int s = e / H, h = e - s * H;
        if (b0 + s < a.B) rec[e] = U[h * 16 + s];
    }
}
__device__ __forceinline__ void stage_record_load(const KArgs& a, int idx, int b0, float* U, int tid, int nthreads) {
    const int H = a.H;
    const float* rec = a.stages + ((long long)idx * a.B + b0) * H;
    for (int e = tid; e < 16 * H; e += nthreads) {
        const int s = e / H, h = e - s * H;
        U[h * 16 + s] = b0 + s < a.B ? rec[e] : 0.0f;
    }
}

// ---- forward walk ----------------------------------------------------------------------------------------------------------------------
struct FwdWalk {
    bool planned;       // a time plan instead of the default integer grid
    int S, n_steps;
    const int* pout;    // the plan's output table
};
struct FwdStep {
    const int* pstep;   // the plan's record of this step (NULL on the default grid)
    float dt;
};
// A planned kernel first refuses a stale table, before its first barrier: `if (!plan_ok(a)) return;` (plan_header_ok)
__device__ __forceinline__ bool plan_ok(const KArgs& a) { return a.plan == nullptr || plan_header_ok(a, n_stages(a.method)); }
__device__ __forceinline__ FwdWalk fwd_walk(const KArgs& a) {
    FwdWalk w;
    w.S = n_stages(a.method);
    w.planned = a.plan != nullptr;
    w.n_steps = w.planned ? a.n_steps_fwd : a.T - 1;
    w.pout = w.planned ? a.plan + plan_off_out(w.S, a.n_steps_fwd) : nullptr;
    return w;
}
__device__ __forceinline__ FwdStep fwd_step(const KArgs& a, const FwdWalk& w, int n) {
    FwdStep st;
    st.pstep = w.planned ? a.plan + plan_off_fwd() + n * plan_step_words(w.S) : nullptr;
    st.dt = w.planned ? __int_as_float(st.pstep[0]) : 1.0f;
    return st;
}
__device__ __forceinline__ StageDesc fwd_stage(const KArgs& a, const FwdWalk& w, const int* pstep, int n, int j) {
    return w.planned ? plan_stage(pstep, j) : default_stage(a.method, (float)n + stage_offset(a.method, j), a.n_pieces);
}

// Element e after stage j of step n: k = KO[e] enters the Butcher registers (Y0, K1, K2), YS[e] gets the next stage input.  After
// the last stage the new state goes to the output rows the step owns: on a plan the rows it brackets -- y1 itself at a grid hit, y0,
// or the linear interpolation between them (solvers.py:166-172) -- else the knot's row (NCDE_OUT_KNOTS) or the final row.
__device__ __forceinline__ void fwd_bookkeep(const KArgs& a, const FwdWalk& w, const int* pstep, int n, int j, float dt, int e, int b0,
                                             const float* KO, float* YS, float* Y0, float* K1, float* K2) {
    float y0 = Y0[e], k1 = K1[e], k2 = K2[e];
    const float yprev = y0;
    bool last;
    const float ys = StageCombine::apply(a.method, j, KO[e], dt, y0, k1, k2, last);
    YS[e] = ys;
    K1[e] = k1;
    K2[e] = k2;
    if (last) {
        Y0[e] = y0;
        const int H = a.H, h = e >> 4, s = e & 15, b = b0 + s;
        if (h < H && b < a.B) {
            if (w.planned) {
                const int q0 = pstep[1], q1 = q0 + pstep[2];
                for (int q = q0; q < q1; ++q) {
                    const int kind = w.pout[2 * q];
                    const float slope = __int_as_float(w.pout[2 * q + 1]);
                    a.out[((long long)b * a.n_out + q) * H + h] = kind == 1 ? y0 : (kind == 0 ? yprev : yprev + slope * (y0 - yprev));
                }
            } else if (a.output == NCDE_OUT_KNOTS) a.out[((long long)b * a.n_out + (n + 1)) * H + h] = y0;
            else if (n == a.T - 2) a.out[((long long)b * a.n_out + 1) * H + h] = y0;
        }
    }
}

// ---- reverse walk (continuous adjoint, or the exact discrete backward when a.discrete) ---------------------------------------------------
struct RevWalk {
    int S;
    bool disc, planned;
    int pw_;                            // words of one step record of the plan
    const int *pfwd, *pout, *padj;      // the plan's forward steps, output table, adjoint steps
    int n_rsteps;
};
struct RevStep {
    int n;              // default grid: the reverse step goes from knot n to knot n-1
    int m;              // the forward step being transposed (discrete mode)
    const int* pstep;   // plan: forward step m (discrete) or adjoint step rstep (continuous)
    float dt;           // continuous mode on a plan: in negated time
};
struct RevStage {
    StageDesc sd;
    float w;            // what the stage's parameter gradient is weighted with: the quadrature weight x dt (continuous), 1 (discrete)
};
// the LDS arrays [Hp][16] of the reverse sweep.  Discrete mode uses KA1, KA2, KY1 as the three d slots of StageTranspose and leaves
// Y0, KY2 alone (YS is then filled from the stage record by the caller)
struct AdjLds {
    float *YS, *AS;                     // stage inputs: state, cotangent
    float *Y0, *KY1, *KY2;              // Butcher registers of y
    float *A0, *KA1, *KA2;              // Butcher registers of a
};
__device__ __forceinline__ RevWalk rev_walk(const KArgs& a) {
    RevWalk w;
    w.S = n_stages(a.method);
    w.disc = a.discrete != 0;
    w.planned = a.plan != nullptr;
    w.pw_ = plan_step_words(w.S);
    w.pfwd = w.planned ? a.plan + plan_off_fwd() : nullptr;
    w.pout = w.planned ? a.plan + plan_off_out(w.S, a.n_steps_fwd) : nullptr;
    w.padj = w.planned ? a.plan + plan_off_adj(w.S, a.n_steps_fwd, a.n_out) : nullptr;
    w.n_rsteps = w.planned ? (w.disc ? a.n_steps_fwd : a.n_steps_adj) : a.T - 1;
    return w;
}
__device__ __forceinline__ RevStep rev_step(const KArgs& a, const RevWalk& w, int rstep) {
    RevStep st;
    st.n = a.T - 1 - rstep;
    st.m = w.n_rsteps - 1 - rstep;
    st.pstep = w.planned ? (w.disc ? w.pfwd + st.m * w.pw_ : w.padj + rstep * w.pw_) : nullptr;
    st.dt = w.planned ? __int_as_float(st.pstep[0]) : 1.0f;
    return st;
}
// Reverse stage j.  Discrete mode walks the stages of the forward step backwards (forward stage S-1-j, at its forward time).  Default
// grid: the continuous adjoint integrates in negated time s from -n, so its stage sits at real time -(-n + offset(j)) = n - offset(j)
// (a negation is exact in fp32, so the two forms are the same bits); the transposed forward stage at (n-1) + offset(S-1-j).
__device__ __forceinline__ RevStage rev_stage(const KArgs& a, const RevWalk& w, const RevStep& st, int j) {
    RevStage r;
    if (w.planned) {
        r.sd = plan_stage(st.pstep, w.disc ? w.S - 1 - j : j);
    } else {
        const float t = w.disc ? (float)(st.n - 1) + stage_offset(a.method, w.S - 1 - j) : (float)st.n - stage_offset(a.method, j);
        r.sd = default_stage(a.method, t, a.n_pieces);
    }
    r.w = w.disc ? 1.0f : stage_weight(a.method, j) * st.dt;
    return r;
}
// index into the stage record of the forward stage that reverse stage j of step `st` transposes
__device__ __forceinline__ int rev_record_index(const RevWalk& w, const RevStep& st, int j) { return st.m * w.S + (w.S - 1 - j); }

// Element e before the first reverse step: a = dL/dz at the last output row (discrete mode on a plan: what the last step's outputs
// send to its y1); continuous: y = the stored z there; discrete: the cotangent of the last stage's k.
__device__ __forceinline__ void adj_init(const KArgs& a, const RevWalk& w, int e, int b0, const AdjLds& L) {
    const int H = a.H, h = e >> 4, s = e & 15, b = b0 + s;
    if (h >= H || b >= a.B) return;
    const long long o = ((long long)b * a.n_out + (a.n_out - 1)) * H + h;
    const int* plast = w.planned ? w.pfwd + (a.n_steps_fwd - 1) * w.pw_ : nullptr;      // the plan's last forward step
    float g = a.grad_out[o];
    if (w.planned && w.disc) g = plan_out_cotangent(a, plast, w.pout, 1, (long long)b * a.n_out, h);
    L.A0[e] = g;
    if (w.disc) {
        L.AS[e] = StageTranspose::seed(a.method, g, w.planned ? __int_as_float(plast[0]) : 1.0f);
    } else {
        const float y = a.z_out[o];
        L.Y0[e] = y; L.YS[e] = y; L.AS[e] = g;
    }
}

// Element e after reverse stage j, exact discrete backward: d = dL/dY of the forward stage.  After the last stage a0 = dL/dy0 of the
// step; it collects what the outputs send to this y0 (= the y1 of step m-1) and AS gets the seed of step m-1.
__device__ __forceinline__ void adj_bookkeep_discrete(const KArgs& a, const RevWalk& w, const RevStep& st, int j, int e, int b0, float d,
                                                      const AdjLds& L) {
    // (all three d slots are read and written back on every stage, whichever of them the stage's formula names: handing the LDS
    // words to StageTranspose as references saves the idle accesses but gives ncde_adj_lowrank 20 B of scratch.  A slot no stage has
    // written yet reads as 0: every kernel zeroes its whole dynamic LDS before the first barrier.)
    float a0 = L.A0[e], ka1 = L.KA1[e], ka2 = L.KA2[e], ky1 = L.KY1[e];
    bool last;
    float next = StageTranspose::apply(a.method, j, d, st.dt, a0, ka1, ka2, ky1, last);
    L.KA1[e] = ka1; L.KA2[e] = ka2; L.KY1[e] = ky1;
    if (last) {
        const int H = a.H, h = e >> 4, s = e & 15, b = b0 + s;
        const bool valid = h < H && b < a.B;
        float dtp = 1.0f;   // dt of the forward step transposed next
        if (w.planned) {
            if (valid) {
                const long long brow = (long long)b * a.n_out;
                a0 = a0 + plan_out_cotangent(a, st.pstep, w.pout, 0, brow, h);
                if (st.m > 0) a0 = a0 + plan_out_cotangent(a, st.pstep - w.pw_, w.pout, 1, brow, h);
                else a0 = a0 + a.grad_out[brow * H + h];      // row 0 of the solution is z0 itself
            }
            if (st.m > 0) dtp = __int_as_float(st.pstep[-w.pw_]);
        } else if (a.output == NCDE_OUT_KNOTS || st.n == 1) {
            a0 = a0 + (valid ? a.grad_out[((long long)b * a.n_out + (a.output == NCDE_OUT_KNOTS ? st.n - 1 : 0)) * H + h] : 0.0f);
        }
        L.A0[e] = a0;
        next = StageTranspose::seed(a.method, a0, dtp);
        if (st.m == 0 && valid) a.grad_z0[(long long)b * H + h] = a0;
    }
    L.AS[e] = next;
}

// Element e after reverse stage j, continuous adjoint in negated time: dy/ds = -f (koy = f(y).dX), da/ds = +a^T df/dy (= d).  At the
// end of a reverse solve t[i] -> t[i-1] (a plan step that names an output row; every step of NCDE_OUT_KNOTS) y is reset to the stored
// z(t[i-1]) and a += dL/dz(t[i-1]).
__device__ __forceinline__ void adj_bookkeep_continuous(const KArgs& a, const RevWalk& w, const RevStep& st, int rstep, int j, int e, int b0,
                                                        float d, float koy, const AdjLds& L) {
    float y0 = L.Y0[e], k1 = L.KY1[e], k2 = L.KY2[e];
    bool last;
    const float ys = StageCombine::apply(a.method, j, -koy, st.dt, y0, k1, k2, last);
    L.YS[e] = ys; L.KY1[e] = k1; L.KY2[e] = k2;
    float a0 = L.A0[e], q1 = L.KA1[e], q2 = L.KA2[e];
    const float as = StageCombine::apply(a.method, j, d, st.dt, a0, q1, q2, last);
    L.KA1[e] = q1; L.KA2[e] = q2;
    if (!last) {
        L.AS[e] = as;
        return;
    }
    const int H = a.H, h = e >> 4, s = e & 15, b = b0 + s;
    const bool valid = h < H && b < a.B;
    int row = -1;       // output row reached by this step
    if (w.planned) row = st.pstep[1];
    else if (a.output == NCDE_OUT_KNOTS) row = st.n - 1;
    if (row >= 0) {
        const long long o = ((long long)b * a.n_out + row) * H + h;
        y0 = valid ? a.z_out[o] : 0.0f;
        a0 = a0 + (valid ? a.grad_out[o] : 0.0f);
    } else if (!w.planned && st.n == 1) {
        a0 = a0 + (valid ? a.grad_out[((long long)b * a.n_out) * H + h] : 0.0f);
    }
    L.Y0[e] = y0; L.YS[e] = y0; L.A0[e] = a0; L.AS[e] = a0;
    if (rstep == w.n_rsteps - 1 && valid) a.grad_z0[(long long)b * H + h] = a0;
}

// one call per element after the family's own field VJP: d = dL/dy of the stage (rows >= H: 0), koy = f(y).dX
__device__ __forceinline__ void adj_bookkeep(const KArgs& a, const RevWalk& w, const RevStep& st, int rstep, int j, int e, int b0, float d,
                                             float koy, const AdjLds& L) {
    if (w.disc) adj_bookkeep_discrete(a, w, st, j, e, b0, d, L);
    else adj_bookkeep_continuous(a, w, st, rstep, j, e, b0, d, koy, L);
}
