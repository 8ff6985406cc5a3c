// The reference's LOW-RANK vector field (src/ncde/vector_fields/sparsity.py:33-55) on the generic 16-sample-tile structure:
//   hh = net_to_hh(z);  P = M_h hh + b_h viewed [H, R];  Q = M_o hh + b_o viewed [R, C];  M = tanh(P Q);  dz/dt = M . dX/dt
// Same design as ncde_generic.hip / ncde_variant.hip (activations in LDS as [unit][sample], fp32 MFMA 16x16x4, the whole time
// loop inside the kernel, per-workgroup parameter-gradient partials; the control input and the inner layers are the generic
// family's own load_dx / dense_relu).  What is new is the head: ONE GEMM over the stacked (H + C) R rows of M_h and M_o -- no
// activation -- into LDS, then the rank-R contraction, tanh and the channel contraction on the VALU, one thread per (h, sample).
// M is never stored.  The continuous adjoint and the exact discrete backward share one kernel, as in ncde_variant.hip.
// The forward stage (lr_heads, lr_contract and the layout of PQ) lives in ncde_lowrank_stage.h, which the online step shares.
#include "ncde_host.h"
#include "ncde_lowrank.h"
#include "ncde_lowrank_stage.h"
#include "ncde_timeloop.h"

namespace {

__device__ void lr_fill_resident(const KArgs& a, const LrDims& d, float* dst, int tid) {
    for (int e = tid; e < d.NT * d.ld; e += LR_THREADS) {
        const int n = e / d.ld, c = e - n * d.ld;
        const float* w = n < d.NH ? a.Wo + (long long)n * d.dlast : a.Wg + (long long)(n - d.NH) * d.dlast;
        float v = 0.0f;
        if (c < d.dlast) v = w[c];
        else if (c == d.dlast) v = n < d.NH ? a.bo[n] : a.bg[n - d.NH];
        dst[e] = v;
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(LR_THREADS) void ncde_fwd_lowrank(KArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = blockIdx.x * NCDE_TILE;
    const TileDims td = tile_dims(a);
    const int H = a.H, Cp = td.Cp, HS = td.HS, DS = td.DS, L = a.n_layers;
    const LrDims d = lr_dims(a, lds);
    float* U = lds;              // stage state [Dp][16] (rows >= H stay 0)
    float* XA = U + DS;          // ping-pong activations of the inner net (2 buffers)
    float* Y0 = XA + 2 * DS;
    float* K1 = Y0 + HS;
    float* K2 = K1 + HS;
    float* KO = K2 + HS;
    float* CIN = KO + HS;        // dX/dt [Cp][16]
    float* PQ = CIN + Cp * 16;   // [NTp][16]
    const int total = 3 * DS + 4 * HS + Cp * 16 + d.NTp * 16;
    for (int e = tid; e < total; e += LR_THREADS) lds[e] = 0.0f;
    if (a.wres_o >= 0) lr_fill_resident(a, d, lds + a.wres_o, tid);
    __syncthreads();
    for (int e = tid; e < HS; e += LR_THREADS) {
        const int h = e >> 4, s = e & 15, b = b0 + s;
        if (h < H && b < a.B) {
            const float v = a.z0[(long long)b * H + h];
            Y0[e] = v;
            U[e] = v;
            a.out[((long long)b * a.n_out) * H + h] = v;
        }
    }
    if (!plan_ok(a)) return;      // (uniform: before the first barrier of the loop)
    const FwdWalk walk = fwd_walk(a);
    for (int n = 0; n < walk.n_steps; ++n) {
        const FwdStep st = fwd_step(a, walk, n);
        for (int j = 0; j < walk.S; ++j) {
            const StageDesc sd = fwd_stage(a, walk, st.pstep, n, j);
            __syncthreads();      // U of this stage is complete (first stage: the z0 load above)
            load_dx(a, b0, sd, CIN, Cp, tid);
            if (a.stages) stage_record_store(a, n * walk.S + j, b0, U, tid, LR_THREADS);
            const float* in = U;
            for (int l = 0; l < L; ++l) {
                float* outb = XA + (l & 1) * DS;
                dense_relu(a.W[l], a.b[l], a.dout[l], a.din[l], in, outb, wave, lane);
                __syncthreads();
                in = outb;
            }
            lr_heads(a, d, in, PQ, wave, lane);
            __syncthreads();
            lr_contract(d, PQ, CIN, KO, HS, tid);
            __syncthreads();
            for (int e = tid; e < HS; e += LR_THREADS) fwd_bookkeep(a, walk, st.pstep, n, j, st.dt, e, b0, KO, U, Y0, K1, K2);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// adjoint / exact discrete backward
// ------------------------------------------------------------------------------------------------
namespace {

// out[i][s] = sum_j W(j)[i] gpre[j][s], i < ru16(K); optionally x relu'(mask[i][s]).  wrow(j): row j of the [N][K] matrix
template <class WRow>
__device__ void lr_bwd_data(WRow wrow, int N, int K, const float* gpre, const float* mask, float* out, int wave, int lane) {
    const int li = lane & 15, lk = lane >> 4;
    const int nit = (K + 15) >> 4, nks = (N + 3) >> 2;
    for (int it = wave; it < nit; it += LR_NW) {
        const int col = 16 * it + li;
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int ks = 0; ks < nks; ++ks) {
            const int k = 4 * ks + lk;
            const float av = (k < N && col < K) ? wrow(k)[col] : 0.0f;
            acc = mfma16(av, gpre[k * 16 + li], acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * it + 4 * lk + r;
            float v = acc[r];
            if (mask) v = mask[row * 16 + li] > 0.0f ? v : 0.0f;
            out[row * 16 + li] = v;
        }
    }
}

// One stage's head backward on the VALU, cotangent AS[h][s]:  gS[h][c] = AS[h] dX[c] (1 - M^2), recomputed in both passes,
//   pass 1, one thread per (h, s):  KOY[h] = sum_c M dX[c];  gP[h][r] = sum_c gS[h][c] Q[r][c]   -> G rows h R + r
//   pass 2, one thread per (c, s):  gQ[r][c] = sum_h P[h][r] gS[h][c]                              -> G rows H R + r C + c
// (ranks >= LR_RREG accumulate in the thread's own words of G)
__device__ void lr_head_vjp(const LrDims& d, const float* PQ, const float* CIN, const float* AS, float* G, float* KOY, int HS, int tid) {
    const int qs = d.C * 16;
    const float* Qb = PQ + d.NH * 16;
    float* GQ = G + d.NH * 16;
    for (int e = tid; e < HS; e += LR_THREADS) {
        const int h = e >> 4, s = e & 15;
        float k = 0.0f;
        if (h < d.H) {
            const float* Ph = PQ + h * d.R * 16 + s;
            float* Gh = G + h * d.R * 16 + s;
            const float ah = AS[e];
            float pr[LR_RREG], gp[LR_RREG];
#pragma unroll
            for (int r = 0; r < LR_RREG; ++r) { pr[r] = r < d.R ? Ph[r * 16] : 0.0f; gp[r] = 0.0f; }
            for (int r = LR_RREG; r < d.R; ++r) Gh[r * 16] = 0.0f;
            for (int c = 0; c < d.C; ++c) {
                const float* Qc = Qb + c * 16 + s;
                const float dx = CIN[c * 16 + s];
                const float m = tanh_dev(lr_rank_sum(d, pr, Ph, Qc));
                k = fmaf(m, dx, k);
                const float gS = (ah * dx) * (1.0f - m * m);
#pragma unroll
                for (int r = 0; r < LR_RREG; ++r)
                    if (r < d.R) gp[r] = fmaf(gS, Qc[r * qs], gp[r]);
                for (int r = LR_RREG; r < d.R; ++r) Gh[r * 16] = fmaf(gS, Qc[r * qs], Gh[r * 16]);
            }
#pragma unroll
            for (int r = 0; r < LR_RREG; ++r)
                if (r < d.R) Gh[r * 16] = gp[r];
        }
        KOY[e] = k;
    }
    for (int e = tid; e < d.C * 16; e += LR_THREADS) {
        const int s = e & 15;
        const float* Qc = Qb + e;         // Q[0][c][s]
        float* Gc = GQ + e;
        const float dx = CIN[e];
        float qr[LR_RREG], gq[LR_RREG];
#pragma unroll
        for (int r = 0; r < LR_RREG; ++r) { qr[r] = r < d.R ? Qc[r * qs] : 0.0f; gq[r] = 0.0f; }
        for (int r = LR_RREG; r < d.R; ++r) Gc[r * qs] = 0.0f;
        for (int h = 0; h < d.H; ++h) {
            const float* Ph = PQ + h * d.R * 16 + s;
            float S = 0.0f;
#pragma unroll
            for (int r = 0; r < LR_RREG; ++r)
                if (r < d.R) S = fmaf(Ph[r * 16], qr[r], S);
            for (int r = LR_RREG; r < d.R; ++r) S = fmaf(Ph[r * 16], Qc[r * qs], S);
            const float m = tanh_dev(S);
            const float gS = (AS[h * 16 + s] * dx) * (1.0f - m * m);
#pragma unroll
            for (int r = 0; r < LR_RREG; ++r)
                if (r < d.R) gq[r] = fmaf(Ph[r * 16], gS, gq[r]);
            for (int r = LR_RREG; r < d.R; ++r) Gc[r * qs] = fmaf(Ph[r * 16], gS, Gc[r * qs]);
        }
#pragma unroll
        for (int r = 0; r < LR_RREG; ++r)
            if (r < d.R) Gc[r * qs] = gq[r];
    }
}

}  // namespace

extern "C" __global__ __launch_bounds__(LR_THREADS) void ncde_adj_lowrank(KArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = blockIdx.x * NCDE_TILE;
    const TileDims td = tile_dims(a);
    const int H = a.H, Cp = td.Cp, HS = td.HS, DS = td.DS, L = a.n_layers;
    const LrDims d = lr_dims(a, lds);
    float* U = lds;                  // stage input (rows >= H stay 0)
    float* XI = U + DS;              // [L] activations of the inner net
    float* GA = XI + L * DS;         // dL/dpre ping
    float* GB = GA + DS;             // pong
    float* DU = GB + DS;             // cotangent of the stage input
    float* AS = DU + DS;             // stage cotangent [Hp][16]
    float* Y0 = AS + HS;
    float* A0 = Y0 + HS;
    float* KY1 = A0 + HS;
    float* KY2 = KY1 + HS;
    float* KA1 = KY2 + HS;
    float* KA2 = KA1 + HS;
    float* KOY = KA2 + HS;
    float* CIN = KOY + HS;           // dX/dt [Cp][16]
    float* PQ = CIN + Cp * 16;       // [NTp][16]
    float* G = PQ + d.NTp * 16;      // gP | gQ, stacked like PQ, [NTp][16] (rows >= NT stay 0)
    float* GL = G + d.NTp * 16;      // the gradient partial, when it fits
    const int total = (4 + L) * DS + 8 * HS + Cp * 16 + 2 * d.NTp * 16 + (a.gacc_in_lds ? a.theta_size : 0);
    for (int e = tid; e < total; e += LR_THREADS) lds[e] = 0.0f;
    if (a.wres_o >= 0) lr_fill_resident(a, d, lds + a.wres_o, tid);
    float* gacc = a.gacc_in_lds ? GL : a.gpart + (long long)blockIdx.x * a.theta_size;
    if (!a.gacc_in_lds)
        for (int e = tid; e < a.theta_size; e += LR_THREADS) gacc[e] = 0.0f;
    __syncthreads();
    if (!plan_ok(a)) return;      // (uniform: before the first barrier of the loop)
    const RevWalk walk = rev_walk(a);
    const AdjLds bk = {U, AS, Y0, KY1, KY2, A0, KA1, KA2};
    for (int e = tid; e < HS; e += LR_THREADS) adj_init(a, walk, e, b0, bk);
    const float* xl = XI + (L - 1) * DS;
    auto head_w = [&](int n) { return gacc + (n < d.NH ? a.gWo_off + (long long)n * d.dlast : a.gWg_off + (long long)(n - d.NH) * d.dlast); };
    auto head_b = [&](int n) { return gacc + (n < d.NH ? a.gbo_off + n : a.gbg_off + (n - d.NH)); };
    auto head_row = [&](int n) { return lr_wrow(a, d, n); };
    for (int rstep = 0; rstep < walk.n_rsteps; ++rstep) {
        const RevStep st = rev_step(a, walk, rstep);
        for (int j = 0; j < walk.S; ++j) {
            const RevStage rs = rev_stage(a, walk, st, j);
            const float w = rs.w;
            __syncthreads();      // U / AS of this stage are complete (first stage: the loads above)
            load_dx(a, b0, rs.sd, CIN, Cp, tid);
            if (walk.disc) stage_record_load(a, rev_record_index(walk, st, j), b0, U, tid, LR_THREADS);
            __syncthreads();
            // ---- the stage forward, every layer kept ------------------------------------------------------------------------
            const float* in = U;
            for (int l = 0; l < L; ++l) {
                dense_relu(a.W[l], a.b[l], a.dout[l], a.din[l], in, XI + l * DS, wave, lane);
                __syncthreads();
                in = XI + l * DS;
            }
            lr_heads(a, d, xl, PQ, wave, lane);
            __syncthreads();
            // ---- heads backwards: f, gP, gQ (VALU) -----------------------------------------------------------------------------
            lr_head_vjp(d, PQ, CIN, AS, G, KOY, HS, tid);
            __syncthreads();
            // ---- dM_h | dM_o += w G (x) x_L, their biases;  dL/dpre_L = (M_h^T gP + M_o^T gQ) * relu'(x_L): one GEMM over the stacked rows
            if (w != 0.0f) dw_acc(G, xl, d.NT, d.dlast, w, head_w, head_b, tid, wave, lane, a.gacc_in_lds);
            lr_bwd_data(head_row, d.NT, d.dlast, G, xl, GA, wave, lane);
            __syncthreads();
            // ---- the inner net backwards (the generic family's) ----------------------------------------------------------------
            float* gpre = GA;
            float* gx = GB;
            for (int l = L - 1; l >= 0; --l) {
                const int N = a.dout[l], K = a.din[l];
                const float* xin = l == 0 ? U : XI + (l - 1) * DS;
                const float* Wl = a.W[l];
                if (w != 0.0f) {
                    float* gW = gacc + a.gW_off[l];
                    float* gb = gacc + a.gb_off[l];
                    dw_acc(gpre, xin, N, K, w, GradRows{gW, K}, GradRows{gb, 1}, tid, wave, lane, a.gacc_in_lds);
                }
                lr_bwd_data([&](int r) { return Wl + (long long)r * K; }, N, K, gpre, l > 0 ? xin : nullptr, l == 0 ? DU : gx, wave, lane);
                __syncthreads();
                float* tmp = gpre; gpre = gx; gx = tmp;
            }
            // ---- Butcher bookkeeping (d = dL/dy of the stage = the first H rows of DU) ----------------------------------------------
            for (int e = tid; e < HS; e += LR_THREADS) adj_bookkeep(a, walk, st, rstep, j, e, b0, (e >> 4) < H ? DU[e] : 0.0f, KOY[e], bk);
        }
    }
    if (a.gacc_in_lds) {
        __syncthreads();
        float* dst = a.gpart + (long long)blockIdx.x * a.theta_size;
        for (int e = tid; e < a.theta_size; e += LR_THREADS) dst[e] = GL[e];
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
namespace {

struct LrPlan {
    bool ok;
    size_t lds_fwd, lds_adj;        // bytes, the resident copy of the heads included
    int res_fwd, res_adj;           // float offset of the LDS-resident stacked head matrix, -1 = streamed from L2
    int gacc_in_lds;
};

LrPlan lr_plan(const NcdeProblem* p, const Layout& y) {
    LrPlan v{};
    v.res_fwd = v.res_adj = -1;
    const size_t HS = (size_t)y.Hp * 16, DS = (size_t)y.Dp * 16, L = (size_t)p->n_layers;
    const size_t NT = (size_t)y.rows + (size_t)y.rows_g, NTp = (NT + 15) & ~(size_t)15;
    const size_t fwd = 3 * DS + 4 * HS + (size_t)y.Cp * 16 + NTp * 16;
    size_t adj = (4 + L) * DS + 8 * HS + (size_t)y.Cp * 16 + 2 * NTp * 16;
    const size_t limit = (size_t)kLdsLimit / sizeof(float);
    v.gacc_in_lds = adj + (size_t)y.theta_size <= limit;
    if (v.gacc_in_lds) adj += (size_t)y.theta_size;
    const size_t res = NT * (size_t)((y.dlast + 1) | 1);
    v.lds_fwd = fwd; v.lds_adj = adj;
    if (fwd + res <= limit) { v.res_fwd = (int)fwd; v.lds_fwd = fwd + res; }
    if (adj + res <= limit) { v.res_adj = (int)adj; v.lds_adj = adj + res; }
    v.ok = fwd <= limit && adj <= limit;
    v.lds_fwd *= sizeof(float); v.lds_adj *= sizeof(float);
    return v;
}

bool lr_refuse(char* why, size_t n, const char* fmt, long long a0 = 0, long long a1 = 0) {
    if (why && n) snprintf(why, n, fmt, a0, a1);
    return false;
}

}  // namespace

bool ncde_lowrank_supported(const NcdeProblem* p, int pass, char* why, size_t n) {
    const Layout y = make_layout(p);
    if (p->field_kind != NCDE_FIELD_LOWRANK || p->field_input != NCDE_INPUT_MATMUL) return lr_refuse(why, n, "not a low-rank field with the matmul input");
    if (p->n_layers < 1) return lr_refuse(why, n, "the low-rank kernels need at least one inner layer");
    if (p->hidden > 128 || p->channels > 128) return lr_refuse(why, n, "the low-rank kernels cover hidden <= 128 and channels <= 128 (got %lld, %lld)", p->hidden, p->channels);
    for (int l = 0; l < p->n_layers; ++l)
        if (p->layer_out[l] > 128) return lr_refuse(why, n, "the low-rank kernels cover layer widths <= 128 (layer %lld: %lld)", l, p->layer_out[l]);
    const LrPlan v = lr_plan(p, y);
    const size_t need = pass == 0 ? v.lds_fwd : v.lds_adj;
    if (need > (size_t)kLdsLimit) return lr_refuse(why, n, "the low-rank kernel of pass %lld needs %lld B of LDS", pass, (long long)need);
    return true;
}

int64_t ncde_lowrank_workspace_bytes(const NcdeProblem* p, int pass) {
    if (!ncde_lowrank_supported(p, pass)) return NCDE_ERR_UNSUPPORTED;
    if (pass == 0) return 256;
    const Layout y = make_layout(p);
    return (int64_t)sizeof(float) * (int64_t)y.n_wg * (int64_t)y.theta_size + 256;
}

int ncde_lowrank_forward(const NcdeProblem* p, float* out, float* stages, hipStream_t st) {
    if (!ncde_lowrank_supported(p, 0)) return NCDE_ERR_UNSUPPORTED;
    const Layout y = make_layout(p);
    const LrPlan v = lr_plan(p, y);
    KArgs a;
    fill_kargs(p, y, &a);
    a.out = out;
    a.stages = stages;
    a.wres_o = v.res_fwd;
    if (ncde_lds_optin((const void*)ncde_fwd_lowrank, v.lds_fwd) != hipSuccess) return NCDE_ERR_HIP;
    hipLaunchKernelGGL(ncde_fwd_lowrank, dim3(y.n_wg), dim3(LR_THREADS), v.lds_fwd, st, a);
    return hipGetLastError() == hipSuccess ? NCDE_OK : NCDE_ERR_HIP;
}

int ncde_lowrank_adjoint(const NcdeProblem* p, const float* src, const float* grad_out, const NcdeGrads* g, void* ws, hipStream_t st,
                         bool main_kernel_only, bool discrete) {
    if (!ncde_lowrank_supported(p, discrete ? 2 : 1)) return NCDE_ERR_UNSUPPORTED;
    const Layout y = make_layout(p);
    const LrPlan v = lr_plan(p, y);
    KArgs a;
    fill_kargs(p, y, &a);
    a.grad_out = grad_out; a.grad_z0 = g->grad_z0;
    if (discrete) { a.stages = const_cast<float*>(src); a.discrete = 1; }
    else a.z_out = src;
    a.gpart = (float*)ws;
    a.gacc_in_lds = v.gacc_in_lds;
    a.wres_o = v.res_adj;
    if (ncde_lds_optin((const void*)ncde_adj_lowrank, v.lds_adj) != hipSuccess) return NCDE_ERR_HIP;
    hipLaunchKernelGGL(ncde_adj_lowrank, dim3(y.n_wg), dim3(LR_THREADS), v.lds_adj, st, a);
    if (hipGetLastError() != hipSuccess) return NCDE_ERR_HIP;
    if (main_kernel_only) return NCDE_OK;
    return launch_reduce_partials(p, y, g, (const float*)ws, y.n_wg, st);
}
