// Generic (runtime-dimension) Neural-CDE kernels for gfx950.
//
// One workgroup = one tile of 16 samples, 4 waves.  All activations live in LDS as [unit][sample]
// (sample fastest), which is simultaneously the B-operand image (k = unit, n = sample) and the
// A-operand image (m = unit, k = sample) of v_mfma_f32_16x16x4_f32, so every GEMM of the forward
// stage, of the VJP and of the weight gradient is an MFMA chain fed from LDS (activations) and
// global/L2 (weights).  The whole time loop runs inside the kernel: the state never leaves the CU.
//
// This family covers ANY (H, layer widths, C, T, B); shape-specialised register-resident kernels
// live in ncde_fast_kernels.h.  Reference semantics restated (paths relative to the reference project):
//   stage loop          modules/torchdiffeq/torchdiffeq/_impl/solvers.py:103-117, fixed_grid.py:6-29,
//                       rk_common.py:106-114
//   f_theta(z).dX/dt    src/ncde/vector_fields/base.py:83-104, modules/torchcde/torchcde/solver.py:112-137
//   dX/dt               modules/torchcde/torchcde/interpolation_linear.py:212-234, interpolation_cubic.py:315-336
//   adjoint sweep       modules/torchdiffeq/torchdiffeq/_impl/adjoint.py:37-145, misc.py:152-159
#include "ncde_common.h"

#include "ncde_generic_stage.h"
#include "ncde_timeloop.h"

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(GEN_THREADS) void ncde_fwd_generic(KArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * NCDE_TILE;
    const TileDims td = tile_dims(a);
    const int H = a.H, Hp = td.Hp, Cp = td.Cp, HS = td.HS, DS = td.DS;
    float* YS = lds;
    float* ACT0 = YS + HS;
    float* ACT1 = ACT0 + DS;
    float* Y0 = ACT1 + DS;
    float* K1 = Y0 + HS;
    float* K2 = K1 + HS;
    float* KO = K2 + HS;
    float* DX = KO + HS;
    const int total = 5 * HS + 2 * DS + Cp * 16;
    for (int e = tid; e < total; e += GEN_THREADS) lds[e] = 0.0f;
    __syncthreads();
    for (int e = tid; e < HS; e += GEN_THREADS) {
        const int h = e >> 4, s = e & 15, b = b0 + s;
        if (h < H && b < a.B) {
            const float v = a.z0[(long long)b * H + h];
            Y0[e] = v;
            YS[e] = v;
            a.out[((long long)b * a.n_out) * H + h] = v;
        }
    }
    int cur_idx = -1;
    if (!plan_ok(a)) return;      // (uniform: before the first barrier)
    const FwdWalk walk = fwd_walk(a);
    for (int n = 0; n < walk.n_steps; ++n) {
        const FwdStep st = fwd_step(a, walk, n);
        for (int j = 0; j < walk.S; ++j) {
            const StageDesc sd = fwd_stage(a, walk, st.pstep, n, j);
            if (a.interp != NCDE_INTERP_LINEAR || sd.idx != cur_idx) {
                load_dx(a, b0, sd, DX, Cp, tid);
                cur_idx = sd.idx;
            }
            __syncthreads();
            if (a.stages) stage_record_store(a, n * walk.S + j, b0, YS, tid, GEN_THREADS);  // the stage input, for the exact discrete backward
            gen_stage_forward(a, YS, ACT0, ACT1, DX, KO, Hp, Cp, tid);
            for (int e = tid; e < HS; e += GEN_THREADS) fwd_bookkeep(a, walk, st.pstep, n, j, st.dt, e, b0, KO, YS, Y0, K1, K2);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// adjoint (reverse sweep of y, a, g_theta)
// ------------------------------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(GEN_THREADS) void ncde_adj_generic(KArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * NCDE_TILE;
    const TileDims td = tile_dims(a);
    const int Hp = td.Hp, Cp = td.Cp, HS = td.HS, DS = td.DS, L = a.n_layers;
    // state arrays [Hp][16]
    float* YS = lds;           // y stage input (= x_0)
    float* AS = YS + HS;       // a stage input
    float* Y0 = AS + HS;
    float* A0 = Y0 + HS;
    float* KY1 = A0 + HS;
    float* KY2 = KY1 + HS;
    float* KA1 = KY2 + HS;
    float* KA2 = KA1 + HS;
    float* KOY = KA2 + HS;     // f(y).dX of the stage
    float* KOA = KOY + HS;     // a^T df/dy of the stage
    float* X = KOA + HS;       // x_1..x_L, [L][Dp][16]
    float* G0 = X + (L > 0 ? L : 1) * DS;  // dL/dx ping
    float* G1 = G0 + DS;       // dL/dpre pong
    float* PW2 = G1 + DS;      // partial buffers of waves 2,3 (waves 0,1 use G0,G1)
    float* DX = PW2 + 2 * DS;
    float* SC = DX + Cp * 16;  // per-wave 16x17 transpose scratch
    float* GL = SC + GEN_NW * 16 * 17;  // parameter-gradient partial when it fits in LDS
    const int total = 10 * HS + ((L > 0 ? L : 1) + 4) * DS + Cp * 16 + GEN_NW * 16 * 17 + (a.gacc_in_lds ? a.theta_size : 0);
    for (int e = tid; e < total; e += GEN_THREADS) lds[e] = 0.0f;
    float* gacc = a.gacc_in_lds ? GL : a.gpart + (long long)blockIdx.x * a.theta_size;
    if (!a.gacc_in_lds)
        for (int e = tid; e < a.theta_size; e += GEN_THREADS) gacc[e] = 0.0f;
    __syncthreads();
    if (!plan_ok(a)) return;      // (uniform: before the first barrier)
    const RevWalk walk = rev_walk(a);
    const AdjLds bk = {YS, AS, Y0, KY1, KY2, A0, KA1, KA2};
    for (int e = tid; e < HS; e += GEN_THREADS) adj_init(a, walk, e, b0, bk);
    for (int rstep = 0; rstep < walk.n_rsteps; ++rstep) {
        const RevStep st = rev_step(a, walk, rstep);
        for (int j = 0; j < walk.S; ++j) {
            const RevStage rs = rev_stage(a, walk, st, j);
            load_dx(a, b0, rs.sd, DX, Cp, tid);
            if (walk.disc) stage_record_load(a, rev_record_index(walk, st, j), b0, YS, tid, GEN_THREADS);
            __syncthreads();
            gen_stage_vjp(a, YS, AS, DX, nullptr, X, G0, G1, PW2, SC, KOY, KOA, gacc, rs.w, Hp, Cp, DS, tid);
            for (int e = tid; e < HS; e += GEN_THREADS) adj_bookkeep(a, walk, st, rstep, j, e, b0, KOA[e], KOY[e], bk);
            __syncthreads();
        }
    }
    if (a.gacc_in_lds) {
        float* dst = a.gpart + (long long)blockIdx.x * a.theta_size;
        for (int e = tid; e < a.theta_size; e += GEN_THREADS) dst[e] = GL[e];
    }
}

// ------------------------------------------------------------------------------------------------
// K4: deterministic reduction of per-workgroup partials + scatter into the caller's gradient buffers
// ------------------------------------------------------------------------------------------------
struct ReduceSegs {
    int n;
    int off[2 * NCDE_MAX_LAYERS + 6];
    int len[2 * NCDE_MAX_LAYERS + 6];
    float* dst[2 * NCDE_MAX_LAYERS + 6];
};

extern "C" __global__ __launch_bounds__(256) void ncde_reduce_partials(const float* __restrict__ gpart, int n_part,
                                                                        int theta_size, ReduceSegs segs) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= theta_size) return;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int p = 0;
    for (; p + 3 < n_part; p += 4) {
        s0 += gpart[(long long)p * theta_size + k];
        s1 += gpart[(long long)(p + 1) * theta_size + k];
        s2 += gpart[(long long)(p + 2) * theta_size + k];
        s3 += gpart[(long long)(p + 3) * theta_size + k];
    }
    for (; p < n_part; ++p) s0 += gpart[(long long)p * theta_size + k];
    const float total = (s0 + s1) + (s2 + s3);
    for (int i = 0; i < segs.n; ++i)
        if (k >= segs.off[i] && k < segs.off[i] + segs.len[i]) segs.dst[i][k - segs.off[i]] = total;
}
