// Forward stage of the LOW-RANK vector field (src/ncde/vector_fields/sparsity.py:33-55), shared by the batch kernels ncde_fwd_lowrank /
// ncde_adj_lowrank (ncde_lowrank.hip) and the online step ncde_stream_step_lowrank (ncde_stream.hip):
//   hh = net_to_hh(z);  P = M_h hh + b_h viewed [H, R];  Q = M_o hh + b_o viewed [R, C];  M = tanh(P Q);  dz/dt = M . dX/dt
// One workgroup = one tile of 16 samples, 4 waves; activations in LDS as [unit][sample], the inner layers are the generic family's
// dense_relu.  The head is ONE GEMM over the stacked (H + C) R rows of M_h and M_o -- no activation -- into LDS (lr_heads), then the
// rank-R contraction, tanh and the channel contraction on the VALU, one thread per (h, sample) (lr_contract).  M is never stored.
// The text of the functions is the one ncde_lowrank.hip carried, moved without an edit (the bitwise before / after
// comparison).
//
// LDS layout of the two small matrices: PQ[n][s], n = the stacked row -- P[h][r] at row h R + r, Q[r][c] at row H R + r C + c.
// In the contraction a wave's lanes differ in s (16) and h (4), never in c: the 16 words Q[r][c][0..15] are consecutive (one
// bank each, the 4 h-groups read them as a broadcast).  P[h][r] of the first four ranks is held in registers over the c loop.
#pragma once
#include "ncde_generic_stage.h"

#define LR_THREADS GEN_THREADS
#define LR_NW GEN_NW
#define LR_RREG 4   // ranks whose P / Q / gradient values a thread keeps in registers (the reference's grids use R = 1..3)

namespace {

struct LrDims {
    int H, C, R, NH, NT, NTp, dlast;      // NH = H R rows of M_h, NT = NH + R C stacked rows, NTp = NT rounded up to 16
    const float* wl;                      // LDS-resident copy of the stacked head matrix [NT][ld] (bias in column dlast), or NULL
    int ld;
};

__device__ __forceinline__ const float* lr_wrow(const KArgs& a, const LrDims& d, int n) {
    if (d.wl) return d.wl + n * d.ld;
    return n < d.NH ? a.Wo + (long long)n * d.dlast : a.Wg + (long long)(n - d.NH) * d.dlast;
}
__device__ __forceinline__ float lr_bias(const KArgs& a, const LrDims& d, int n) {
    if (d.wl) return d.wl[n * d.ld + d.dlast];
    return n < d.NH ? a.bo[n] : a.bg[n - d.NH];
}

// PQ[n][s] = sum_k Wst[n][k] xl[k][s] + bst[n] for the stacked rows n < NT (rows NT .. NTp-1 come out as 0); no activation
__device__ void lr_heads(const KArgs& a, const LrDims& d, const float* xl, float* PQ, int wave, int lane) {
    const int li = lane & 15, lk = lane >> 4;
    const int ntiles = d.NTp >> 4, nks = (d.dlast + 3) >> 2;
    for (int t = wave; t < ntiles; t += LR_NW) {
        const int rowA = 16 * t + li;
        const bool rv = rowA < d.NT;
        const float* wrow = lr_wrow(a, d, rv ? rowA : 0);
        f32x4 acc;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * t + 4 * lk + r;
            acc[r] = row < d.NT ? lr_bias(a, d, row) : 0.0f;
        }
#pragma unroll 4
        for (int ks = 0; ks < nks; ++ks) {
            const int k = 4 * ks + lk;
            const float av = (rv && k < d.dlast) ? wrow[k] : 0.0f;
            acc = mfma16(av, xl[k * 16 + li], acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * t + 4 * lk + r;
            PQ[row * 16 + li] = row < d.NT ? acc[r] : 0.0f;
        }
    }
}

// S[h][c] = sum_r P[h][r] Q[r][c] for one (h, s): Ph -> P[h][0][s], Qc -> Q[0][c][s], pr = P[h][0..3] (registers)
__device__ __forceinline__ float lr_rank_sum(const LrDims& d, const float (&pr)[LR_RREG], const float* Ph, const float* Qc) {
    const int qs = d.C * 16;
    float S = 0.0f;
#pragma unroll
    for (int r = 0; r < LR_RREG; ++r)
        if (r < d.R) S = fmaf(pr[r], Qc[r * qs], S);
    for (int r = LR_RREG; r < d.R; ++r) S = fmaf(Ph[r * 16], Qc[r * qs], S);
    return S;
}

// KO[h][s] = sum_c tanh(S[h][c]) dX[c][s]      (rows h >= H come out as 0)
__device__ void lr_contract(const LrDims& d, const float* PQ, const float* CIN, float* KO, int HS, int tid) {
    for (int e = tid; e < HS; e += LR_THREADS) {
        const int h = e >> 4, s = e & 15;
        float k = 0.0f;
        if (h < d.H) {
            const float* Ph = PQ + h * d.R * 16 + s;
            const float* Qs = PQ + d.NH * 16 + s;
            float pr[LR_RREG];
#pragma unroll
            for (int r = 0; r < LR_RREG; ++r) pr[r] = r < d.R ? Ph[r * 16] : 0.0f;
            for (int c = 0; c < d.C; ++c) k = fmaf(tanh_dev(lr_rank_sum(d, pr, Ph, Qs + c * 16)), CIN[c * 16 + s], k);
        }
        KO[e] = k;
    }
}

__device__ __forceinline__ LrDims lr_dims(const KArgs& a, const float* lds) {
    LrDims d;
    d.H = a.H; d.C = a.C; d.R = a.rank;
    d.NH = a.rows; d.NT = a.rows + a.rows_g; d.NTp = ru16(d.NT);
    d.dlast = a.dout[a.n_layers - 1];
    d.ld = (d.dlast + 1) | 1;
    d.wl = a.wres_o >= 0 ? lds + a.wres_o : nullptr;
    return d;
}

}  // namespace
