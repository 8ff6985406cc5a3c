// Forward stage of the vector-field VARIANTS (gated heads, reset net, evaluate / derivative inputs), shared by the batch kernel
// ncde_fwd_variant (ncde_variant.hip; its adjoint reuses the building blocks) and the online field step ncde_stream_step_field
// (ncde_stream.hip).  One workgroup = one tile of 16 samples, 4 waves; activations in LDS as [unit][sample], as in
// ncde_generic_stage.h.  The text of vr_stage_forward is the stage body ncde_fwd_variant carried inline, moved without a change of
// operation order (the bitwise before / after comparison).
#pragma once
#include "ncde_generic_stage.h"

#define VR_NW GEN_NW
#define VR_THREADS GEN_THREADS

namespace {

__device__ __forceinline__ float sigmoid_dev(float x) {
    const float e = __builtin_amdgcn_exp2f(x * -1.4426950408889634f);  // exp(-x)
    return __builtin_amdgcn_rcpf(1.0f + e);
}

// control input of the stage for the 16 samples of the tile -> CIN[c*16 + s]:
// value = false: dX/dt(t) (interpolation_linear.py:231-234, interpolation_cubic.py:331-336)
// value = true : X(t)     (interpolation_linear.py:221-229, interpolation_cubic.py:324-329)
__device__ void vr_load_cin(const KArgs& a, int b0, const StageDesc& sd, bool value, float* CIN, int Cp, int tid) {
    const int idx = sd.idx;
    const float frac = sd.frac, kdt = sd.kdt;
    for (int e = tid; e < 16 * Cp; e += VR_THREADS) {
        const int s = e / Cp, c = e - s * Cp;
        const int b = b0 + s;
        float v = 0.0f;
        if (c < a.C && b < a.B) {
            const float* p = a.coeffs + (long long)b * a.cs_b + (long long)idx * a.cs_t;
            if (a.interp == NCDE_INTERP_LINEAR) {
                const float d = p[a.cs_t + c] - p[c];
                v = value ? p[c] + (frac * d) / kdt : (kdt != 1.0f ? d / kdt : d);
            } else if (a.interp == NCDE_INTERP_QUINTIC) {
                v = quintic_eval(p + c, a.C, frac, value);
            } else {
                const float aa = p[c], bb = p[a.C + c], cc = p[2 * a.C + c], dd = p[3 * a.C + c];
                if (value) {
                    float inner = 0.5f * cc + (dd * frac) / 3.0f;
                    inner = bb + inner * frac;
                    v = aa + inner * frac;
                } else {
                    const float inner = cc + dd * frac;
                    v = bb + inner * frac;
                }
            }
        }
        CIN[c * 16 + s] = v;
    }
}

// out[n][s] = act(sum_k W[n][k] in[k][s] + bias[n]), n < ru16(N) (rows >= N come out as act(0) masked to 0)
// ACT: 0 = relu, 1 = sigmoid
// wl != NULL: the matrix is resident in LDS, zero-padded to [ru16(N)][ru16(K)] with row stride ru16(K) + 1 and the bias in
// column ru16(K): at the model sizes of the reference's vector-field grids the first weight loads of every phase of a stage
// are otherwise an exposed L2 round trip, and with the padding the inner loops carry no guards (a guarded load compiles to
// an exec-mask branch per element).
template <int ACT>
__device__ void vr_dense(const float* __restrict__ W, const float* __restrict__ bias, int N, int K, const float* in, float* out,
                         int wave, int lane, const float* wl = nullptr) {
    const int li = lane & 15, lk = lane >> 4;
    const int ntiles = (N + 15) >> 4, nks = (K + 3) >> 2;
    for (int t = wave; t < ntiles; t += VR_NW) {
        const int rowA = 16 * t + li;
        const bool rv = rowA < N;
        const float* wrow = W + (long long)(rv ? rowA : 0) * K;
        f32x4 acc;
        if (wl) {
            const int Kp = ru16(K);
            const float* lrow = wl + rowA * (Kp + 1) + lk;
            const float* brow = in + lk * 16 + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = wl[(16 * t + 4 * lk + r) * (Kp + 1) + Kp];
            f32x4 acc2 = (f32x4){0.f, 0.f, 0.f, 0.f};
            for (int kb = 0; kb < Kp; kb += 16) {
                float av[4], bv[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) { av[e] = lrow[kb + 4 * e]; bv[e] = brow[(kb + 4 * e) * 16]; }
                acc = mfma16(av[0], bv[0], acc);
                acc2 = mfma16(av[1], bv[1], acc2);
                acc = mfma16(av[2], bv[2], acc);
                acc2 = mfma16(av[3], bv[3], acc2);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] += acc2[r];
        } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * t + 4 * lk + r;
            acc[r] = row < N ? bias[row] : 0.0f;
        }
#pragma unroll 4
        for (int ks = 0; ks < nks; ++ks) {
            const int k = 4 * ks + lk;
            const float av = (rv && k < K) ? wrow[k] : 0.0f;
            acc = mfma16(av, in[k * 16 + li], acc);
        }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * t + 4 * lk + r;
            const float v = ACT == 0 ? fmaxf(acc[r], 0.0f) : sigmoid_dev(acc[r]);
            out[row * 16 + li] = row < N ? v : 0.0f;
        }
    }
}

// x_1 .. x_L of the inner net for input `in`; all layers kept when X_all (adjoint), else ping-pong into A0/A1.
// Returns the buffer holding x_L.
__device__ const float* vr_net(const KArgs& a, const float* in, float* X, int DS, bool keep_all, int wave, int lane, const float* lds) {
    for (int l = 0; l < a.n_layers; ++l) {
        float* outb = keep_all ? X + l * DS : X + (l & 1) * DS;
        vr_dense<0>(a.W[l], a.b[l], a.dout[l], a.din[l], in, outb, wave, lane, a.wres[l] >= 0 ? lds + a.wres[l] : nullptr);
        __syncthreads();
        in = outb;
    }
    return in;
}

struct HeadTile {
    int rowA;       // weight row this lane streams (A operand), -1 = none
    int rowD[4];    // row of D register r, -1 = none
    int hD[4];      // state index h of D register r
};

// tile q of the head: matmul -> (hb, cq) with rows (h = 4hb+g, c = 4cq+r); direct -> rows 16q .. 16q+15 = h
__device__ __forceinline__ HeadTile vr_head_tile(const KArgs& a, int q, int ncq, int li, int lk, int& cq_out) {
    HeadTile t;
    if (a.field_input == NCDE_INPUT_MATMUL) {
        const int hb = q / ncq, cq = q - hb * ncq;
        cq_out = cq;
        const int hA = 4 * hb + (li >> 2), cA = 4 * cq + (li & 3), hD = 4 * hb + lk;
        t.rowA = (hA < a.H && cA < a.C) ? hA * a.C + cA : -1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = 4 * cq + r;
            t.rowD[r] = (hD < a.H && c < a.C) ? hD * a.C + c : -1;
            t.hD[r] = hD;
        }
    } else {
        cq_out = 0;
        t.rowA = 16 * q + li < a.H ? 16 * q + li : -1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int h = 16 * q + 4 * lk + r;
            t.rowD[r] = h < a.H ? h : -1;
            t.hD[r] = h;
        }
    }
    return t;
}

__device__ __forceinline__ f32x4 vr_head_gemm(const float* __restrict__ W, const float* __restrict__ bias, const HeadTile& t, int K,
                                              const float* in, int li, int lk, const float* wl = nullptr) {
    f32x4 acc;
    if (wl) {      // an absent row (rowA < 0) reads row 0 and multiplies by zero
        const int Kp = ru16(K);
        const float* lrow = wl + (t.rowA >= 0 ? t.rowA : 0) * (Kp + 1) + lk;
        const float* brow = in + lk * 16 + li;
        const float am = t.rowA >= 0 ? 1.0f : 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float bvv = wl[(t.rowD[r] >= 0 ? t.rowD[r] : 0) * (Kp + 1) + Kp];
            acc[r] = t.rowD[r] >= 0 ? bvv : 0.0f;
        }
        f32x4 acc2 = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int kb = 0; kb < Kp; kb += 16) {
            float av[4], bv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) { av[e] = lrow[kb + 4 * e] * am; bv[e] = brow[(kb + 4 * e) * 16]; }
            acc = mfma16(av[0], bv[0], acc);
            acc2 = mfma16(av[1], bv[1], acc2);
            acc = mfma16(av[2], bv[2], acc);
            acc2 = mfma16(av[3], bv[3], acc2);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] += acc2[r];
        return acc;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = t.rowD[r] >= 0 ? bias[t.rowD[r]] : 0.0f;
    const float* wrow = W + (long long)(t.rowA >= 0 ? t.rowA : 0) * K;
    const int nks = (K + 3) >> 2;
#pragma unroll 4
    for (int ks = 0; ks < nks; ++ks) {
        const int k = 4 * ks + lk;
        const float av = (t.rowA >= 0 && k < K) ? wrow[k] : 0.0f;
        acc = mfma16(av, in[k * 16 + li], acc);
    }
    return acc;
}

// One evaluation of the field at the stage input U [d0][16] (rows < H: the stage state, rows H..: the control input, which the
// caller has written): reset gate (gru: RG, RU), the inner net (ping-pong in XA; gru: a second pass on RU in XB), the head tiles,
// tanh (x sigmoid of the gate head), and -- matmul -- the contraction with the dX/dt image CIN [Cp][16]; KO[h][s], h < Hp, receives
// the stage derivative (rows >= H: 0).  wl_o / wl_g / wl_r and a.wres[]: LDS-resident copies of the weights (NULL / -1: streamed
// from L2); RU, RG, XB are touched by the gru field only.  Called by all threads behind a barrier that covers U and CIN; ends with
// a workgroup barrier.
__device__ void vr_stage_forward(const KArgs& a, const float* U, float* RU, float* RG, float* XA, float* XB, const float* CIN, float* KO,
                                 const float* wl_o, const float* wl_g, const float* wl_r, const float* lds, int Hp, int Cp, int DS, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int d0 = a.d0, L = a.n_layers;
    const bool matmul = a.field_input == NCDE_INPUT_MATMUL, gru = a.field_kind == NCDE_FIELD_GRU, gated = a.field_kind != NCDE_FIELD_ORIGINAL;
    const int dlast = L ? a.dout[L - 1] : d0;
    const int ncq = Cp >> 2, ngrp = matmul ? (Hp >> 2) : (Hp >> 4), per_grp = matmul ? ncq : 1;
    if (gru) {
        vr_dense<1>(a.Wr, a.br, d0, d0, U, RG, wave, lane, wl_r);
        __syncthreads();
        for (int e = tid; e < ru16(d0) * 16; e += VR_THREADS) RU[e] = RG[e] * U[e];
        __syncthreads();
    }
    const float* xi = vr_net(a, U, XA, DS, false, wave, lane, lds);
    const float* xr = gru ? vr_net(a, RU, XB, DS, false, wave, lane, lds) : xi;
    // groups of head tiles: matmul -> one h-block (all its channel quads, contraction accumulated in a
    // register); evaluate / derivative -> one 16-row tile
    for (int grp = wave; grp < ngrp; grp += VR_NW) {
        float ksum = 0.0f;
        for (int qi = 0; qi < per_grp; ++qi) {
            int cq;
            const HeadTile ht = vr_head_tile(a, grp * per_grp + qi, ncq, li, lk, cq);
            const f32x4 pt = vr_head_gemm(a.Wo, a.bo, ht, dlast, xr, li, lk, wl_o);
            f32x4 ps = pt;
            if (gated) ps = vr_head_gemm(a.Wg, a.bg, ht, dlast, xi, li, lk, wl_g);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float m = tanh_dev(pt[r]);
                if (gated) m = sigmoid_dev(ps[r]) * m;
                if (matmul) ksum = fmaf(m, CIN[(4 * cq + r) * 16 + li], ksum);
                else if (ht.hD[r] < Hp) KO[ht.hD[r] * 16 + li] = ht.rowD[r] >= 0 ? m : 0.0f;
            }
        }
        if (matmul && 4 * grp + lk < Hp) KO[(4 * grp + lk) * 16 + li] = ksum;
    }
    __syncthreads();
}

}  // namespace
