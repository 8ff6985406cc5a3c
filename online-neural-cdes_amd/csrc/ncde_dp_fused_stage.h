// The stage machinery of the two fused dopri5 kernels that differentiate the vector field, ncde_dpf_adj (adaptive continuous adjoint,
// one attempt per launch) and ncde_dpf_tape (persistent reverse sweep of an adjoint=False solve), both in ncde_adaptive_fast.hip:
// the pack layout of their weight image, ONE layout of their dynamic LDS (the host's dpa_lds_bytes reads its BYTES), the pointers a
// wave derives from it, the weight prologue, the dX/dt loader (ncde_dpf_fwd uses it too), the stage-input exchange and the stage body
// -- forward recompute, output tiles, Wo^T dP, cross-wave sum, hidden backward -- stated once.  One workgroup = one 16-sample tile, 4
// waves (the structure of ncde_adj_fast, ncde_fast_kernels.h).  The body is the text both kernels carried, moved without a change of
// operation order.  ncde_dpf_tape runs on all of it; ncde_dpf_adj shares the layout, the prologue, the loader, the exchange and the
// hidden-layer write-out and keeps its two-sum stage body inline (registers, bits, times).
#pragma once
#include "ncde_common.h"
#include "ncde_dp_defs.h"
#include "ncde_fastdefs.h"

// Weight image of the two kernels (written once per solve by ncde_dpa_pack).
template <int H, int HH, int C, int NL>
struct DpaPack {
    static constexpr int NW = 4, CP = (C + 3) & ~3, CQ = CP / 4, HB = H / 4, HT = HH / 16, KH = HH / 4, NB = HB / NW, NTILE = NB * CQ;
    // per wave and lane (registers): the A operands of the wave's own output tiles, the hidden-layer biases
    static constexpr int O_WO = 0, LANE = NB * CQ * KH, LANE4 = (LANE + 3) / 4;
    static constexpr int WAVE = LANE4 * 256;                    // floats per wave: [chunk of 4][lane][4]
    // shared operand images (LDS): [tile][chunk of 4 k-steps][lane][4] -- one ds_read_b128 feeds four MFMAs
    static constexpr int WOT = NW * NTILE * HT * 256, BOL = NW * NTILE * 16;
    static constexpr int I_W0 = 0, I_W1 = I_W0 + HT * (HB / 4) * 256, I_W1T = I_W1 + HT * (KH / 4) * 256, I_W0T = I_W1T + HT * (KH / 4) * 256,
                         I_WOT = I_W0T + NW * (KH / 4) * 256, I_BOL = I_WOT + WOT, I_B0 = I_BOL + BOL, I_B1 = I_B0 + HT * 16,
                         IMGS = I_B1 + HT * 16;      // I_B0 / I_B1: hidden-layer biases [t][g][r] (the accumulator a lane starts a tile with)
    static constexpr int TOTAL = NW * WAVE + IMGS;
};

// Dynamic LDS of the two kernels, offsets in floats.  The wave-private [unit][sample] images (row stride XS) keep only the rows the
// wave's own weight-gradient tiles read.
template <int H, int HH, int C, int NL>
struct DpaLayout {
    typedef DpaPack<H, HH, C, NL> PK;
    static constexpr int NW = 4, NT = 256, CP = PK::CP, XS = 20;
    static constexpr int R_Z = 0, R_X = 16, R_XL = R_X + 16 * (NL - 1), R_DP = R_XL + HH, PRIV = (R_DP + HH) * XS;      // image rows of a wave
    static constexpr int O_ZX = 0,                            // [2][H*16]   stage-state exchange
                         O_DXS = O_ZX + 2 * H * 16,           // [2][16*CP]  dX/dt of the stage, by parity
                         O_D2S = O_DXS + 2 * 16 * CP,         // [2][16*CP]  d2X/dt2 (cubic control: the vjp_t component)
                         O_RED = O_D2S + 2 * 16 * CP,         // [NW][HH*16] dL/dx_L partials
                         O_IMG = O_RED + NW * HH * 16,        // operand images (DpaPack::I_*)
                         O_PRIV = O_IMG + PK::IMGS,           // [NW][PRIV]
                         O_SH = O_PRIV + NW * PRIV;           // 16 doubles: the workgroup's partial sums
    static constexpr size_t BYTES = 4 * (size_t)O_SH + 16 * sizeof(double);
    static constexpr int EPT = (16 * CP + NT - 1) / NT;       // (sample, channel) entries of a stage's dX/dt per thread
};

// dX/dt (and, with D2, d2X/dt2) of the control path at the stage `sd` for one (sample, channel)
template <bool D2>
__device__ __forceinline__ void dp_control_derivative(const KArgs& a, const StageDesc& sd, bool linear, int b, int cc, float& v, float& v2) {
    const int Cr = a.C;
    const float* p = a.coeffs + (long long)b * a.cs_b + (long long)sd.idx * a.cs_t;
    if (linear) {
        v = p[a.cs_t + cc] - p[cc];
        if (sd.kdt != 1.0f) v = v / sd.kdt;
    } else {
        const float bb = p[Cr + cc], c2 = p[2 * Cr + cc], dd = p[3 * Cr + cc];
        const float inner = c2 + dd * sd.frac;
        v = bb + inner * sd.frac;
        if (D2) v2 = inner + dd * sd.frac;
    }
}


// The taped sweep: ONE sum, weight 1.
template <int NTILE, int HT>
struct DpaGradOne {
    f32x4 gWo[NTILE][HT], gW1, gW0, gbo;
    float gb1, gb0;
    __device__ __forceinline__ void clear() {
        const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
        gW1 = gW0 = gbo = zero4;
        gb1 = gb0 = 0.0f;
#pragma unroll
        for (int i = 0; i < NTILE; ++i)
#pragma unroll
            for (int t = 0; t < HT; ++t) gWo[i][t] = zero4;
    }
    __device__ __forceinline__ void add_bo(const f32x4& sm) {
#pragma unroll
        for (int r = 0; r < 4; ++r) gbo[r] += sm[r];
    }
    __device__ __forceinline__ void add_b(float& gb, float sm) { gb += sm; }
    __device__ __forceinline__ void add_vt(float) {}      // (the sweep reads the stage's vt itself)
    __device__ __forceinline__ void add_wo(int tau, const f32x4& av, const f32x4 (&xB)[HT]) {
#pragma unroll
        for (int tt = 0; tt < HT; ++tt)
#pragma unroll
            for (int q = 0; q < 4; ++q) gWo[tau][tt] = mfma16(av[q], xB[tt][q], gWo[tau][tt]);
    }
    __device__ __forceinline__ void add_w(f32x4& gw, const f32x4& av, const f32x4& bv) {
#pragma unroll
        for (int q = 0; q < 4; ++q) gw = mfma16(av[q], bv[q], gw);
    }
};

// What a wave of either kernel derives from (lds, tid), and the shared text on it.
template <int H, int HH, int C, int NL>
struct DpaStage : DpaLayout<H, HH, C, NL> {
    typedef DpaLayout<H, HH, C, NL> L;
    typedef DpaPack<H, HH, C, NL> PK;
    static constexpr int NW = L::NW, NT = L::NT, CP = L::CP, XS = L::XS, EPT = L::EPT;
    static constexpr int CQ = PK::CQ, HB = PK::HB, HT = PK::HT, KH = PK::KH, NB = PK::NB, NTILE = PK::NTILE, HT0 = H / 16;
    static_assert(H % (4 * NW) == 0 && HH % 16 == 0 && H % 16 == 0 && NB <= 4 && NTILE <= 16 && KH <= 16, "shape not tileable");
    static_assert(HT * HT == NW && HT * HT0 == NW, "one dW1 tile and one dW0 tile per wave");

    int tid, lane, wave, s, g;
    float *zx, *dxs, *d2s, *red, *simg;
    double* sh;
    float* priv;       // the wave's images: rows R_Z (z, the 16 rows its dW0 tile reads), R_X (x_1 .. x_{NL-1}, the rows of its dW1 tile) ..
    float* zimg;
    float* xLimg;      // x_NL, all rows (B operand of dWo)
    float* dpimg;      // [HH][XS] dL/dpre of the current layer
    float* dptile;     // [16][XS] dP of the current output tile (aliases dpimg: disjoint phases)
    int tr1, tc1, tr0, tc0;      // the wave's dW1 tile and dW0 tile
    const float *w0i, *w1i, *w1ti, *w0ti, *woTw, *boLw, *b0i, *b1i;

    __device__ __forceinline__ DpaStage(float* lds, int tid_) {
        tid = tid_;
        lane = tid & 63;
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        s = lane & 15;
        g = lane >> 4;
        zx = lds + L::O_ZX;
        dxs = lds + L::O_DXS;
        d2s = lds + L::O_D2S;
        red = lds + L::O_RED;
        simg = lds + L::O_IMG;
        sh = reinterpret_cast<double*>(lds + L::O_SH);
        priv = lds + L::O_PRIV + wave * L::PRIV;
        zimg = priv + L::R_Z * XS;
        xLimg = priv + L::R_XL * XS;
        dpimg = priv + L::R_DP * XS;
        dptile = dpimg;
        tr1 = wave / HT, tc1 = wave - tr1 * HT;
        tr0 = wave / HT0, tc0 = wave - tr0 * HT0;
        w0i = simg + PK::I_W0 + lane * 4;
        w1i = simg + PK::I_W1 + lane * 4;
        w1ti = simg + PK::I_W1T + lane * 4;
        w0ti = simg + PK::I_W0T + (wave * (KH / 4) * 64 + lane) * 4;
        woTw = simg + PK::I_WOT + wave * NTILE * HT * 256;
        boLw = simg + PK::I_BOL + wave * NTILE * 16;
        b0i = simg + PK::I_B0 + g * 4;
        b1i = simg + PK::I_B1 + g * 4;
    }

    // weights: the wave's Wo rows -> registers (from the per-lane image), operand images -> LDS (visible after the next barrier)
    __device__ __forceinline__ void load_weights(const float* WP, float (&wo)[NB][CQ][KH]) const {
        const float* wp = WP + (long long)wave * PK::WAVE + lane * 4;
        float wreg[PK::LANE4 * 4];
#pragma unroll
        for (int i4 = 0; i4 < PK::LANE4; ++i4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(wp + i4 * 256);
#pragma unroll
            for (int q = 0; q < 4; ++q) wreg[4 * i4 + q] = v[q];
        }
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int cq = 0; cq < CQ; ++cq)
#pragma unroll
                for (int ks = 0; ks < KH; ++ks) wo[nb][cq][ks] = wreg[PK::O_WO + (nb * CQ + cq) * KH + ks];
        const f32x4* src = reinterpret_cast<const f32x4*>(WP + (long long)NW * PK::WAVE);
        f32x4* dst = reinterpret_cast<f32x4*>(simg);
        constexpr int NV = PK::IMGS / 4;
        int e = tid;
        for (; e + 7 * NT < NV; e += 8 * NT) {      // eight 16-byte loads in flight per thread
            f32x4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = src[e + u * NT];
#pragma unroll
            for (int u = 0; u < 8; ++u) dst[e + u * NT] = v[u];
        }
        for (; e < NV; e += NT) dst[e] = src[e];
    }

    // dX/dt (and d2X/dt2) of a stage: loaded into registers early, stored to a parity slot before the stage's last barrier
    __device__ __forceinline__ void stage_load(const KArgs& a, const StageDesc sd, bool cubic, int b0, float (&dxv)[EPT], float (&d2v)[EPT]) const {
#pragma unroll
        for (int q = 0; q < EPT; ++q) {
            const int e = tid + q * NT;
            const int es = e / CP, cc = e - es * CP;
            float v = 0.0f, v2 = 0.0f;
            if (e < 16 * CP && cc < a.C && b0 + es < a.B) dp_control_derivative<true>(a, sd, !cubic, b0 + es, cc, v, v2);
            dxv[q] = v;
            d2v[q] = v2;
        }
    }
    __device__ __forceinline__ void stage_store(int slot, const float (&dxv)[EPT], const float (&d2v)[EPT]) const {
#pragma unroll
        for (int q = 0; q < EPT; ++q) {
            const int e = tid + q * NT;
            if (e < 16 * CP) {
                dxs[(slot & 1) * 16 * CP + e] = dxv[q];
                d2s[(slot & 1) * 16 * CP + e] = d2v[q];
            }
        }
    }
    // owned stage inputs -> the layer-0 B operand of every wave (publishes the dX slot stored before it, too)
    __device__ __forceinline__ void exchange(int& zpar, const float (&ys)[NB], float (&zreg)[HB]) const {
        float* zw = zx + zpar * H * 16;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) zw[(4 * (wave * NB + nb) + g) * 16 + s] = ys[nb];
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < HB; ++ks) zreg[ks] = zw[(4 * ks + g) * 16 + s];
        zpar ^= 1;
    }

    // One stage evaluation at the stage input in zreg, with dX/dt in parity slot `dslot`: kout = f dX/dt for the owned entries and
    // vt = as_^T (d/dt of f dX/dt) per lane; with VJP also vy = as_^T df/dy for them and G += as_^T df/dtheta.
    template <bool VJP, class Grad>
    __device__ __forceinline__ void eval(int dslot, const float (&wo)[NB][CQ][KH], const float (&zreg)[HB], const float (&as_)[NB], Grad& G,
                                         float (&kout)[NB], f32x4& vy, float& vt) const {
        const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
        const float* dxp = dxs + (dslot & 1) * 16 * CP + s * CP;
        const float* d2p = d2s + (dslot & 1) * 16 * CP + s * CP;
        // ---- forward recompute; keep x_1..x_NL (registers) and the image rows the weight-gradient tiles read (LDS) -----------------------
        float xc[KH];               // the layer just computed (x_NL after the loop)
        unsigned relu_mask = 0;     // bit (8 l + ks): x_{l+1}[4 ks + g] > 0, for the layers below the last
        {
            f32x4 acc[HT];
#pragma unroll
            for (int tt = 0; tt < HT; ++tt) acc[tt] = *reinterpret_cast<const f32x4*>(b0i + tt * 16);
#pragma unroll
            for (int q4 = 0; q4 < HB / 4; ++q4) {
                f32x4 a4[HT];
#pragma unroll
                for (int tt = 0; tt < HT; ++tt) a4[tt] = *reinterpret_cast<const f32x4*>(w0i + (tt * (HB / 4) + q4) * 256);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int tt = 0; tt < HT; ++tt) acc[tt] = mfma16(a4[tt][i], zreg[4 * q4 + i], acc[tt]);
            }
#pragma unroll
            for (int tt = 0; tt < HT; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) xc[4 * tt + r] = relu_dev(acc[tt][r]);
#pragma unroll
            for (int l = 1; l < NL; ++l) {
                // x_l is complete: its image rows for the wave's dW1 tile, its mask bits
                if (VJP) {
#pragma unroll
                    for (int q4 = 0; q4 < KH / 4; ++q4)
                        if (q4 == tc1) {
#pragma unroll
                            for (int i = 0; i < 4; ++i) priv[((L::R_X + 16 * (l - 1)) + 4 * i + g) * XS + s] = xc[4 * q4 + i];
                        }
                }
#pragma unroll
                for (int ks = 0; ks < KH; ++ks) relu_mask |= (xc[ks] > 0.0f ? 1u : 0u) << (8 * (l - 1) + ks);
#pragma unroll
                for (int tt = 0; tt < HT; ++tt) acc[tt] = *reinterpret_cast<const f32x4*>(b1i + tt * 16);
#pragma unroll
                for (int q4 = 0; q4 < KH / 4; ++q4) {
                    f32x4 a4[HT];
#pragma unroll
                    for (int tt = 0; tt < HT; ++tt) a4[tt] = *reinterpret_cast<const f32x4*>(w1i + (tt * (KH / 4) + q4) * 256);
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int tt = 0; tt < HT; ++tt) acc[tt] = mfma16(a4[tt][i], xc[4 * q4 + i], acc[tt]);
                }
#pragma unroll
                for (int tt = 0; tt < HT; ++tt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) xc[4 * tt + r] = relu_dev(acc[tt][r]);
            }
        }
        f32x4 xB[HT];      // B operands of the dWo GEMM: x_NL[j = 16t + n][samples 4g..4g+3]
        if (VJP) {
#pragma unroll
            for (int q4 = 0; q4 < HB / 4; ++q4)
                if (q4 == tc0) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) zimg[(4 * i + g) * XS + s] = zreg[4 * q4 + i];
                }
#pragma unroll
            for (int ks = 0; ks < KH; ++ks) xLimg[(4 * ks + g) * XS + s] = xc[ks];
            wave_lds_order();
#pragma unroll
            for (int tt = 0; tt < HT; ++tt) xB[tt] = *reinterpret_cast<const f32x4*>(xLimg + (16 * tt + s) * XS + 4 * g);
        }
        // ---- output tiles owned by this wave --------------------------------------------------------------------------------------------
        f32x4 accJ[HT];
#pragma unroll
        for (int tt = 0; tt < HT; ++tt) accJ[tt] = zero4;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) kout[nb] = 0.0f;
        vt = 0.0f;
#pragma unroll
        for (int cq = 0; cq < CQ; ++cq) {
            f32x4 o[NB];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) o[nb] = *reinterpret_cast<const f32x4*>(boLw + ((nb * CQ + cq) * 4 + g) * 4);
#pragma unroll
            for (int ks = 0; ks < KH; ++ks)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) o[nb] = mfma16(wo[nb][cq][ks], xc[ks], o[nb]);
            const f32x4 dx = *reinterpret_cast<const f32x4*>(dxp + 4 * cq);
            const f32x4 d2 = *reinterpret_cast<const f32x4*>(d2p + 4 * cq);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int tau = nb * CQ + cq;
                f32x4 dP;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float m = tanh_prescaled(o[nb][r]);
                    kout[nb] = fmaf(m, dx[r], kout[nb]);
                    dP[r] = (as_[nb] * dx[r]) * (1.0f - m * m);
                    vt = fmaf(as_[nb] * m, d2[r], vt);
                }
                if (VJP) {
#pragma unroll
                    for (int tt = 0; tt < HT; ++tt) {      // dL/dx_L partial: k-step <-> r
                        const f32x4 av = *reinterpret_cast<const f32x4*>(woTw + ((tau * HT + tt) * 64 + lane) * 4);
#pragma unroll
                        for (int r = 0; r < 4; ++r) accJ[tt] = mfma16(av[r], dP[r], accJ[tt]);
                    }
                    {      // bias gradient: sum over the 16 samples now, kept by the lanes with s == tau
                        f32x4 sm;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            sm[r] = row16_sum(dP[r]);
                            dptile[(4 * g + r) * XS + s] = dP[r];
                        }
                        if (s == tau) G.add_bo(sm);
                    }
                    wave_lds_order();
                    const f32x4 av = *reinterpret_cast<const f32x4*>(dptile + s * XS + 4 * g);
                    wave_lds_order();
                    G.add_wo(tau, av, xB);
                }
            }
        }
        vy = zero4;      // a^T df/dy for the state entries this wave owns
        if (!VJP) return;
        G.add_vt(vt);
        // ---- sum the dL/dx_L partials over the waves ------------------------------------------------------------------------------------
        float gpre[KH];
#pragma unroll
        for (int tt = 0; tt < HT; ++tt)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[wave * HH * 16 + (4 * (4 * tt + r) + g) * 16 + s] = accJ[tt][r];
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < KH; ++ks) {
            float v = red[(4 * ks + g) * 16 + s];
#pragma unroll
            for (int wv = 1; wv < NW; ++wv) v += red[wv * HH * 16 + (4 * ks + g) * 16 + s];
            gpre[ks] = xc[ks] > 0.0f ? v : 0.0f;
        }
        // ---- hidden layers backward (shared W1), then W0 ----------------------------------------------------------------------------------
        auto bias_sum = [&](auto& gb) {      // unit 4 ks + g: sum over the samples, kept by the lane with s == ks
#pragma unroll
            for (int ks = 0; ks < KH; ++ks) {
                const float sm = row16_sum(gpre[ks]);
                if (s == ks) G.add_b(gb, sm);
                dpimg[(4 * ks + g) * XS + s] = gpre[ks];
            }
            wave_lds_order();
        };
        auto grad_tile = [&](auto& gw, int tr, const float* bimg) {      // the wave's 16 x 16 tile of dW: rows 16 tr.. of dL/dpre, 16 image rows
            const f32x4 av = *reinterpret_cast<const f32x4*>(dpimg + (16 * tr + s) * XS + 4 * g);
            const f32x4 bv = *reinterpret_cast<const f32x4*>(bimg + s * XS + 4 * g);
            G.add_w(gw, av, bv);
            wave_lds_order();
        };
#pragma unroll
        for (int l = NL - 1; l >= 1; --l) {
            bias_sum(G.gb1);
            grad_tile(G.gW1, tr1, priv + (L::R_X + 16 * (l - 1)) * XS);
            f32x4 acc[HT];
#pragma unroll
            for (int tt = 0; tt < HT; ++tt) acc[tt] = zero4;
#pragma unroll
            for (int q4 = 0; q4 < KH / 4; ++q4) {
                f32x4 a4[HT];
#pragma unroll
                for (int tt = 0; tt < HT; ++tt) a4[tt] = *reinterpret_cast<const f32x4*>(w1ti + (tt * (KH / 4) + q4) * 256);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int tt = 0; tt < HT; ++tt) acc[tt] = mfma16(a4[tt][i], gpre[4 * q4 + i], acc[tt]);
            }
#pragma unroll
            for (int tt = 0; tt < HT; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) gpre[4 * tt + r] = ((relu_mask >> (8 * (l - 1) + 4 * tt + r)) & 1u) ? acc[tt][r] : 0.0f;
        }
        bias_sum(G.gb0);
        grad_tile(G.gW0, tr0, zimg);
#pragma unroll
        for (int q4 = 0; q4 < KH / 4; ++q4) {
            const f32x4 a4 = *reinterpret_cast<const f32x4*>(w0ti + q4 * 256);
#pragma unroll
            for (int i = 0; i < 4; ++i) vy = mfma16(a4[i], gpre[4 * q4 + i], vy);
        }
    }

    // dW1 / dW0 / db1 / db0 of this workgroup -> its partial `gp` in parameter order (the lane with s == ks holds the bias sums of unit
    // 4 ks + g); dWo / dbo are written by the kernels, each in its own order
    __device__ __forceinline__ void store_hidden_grads(const KArgs& a, float* gp, const f32x4& gW1, const f32x4& gW0, float gb1, float gb0) const {
        const int Hr = a.H, HHr = a.dout[0];
        if (NL > 1) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (16 * tr1 + 4 * g + r < HHr && 16 * tc1 + s < HHr) gp[a.gW_off[1] + (16 * tr1 + 4 * g + r) * HHr + 16 * tc1 + s] = gW1[r];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (16 * tr0 + 4 * g + r < HHr && 16 * tc0 + s < Hr) gp[a.gW_off[0] + (16 * tr0 + 4 * g + r) * Hr + 16 * tc0 + s] = gW0[r];
        if (wave == 0 && s < KH && 4 * s + g < HHr) {
            if (NL > 1) gp[a.gb_off[1] + 4 * s + g] = gb1;
            gp[a.gb_off[0] + 4 * s + g] = gb0;
        }
    }
};
