// Control-path coefficient construction on the GPU (the step immediately before the
// hot path).  HBM-bound per-series scans: one thread per (sample, channel) series, adjacent threads = adjacent
// channels so every time step is a coalesced row access.  Reference semantics restated (relative to
// /root/reference/modules/torchcde/torchcde):
//   forward fill + rectilinear interleave     interpolation_linear.py:85-128, misc.py:103-126
//   NaN fill of the linear knots              interpolation_linear.py:13-82, 131-180
//   natural cubic coefficients                interpolation_cubic.py:7-53 (tridiagonal solve: misc.py:13-67)
//   causal fills, linear / rectilinear hybrid  interpolation_linear.py:159-173, misc.py:103-126, src/ncde/interpolation.py:191-253
// All on the default integer time grid, fp32, operation order of the reference (build uses -ffp-contract=off).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "ncde_hip.h"
#include "ncde_host.h"

namespace {

// linear knots with missing values: leading gap <- first observation, trailing gap <- last observation,
// interior gaps <- linear interpolation between the neighbours, all-NaN series <- 0.
// rect >= 0: rectilinear preparation first (forward fill, every row twice, time channel advanced one slot).
// One series (one sample, one channel); xs / os are strided views (global memory or an LDS copy).
// mode 0: linear knots, NaN filled (L rows out);  1: rectilinear value channel (2L-1 rows out);  2: rectilinear time channel
// tg: the user time grid the observations sit on (interpolation_linear.py:131-180 with t=...), NULL = the integer grid; it only
// enters the ratio of the interior-gap fill (the rectilinear preparation leaves no interior gap).
__device__ void linear_series(const float* xs, long long sx, float* os, long long so, int L, int mode, const float* tg = nullptr) {
    if (mode == 2) {  // time channel: t_0, t_1, t_1, t_2, t_2, ... (advanced by one slot)
        const int T = 2 * L - 1;
        for (int i = 0; i < L; ++i) {
            const float v = xs[i * sx];
            if (i > 0) os[(2 * i - 1) * so] = v;
            if (2 * i < T) os[(2 * i) * so] = v;
        }
        return;
    }
    if (mode == 1) {  // forward fill; a leading gap takes the first observation (0 if there is none)
        const int T = 2 * L - 1;
        float first = 0.0f;
        for (int i = 0; i < L; ++i) {
            const float v = xs[i * sx];
            if (!isnan(v)) { first = v; break; }
        }
        float last = first;
        for (int i = 0; i < L; ++i) {
            const float v = xs[i * sx];
            if (!isnan(v)) last = v;
            os[(2 * i) * so] = last;
            if (2 * i + 1 < T) os[(2 * i + 1) * so] = last;
        }
        return;
    }
    int prev = -1;  // index of the last observation seen
    float prev_v = 0.0f;
    for (int i = 0; i < L; ++i) {
        const float v = xs[i * sx];
        if (isnan(v)) continue;
        if (prev < 0) {
            for (int k = 0; k < i; ++k) os[k * so] = v;
        } else {
            for (int k = prev + 1; k < i; ++k) {
                const float ratio = tg ? (tg[k] - tg[prev]) / (tg[i] - tg[prev]) : ((float)k - (float)prev) / ((float)i - (float)prev);
                os[k * so] = prev_v + ratio * (v - prev_v);
            }
        }
        os[i * so] = v;
        prev = i;
        prev_v = v;
    }
    if (prev < 0) {
        for (int k = 0; k < L; ++k) os[k * so] = 0.0f;
    } else {
        for (int k = prev + 1; k < L; ++k) os[k * so] = prev_v;
    }
}

// v1: one thread per series straight on global memory (any size; coalescing limited to C*4-byte runs)
__global__ __launch_bounds__(256) void ncde_linear_coeffs_kernel(const float* __restrict__ x, int B, int L, int C, int rect,
                                                                  float* __restrict__ out, const float* __restrict__ tg) {
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (tid >= (long long)B * C) return;
    const int b = (int)(tid / C), c = (int)(tid - (long long)b * C);
    const int T = rect >= 0 ? 2 * L - 1 : L;
    linear_series(x + (long long)b * L * C + c, C, out + (long long)b * T * C + c, C, L, rect < 0 ? 0 : (c == rect ? 2 : 1), tg);
}

// v2: one workgroup per sample, the whole [L][C] series staged in LDS: fully coalesced loads and stores, and the
// per-channel fills as WAVE SCANS along time (lane <-> time step): index of the last observation at or before i
// (inclusive prefix max) and of the next one at or after i (suffix min), 64 time steps per scan, carried across chunks.
// The arithmetic per element is exactly linear_series()'s, so the result is bit-identical to v1.
__device__ __forceinline__ int wave_prefix_max(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d, 64);
        if (lane >= d) v = max(v, o);
    }
    return v;
}
__device__ __forceinline__ int wave_suffix_min(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_down(v, d, 64);
        if (lane + d < 64) v = min(v, o);
    }
    return v;
}

__global__ __launch_bounds__(256) void ncde_linear_coeffs_lds_kernel(const float* __restrict__ x, int B, int L, int C, int rect,
                                                                     float* __restrict__ out, const float* __restrict__ tg) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int T = rect >= 0 ? 2 * L - 1 : L;
    float* xin = sm;                                   // [L][C] raw
    int* prv = reinterpret_cast<int*>(sm + L * C);     // [L][C] index of the last observation <= i (-1: none)
    int* nxt = prv + L * C;                            // [L][C] index of the next observation >= i (L: none)   (linear fill only)
    const float* src = x + (long long)b * L * C;
    if (((L * C) & 3) == 0 && ((((long long)b * L * C) & 3) == 0)) {
        for (int e = tid; e < (L * C) >> 2; e += 256) reinterpret_cast<float4*>(xin)[e] = reinterpret_cast<const float4*>(src)[e];
    } else {
        for (int e = tid; e < L * C; e += 256) xin[e] = src[e];
    }
    __syncthreads();
    // scans along time, thread <-> (time chunk k, channel c): a short serial pass over the chunk, then the carry from the
    // nearest earlier (later) chunk that holds an observation
    {
        const int nch = C <= 256 ? (256 / C < 64 ? 256 / C : 64) : 1;       // chunks per channel
        const int cl = (L + nch - 1) / nch;                                 // time steps per chunk
        int* car = nxt + (rect < 0 ? L * C : 0);                            // [nch][C] chunk summaries (behind the index arrays)
        const int k = tid / C, c = tid - k * C;
        const bool act = C <= 256 && k < nch;
        const int i0 = k * cl, i1 = min(L, i0 + cl);
        for (int cc = act ? c : C; cc < C; cc += 256) {
            int last = -1;
            for (int i = i0; i < i1; ++i) {
                if (!isnan(xin[i * C + cc])) last = i;
                prv[i * C + cc] = last;
            }
            car[k * C + cc] = last;
        }
        __syncthreads();
        for (int cc = act ? c : C; cc < C; cc += 256) {
            int cin = -1;
            for (int kk = k - 1; kk >= 0 && cin < 0; --kk) cin = car[kk * C + cc];
            for (int i = i0; i < i1 && prv[i * C + cc] < 0; ++i) prv[i * C + cc] = cin;
        }
        if (rect < 0) {
            __syncthreads();
            for (int cc = act ? c : C; cc < C; cc += 256) {
                int next = L;
                for (int i = i1 - 1; i >= i0; --i) {
                    if (!isnan(xin[i * C + cc])) next = i;
                    nxt[i * C + cc] = next;
                }
                car[k * C + cc] = next;
            }
            __syncthreads();
            for (int cc = act ? c : C; cc < C; cc += 256) {
                int cin = L;
                for (int kk = k + 1; kk < nch && cin >= L; ++kk) cin = car[kk * C + cc];
                for (int i = i1 - 1; i >= i0 && nxt[i * C + cc] >= L; --i) nxt[i * C + cc] = cin;
            }
        }
    }
    __syncthreads();
    float* dst = out + (long long)b * T * C;
    // output: thread <-> (row offset, channel), rows strided by the rows one pass covers: no division in the loops,
    // consecutive threads write consecutive addresses
    const int rp = 256 / C > 0 ? 256 / C : 1;
    const int r0 = tid / C, c = tid - r0 * C;
    const bool active = C <= 256 ? r0 < rp : true;
    if (rect >= 0 && (C & 3) == 0 && C <= 1024 && ((((long long)b * T * C) & 3) == 0)) {
        // 16-byte stores: thread <-> (row offset, channel quad)
        const int CQ = C >> 2, rp4 = 256 / CQ > 0 ? 256 / CQ : 1;
        const int q0 = tid / CQ, cq = tid - q0 * CQ;
        if (q0 < rp4) {
            int first[4] = {-2, -2, -2, -2};
            for (int t = q0; t < T; t += rp4) {
                float4 v4;
                float* vv = reinterpret_cast<float*>(&v4);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int cc = 4 * cq + u;
                    if (cc == rect) {
                        vv[u] = xin[((t + 1) >> 1) * C + cc];
                    } else {
                        int p = prv[(t >> 1) * C + cc];
                        if (p < 0) {
                            if (first[u] == -2) {
                                first[u] = -1;
                                if (prv[(L - 1) * C + cc] >= 0) {
                                    int lo = 0, hi = L - 1;
                                    while (lo < hi) {
                                        const int mid = (lo + hi) >> 1;
                                        if (prv[mid * C + cc] >= 0) hi = mid; else lo = mid + 1;
                                    }
                                    first[u] = lo;
                                }
                            }
                            p = first[u];
                        }
                        vv[u] = p >= 0 ? xin[p * C + cc] : 0.0f;
                    }
                }
                *reinterpret_cast<float4*>(dst + t * C + 4 * cq) = v4;
            }
        }
    } else if (rect >= 0) {
        // value channels = forward fill of row t/2 (leading gap: the first observation, 0 if none);
        // time channel advanced by one slot: row (t+1)/2
        int first = -2;                                 // first observation of this channel, found lazily (-1: none)
        for (int cc = c; cc < C && active; cc += 256) {
            for (int t = r0; t < T; t += rp) {
                float v;
                if (cc == rect) {
                    v = xin[((t + 1) >> 1) * C + cc];
                } else {
                    int p = prv[(t >> 1) * C + cc];
                    if (p < 0) {
                        if (first == -2) {              // smallest j with prv[j] >= 0 (prv is monotone in j)
                            first = -1;
                            if (prv[(L - 1) * C + cc] >= 0) {
                                int lo = 0, hi = L - 1;
                                while (lo < hi) {
                                    const int mid = (lo + hi) >> 1;
                                    if (prv[mid * C + cc] >= 0) hi = mid; else lo = mid + 1;
                                }
                                first = lo;
                            }
                        }
                        p = first;
                    }
                    v = p >= 0 ? xin[p * C + cc] : 0.0f;
                }
                dst[t * C + cc] = v;
            }
            first = -2;
        }
    } else {
        for (int cc = c; cc < C && active; cc += 256) {
            for (int i = r0; i < L; i += rp) {
                const int e = i * C + cc;
                const int p = prv[e], q = nxt[e];
                float v;
                if (p == i) v = xin[e];
                else if (p < 0) v = q < L ? xin[q * C + cc] : 0.0f;                // leading gap / no observation
                else if (q >= L) v = xin[p * C + cc];                              // trailing gap
                else {
                    const float pv = xin[p * C + cc], qv = xin[q * C + cc];
                    const float ratio = tg ? (tg[i] - tg[p]) / (tg[q] - tg[p]) : ((float)i - (float)p) / ((float)q - (float)p);
                    v = pv + ratio * (qv - pv);
                }
                dst[e] = v;
            }
        }
    }
}

// natural cubic spline on the integer grid.  out[b][p][4C] = a | b | 2c | 3d of piece p.
// ws[b][i][c] keeps the forward-swept right-hand side; the swept diagonal depends on i only (recomputed).
// Series with missing values (interpolation_cubic.py:77-165): ends filled from the first / last observation, spline
// through the observed knots only (non-uniform spacing, so the swept diagonal is per series: wd), then every unit
// interval [time, time+1) gets the piece that covers it, re-expanded around `time` (offset = t_knot - time).
// tg: user time grid (interpolation_cubic.py:56-165 with t=...), NULL = integer grid: knot spacing and the re-expansion offsets.
__device__ void cubic_series_missing(const float* xs, float* os, float* wb, float* wd, int L, int C, int first, int last,
                                     const float* tg = nullptr) {
    const long long sC = C;
    auto val = [&](int i) { return i < first ? xs[first * sC] : (i > last ? xs[last * sC] : xs[i * sC]); };
    // forward sweep over the knots: knot p is processed when the next knot q is known (r_p = 1/(t_q - t_p))
    int pp = -1, p = 0;                 // index 0 is always a knot after the fill
    float xp = val(0), r_prev = 0.0f, scaled_prev = 0.0f, nd_prev = 0.0f, nb_prev = 0.0f;
    for (int q = 1; q < L; ++q) {
        const float xq = val(q);
        if (isnan(xq)) continue;
        const float td = tg ? tg[q] - tg[p] : (float)q - (float)p;
        const float r = 1.0f / td, r2 = r * r;
        const float three = 3.0f * (xq - xp);
        const float scaled = three * r2;
        float diag, rhs;
        if (pp < 0) { diag = r * 2.0f; rhs = scaled; }
        else { diag = (r + r_prev) * 2.0f; rhs = scaled + scaled_prev; }
        float nd, nb;
        if (pp < 0) { nd = diag; nb = rhs; }
        else {
            const float w = r_prev / nd_prev;
            nd = diag - w * r_prev;
            nb = rhs - w * nb_prev;
        }
        wd[p * sC] = nd;
        wb[p * sC] = nb;
        pp = p; p = q; xp = xq; r_prev = r; scaled_prev = scaled; nd_prev = nd; nb_prev = nb;
    }
    if (pp == 0) {      // exactly one interval swept (pp is the left knot of the last one; a second interval makes it > 0)
        // two knots only (the filled ends; nothing observed in between): the reference's length-2 branch (interpolation_cubic.py:16-20),
        // the straight line b = dx / dt with 2c = 3d = 0 EXACTLY -- the three-point sweep below on two knots gives the same line up to
        // rounding only (b off by an ulp, 2c / 3d a residue).  Re-expanded around every grid point like any other piece.
        const float td = tg ? tg[L - 1] - tg[0] : (float)(L - 1) - 0.0f;
        const float x0 = val(0), b_k = (val(L - 1) - x0) / td;
        for (int time = 0; time < L - 1; ++time) {
            const float off = tg ? tg[0] - tg[time] : 0.0f - (float)time;
            float* o = os + (long long)time * 4 * C;
            o[0] = x0 + (0.0f - b_k) * off;
            o[C] = b_k;
            o[2 * C] = 0.0f;
            o[3 * C] = 0.0f;
        }
        return;
    }
    // last knot (index L-1): diag = (0 + r_prev) * 2, rhs = 0 + scaled_prev
    float kd_next;
    {
        const float diag = (0.0f + r_prev) * 2.0f, rhs = 0.0f + scaled_prev;
        const float w = r_prev / nd_prev;
        const float nd = diag - w * r_prev, nb = rhs - w * nb_prev;
        kd_next = nb / nd;
    }
    // back substitution, coefficients per knot interval, expansion onto the unit intervals (right to left)
    int q = L - 1;
    float xq = val(q);
    for (int i = L - 2; i >= 0; --i) {
        const float xi = val(i);
        if (isnan(xi)) continue;
        const float td = tg ? tg[q] - tg[i] : (float)q - (float)i;
        const float r = 1.0f / td, r2 = r * r;
        const float kd = (wb[i * sC] - r * kd_next) / wd[i * sC];
        const float three = 3.0f * (xq - xi), six = 2.0f * three;
        const float two_c = ((six * r - 4.0f * kd) - 2.0f * kd_next) * r;
        const float three_d = (-six * r + 3.0f * (kd + kd_next)) * r2;
        for (int time = q - 1; time >= i; --time) {
            const float off = tg ? tg[i] - tg[time] : (float)i - (float)time;
            const float a_in = (0.5f * two_c - three_d * off / 3.0f) * off;
            float* o = os + (long long)time * 4 * C;
            o[0] = xi + (a_in - kd) * off;
            o[C] = kd + (three_d * off - two_c) * off;
            o[2 * C] = two_c - 2.0f * three_d * off;
            o[3 * C] = three_d;
        }
        q = i; xq = xi; kd_next = kd;
    }
}

// one (sample, channel) series straight on global memory: any size, missing values included
__device__ void cubic_series_global(const float* __restrict__ x, int L, int C, float* __restrict__ out, float* __restrict__ ws,
                                    const float* __restrict__ diag_swept, float* __restrict__ ws_d, int b, int c,
                                    const float* __restrict__ tg = nullptr) {
    const float* xs = x + (long long)b * L * C + c;
    float* os = out + (long long)b * (L - 1) * 4 * C + c;
    // missing values?  (NaN anywhere in the series)
    int first = -1, last = -1, n_obs = 0;
    for (int i = 0; i < L; ++i)
        if (!isnan(xs[(long long)i * C])) {
            if (first < 0) first = i;
            last = i;
            ++n_obs;
        }
    if (n_obs == 0) {  // no observation at all: the zero path
        for (int i = 0; i < L - 1; ++i) {
            float* o = os + (long long)i * 4 * C;
            o[0] = 0.0f; o[C] = 0.0f; o[2 * C] = 0.0f; o[3 * C] = 0.0f;
        }
        return;
    }
    if (L == 2) {
        const float x0 = xs[first * (long long)C], x1 = xs[last * (long long)C];   // ends filled from the observations
        os[0] = x0;
        os[C] = tg ? (x1 - x0) / (tg[1] - tg[0]) : x1 - x0;
        os[2 * C] = 0.0f;
        os[3 * C] = 0.0f;
        return;
    }
    float* wb = ws + (long long)b * L * C + c;
    if (n_obs < L || tg) {      // a user grid is non-uniform spacing: the same sweep as for missing values (every point a knot)
        cubic_series_missing(xs, os, wb, ws_d + (long long)b * L * C + c, L, C, first, last, tg);
        return;
    }
    // rhs_i = 3 (x_i - x_{i-1}) + 3 (x_{i+1} - x_i) with unit knot spacing; Thomas forward sweep
    float x_prev = xs[0], x_cur = xs[C];
    float scaled_prev = (3.0f * (x_cur - x_prev)) * 1.0f;  // three_path_diffs * reciprocal^2
    float nb_prev = scaled_prev;                            // rhs_0
    wb[0] = nb_prev;
    for (int i = 1; i < L; ++i) {
        float rhs;
        if (i < L - 1) {
            const float x_next = xs[(long long)(i + 1) * C];
            const float scaled = (3.0f * (x_next - x_cur)) * 1.0f;
            rhs = scaled + scaled_prev;
            scaled_prev = scaled;
            x_prev = x_cur;
            x_cur = x_next;
        } else {
            rhs = 0.0f + scaled_prev;
        }
        const float w = 1.0f / diag_swept[i - 1];
        const float nb = rhs - w * nb_prev;
        wb[(long long)i * C] = nb;
        nb_prev = nb;
    }
    // back substitution and coefficients, last piece first
    float kd_next = nb_prev / diag_swept[L - 1];
    for (int i = L - 2; i >= 0; --i) {
        const float kd = (wb[(long long)i * C] - 1.0f * kd_next) / diag_swept[i];
        const float xi = xs[(long long)i * C], xi1 = xs[(long long)(i + 1) * C];
        const float six = 2.0f * (3.0f * (xi1 - xi));
        float* o = os + (long long)i * 4 * C;
        o[0] = xi;
        o[C] = kd;
        o[2 * C] = (six * 1.0f - 4.0f * kd - 2.0f * kd_next) * 1.0f;
        o[3 * C] = (-six * 1.0f + 3.0f * (kd + kd_next)) * 1.0f;
        kd_next = kd;
    }
}

__global__ __launch_bounds__(64) void ncde_cubic_coeffs_kernel(const float* __restrict__ x, int B, int L, int C,
                                                                 float* __restrict__ out, float* __restrict__ ws,
                                                                 const float* __restrict__ diag_swept, float* __restrict__ ws_d,
                                                                 const float* __restrict__ tg) {
    // one wave per workgroup: the serial recurrences are latency-bound, so many small workgroups (all CUs, many waves in
    // flight) beat few large ones -- 32768 series at cfg4 are only 128 workgroups of 256
    const long long tid = (long long)blockIdx.x * 64 + threadIdx.x;
    if (tid >= (long long)B * C) return;
    const int b = (int)(tid / C), c = (int)(tid - (long long)b * C);
    cubic_series_global(x, L, C, out, ws, diag_swept, ws_d, b, c, tg);
}

// LDS-staged variant for complete series (no missing values): one wave = NSMP whole samples (lane <-> (sample, channel)).
//   * the samples' [L][C] blocks come in with 16-byte loads (one contiguous region per workgroup) into LDS, sample stride
//     padded so that the 64 lanes of a time step hit distinct banks;
//   * the swept diagonal d_i and 1/d_{i-1} depend on i only (constant-coefficient system on the integer grid): read from a
//     table, so the forward sweep is one multiply-subtract per step and series, its result kept in LDS (no global scratch);
//   * back substitution is the chain only (the one true division per step: bit-exactness with the reference's x / d rules
//     out a reciprocal), its result kd_i written over the swept right-hand side in LDS;
//   * the a | b | 2c | 3d rows are then an embarrassingly parallel pass over (sample, piece, section, four channels): LDS
//     reads, one 16-byte store per item, consecutive lanes on consecutive addresses.
// Arithmetic per element is exactly cubic_series_global()'s, so the output is bit-identical (golden g8).  A workgroup
// that finds a NaN among its samples falls back to cubic_series_global for all of them.
#define CUBIC_NT 256
__global__ __launch_bounds__(CUBIC_NT) void ncde_cubic_coeffs_lds_kernel(const float* __restrict__ x, int B, int L, int C, int NSMP,
                                                                     int sstride, float* __restrict__ out, float* __restrict__ ws,
                                                                     const float* __restrict__ diag_swept, float* __restrict__ ws_d) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* xs = lds;                                 // [NSMP][sstride]  (sample block [L][C] + padding)
    float* nbs = xs + (size_t)NSMP * sstride;        // [NSMP][sstride]  forward-swept right-hand side
    float* dtab = nbs + (size_t)NSMP * sstride;      // [L] swept diagonal d_i
    float* wtab = dtab + ((L + 3) & ~3);             // [L] 1 / d_{i-1}
    const int lane = threadIdx.x;      // all CUBIC_NT threads stage and emit; the first 64 (one wave) run the chains
    const int b0 = blockIdx.x * NSMP;
    const int nsmp = min(NSMP, B - b0);
    const int LC = L * C;
    // ---- stage the samples (contiguous region of nsmp * L * C floats), detect missing values ------------------------------
    const float* src = x + (long long)b0 * LC;
    bool bad = false;
    if ((LC & 3) == 0 && (((uintptr_t)src) & 15) == 0) {
        const int nv = LC >> 2, tot = nsmp * nv;
        int e = lane;
        for (; e + 3 * CUBIC_NT < tot; e += 4 * CUBIC_NT) {      // four 16-byte loads in flight per lane
            float4 v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const float4*>(src + 4LL * (e + CUBIC_NT * q));
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ee = e + CUBIC_NT * q, sm = ee / nv, k = ee - sm * nv;
                bad = bad || isnan(v[q].x) || isnan(v[q].y) || isnan(v[q].z) || isnan(v[q].w);
                *reinterpret_cast<float4*>(xs + (size_t)sm * sstride + 4 * k) = v[q];
            }
        }
        for (; e < tot; e += CUBIC_NT) {
            const int sm = e / nv, k = e - sm * nv;
            const float4 v = *reinterpret_cast<const float4*>(src + 4LL * e);
            bad = bad || isnan(v.x) || isnan(v.y) || isnan(v.z) || isnan(v.w);
            *reinterpret_cast<float4*>(xs + (size_t)sm * sstride + 4 * k) = v;
        }
    } else {
        for (int e = lane; e < nsmp * LC; e += CUBIC_NT) {
            const int sm = e / LC, k = e - sm * LC;
            const float v = src[e];
            bad = bad || isnan(v);
            xs[(size_t)sm * sstride + k] = v;
        }
    }
    for (int i = lane; i < L; i += CUBIC_NT) {
        dtab[i] = diag_swept[i];
        wtab[i] = i > 0 ? 1.0f / diag_swept[i - 1] : 0.0f;      // the same division cubic_series_global does per step
    }
    if (__syncthreads_or(bad)) {      // missing values somewhere in this workgroup: the general per-series path
        for (int e = lane; e < nsmp * C; e += CUBIC_NT) cubic_series_global(x, L, C, out, ws, diag_swept, ws_d, b0 + e / C, e % C);
        return;
    }
    const int sm = lane / C, c = lane - sm * C;
    const bool live = sm < nsmp && lane < 64;
    const float* xl = xs + (size_t)(live ? sm : 0) * sstride + c;
    float* nl = nbs + (size_t)(live ? sm : 0) * sstride + c;
    if (L == 2) {
        if (live) {
            float* os = out + (long long)(b0 + sm) * (L - 1) * 4 * C + c;
            os[0] = xl[0]; os[C] = xl[C] - xl[0]; os[2 * C] = 0.0f; os[3 * C] = 0.0f;
        }
        return;
    }
    // The two recurrences are latency chains (forward: multiply-subtract; backward: subtract + true division, ~60 cycles), so
    // everything that is NOT on the chain -- LDS reads, the right-hand side, the coefficient rows -- is done for a block of
    // CUBIC_BLK steps at a time around a register-only chain.
    constexpr int BLK = 8;
    // ---- forward sweep (same operation order as cubic_series_global) --------------------------------------------------------
    // full blocks are branch-free (guards inside an unrolled block turn every load into its own branch + wait); the tail
    // runs step by step
    if (lane < 64) {
        float x_cur = xl[C];
        float scaled_prev = (3.0f * (x_cur - xl[0])) * 1.0f;
        float nb_prev = scaled_prev;
        nl[0] = nb_prev;
        int i0 = 1;
        for (; i0 + BLK <= L - 1; i0 += BLK) {      // steps i0 .. i0+BLK-1, all < L-1
            float xn[BLK], wv[BLK], rhs[BLK], nbv[BLK];
#pragma unroll
            for (int k = 0; k < BLK; ++k) {
                xn[k] = xl[(i0 + k + 1) * C];
                wv[k] = wtab[i0 + k];               // 1 / d_{i-1}
            }
#pragma unroll
            for (int k = 0; k < BLK; ++k) {
                const float scaled = (3.0f * (xn[k] - x_cur)) * 1.0f;
                rhs[k] = scaled + scaled_prev;
                scaled_prev = scaled;
                x_cur = xn[k];
            }
#pragma unroll
            for (int k = 0; k < BLK; ++k) {
                nbv[k] = rhs[k] - wv[k] * nb_prev;
                nb_prev = nbv[k];
            }
#pragma unroll
            for (int k = 0; k < BLK; ++k) nl[(i0 + k) * C] = nbv[k];
        }
        for (int i = i0; i < L; ++i) {
            float rhs;
            if (i < L - 1) {
                const float x_next = xl[(i + 1) * C];
                const float scaled = (3.0f * (x_next - x_cur)) * 1.0f;
                rhs = scaled + scaled_prev;
                scaled_prev = scaled;
                x_cur = x_next;
            } else {
                rhs = 0.0f + scaled_prev;
            }
            const float nb = rhs - wtab[i] * nb_prev;
            nl[i * C] = nb;
            nb_prev = nb;
        }
    }
    // ---- back substitution: the chain only; kd_i overwrites the swept right-hand side in place --------------------------------
    if (lane < 64) {
        float kd_next = nl[(L - 1) * C] / dtab[L - 1];
        nl[(L - 1) * C] = kd_next;
        int ib = L - 2;
        for (; ib - BLK + 1 >= 0; ib -= BLK) {      // pieces ib .. ib-BLK+1
            float nbv[BLK], dv[BLK], kdv[BLK + 1];
#pragma unroll
            for (int k = 0; k < BLK; ++k) {
                nbv[k] = nl[(ib - k) * C];
                dv[k] = dtab[ib - k];
            }
            kdv[0] = kd_next;
#pragma unroll
            for (int k = 0; k < BLK; ++k) kdv[k + 1] = (nbv[k] - 1.0f * kdv[k]) / dv[k];      // the chain: one true division per step
#pragma unroll
            for (int k = 0; k < BLK; ++k) nl[(ib - k) * C] = kdv[k + 1];
            kd_next = kdv[BLK];
        }
        for (int i = ib; i >= 0; --i) {
            const float kd = (nl[i * C] - 1.0f * kd_next) / dtab[i];
            nl[i * C] = kd;
            kd_next = kd;
        }
    }
    __syncthreads();
    // ---- coefficient rows a | b | 2c | 3d: embarrassingly parallel over (sample, piece, section, channels) -----------------------
    // out[b][p][4C]; one item = one 16-byte store (four channels of one section) when C % 4 == 0, else one float
    const int C4 = 4 * C;
    if ((C & 3) == 0 && ((uintptr_t)out & 15) == 0) {
        const int cq = C >> 2, per_row = 4 * cq, per_smp = (L - 1) * per_row;
        for (int e = lane; e < nsmp * per_smp; e += CUBIC_NT) {
            const int s2 = e / per_smp, r = e - s2 * per_smp;
            const int pp = r / per_row, q4 = r - pp * per_row;
            const int part = q4 / cq, q = q4 - part * cq;
            const float* xa = xs + (size_t)s2 * sstride + pp * C + 4 * q;
            const float* ka = nbs + (size_t)s2 * sstride + pp * C + 4 * q;
            const float4 xi = *reinterpret_cast<const float4*>(xa), xi1 = *reinterpret_cast<const float4*>(xa + C);
            const float4 kd = *reinterpret_cast<const float4*>(ka), kn = *reinterpret_cast<const float4*>(ka + C);
            float4 v;
            if (part == 0) v = xi;
            else if (part == 1) v = kd;
            else {
                const float xv[4] = {xi.x, xi.y, xi.z, xi.w}, x1[4] = {xi1.x, xi1.y, xi1.z, xi1.w};
                const float kv[4] = {kd.x, kd.y, kd.z, kd.w}, k1[4] = {kn.x, kn.y, kn.z, kn.w};
                float o[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float six = 2.0f * (3.0f * (x1[t] - xv[t]));
                    o[t] = part == 2 ? (six * 1.0f - 4.0f * kv[t] - 2.0f * k1[t]) * 1.0f : (-six * 1.0f + 3.0f * (kv[t] + k1[t])) * 1.0f;
                }
                v = make_float4(o[0], o[1], o[2], o[3]);
            }
            *reinterpret_cast<float4*>(out + ((long long)(b0 + s2) * (L - 1) + pp) * C4 + part * C + 4 * q) = v;
        }
    } else {
        const int per_smp = (L - 1) * C4;
        for (int e = lane; e < nsmp * per_smp; e += CUBIC_NT) {
            const int s2 = e / per_smp, r = e - s2 * per_smp;
            const int pp = r / C4, q4 = r - pp * C4;
            const int part = q4 / C, c2 = q4 - part * C;
            const float xi = xs[(size_t)s2 * sstride + pp * C + c2], xi1 = xs[(size_t)s2 * sstride + (pp + 1) * C + c2];
            const float kd = nbs[(size_t)s2 * sstride + pp * C + c2], kn = nbs[(size_t)s2 * sstride + (pp + 1) * C + c2];
            const float six = 2.0f * (3.0f * (xi1 - xi));
            float v = xi;
            if (part == 1) v = kd;
            else if (part == 2) v = (six * 1.0f - 4.0f * kd - 2.0f * kn) * 1.0f;
            else if (part == 3) v = (-six * 1.0f + 3.0f * (kd + kn)) * 1.0f;
            out[((long long)(b0 + s2) * (L - 1) + pp) * C4 + q4] = v;
        }
    }
}

// swept diagonal of the natural-spline system on the unit grid: d_0 = 2, d_i = diag_i - (1/d_{i-1}) * 1
// (one wave; the interior iteration d <- 4 - 1/d reaches its fp32 fixed point after a handful of steps, after which every
// lane fills its share of the table: the serial part is ~10 steps, not L)
__global__ void ncde_cubic_diag_kernel(int L, float* diag_swept) {
    if (blockIdx.x != 0) return;
    auto next = [](float d_prev, int i, int L_) {
        float diag = (i < L_ - 1 ? 1.0f : 0.0f) + (i > 0 ? 1.0f : 0.0f);
        diag *= 2.0f;
        if (i == 0) return diag;
        const float w = 1.0f / d_prev;
        return diag - w * 1.0f;
    };
    float d_prev = 0.0f;
    int i = 0;
    for (; i < L; ++i) {                       // every lane runs the same serial prefix (uniform)
        const float d = next(d_prev, i, L);
        if (threadIdx.x == 0) diag_swept[i] = d;
        const bool fixed = i > 0 && i < L - 2 && d == d_prev;
        d_prev = d;
        if (fixed) { ++i; break; }
    }
    // interior entries i .. L-2 all equal the fixed point; the last one sees diag = 2
    for (int k = i + (int)threadIdx.x; k < L - 1; k += (int)blockDim.x) diag_swept[k] = d_prev;
    if (threadIdx.x == 0 && i < L) diag_swept[L - 1] = next(d_prev, L - 1, L);
}


// Smoothed-linear control path on its refined knot grid (src/ncde/interpolation.py:151-191: the matching polynomial after every
// interior knot k, built from rows k-1, k, k+1 of the linear coefficients, in the reference's operation order; fp32, no contraction).
// One thread per (sample, piece, channel).  Piece 0 is linear; eps < 1: piece 1 + 2(k-1) is the matching piece of knot k on
// [k, k+eps], the next one the linear remainder on [k+eps, k+1]; eps == 1: piece k is the matching piece of knot k.
struct SmoothScal { float eps, inv_e2, inv_3e2, inv_e3, four_eps, inv_2e3, e2, neg_inv_10e2; };
__global__ __launch_bounds__(256) void ncde_smooth_coeffs_kernel(const float* __restrict__ x, int B, int T, int C, int P, int order, bool split,
                                                                 SmoothScal k, float* __restrict__ out) {
    const int W = order == 3 ? 4 : 6;
    const long long total = (long long)B * P * C;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int c = (int)(e % C), p = (int)((e / C) % P), b = (int)(e / ((long long)C * P));
        const int kn = p == 0 ? 0 : (split ? 1 + ((p - 1) >> 1) : p);
        const bool match = p > 0 && (!split || ((p - 1) & 1) == 0);
        const float* xr = x + ((long long)b * T + kn) * C + c;
        const float xk = xr[0], xn = xr[C];
        float v[6] = {xk, xn - xk, 0.0f, 0.0f, 0.0f, 0.0f};
        if (p > 0) {
            const float xp = xr[-C];
            const float x_eps = xk + k.eps * (xn - xk);
            const float d_prev = xk - xp, d_next = xn - xk;
            if (!match) {
                v[0] = x_eps;
            } else if (order == 3) {
                const float Bq = k.inv_e2 * (3.0f * (x_eps - d_prev * k.eps - xk) - k.eps * (d_next - d_prev));
                const float Aq = k.inv_3e2 * (d_next - d_prev - 2.0f * Bq * k.eps);
                v[1] = d_prev; v[2] = 2.0f * Bq; v[3] = 3.0f * Aq;
            } else {
                const float Cq = k.inv_e3 * (10.0f * (x_eps - d_prev * k.eps - xk) - k.four_eps * (d_next - d_prev));
                const float Bq = k.inv_2e3 * (2.0f * (d_next - d_prev) - 3.0f * Cq * k.e2);
                const float Aq = k.neg_inv_10e2 * (6.0f * Bq * k.eps + 3.0f * Cq);
                v[1] = d_prev; v[3] = 3.0f * Cq; v[4] = 4.0f * Bq; v[5] = 5.0f * Aq;
            }
        }
        float* o = out + ((long long)b * P + p) * (W * C) + c;
        for (int q = 0; q < W; ++q) o[q * C] = v[q];
    }
}

// Transpose of the cubic builder above: dL/d(rows) [B, P, 4C] -> dL/dx [B, T, C].  In exact arithmetic the rows are linear in x with
// weights that depend on eps only (jump_k = x[k+1] - 2 x[k] + x[k-1]):
//   piece 0            a = x[0]                        b = x[1] - x[0]
//   matching piece M(k) a = x[k]                        b = x[k] - x[k-1]      2c = (4 / eps) jump_k      3d = (-3 / eps^2) jump_k
//   linear rest  R(k)  a = x[k] + eps (x[k+1] - x[k])  b = x[k+1] - x[k]      (eps < 1 only)
// Gather form: one thread per (sample, knot t, channel) sums what the pieces that read x[t] hand back, in ascending piece order --
// piece 0 (t <= 1), M(t-1), R(t-1), M(t), R(t), M(t+1): at most 5 pieces (3 for eps == 1).  Plain loads and one store per element,
// no atomics, no workspace: bit-reproducible, and grad_x is written completely.
struct SmoothBwdScal { float w2, w3, eps, one_m_eps; };
__global__ __launch_bounds__(256) void ncde_smooth_coeffs_bwd_kernel(const float* __restrict__ g, int B, int T, int C, int P, bool split,
                                                                     SmoothBwdScal k, float* __restrict__ gx) {
    const long long total = (long long)B * T * C, row = 4LL * C;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int c = (int)(e % C), t = (int)((e / C) % T), b = (int)(e / ((long long)C * T));
        const float* gs = g + (long long)b * P * row + c;
        auto piece = [&](int kn) { return gs + (long long)(split ? 1 + 2 * (kn - 1) : kn) * row; };      // M(kn); R(kn) is the next row
        auto interior = [&](int kn) { return kn >= 1 && kn <= T - 2; };
        float acc = 0.0f;
        if (t <= 1) acc = t == 0 ? gs[0] - gs[C] : gs[C];
        if (interior(t - 1)) {                 // x[t] is the knot after: it enters the jump, and the rest piece's end
            const float* r = piece(t - 1);
            acc += k.w2 * r[2 * C] + k.w3 * r[3 * C];
            if (split) acc += k.eps * r[row] + r[row + C];
        }
        if (interior(t)) {                     // x[t] is the knot itself
            const float* r = piece(t);
            const float s = k.w2 * r[2 * C] + k.w3 * r[3 * C];
            acc += (r[0] + r[C]) - 2.0f * s;
            if (split) acc += k.one_m_eps * r[row] - r[row + C];
        }
        if (interior(t + 1)) {                 // x[t] is the knot before: the incoming slope and the jump
            const float* r = piece(t + 1);
            acc += (k.w2 * r[2 * C] + k.w3 * r[3 * C]) - r[C];
        }
        gx[e] = acc;
    }
}

// Hermite cubic with backward differences (include/ncde_hip.h states the formulas, which are the contract: fp32, this operation order,
// no contraction).  One thread per (sample, piece, channel), channels fastest: the three knot loads and the four stores of a wave are
// contiguous runs.  Piece i reads knots i-1, i, i+1 only; piece 0 takes its own slope for the one before it and comes out linear.
__global__ __launch_bounds__(256) void ncde_hermite_coeffs_kernel(const float* __restrict__ knots, const float* __restrict__ t, int B, int L, int C,
                                                                  float* __restrict__ out) {
    const int P = L - 1;
    const long long total = (long long)B * P * C;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int c = (int)(e % C), i = (int)((e / C) % P), b = (int)(e / ((long long)C * P));
        const float* kr = knots + ((long long)b * L + i) * C + c;
        const float xk = kr[0], xn = kr[C];
        const float h = t ? t[i + 1] - t[i] : 1.0f;
        const float d = (xn - xk) / h;
        float dprev = d;
        if (i > 0) dprev = (xk - kr[-C]) / (t ? t[i] - t[i - 1] : 1.0f);
        const float two_c = 2.0f * (3.0f * ((xn - xk) / h - dprev) - d + dprev) / h;
        const float three_d = (1.0f / (h * h)) * (d - dprev) - two_c / h;
        float* o = out + ((long long)b * P + i) * (4 * C) + c;
        o[0] = xk;
        o[C] = dprev;
        o[2 * C] = two_c;
        o[3 * C] = three_d;
    }
}

// ---- causal control paths (interpolation_linear.py:159-173, misc.py:103-126, src/ncde/interpolation.py:191-253) ----------------------
// Everything below copies values and compares them; nothing is computed, so the results carry the bits of the input.

// initial value + forward fill: one workgroup per sample, thread <-> (time chunk k, channel c) as in ncde_linear_coeffs_lds_kernel:
// a serial pass over the chunk (rows coalesced over the channels), then the leading gap of the chunk takes the last value of the
// nearest earlier chunk that holds one.  C > 256: one chunk, the threads loop over the channels (no carry).
__global__ __launch_bounds__(256) void ncde_fill_kernel(const float* __restrict__ x, int L, int C, int has_initial, float initial, int ffill,
                                                        float* out) {
    __shared__ float car_v[256];      // [nch][C] last value of the chunk
    __shared__ int car_has[256];      //          ... if it holds one
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* xs = x + (long long)b * L * C;
    float* os = out + (long long)b * L * C;
    const int nch = C <= 256 ? 256 / C : 1;
    const int cl = (L + nch - 1) / nch;
    const int k = tid / C, c = tid - k * C;
    const bool act = k < nch;
    const int i0 = min(L, k * cl), i1 = min(L, i0 + cl);
    for (int cc = act ? c : C; cc < C; cc += 256) {
        float last = 0.0f;
        int has = 0;
        for (int i = i0; i < i1; ++i) {
            float v = xs[i * C + cc];
            if (i == 0 && has_initial && isnan(v)) v = initial;
            if (ffill) {
                if (!isnan(v)) { last = v; has = 1; }
                else if (has) v = last;
            }
            os[i * C + cc] = v;
        }
        if (C <= 256) { car_v[k * C + cc] = last; car_has[k * C + cc] = has; }
    }
    __syncthreads();
    if (ffill && C <= 256 && act && k > 0) {
        int kk = k - 1;
        while (kk >= 0 && !car_has[kk * C + c]) --kk;
        if (kk >= 0) {
            const float cin = car_v[kk * C + c];
            for (int i = i0; i < i1 && isnan(os[i * C + c]); ++i) os[i * C + c] = cin;      // this thread's own stores of the first pass
        }
    }
}

__device__ __forceinline__ int wave_inclusive_sum(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// hybrid scheme, pass 1: one workgroup per sample; thread <-> row of the full table, 256 rows per chunk.  Row 0 is kept, row 2i+1
// iff t_{i+1} != t_i, row 2i+2 iff a rectilinear channel differs between i and i+1.  Exclusive prefix sum of the keep flags: wave
// scan, the four wave totals through LDS, the chunk total carried in a register.  pos[b][r] = position of row r among the kept
// rows (-1: dropped), last_row[b] = the last kept row, lengths[b] = how many are kept.  Workgroup 0 also writes the channel map
// pass 2 reads: -2 time, -1 rectilinear, n >= 0 the n-th linear channel.
__global__ __launch_bounds__(256) void ncde_hybrid_count_kernel(const float* __restrict__ xf, int L, int C, const int* __restrict__ rect_idx, int n_rect,
                                                                int* __restrict__ pos, int* __restrict__ last_row, int* __restrict__ cmap,
                                                                int* __restrict__ lengths) {
    __shared__ int wsum[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int R = 2 * L - 1;
    if (b == 0) {
        for (int c = tid; c < C; c += 256) {
            int below = 0;
            bool is_rect = false;
            for (int q = 0; q < n_rect; ++q) {
                const int rc = rect_idx[q];
                is_rect = is_rect || rc == c;
                below += (rc > 0 && rc < c) ? 1 : 0;
            }
            cmap[c] = c == 0 ? -2 : (is_rect ? -1 : c - 1 - below);
        }
    }
    const float* xs = xf + (long long)b * L * C;
    int* ps = pos + (long long)b * R;
    int carry = 0, my_row = -1, my_pos = -1;
    for (int base = 0; base < R; base += 256) {
        const int r = base + tid;
        int keep = 0;
        if (r == 0) {
            keep = 1;
        } else if (r < R && (r & 1)) {
            const int i = r >> 1;
            keep = xs[(i + 1) * C] != xs[i * C] ? 1 : 0;
        } else if (r < R) {
            const int j = r >> 1;
            for (int q = 0; q < n_rect; ++q) {
                const int rc = rect_idx[q];
                if (rc > 0 && rc < C && xs[j * C + rc] != xs[(j - 1) * C + rc]) keep = 1;
            }
        }
        const int incl = wave_inclusive_sum(keep, lane);
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int ww = 0; ww < 4; ++ww) {
            const int s = wsum[ww];
            before += ww < w ? s : 0;
            total += s;
        }
        const int p = carry + before + incl - keep;
        if (r < R) ps[r] = keep ? p : -1;
        if (keep) { my_row = r; my_pos = p; }
        carry += total;
        __syncthreads();      // wsum is written again by the next chunk
    }
    if (my_pos == carry - 1) last_row[b] = my_row;      // exactly one thread: row 0 is always kept
    if (tid == 0) lengths[b] = carry;
}

// batch maximum of the kept counts: one workgroup, a fixed reduction order
__global__ __launch_bounds__(256) void ncde_hybrid_max_kernel(const int* __restrict__ lengths, int B, int* __restrict__ max_len) {
    __shared__ int wmax[4];
    const int tid = threadIdx.x;
    int m = 0;
    for (int b = tid; b < B; b += 256) m = max(m, lengths[b]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = max(m, __shfl_down(m, d, 64));
    if ((tid & 63) == 0) wmax[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) *max_len = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
}

// hybrid scheme, pass 2: one workgroup per sample, thread <-> (row offset, channel) as the output loops of
// ncde_linear_coeffs_lds_kernel.  Kept rows go to out[b][pos]; rows lengths[b] .. T-1 repeat the last kept row (read from the
// source, not from `out`).  The positions of a sample are a bijection onto 0 .. lengths[b]-1, so every element of out[b] is written.
__global__ __launch_bounds__(256) void ncde_hybrid_write_kernel(const float* __restrict__ xf, const float* __restrict__ xl, int L, int C, int NL,
                                                                const int* __restrict__ pos, const int* __restrict__ last_row,
                                                                const int* __restrict__ cmap, const int* __restrict__ lengths, int T,
                                                                float* __restrict__ out) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int R = 2 * L - 1;
    const float* xs = xf + (long long)b * L * C;
    const float* xls = xl + (long long)b * L * NL;      // (not dereferenced when NL == 0)
    const int* ps = pos + (long long)b * R;
    float* os = out + (long long)b * T * C;
    const int count = max(lengths[b], 0), lr = last_row[b];
    const int rp = 256 / C > 0 ? 256 / C : 1;
    const int r0 = tid / C, c = tid - r0 * C;
    const bool active = C <= 256 ? r0 < rp : true;
    for (int cc = c; cc < C && active; cc += 256) {
        const int m = cmap[cc];
        // row r of the full table: time and the linear channels are those of raw index (r+1)/2, the rectilinear ones of r/2
        auto value = [&](int r) { return m == -2 ? xs[((r + 1) >> 1) * C] : (m == -1 ? xs[(r >> 1) * C + cc] : xls[((r + 1) >> 1) * NL + m]); };
        for (int r = r0; r < R; r += rp) {
            const int p = ps[r];
            if (p >= 0 && p < T) os[p * C + cc] = value(r);
        }
        if (count < T && lr >= 0 && lr < R) {
            const float v = value(lr);
            for (int p = count + r0; p < T; p += rp) os[p * C + cc] = v;
        }
    }
}

}  // namespace

extern "C" {

int ncde_prepare_smooth_backward(const float* grad_rows, int B, int T, int C, double eps, int order, float* grad_x, void* stream) {
    if (!grad_rows || !grad_x || B < 1 || T < 2 || C < 1 || (order != 3 && order != 5) || !(eps > 0.0) || eps > 1.0) return NCDE_ERR_INVALID;
    if (order != 3)
        return ncde_fail_text(NCDE_ERR_UNSUPPORTED, "ncde_prepare_smooth_backward: order 5 (quintic matching) has no transpose kernel; order 3 only");
    const int P = ncde_smooth_pieces(T, eps);
    SmoothBwdScal k;      // evaluated in double, rounded once
    k.w2 = (float)(4.0 / eps); k.w3 = (float)(-3.0 / (eps * eps)); k.eps = (float)eps; k.one_m_eps = (float)(1.0 - eps);
    const long long total = (long long)B * T * C;
    const unsigned grid = (unsigned)std::min<long long>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(ncde_smooth_coeffs_bwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, grad_rows, B, T, C, P, eps < 1.0, k, grad_x);
    return hipGetLastError() == hipSuccess ? NCDE_OK : NCDE_ERR_HIP;
}

int ncde_smooth_pieces(int T, double eps) {
    if (T < 2 || !(eps > 0.0) || eps > 1.0) return NCDE_ERR_INVALID;
    return eps < 1.0 ? 2 * T - 3 : T - 1;
}

int ncde_prepare_smooth(const float* x, int B, int T, int C, double eps, int order, float* out, void* stream) {
    if (!x || !out || B < 1 || T < 2 || C < 1 || (order != 3 && order != 5) || !(eps > 0.0) || eps > 1.0) return NCDE_ERR_INVALID;
    const int P = ncde_smooth_pieces(T, eps);
    SmoothScal k;      // the reference's Python scalars, evaluated in double and rounded once where they meet an fp32 tensor
    const double e2 = std::pow(eps, 2.0), e3 = std::pow(eps, 3.0);
    k.eps = (float)eps; k.inv_e2 = (float)(1.0 / e2); k.inv_3e2 = (float)(1.0 / (3.0 * e2));
    k.inv_e3 = (float)(1.0 / e3); k.four_eps = (float)(4.0 * eps); k.inv_2e3 = (float)(1.0 / (2.0 * e3));
    k.e2 = (float)e2; k.neg_inv_10e2 = (float)(-(1.0 / (10.0 * e2)));
    const long long total = (long long)B * P * C;
    const unsigned grid = (unsigned)std::min<long long>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(ncde_smooth_coeffs_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, B, T, C, P, order, eps < 1.0, k, out);
    return hipGetLastError() == hipSuccess ? NCDE_OK : NCDE_ERR_HIP;
}

int64_t ncde_prepare_workspace_bytes(int kind, int B, int L, int C) {
    if (B < 1 || L < 2 || C < 1) return NCDE_ERR_INVALID;
    if (kind == NCDE_INTERP_CUBIC) return (int64_t)sizeof(float) * (2 * (int64_t)B * L * C + L) + 256;
    return 256;
}

// ---- launch plans: which kernel a builder call runs, with how much LDS -- decided in ONE place, read by the launch and by the
// ncde_prepare_kernel_name query alike (so a test that means to reach a kernel can assert that it does)
enum PrepareKernel { PREP_LINEAR_LDS, PREP_LINEAR_GLOBAL, PREP_CUBIC_LDS, PREP_CUBIC_GLOBAL };
struct PreparePlan {
    PrepareKernel kernel;
    size_t lds;             // dynamic LDS bytes (0: none)
    int nsmp, sstride;      // PREP_CUBIC_LDS: samples per workgroup, LDS stride of one sample in floats
};

static bool prepare_plan(int kind, int B, int L, int C, bool has_grid, int rectilinear_time_index, PreparePlan* p) {
    if (B < 1 || L < 2 || C < 1) return false;
    p->lds = 0; p->nsmp = 0; p->sstride = 0;
    if (kind == NCDE_INTERP_LINEAR) {
        if (rectilinear_time_index >= C) return false;
        const bool rect = rectilinear_time_index >= 0;
        const size_t lds = sizeof(float) * ((size_t)L * C * (rect ? 2 : 3) + 64 * (size_t)C);
        if (lds <= 64 * 1024 && C <= 256) {   // the series fits LDS: staged, coalesced, scan-parallel variant
            p->kernel = PREP_LINEAR_LDS;
            p->lds = lds;
        } else {
            p->kernel = PREP_LINEAR_GLOBAL;
        }
        return true;
    }
    if (kind != NCDE_INTERP_CUBIC) return false;
    p->kernel = PREP_CUBIC_GLOBAL;
    // LDS-staged variant: NSMP whole samples per wave (lane <-> (sample, channel)), as many as fit 64 lanes and the LDS budget
    if (C <= 64 && !has_grid) {      // (constant-coefficient system: the default grid only)
        const int LC = L * C;
        int sstride = LC + ((C - (LC % 32)) % 32 + 32) % 32;      // stride == C (mod 32): the lanes of one time step fall on distinct banks
        sstride = (sstride + 3) & ~3;
        int nsmp = 64 / C;
        auto lds_of = [&](int ns) { return sizeof(float) * ((size_t)2 * ns * sstride + 2 * ((L + 3) & ~3)); };
        // the recurrences are latency chains: prefer several resident workgroups per CU (<= 28 KB each: measured best at cfg4 size) over full waves
        const char* ev = ncde_dev_env("NCDE_CUBIC_LDS_KB");
        const size_t budget = (size_t)(ev && atoi(ev) > 0 ? atoi(ev) : 28) * 1024;
        while (nsmp > 1 && lds_of(nsmp) > budget) --nsmp;
        if (lds_of(nsmp) <= (size_t)150 * 1024) {
            p->kernel = PREP_CUBIC_LDS;
            p->lds = lds_of(nsmp);
            p->nsmp = nsmp;
            p->sstride = sstride;
        }
    }
    return true;
}

const char* ncde_prepare_kernel_name(int kind, int B, int L, int C, int has_grid, int rectilinear_time_index) {
    PreparePlan p;
    // the rectilinear preparation leaves no gap the grid could enter: the grid plays no part in the choice for the linear builder
    if (!prepare_plan(kind, B, L, C, has_grid != 0, rectilinear_time_index, &p)) return nullptr;
    static thread_local char name[64];
    switch (p.kernel) {
        case PREP_LINEAR_LDS: return "ncde_linear_coeffs_lds";
        case PREP_LINEAR_GLOBAL: return "ncde_linear_coeffs";
        case PREP_CUBIC_GLOBAL: return "ncde_cubic_coeffs";
        case PREP_CUBIC_LDS: snprintf(name, sizeof(name), "ncde_cubic_coeffs_lds<nsmp=%d>", p.nsmp); return name;
    }
    return nullptr;
}

int ncde_prepare_linear_grid(const float* x, const float* t, int B, int L, int C, int rectilinear_time_index, float* out, void* stream) {
    PreparePlan p;
    if (!x || !out || !prepare_plan(NCDE_INTERP_LINEAR, B, L, C, t != nullptr, rectilinear_time_index, &p)) return NCDE_ERR_INVALID;
    const float* tg = rectilinear_time_index < 0 ? t : nullptr;      // the rectilinear preparation leaves no gap the grid could enter
    const long long n = (long long)B * C;
    const int rect = rectilinear_time_index < 0 ? -1 : rectilinear_time_index;
    if (p.kernel == PREP_LINEAR_LDS) {
        if (ncde_lds_optin((const void*)ncde_linear_coeffs_lds_kernel, p.lds) != hipSuccess)
            return NCDE_ERR_HIP;
        hipLaunchKernelGGL(ncde_linear_coeffs_lds_kernel, dim3(B), dim3(256), p.lds, (hipStream_t)stream, x, B, L, C, rect, out, tg);
    } else {
        hipLaunchKernelGGL(ncde_linear_coeffs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, B, L, C, rect, out, tg);
    }
    return hipGetLastError() == hipSuccess ? NCDE_OK : NCDE_ERR_HIP;
}

int ncde_prepare_linear(const float* x, int B, int L, int C, int rectilinear_time_index, float* out, void* stream) {
    return ncde_prepare_linear_grid(x, nullptr, B, L, C, rectilinear_time_index, out, stream);
}

int ncde_prepare_cubic_grid(const float* x, const float* t, int B, int L, int C, float* out, void* workspace, size_t workspace_bytes, void* stream) {
    PreparePlan p;
    if (!x || !out || !workspace || !prepare_plan(NCDE_INTERP_CUBIC, B, L, C, t != nullptr, -1, &p)) return NCDE_ERR_INVALID;
    if ((int64_t)workspace_bytes < ncde_prepare_workspace_bytes(NCDE_INTERP_CUBIC, B, L, C)) return NCDE_ERR_WORKSPACE;
    float* ws = (float*)workspace;
    float* ws_d = ws + (size_t)B * L * C;
    float* diag = ws_d + (size_t)B * L * C;
    hipLaunchKernelGGL(ncde_cubic_diag_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, L, diag);
    const long long n = (long long)B * C;
    if (p.kernel == PREP_CUBIC_LDS) {
        if (ncde_lds_optin((const void*)ncde_cubic_coeffs_lds_kernel, p.lds) != hipSuccess)
            return NCDE_ERR_HIP;
        hipLaunchKernelGGL(ncde_cubic_coeffs_lds_kernel, dim3((unsigned)((B + p.nsmp - 1) / p.nsmp)), dim3(CUBIC_NT), p.lds, (hipStream_t)stream, x, B, L, C,
                           p.nsmp, p.sstride, out, ws, diag, ws_d);
        return hipGetLastError() == hipSuccess ? NCDE_OK : NCDE_ERR_HIP;
    }
    hipLaunchKernelGGL(ncde_cubic_coeffs_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, x, B, L, C, out,
                       ws, diag, ws_d, t);
    return hipGetLastError() == hipSuccess ? NCDE_OK : NCDE_ERR_HIP;
}

int ncde_prepare_cubic(const float* x, int B, int L, int C, float* out, void* workspace, size_t workspace_bytes, void* stream) {
    return ncde_prepare_cubic_grid(x, nullptr, B, L, C, out, workspace, workspace_bytes, stream);
}

// ---- Hermite cubic with backward differences: one elementwise launch, the same for every shape ---------------------------------------
static bool hermite_shape_ok(int B, int L, int C) { return B >= 1 && L >= 2 && C >= 1 && 4LL * C <= 0x7fffffffLL; }      // (a row of 4C is indexed with int)

const char* ncde_prepare_hermite_kernel_name(int B, int L, int C) { return hermite_shape_ok(B, L, C) ? "ncde_hermite_coeffs" : nullptr; }

int ncde_prepare_hermite(const float* knots, const float* t, int B, int L, int C, float* out, void* stream) {
    if (!knots || !out || knots == out || !hermite_shape_ok(B, L, C)) return NCDE_ERR_INVALID;
    const long long total = (long long)B * (L - 1) * C;
    const unsigned grid = (unsigned)std::min<long long>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(ncde_hermite_coeffs_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, knots, t, B, L, C, out);
    return hipGetLastError() == hipSuccess ? NCDE_OK : NCDE_ERR_HIP;
}

// ---- causal control paths: fills and the linear / rectilinear hybrid scheme -----------------------------------------------------
// one sample is indexed with int: its largest table, (2L-1) x C, has to stay below 2^31 elements
static bool causal_shape_ok(int B, int L, int C) {
    return B >= 1 && L >= 1 && C >= 1 && (2 * (long long)L - 1) * C <= 0x7fffffffLL;
}

int ncde_prepare_fill(const float* x, int B, int L, int C, int has_initial, double initial_value, int forward_fill, float* out, void* stream) {
    if (!x || !out || x == out || !causal_shape_ok(B, L, C)) return NCDE_ERR_INVALID;
    hipLaunchKernelGGL(ncde_fill_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, x, L, C, has_initial != 0 ? 1 : 0, (float)initial_value,
                       forward_fill != 0 ? 1 : 0, out);
    return hipGetLastError() == hipSuccess ? NCDE_OK : NCDE_ERR_HIP;
}

// workspace of the hybrid scheme (int32): pos [B][2L-1] | last_row [B] | cmap [C]
int64_t ncde_prepare_hybrid_workspace_bytes(int B, int L, int C) {
    if (L < 2 || C < 2 || !causal_shape_ok(B, L, C)) return NCDE_ERR_INVALID;
    return (int64_t)sizeof(int) * ((int64_t)B * (2 * (int64_t)L - 1) + B + C) + 256;
}

int ncde_prepare_hybrid_count(const float* x_filled, int B, int L, int C, const int* rect_idx, int n_rect, void* workspace,
                              size_t workspace_bytes, int* lengths, int* max_len, void* stream) {
    const int64_t need = ncde_prepare_hybrid_workspace_bytes(B, L, C);
    if (need < 0 || !x_filled || !workspace || !lengths || !max_len || n_rect < 0 || n_rect > C - 1 || (n_rect > 0 && !rect_idx))
        return NCDE_ERR_INVALID;
    if ((int64_t)workspace_bytes < need) return NCDE_ERR_WORKSPACE;
    int* pos = (int*)workspace;
    int* last_row = pos + (size_t)B * (2 * (size_t)L - 1);
    int* cmap = last_row + B;
    hipLaunchKernelGGL(ncde_hybrid_count_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, x_filled, L, C, rect_idx, n_rect, pos, last_row, cmap,
                       lengths);
    hipLaunchKernelGGL(ncde_hybrid_max_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const int*)lengths, B, max_len);
    return hipGetLastError() == hipSuccess ? NCDE_OK : NCDE_ERR_HIP;
}

int ncde_prepare_hybrid_write(const float* x_filled, const float* x_linear, int B, int L, int C, int n_rect, const void* workspace,
                              size_t workspace_bytes, const int* lengths, int T, float* out, void* stream) {
    const int64_t need = ncde_prepare_hybrid_workspace_bytes(B, L, C);
    if (need < 0 || !x_filled || !workspace || !lengths || !out || n_rect < 0 || n_rect > C - 1 || T < 1 || T > 2 * L - 1) return NCDE_ERR_INVALID;
    const int NL = C - 1 - n_rect;
    if (NL > 0 && !x_linear) return NCDE_ERR_INVALID;
    if ((int64_t)workspace_bytes < need) return NCDE_ERR_WORKSPACE;
    const int* pos = (const int*)workspace;
    const int* last_row = pos + (size_t)B * (2 * (size_t)L - 1);
    const int* cmap = last_row + B;
    hipLaunchKernelGGL(ncde_hybrid_write_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, x_filled, x_linear, L, C, NL, pos, last_row, cmap, lengths,
                       T, out);
    return hipGetLastError() == hipSuccess ? NCDE_OK : NCDE_ERR_HIP;
}

}  // extern "C"
