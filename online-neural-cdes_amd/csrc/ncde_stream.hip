// Online inference: advance the CDE state of B independent streams by m new observation rows in ONE launch.
//
// One workgroup = one tile of 16 streams, 4 waves, the LDS plan of ncde_fwd_generic plus three dX/dt images and the last filled row.
// Per new row: fill it from the stream's last row (copies and compares only), form the one (linear) or two (rectilinear: time moves,
// then the values move) pieces' dX/dt in LDS, run the Butcher stages of the method per piece on gen_stage_forward -- the stage
// arithmetic and its order are those of ncde_fwd_generic on the default grid with step 1 -- and read W_f z + b_f out.  The state
// (z, last row, previous piece's dX/dt, observation count) is loaded once and written back once per launch, for the streams that
// received a row only.
//
// Which derivative a stage reads is the reference's left-piece rule (interpolation_linear.py:212-219: bucketize(right=False) - 1):
// stage 1 of a step sits ON a knot and reads the piece to its left -- the previous piece, or its own at the very first step of a
// stream -- every later stage reads the step's own piece.  The clamp is per stream, from the stream's own count.
//
// The Hermite cubic with backward differences (ncde_stream_step_hermite, the HERMITE instantiation of the same body) is the one cubic
// with that property: its piece reads the new row, the last row and the previous piece's slope.  The row is filled and differenced
// exactly as on the linear path (DXA = dn, DXL = b: per stream the previous dn, or its own at the first step); stage 1 reads b -- the
// left piece's end slope at frac = 1 in exact arithmetic --, every later stage the image b + (2c + 3d s) s, rebuilt into the DXB slot
// (free: no rectilinear form) by the combine phase of the stage before it, under that phase's barrier.  s is per stream: the frac
// default_stage hands load_dx at the stream's own step index, (n + offset) - n in fp32.
#include <cstdarg>
#include <cstddef>
#include <cstdio>

#include "ncde_common.h"
#include "ncde_generic_stage.h"
#include "ncde_host.h"

struct StreamArgs {
    int m, rect, ti, n_out;
    const float* x;
    long long xs_m, xs_b;
    const unsigned char* active;
    float init;
    float* z;
    float* last;
    float* pdx;
    int* count;
    const float* Wf;
    const float* bf;
    float* out;
    float* z_out;
};

template <bool HERMITE>
__device__ __forceinline__ void stream_step_body(const KArgs& a, const StreamArgs& q) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * NCDE_TILE;
    const int H = a.H, C = a.C, Hp = ru16(H), Cp = ru4(C);
    int Dp = Hp;
    for (int l = 0; l < a.n_layers; ++l) Dp = max(Dp, ru16(a.dout[l]));
    const int HS = Hp * 16, DS = Dp * 16, CS = Cp * 16;
    float* YS = lds;
    float* ACT0 = YS + HS;
    float* ACT1 = ACT0 + DS;
    float* Y0 = ACT1 + DS;
    float* K1 = Y0 + HS;
    float* K2 = K1 + HS;
    float* KO = K2 + HS;
    float* DXL = KO + HS;        // stage 1 of the first piece: the piece to the left (per stream: the previous one, or its own)
    float* DXA = DXL + CS;       // first piece
    float* DXB = DXA + CS;       // second piece (rectilinear); HERMITE: the stage image
    float* LAST = DXB + CS;      // last filled row
    float* PDX = LAST + CS;      // dX/dt of the last piece taken
    int* CNT = (int*)(PDX + CS); // observations received; then: steps at this row (0: no; else the step's index + 1), received a row in this launch
    int* STEP = CNT + 16;
    int* EVER = STEP + 16;
    const int total = 5 * HS + 2 * DS + 5 * CS + 48;
    for (int e = tid; e < total; e += GEN_THREADS) lds[e] = 0.0f;
    __syncthreads();
    // 1. load the state
    for (int e = tid; e < HS; e += GEN_THREADS) {
        const int h = e >> 4, s = e & 15, b = b0 + s;
        if (h < H && b < a.B) {
            const float v = q.z[(long long)b * H + h];
            Y0[e] = v;
            YS[e] = v;
        }
    }
    for (int e = tid; e < 16 * Cp; e += GEN_THREADS) {
        const int s = e / Cp, c = e - s * Cp, b = b0 + s;
        if (c < C && b < a.B) {
            LAST[c * 16 + s] = q.last[(long long)b * C + c];
            PDX[c * 16 + s] = q.pdx[(long long)b * C + c];
        }
    }
    if (tid < 16 && b0 + tid < a.B) CNT[tid] = q.count[b0 + tid];
    __syncthreads();
    const int S = n_stages(a.method);
    const int n_pieces = q.rect ? 2 : 1;
    for (int r = 0; r < q.m; ++r) {
        // 2. fill the new row, 3. the pieces' dX/dt
        for (int e = tid; e < 16 * Cp; e += GEN_THREADS) {
            const int s = e / Cp, c = e - s * Cp, b = b0 + s;
            float dl = 0.0f, da = 0.0f, db = 0.0f;
            if (c < C && b < a.B && (!q.active || q.active[(long long)r * a.B + b])) {
                const int cnt = CNT[s];
                const float xv = q.x[(long long)r * q.xs_m + (long long)b * q.xs_b + c];
                const float last = LAST[c * 16 + s];
                const float fill = xv != xv ? (cnt == 0 ? q.init : last) : xv;
                if (cnt > 0) {
                    const float mid = (q.rect && c != q.ti) ? last : fill;      // rectilinear: the lagged row (new time, old values)
                    da = mid - last;
                    db = fill - mid;
                    dl = cnt == 1 ? da : PDX[c * 16 + s];
                    PDX[c * 16 + s] = q.rect ? db : da;
                }
                LAST[c * 16 + s] = fill;
            }
            DXL[c * 16 + s] = dl;
            DXA[c * 16 + s] = da;
            DXB[c * 16 + s] = db;
        }
        __syncthreads();
        if (tid < 16) {
            const int b = b0 + tid;
            const int act = b < a.B && (!q.active || q.active[(long long)r * a.B + b]);
            STEP[tid] = act ? CNT[tid] : 0;       // the first row of a stream (count 0) initialises it: no solver step
            CNT[tid] += act;
            EVER[tid] |= act;
        }
        __syncthreads();
        int any_step = 0;      // (uniform: every thread reads the same 16 flags)
#pragma unroll
        for (int s = 0; s < 16; ++s) any_step |= STEP[s];
        // 4. the Butcher stages, one step per piece
        if (any_step) {
            for (int pc = 0; pc < n_pieces; ++pc) {
                const float* dx_own = (HERMITE || pc != 0) ? DXB : DXA;
                const float* dx_left = pc == 0 ? DXL : DXA;
                for (int j = 0; j < S; ++j) {
                    gen_stage_forward(a, YS, ACT0, ACT1, j == 0 ? dx_left : dx_own, KO, Hp, Cp, tid);
                    for (int e = tid; e < HS; e += GEN_THREADS) {
                        if (!STEP[e & 15]) continue;
                        float y0 = Y0[e], k1 = K1[e], k2 = K2[e];
                        bool last;
                        const float ys = StageCombine::apply(a.method, j, KO[e], 1.0f, y0, k1, k2, last);
                        YS[e] = ys;
                        K1[e] = k1;
                        K2[e] = k2;
                        if (last) Y0[e] = y0;
                    }
                    if constexpr (HERMITE) {
                        if (j + 1 < S) {      // the next stage's dX/dt (its reader starts behind the barrier; the last reader of DXB is done)
                            for (int e = tid; e < CS; e += GEN_THREADS) {
                                const float frac = default_stage(a.method, (float)(STEP[e & 15] - 1) + stage_offset(a.method, j + 1), 0x7fffffff).frac;
                                const float bb = DXL[e], dn = DXA[e];
                                const float two_c = 2.0f * (3.0f * (dn - bb) - dn + bb);
                                const float three_d = (dn - bb) - two_c;
                                const float inner = two_c + three_d * frac;
                                DXB[e] = bb + inner * frac;
                            }
                        }
                    }
                    __syncthreads();
                }
            }
        }
        // 5. readout of every stream of the tile (a stream without a row: of its unchanged z)
        if (q.Wf) {
            for (int e = tid; e < 16 * q.n_out; e += GEN_THREADS) {
                const int s = e / q.n_out, o = e - s * q.n_out, b = b0 + s;
                if (b < a.B) {
                    const float* w = q.Wf + (long long)o * H;
                    float acc = q.bf ? q.bf[o] : 0.0f;
                    for (int h = 0; h < H; ++h) acc = fmaf(w[h], Y0[h * 16 + s], acc);
                    q.out[((long long)r * a.B + b) * q.n_out + o] = acc;
                }
            }
        }
        if (q.z_out) {
            for (int e = tid; e < 16 * H; e += GEN_THREADS) {
                const int s = e / H, h = e - s * H, b = b0 + s;
                if (b < a.B) q.z_out[((long long)r * a.B + b) * H + h] = Y0[h * 16 + s];
            }
        }
    }
    __syncthreads();
    // 6. write the state back: only the streams that received a row
    for (int e = tid; e < 16 * H; e += GEN_THREADS) {
        const int s = e / H, h = e - s * H, b = b0 + s;
        if (b < a.B && EVER[s]) q.z[(long long)b * H + h] = Y0[h * 16 + s];
    }
    for (int e = tid; e < 16 * Cp; e += GEN_THREADS) {
        const int s = e / Cp, c = e - s * Cp, b = b0 + s;
        if (c < C && b < a.B && EVER[s]) {
            q.last[(long long)b * C + c] = LAST[c * 16 + s];
            q.pdx[(long long)b * C + c] = PDX[c * 16 + s];
        }
    }
    if (tid < 16 && b0 + tid < a.B && EVER[tid]) q.count[b0 + tid] = CNT[tid];
}

extern "C" __global__ __launch_bounds__(GEN_THREADS) void ncde_stream_step_kernel(KArgs a, StreamArgs q) { stream_step_body<false>(a, q); }
extern "C" __global__ __launch_bounds__(GEN_THREADS) void ncde_stream_step_hermite_kernel(KArgs a, StreamArgs q) { stream_step_body<true>(a, q); }

namespace {

int sfail(int code, const char* fmt, ...) {
    char buf[384];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return ncde_fail_text(code, buf);
}

// The problem as the stream step reads it: batch, channels, hidden, method, flags and the field.  coeffs, z0, n_knots, output and the
// time plan are NOT read (the rows arrive through NcdeStream, the state lives in its buffers).
// hermite: the Hermite step's problem says interp = NCDE_INTERP_CUBIC; the LDS plan is the same (the stage image takes the DXB slot).
int stream_problem(const NcdeProblem* in, NcdeProblem* p, Layout* y, size_t* lds, bool hermite = false) {
    if (!in) return sfail(NCDE_ERR_INVALID, "problem is NULL");
    if (in->abi_version < 1 || in->abi_version > NCDE_ABI_VERSION)
        return sfail(NCDE_ERR_INVALID, "abi_version %d not in [1, %d]", in->abi_version, NCDE_ABI_VERSION);
    memset(p, 0, sizeof(*p));
    memcpy(p, in, in->abi_version >= 3 ? sizeof(NcdeProblem) : (in->abi_version == 2 ? offsetof(NcdeProblem, time_plan) : offsetof(NcdeProblem, field_kind)));
    p->abi_version = NCDE_ABI_VERSION;
    p->reserved_ = 0;
    p->time_plan = nullptr;
    p->output = NCDE_OUT_KNOTS;
    if (p->batch < 1 || p->channels < 1 || p->hidden < 1) return sfail(NCDE_ERR_INVALID, "batch/channels/hidden must be >= 1");
    if (hermite && p->interp != NCDE_INTERP_CUBIC)
        return sfail(NCDE_ERR_INVALID, "online Hermite step: the path's coefficients are a|b|2c|3d, interp must be NCDE_INTERP_CUBIC (interp %d)", p->interp);
    if (!hermite && p->interp != NCDE_INTERP_LINEAR)
        return sfail(NCDE_ERR_INVALID, "online step: only a linear or rectilinear path is causal (interp %d)", p->interp);
    if (p->method != NCDE_EULER && p->method != NCDE_MIDPOINT && p->method != NCDE_RK4_38)
        return sfail(NCDE_ERR_INVALID, "Invalid method %d. Must be one of {euler, midpoint, rk4}", p->method);
    if (p->n_layers < 0 || p->n_layers > NCDE_MAX_LAYERS) return sfail(NCDE_ERR_INVALID, "n_layers %d outside [0, %d]", p->n_layers, NCDE_MAX_LAYERS);
    if (p->field_kind < NCDE_FIELD_ORIGINAL || p->field_kind > NCDE_FIELD_LOWRANK) return sfail(NCDE_ERR_INVALID, "unknown field_kind %d", p->field_kind);
    if (p->field_input < NCDE_INPUT_MATMUL || p->field_input > NCDE_INPUT_DERIVATIVE)
        return sfail(NCDE_ERR_INVALID, "vector_field_type string not recognised (field_input %d)", p->field_input);
    if (p->field_kind != NCDE_FIELD_ORIGINAL || p->field_input != NCDE_INPUT_MATMUL)
        return sfail(NCDE_ERR_UNSUPPORTED, "online step: the original field with the matmul input only (field_kind %d, field_input %d)", p->field_kind,
                     p->field_input);
    int d = p->hidden;
    for (int l = 0; l < p->n_layers; ++l) {
        if (p->layer_in[l] != d) return sfail(NCDE_ERR_INVALID, "layer %d: in=%d does not chain from %d", l, p->layer_in[l], d);
        if (p->layer_out[l] < 1) return sfail(NCDE_ERR_INVALID, "layer %d: out=%d", l, p->layer_out[l]);
        if (!p->layer_W[l] || !p->layer_b[l]) return sfail(NCDE_ERR_INVALID, "layer %d: NULL weight/bias", l);
        d = p->layer_out[l];
    }
    if (!p->Wo || !p->bo) return sfail(NCDE_ERR_INVALID, "NULL Wo/bo");
    *y = make_layout(p);
    if (y->lds_fwd > (size_t)kLdsLimit) return sfail(NCDE_ERR_UNSUPPORTED, "generic forward needs %zu B of LDS (> %d)", y->lds_fwd, kLdsLimit);
    *lds = sizeof(float) * (size_t)(5 * y->HS + 2 * y->DS + 5 * y->Cp * 16 + 48);
    if (*lds > (size_t)kLdsLimit) return sfail(NCDE_ERR_UNSUPPORTED, "online step needs %zu B of LDS (> %d)", *lds, kLdsLimit);
    return NCDE_OK;
}

}  // namespace

extern "C" int64_t ncde_stream_workspace_bytes(const NcdeProblem* p) {
    NcdeProblem q;
    Layout y;
    size_t lds;
    const int rc = stream_problem(p, &q, &y, &lds);
    return rc == NCDE_OK ? 0 : rc;
}

extern "C" const char* ncde_stream_kernel_name(const NcdeProblem* p) {
    NcdeProblem q;
    Layout y;
    size_t lds;
    return stream_problem(p, &q, &y, &lds) == NCDE_OK ? "ncde_stream_step" : nullptr;
}

static int stream_launch(const NcdeProblem* p, const NcdeStream* s, void* stream, bool hermite) {
    NcdeProblem q;
    Layout y;
    size_t lds;
    const int rc = stream_problem(p, &q, &y, &lds, hermite);
    if (rc != NCDE_OK) return rc;
    if (!s) return sfail(NCDE_ERR_INVALID, "stream is NULL");
    if (s->n_rows < 1) return sfail(NCDE_ERR_INVALID, "n_rows %d: at least one new row", s->n_rows);
    if (!s->x || !s->z || !s->last_row || !s->prev_dx || !s->count) return sfail(NCDE_ERR_INVALID, "NULL x / z / last_row / prev_dx / count");
    if (s->x_stride_b < q.channels || s->x_stride_m < 0) return sfail(NCDE_ERR_INVALID, "x strides (%lld, %lld): rows of %d channels", (long long)s->x_stride_m, (long long)s->x_stride_b, q.channels);
    if (s->rectilinear && (s->time_index < 0 || s->time_index >= q.channels))
        return sfail(NCDE_ERR_INVALID, "Time index must be in [0, %d], was given %d.", q.channels - 1, s->time_index);
    if (hermite && s->rectilinear) return sfail(NCDE_ERR_INVALID, "online Hermite step: rectilinear must be 0 (the scheme has no rectilinear form)");
    if (s->Wf ? (s->n_out < 1 || !s->out) : !s->z_out) return sfail(NCDE_ERR_INVALID, "readout: Wf needs n_out >= 1 and out; without Wf pass z_out");
    KArgs a;
    fill_kargs(&q, y, &a);
    StreamArgs k{};
    k.m = s->n_rows; k.rect = s->rectilinear != 0; k.ti = s->time_index; k.n_out = s->Wf ? s->n_out : 0;
    k.x = s->x; k.xs_m = s->x_stride_m; k.xs_b = s->x_stride_b;
    k.active = s->active; k.init = s->initial_value_if_nan;
    k.z = s->z; k.last = s->last_row; k.pdx = s->prev_dx; k.count = s->count;
    k.Wf = s->Wf; k.bf = s->bf; k.out = s->out; k.z_out = s->z_out;
    void (*kernel)(KArgs, StreamArgs) = hermite ? ncde_stream_step_hermite_kernel : ncde_stream_step_kernel;
    if (ncde_lds_optin((const void*)kernel, lds) != hipSuccess) return sfail(NCDE_ERR_HIP, "LDS opt-in of %zu B failed", lds);
    hipLaunchKernelGGL(kernel, dim3(y.n_wg), dim3(GEN_THREADS), lds, (hipStream_t)stream, a, k);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return sfail(NCDE_ERR_HIP, "%s launch failed: %s", hermite ? "ncde_stream_step_hermite" : "ncde_stream_step", hipGetErrorString(e));
    return NCDE_OK;
}

extern "C" int ncde_stream_step(const NcdeProblem* p, const NcdeStream* s, void* stream) { return stream_launch(p, s, stream, false); }

extern "C" int64_t ncde_stream_hermite_workspace_bytes(const NcdeProblem* p) {
    NcdeProblem q;
    Layout y;
    size_t lds;
    const int rc = stream_problem(p, &q, &y, &lds, true);
    return rc == NCDE_OK ? 0 : rc;
}

extern "C" const char* ncde_stream_hermite_kernel_name(const NcdeProblem* p) {
    NcdeProblem q;
    Layout y;
    size_t lds;
    return stream_problem(p, &q, &y, &lds, true) == NCDE_OK ? "ncde_stream_step_hermite" : nullptr;
}

extern "C" int ncde_stream_step_hermite(const NcdeProblem* p, const NcdeStream* s, void* stream) { return stream_launch(p, s, stream, true); }
