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
//
// The phases are device functions of their own (stream_load_state .. stream_store_state); ncde_stream_stack_step runs them layer by
// layer for a chain of linear CDEs in one launch (see StreamStackArgs), ncde_stream_step_field / ncde_stream_step_field_hermite run
// them around the stage of the vector-field variants (the minimal-gated field, the evaluate / derivative inputs; see above that
// kernel), and ncde_stream_step_lowrank around the stage of the low-rank field, on all three paths (see above that kernel).
//
// The linear / rectilinear hybrid path (the HYBRID instantiations: ncde_stream_step_hybrid, ncde_stream_step_field_hybrid,
// ncde_stream_step_lowrank_hybrid; see "The hybrid step" below): a per-channel mask says which channels step rectilinearly, and the
// second piece of a row is taken per stream, only where one of those channels changed.
#include <cstdarg>
#include <cstddef>
#include <cstdio>

#include "ncde_common.h"
#include "ncde_generic_stage.h"
#include "ncde_host.h"
#include "ncde_lowrank_stage.h"
#include "ncde_timeloop.h"
#include "ncde_variant_stage.h"

struct StreamArgs {
    int m, rect, ti, n_out;
    const float* x;
    long long xs_m, xs_b;
    const unsigned char* active;
    const unsigned char* rmask;      // HYBRID: uint8 [C], 1 = the channel steps rectilinearly; NULL on every other kernel, which never reads it
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

// The LDS of one 16-stream tile.  StreamScratch: what a stage works in -- one set per workgroup, whatever the number of layers.
// StreamState: what a layer carries from row to row.
struct StreamScratch {
    float *YS, *ACT0, *ACT1, *K1, *K2, *KO;
    float* DXL;      // stage 1 of the first piece: the piece to the left (per stream: the previous one, or its own)
    float* DXA;      // first piece
    float* DXB;      // second piece (rectilinear); HERMITE: the stage image
    int* STEP;       // steps at this row (0: no; else the step's index + 1)
    int* EVER;       // received a row in this launch
    int* HASB;       // HYBRID: takes the second piece at this row (a sparse channel changed); NULL otherwise
    float* XS;       // the field step's evaluate input: the start rows of the two pieces, 2 CS; NULL on every other plan
};
struct StreamState {
    float* Y0;
    float* LAST;     // last filled row
    float* PDX;      // dX/dt of the last piece taken
    int* CNT;        // observations received
};

// THE LDS PLAN of a tile, for the host's byte count and the kernels' carve alike (offsets and total in floats; -1: no such area):
//   YS / U | ACT0 | ACT1 | K1 | K2 | KO | DXL | DXA | DXB | XS | STEP | EVER | HASB | the layers' states | PQ
// HS, DS, CS: the rounded [Hp][16], [Dp][16], [Cp][16] (a stack: the widest of its layers).  The first area holds the stage input: HS
// wide, or DS for the field step, whose U carries the control rows.  XS: the field step off the hybrid path; HASB: the hybrid kinds;
// PQ [NTp][16]: the low-rank step.  state_floats: stream_state_floats of the layer, or their sum over a stack.
enum StreamFamily { kFamStep = 0, kFamField = 1, kFamLowrank = 2 };
struct StreamPlan {
    int act0, act1, k1, k2, ko, dxl, dxa, dxb, xs, step, ever, hasb, states, pq;
    long long total;
};
__host__ __device__ __forceinline__ int stream_state_floats(int HS, int CS) { return HS + 2 * CS + 16; }      // Y0 | LAST | PDX | CNT
__host__ __device__ __forceinline__ StreamPlan stream_plan(int family, bool hybrid, int HS, int DS, int CS, long long NTp, int state_floats) {
    StreamPlan n;
    n.act0 = family == kFamField ? DS : HS;
    n.act1 = n.act0 + DS;
    n.k1 = n.act1 + DS;
    n.k2 = n.k1 + HS;
    n.ko = n.k2 + HS;
    n.dxl = n.ko + HS;
    n.dxa = n.dxl + CS;
    n.dxb = n.dxa + CS;
    n.xs = (family == kFamField && !hybrid) ? n.dxb + CS : -1;
    n.step = n.dxb + CS + (n.xs >= 0 ? 2 * CS : 0);
    n.ever = n.step + 16;
    n.hasb = hybrid ? n.ever + 16 : -1;
    n.states = n.ever + (hybrid ? 32 : 16);
    n.pq = n.states + state_floats;
    n.total = n.pq + (family == kFamLowrank ? 16 * NTp : 0);
    return n;
}
__device__ __forceinline__ StreamScratch stream_carve_scratch(float* lds, const StreamPlan& n) {
    StreamScratch w;
    w.YS = lds;
    w.ACT0 = lds + n.act0;
    w.ACT1 = lds + n.act1;
    w.K1 = lds + n.k1;
    w.K2 = lds + n.k2;
    w.KO = lds + n.ko;
    w.DXL = lds + n.dxl;
    w.DXA = lds + n.dxa;
    w.DXB = lds + n.dxb;
    w.XS = n.xs >= 0 ? lds + n.xs : nullptr;
    w.STEP = (int*)(lds + n.step);
    w.EVER = (int*)(lds + n.ever);
    w.HASB = n.hasb >= 0 ? (int*)(lds + n.hasb) : nullptr;
    return w;
}
// layer l's state: behind those of the layers below it
__device__ __forceinline__ StreamState stream_carve_state(float* states, const KArgs* a, int l) {
    for (int i = 0; i < l; ++i) states += stream_state_floats(ru16(a[i].H) * 16, ru4(a[i].C) * 16);
    StreamState t;
    t.Y0 = states;
    t.LAST = t.Y0 + ru16(a[l].H) * 16;
    t.PDX = t.LAST + ru4(a[l].C) * 16;
    t.CNT = (int*)(t.PDX + ru4(a[l].C) * 16);
    return t;
}

// 1. load a layer's state (YS != NULL: z is the first stage input as well)
__device__ __forceinline__ void stream_load_state(const KArgs& a, const StreamArgs& q, const StreamState& t, float* YS, int b0, int tid) {
    const int H = a.H, C = a.C, HS = ru16(H) * 16, Cp = ru4(C);
    for (int e = tid; e < HS; e += GEN_THREADS) {
        const int h = e >> 4, s = e & 15, b = b0 + s;
        if (h < H && b < a.B) {
            const float v = q.z[(long long)b * H + h];
            t.Y0[e] = v;
            if (YS) YS[e] = v;
        }
    }
    for (int e = tid; e < 16 * Cp; e += GEN_THREADS) {
        const int s = e / Cp, c = e - s * Cp, b = b0 + s;
        if (c < C && b < a.B) {
            t.LAST[c * 16 + s] = q.last[(long long)b * C + c];
            t.PDX[c * 16 + s] = q.pdx[(long long)b * C + c];
        }
    }
    if (tid < 16 && b0 + tid < a.B) t.CNT[tid] = q.count[b0 + tid];
}

// 2. fill row r, 3. the pieces' dX/dt; then the row's bookkeeping.  from: the row as a [c][s] image in LDS (the layer below of a
// stack: its Y0 after its step for this row), NULL: row r of q.x.  Returns whether any stream of the tile steps (uniform: every
// thread reads the same 16 flags).  Ends behind a barrier.
// starts != NULL (the field step's evaluate input): two further [c][s] images, the START ROWS of the two pieces -- starts[..] the
// stream's last row before this fill, starts[CS + ..] the lagged row -- written in all 16 Cp entries like the dX/dt images (zero
// for a stream that does not step).
// HYBRID (see "The hybrid step" below): the lagged row holds the old values of the channels of q.rmask only, and the second piece
// is per stream.  any_b (uniform, like the return value): whether any stream of the tile takes it at this row.
template <bool HYBRID>
__device__ __forceinline__ int stream_fill_row(const KArgs& a, const StreamArgs& q, const StreamScratch& w, const StreamState& t, const float* from,
                                               int r, int b0, int tid, float* starts, int* any_b) {
    const int C = a.C, Cp = ru4(C);
    for (int e = tid; e < 16 * Cp; e += GEN_THREADS) {
        const int s = e / Cp, c = e - s * Cp, b = b0 + s;
        float dl = 0.0f, da = 0.0f, db = 0.0f, xa = 0.0f, xb = 0.0f;
        if (c < C && b < a.B && (!q.active || q.active[(long long)r * a.B + b])) {
            const int cnt = t.CNT[s];
            const float xv = from ? from[c * 16 + s] : q.x[(long long)r * q.xs_m + (long long)b * q.xs_b + c];
            const float last = t.LAST[c * 16 + s];
            const float fill = xv != xv ? (cnt == 0 ? q.init : last) : xv;
            if (cnt > 0) {
                float mid;
                if constexpr (HYBRID) mid = q.rmask[c] ? last : fill;      // hybrid: the lagged row keeps the sparse channels' old values
                else mid = (q.rect && c != q.ti) ? last : fill;            // rectilinear: the lagged row (new time, old values)
                da = mid - last;
                db = fill - mid;
                dl = cnt == 1 ? da : t.PDX[c * 16 + s];
                if constexpr (HYBRID) t.PDX[c * 16 + s] = da;      // (db below, behind the barrier, where the stream takes the second piece)
                else t.PDX[c * 16 + s] = q.rect ? db : da;
                xa = last;
                xb = mid;
            }
            t.LAST[c * 16 + s] = fill;
        }
        w.DXL[c * 16 + s] = dl;
        w.DXA[c * 16 + s] = da;
        w.DXB[c * 16 + s] = db;
        if (starts) {
            starts[c * 16 + s] = xa;
            starts[Cp * 16 + c * 16 + s] = xb;
        }
    }
    __syncthreads();
    if (tid < 16) {
        const int b = b0 + tid;
        const int act = b < a.B && (!q.active || q.active[(long long)r * a.B + b]);
        w.STEP[tid] = act ? t.CNT[tid] : 0;       // the first row of a stream (count 0) initialises it: no solver step
        t.CNT[tid] += act;
        w.EVER[tid] |= act;
        if constexpr (HYBRID) {      // db != 0 somewhere in the stream's column of the image (zero for a stream that does not step)
            int has = 0;
            for (int c = 0; c < C; ++c) has |= w.DXB[c * 16 + tid] != 0.0f;
            w.HASB[tid] = has;       // written every row: the flag of the row before is gone
        }
    }
    __syncthreads();
    int any_step = 0;
#pragma unroll
    for (int s = 0; s < 16; ++s) any_step |= w.STEP[s];
    if constexpr (HYBRID) {
        int any = 0;
#pragma unroll
        for (int s = 0; s < 16; ++s) any |= w.HASB[s];
        *any_b = any;
        // prev_dx of a stream that takes the second piece is that piece's.  The same thread owns (c, s) in the loop above at every
        // row, and the state is stored behind a barrier: no barrier of its own.
        for (int e = tid; e < 16 * Cp; e += GEN_THREADS) {
            const int s = e / Cp, c = e - s * Cp;
            if (c < C && w.HASB[s]) t.PDX[c * 16 + s] = w.DXB[c * 16 + s];
        }
    }
    return any_step;
}

// 4. the Butcher stages, one step per piece.  stream_combine: the bookkeeping of stage j for the streams that step (the caller's
// barrier follows).  flags: which streams take the piece -- STEP, or on the second piece of a hybrid row HASB; a stream that does
// not keeps its YS / K1 / K2 / Y0.
__device__ __forceinline__ void stream_combine(const KArgs& a, const StreamScratch& w, const StreamState& t, const int* flags, int j, int HS, int tid) {
    for (int e = tid; e < HS; e += GEN_THREADS) {
        if (!flags[e & 15]) continue;
        float y0 = t.Y0[e], k1 = w.K1[e], k2 = w.K2[e];
        bool last;
        const float ys = StageCombine::apply(a.method, j, w.KO[e], 1.0f, y0, k1, k2, last);
        w.YS[e] = ys;
        w.K1[e] = k1;
        w.K2[e] = k2;
        if (last) t.Y0[e] = y0;
    }
}
// HERMITE: the image stage j > 0 of the step reads, rebuilt into the DXB slot from b = DXL and dn = DXA at the stream's own frac.
// start == NULL: the slope b + (2c + 3d s) s.  start != NULL (the field step's evaluate input; the streams' last rows before the
// fill): the value start + (b + (2c / 2 + 3d s / 3) s) s, in the operation order of the batch loaders (vr_load_cin).
__device__ __forceinline__ void stream_hermite_image(const KArgs& a, const StreamScratch& w, int j, int CS, int tid, const float* start = nullptr) {
    for (int e = tid; e < CS; e += GEN_THREADS) {
        const float frac = default_stage(a.method, (float)(w.STEP[e & 15] - 1) + stage_offset(a.method, j), 0x7fffffff).frac;
        const float bb = w.DXL[e], dn = w.DXA[e];
        const float two_c = 2.0f * (3.0f * (dn - bb) - dn + bb);
        const float three_d = (dn - bb) - two_c;
        if (start) {
            float inner = 0.5f * two_c + (three_d * frac) / 3.0f;
            inner = bb + inner * frac;
            w.DXB[e] = start[e] + inner * frac;
        } else {
            const float inner = two_c + three_d * frac;
            w.DXB[e] = bb + inner * frac;
        }
    }
}
// A stage object is what a family adds to the body: Stage(a, w, lds, PQ, tid), and
//   kFamily, tail_rows(a)    the family whose plan its kernels carve (stream_plan), and the rows NTp of its PQ (0: none)
//   starts()                 the start rows the fill leaves and the Hermite image reads (the field step's evaluate input), or NULL
//   stage(pc, j, n_pieces, dx)  stage j of piece pc: whatever the field needs before it (the field step rewrites the control rows
//                            of U, behind a barrier of its own), then one evaluation of the field at YS with the image dx into KO,
//                            ending behind a barrier (gen_stage_forward, vr_stage_forward, or the low-rank stage)
// HYBRID: the second piece (n_pieces = 2 only where a stream of the tile takes it: uniform) combines under HASB -- every stream at
// the start of a piece has YS = Y0 (from the load, or from the last combine it took part in), so one that sits the piece out
// keeps both, and the KO the stage forms for it is never read.
template <bool HERMITE, bool HYBRID, class Stage>
__device__ __forceinline__ void stream_stages(const KArgs& a, const StreamScratch& w, const StreamState& t, int n_pieces, int tid, const Stage& stage) {
    const int HS = ru16(a.H) * 16, CS = ru4(a.C) * 16;
    const int S = n_stages(a.method);
    for (int pc = 0; pc < n_pieces; ++pc) {
        const float* dx_own = (HERMITE || pc != 0) ? w.DXB : w.DXA;
        const float* dx_left = pc == 0 ? w.DXL : w.DXA;
        const int* flags = (HYBRID && pc != 0) ? w.HASB : w.STEP;
        for (int j = 0; j < S; ++j) {
            stage.stage(pc, j, n_pieces, j == 0 ? dx_left : dx_own);
            stream_combine(a, w, t, flags, j, HS, tid);
            if constexpr (HERMITE) {      // the next stage's image (its reader starts behind the barrier; the last reader of DXB is done)
                if (j + 1 < S) stream_hermite_image(a, w, j + 1, CS, tid, stage.starts());
            }
            __syncthreads();
        }
    }
}
// the original field's stage
struct StreamGenStage {
    static constexpr int kFamily = kFamStep;
    const KArgs& a;
    const StreamScratch& w;
    int tid;
    __device__ __forceinline__ StreamGenStage(const KArgs& a_, const StreamScratch& w_, float*, float*, int tid_) : a(a_), w(w_), tid(tid_) {}
    static __device__ __forceinline__ int tail_rows(const KArgs&) { return 0; }
    __device__ __forceinline__ float* starts() const { return nullptr; }
    __device__ __forceinline__ void stage(int, int, int, const float* dx) const { gen_stage_forward(a, w.YS, w.ACT0, w.ACT1, dx, w.KO, ru16(a.H), ru4(a.C), tid); }
};

// 5. readout of every stream of the tile at row r (a stream without a row: of its unchanged z)
__device__ __forceinline__ void stream_readout(const KArgs& a, const StreamArgs& q, const StreamState& t, int r, int b0, int tid) {
    const int H = a.H;
    if (q.Wf) {
        for (int e = tid; e < 16 * q.n_out; e += GEN_THREADS) {
            const int s = e / q.n_out, o = e - s * q.n_out, b = b0 + s;
            if (b < a.B) {
                const float* wf = q.Wf + (long long)o * H;
                float acc = q.bf ? q.bf[o] : 0.0f;
                for (int h = 0; h < H; ++h) acc = fmaf(wf[h], t.Y0[h * 16 + s], acc);
                q.out[((long long)r * a.B + b) * q.n_out + o] = acc;
            }
        }
    }
    if (q.z_out) {
        for (int e = tid; e < 16 * H; e += GEN_THREADS) {
            const int s = e / H, h = e - s * H, b = b0 + s;
            if (b < a.B) q.z_out[((long long)r * a.B + b) * H + h] = t.Y0[h * 16 + s];
        }
    }
}

// 6. write a layer's state back: only the streams that received a row
__device__ __forceinline__ void stream_store_state(const KArgs& a, const StreamArgs& q, const StreamScratch& w, const StreamState& t, int b0, int tid) {
    const int H = a.H, C = a.C, Cp = ru4(C);
    for (int e = tid; e < 16 * H; e += GEN_THREADS) {
        const int s = e / H, h = e - s * H, b = b0 + s;
        if (b < a.B && w.EVER[s]) q.z[(long long)b * H + h] = t.Y0[h * 16 + s];
    }
    for (int e = tid; e < 16 * Cp; e += GEN_THREADS) {
        const int s = e / Cp, c = e - s * Cp, b = b0 + s;
        if (c < C && b < a.B && w.EVER[s]) {
            q.last[(long long)b * C + c] = t.LAST[c * 16 + s];
            q.pdx[(long long)b * C + c] = t.PDX[c * 16 + s];
        }
    }
    if (tid < 16 && b0 + tid < a.B && w.EVER[tid]) q.count[b0 + tid] = t.CNT[tid];
}

// The hybrid step (HYBRID; DESIGN.md 5.14 "Hybrid step"): the online half of linear_rectilinear_hybrid_coeffs.  Time is channel 0;
// q.rmask [C] marks the sparse channels R, every other channel is linear.  A new row of a stream with count > 0 adds
//   piece A   time and the linear channels move:  da[c] = fill[c] - last[c] (c not in R), 0 (c in R);  stage 1 reads prev_dx (da itself
//             at count == 1), the later stages da;
//   piece B   the sparse channels move:  db[c] = fill[c] - last[c] (c in R), 0 elsewhere;  stage 1 reads da, the later stages db.
// Piece B is taken by the streams with db != 0 in some channel only (the builder keeps a knot only where a sparse channel
// changed): the fill phase leaves that per stream in HASB, 16 flags next to STEP and EVER, rewritten at every row between the fill
// phase's two barriers.  Piece B combines under HASB (a flag implies STEP: db is zero for a stream that does not step), and is
// skipped altogether -- S stages instead of 2 S -- where no stream of the tile takes it; that branch is uniform, read from the 16
// flags as any_step is.  prev_dx after the row is db where B was taken and da otherwise.  Precondition: a stream's time strictly
// increases, so piece A always exists (not checked).
// LDS: the plan of the non-hybrid kind plus the 16 flags; the field step drops XS (no evaluate input on this path).

// One layer at one row: fill (from: see stream_fill_row), the pieces' stages where a stream of the tile steps, readout.  The number
// of pieces is launch-wide (q.rect) or, HYBRID, the tile-wide any_b of this row: uniform either way.
template <bool HERMITE, bool HYBRID, class Stage>
__device__ __forceinline__ void stream_row(const KArgs& a, const StreamArgs& q, const StreamScratch& w, const StreamState& t, const float* from, int r,
                                           int b0, int tid, const Stage& stage) {
    int any_b = 0;
    const int any_step = stream_fill_row<HYBRID>(a, q, w, t, from, r, b0, tid, stage.starts(), &any_b);
    const int n_pieces = (HYBRID ? any_b : q.rect) ? 2 : 1;
    if (any_step) stream_stages<HERMITE, HYBRID>(a, w, t, n_pieces, tid, stage);
    stream_readout(a, q, t, r, b0, tid);
}

// THE BODY of every step kernel: carve and clear the plan, load the state, per row the L layers bottom up, store the state.  L = 1
// but for the stacked step (STACK, below), whose scratch is sized by its widest layer and whose states lie one behind the other.
// a, q: the kernel's argument blocks, read only (__restrict__: without it the register allocator leaves an unused 20-byte frame in
// several of the kernels, DESIGN.md 5.14 "One body").
template <class Stage, bool HERMITE, bool HYBRID = false, bool STACK = false>
__device__ __forceinline__ void stream_body(const KArgs* __restrict__ a, const StreamArgs* __restrict__ q, int L) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * NCDE_TILE;
    int HS = 0, DS = 0, CS = 0, state_floats = 0;
    for (int l = 0; l < L; ++l) {
        const TileDims td = tile_dims(a[l], a[l].d0);
        HS = max(HS, td.HS);
        DS = max(DS, td.DS);
        CS = max(CS, td.Cp * 16);
        state_floats += stream_state_floats(td.HS, td.Cp * 16);
    }
    const StreamPlan n = stream_plan(Stage::kFamily, HYBRID, HS, DS, CS, Stage::tail_rows(a[0]), state_floats);
    const StreamScratch w = stream_carve_scratch(lds, n);
    float* states = lds + n.states;
    for (int e = tid; e < (int)n.total; e += GEN_THREADS) lds[e] = 0.0f;
    __syncthreads();
    for (int l = 0; l < L; ++l) stream_load_state(a[l], q[l], stream_carve_state(states, a, l), STACK ? nullptr : w.YS, b0, tid);
    __syncthreads();
    const Stage stage0(a[0], w, lds, lds + n.pq, tid);      // the one layer's stage object: built once per launch (a stack: one per layer and row)
    for (int r = 0; r < q[0].m; ++r) {
        const float* below = nullptr;
        for (int l = 0; l < L; ++l) {
            const StreamState t = stream_carve_state(states, a, l);
            if constexpr (STACK) {
                // the stage input of this layer (the last readers of YS, the layer before, ended behind a barrier; readers start behind fill's)
                for (int e = tid; e < ru16(a[l].H) * 16; e += GEN_THREADS) w.YS[e] = t.Y0[e];
            }
            if constexpr (STACK) stream_row<HERMITE, HYBRID>(a[l], q[l], w, t, below, r, b0, tid, Stage(a[l], w, lds, lds + n.pq, tid));
            else stream_row<HERMITE, HYBRID>(a[l], q[l], w, t, below, r, b0, tid, stage0);
            if constexpr (STACK) below = t.Y0;
        }
    }
    __syncthreads();
    for (int l = 0; l < L; ++l) stream_store_state(a[l], q[l], w, stream_carve_state(states, a, l), b0, tid);
}

extern "C" __global__ __launch_bounds__(GEN_THREADS) void ncde_stream_step_kernel(KArgs a, StreamArgs q) { stream_body<StreamGenStage, false>(&a, &q, 1); }
extern "C" __global__ __launch_bounds__(GEN_THREADS) void ncde_stream_step_hermite_kernel(KArgs a, StreamArgs q) { stream_body<StreamGenStage, true>(&a, &q, 1); }
extern "C" __global__ __launch_bounds__(GEN_THREADS) void ncde_stream_step_hybrid_kernel(KArgs a, StreamArgs q) { stream_body<StreamGenStage, false, true>(&a, &q, 1); }

// The stacked step (ncde_stream_stack_step): n_stack chained linear layers, layer l + 1 reading layer l's hidden state as its
// observation.  Everything a layer reads of the one below is per stream, so the tile's workgroup walks the layers of a row with
// barriers only: layer l's new row is the Y0 image of layer l - 1 after that layer's step for this row -- [h][s] there, [c][s]
// here, the same image.  Layer 0's q carries the rows, the mask and the fill value; the host copies m / active / init into
// every layer's q.  The scratch is shared and sized by the widest layer, the state is per layer.
//
// Narrow after wide, wide after narrow: nothing is re-zeroed between layers, because every scratch element a layer READS it has
// WRITTEN itself since the previous layer left: YS rows < Hp from its own Y0 (whose pad rows and pad samples are zero from the
// launch's clear and stay zero: KO's pad rows are sums of tanh(0) = 0 terms); DXL / DXA / DXB all 16 Cp entries by its fill
// phase, zeros where c >= C or the sample is beyond B; ACT0 / ACT1 rows < ru16(dout) by dense_relu before the next layer of the
// field reads rows < ru4(dout) of them; KO rows < Hp by every stage; K1 / K2 by stage 1 / 2 of a step before stage 2 / 3 reads
// them (midpoint and euler carry them through without using them).  Rows beyond its own extents a layer does not read.
struct StreamStackArgs {
    int n_stack;
    KArgs a[NCDE_STREAM_MAX_STACK];
    StreamArgs q[NCDE_STREAM_MAX_STACK];
};
static_assert(sizeof(StreamStackArgs) <= 4096, "the stacked step passes every layer's arguments by value: HIP's kernel arguments end at 4 KiB");

extern "C" __global__ __launch_bounds__(GEN_THREADS) void ncde_stream_stack_step_kernel(StreamStackArgs k) {
    stream_body<StreamGenStage, false, false, true>(k.a, k.q, k.n_stack);
}

// The field step (ncde_stream_step_field): the same phases around the stage of the vector-field VARIANTS (vr_stage_forward,
// ncde_variant_stage.h) -- the minimal-gated field, and the evaluate / derivative inputs of the original and the minimal-gated field.
//
// The field input U [d0][16] takes the place of YS: rows < H are the stage state, rows H .. H + C - 1 (direct inputs: d0 = H + C)
// the control input, rewritten before EVERY stage from the images of the fill phase:
//   matmul / derivative  the dX/dt image of the left-piece rule above (stage 1: DXL, or DXA for the second rectilinear piece; later
//                        stages the piece's own); matmul hands it to the contraction, derivative copies it into U.
//   evaluate             X at the stage time.  Stage 1 sits on the piece's first knot and reads that knot's ROW itself: the stream's
//                        last row before this fill (first piece) or the lagged row (second rectilinear piece), the two images
//                        stream_fill_row leaves in XS.  Stage j > 0 reads start + frac_j * own, frac_j per stream the frac
//                        default_stage hands the batch loaders at the stream's own step index n = count - 1 (linear), 2 (count - 1)
//                        and 2 (count - 1) + 1 (rectilinear): (n + offset_j) - n in fp32.  (The batch kernel forms the knot row as
//                        prev + 1 (next - prev) on the left piece: equal up to one rounding.  The torch-op step reads the row, too.)
// Every weight is streamed (wres = -1): one step per launch does not repay filling resident copies, so the sums run in the order of
// a batch ncde_fwd_variant solve WITHOUT residency.
//
// LDS, in floats (HS = ru16(H) 16, DS = 16 max(ru16(d0), ru16(layer widths), ru16(H)), CS = ru4(C) 16):
//   U, ACT0, ACT1 3 DS | K1, K2, KO 3 HS | DXL, DXA, DXB 3 CS | XS 2 CS | STEP, EVER 32 | state HS + 2 CS + 16     = 3 DS + 4 HS + 7 CS + 48
// What is read is inside what the launch cleared or a phase wrote, area by area:
//   U rows < Hp       from Y0 at load and by every combine; rows H .. Hp - 1 receive y0 + dt k of pad rows = 0 there (Y0's pad rows are
//                     zero from the clear, KO's are written as 0 by the heads), pad samples >= B never step and stay 0.
//   U rows H .. d0-1  all 16 samples before every stage (after the combine, which may have zeroed rows < Hp among them); samples >= B
//                     and channels of a stream that does not step read the images' zeros.  Rows d0 .. ru16(d0) - 1 stay zero: no
//                     phase but the combine (rows < Hp, zeros) writes them.  The first layer reads rows < ru4(d0).
//   ACT0 / ACT1       rows < ru16(dout) by vr_dense (rows >= dout as 0) before the next layer or the heads read rows < ru4(dout).
//   KO rows < Hp      by every stage; K1 / K2 by stage 1 / 2 of a step before stage 2 / 3 reads them.
//   DXL, DXA, DXB, XS all 16 Cp entries by every fill, zeros where c >= C, the sample is beyond B or the stream does not step.
// Every barrier sits in uniform control flow: the branches around stages are the tile-wide any_step and the launch-wide field input.
// the evaluate input of stage j of piece pc: X at the stage time -> UC [c][s], c < C (see above)
__device__ void stream_field_value(const KArgs& a, float* UC, const float* start, const float* own, const int* STEP, int j, int n_pieces, int pc, int tid) {
    const float off = stage_offset(a.method, j);
    for (int e = tid; e < a.C * 16; e += GEN_THREADS) {
        float v = start[e];
        if (j > 0) {
            const int n = (STEP[e & 15] - 1) * n_pieces + pc;
            const float frac = default_stage(a.method, (float)n + off, 0x7fffffff).frac;
            v = v + frac * own[e];
        }
        UC[e] = v;
    }
}

// HERMITE (ncde_stream_step_field_hermite): the same five pairs on the Hermite cubic with backward differences, one piece per row.
// The fill leaves b = DXL, dn = DXA and the stream's last row before the fill in XS, as above.  Stage 1 sits on the knot and reads b
// (matmul / derivative) or the knot's row XS (evaluate).  The image of stage j > 1 -- the slope b + (2c + 3d s) s, or for evaluate
// the value XS + (b + (2c / 2 + 3d s / 3) s) s -- is rebuilt into the DXB slot (free: no rectilinear form; all 16 Cp entries, zeros
// where the fill left zeros) by the combine phase of the stage before it, under that phase's barrier, as in stream_stages<true>.
// Same plan, same areas; the second half of XS is written by the fill and not read.
//
// HYBRID (ncde_stream_step_field_hybrid; "The hybrid step" above): the matmul and derivative inputs -- the host refuses evaluate,
// whose stage offset needs the stream's knot index, which the state does not carry.  No XS, 16 flags more:
//   U, ACT0, ACT1 3 DS | K1, K2, KO 3 HS | DXL, DXA, DXB 3 CS | STEP, EVER, HASB 48 | state HS + 2 CS + 16     = 3 DS + 4 HS + 5 CS + 64
// The branch around the second piece is the tile-wide any_b; its combine runs under HASB, so a stream that sits the piece out
// keeps U rows < Hp, K1, K2 and Y0 (its control rows of U are rewritten from the images, whose entries are its own).
template <bool HERMITE>
struct StreamFieldStage {
    static constexpr int kFamily = kFamField;
    const KArgs& a;
    const StreamScratch& w;      // (w.YS: U)
    float* lds;
    const TileDims td;
    int tid;
    __device__ __forceinline__ StreamFieldStage(const KArgs& a_, const StreamScratch& w_, float* lds_, float*, int tid_)
        : a(a_), w(w_), lds(lds_), td(tile_dims(a_, a_.d0)), tid(tid_) {}
    static __device__ __forceinline__ int tail_rows(const KArgs&) { return 0; }
    // the pieces' start rows (HYBRID: evaluate is refused by the host, XS does not exist)
    __device__ __forceinline__ float* starts() const { return a.field_input == NCDE_INPUT_EVALUATE ? w.XS : nullptr; }
    __device__ __forceinline__ void stage(int pc, int j, int n_pieces, const float* img) const {
        float* UC = w.YS + a.H * 16;      // the control rows of U
        if (a.field_input != NCDE_INPUT_MATMUL) {
            const bool evaluate = a.field_input == NCDE_INPUT_EVALUATE;
            const float* start = evaluate ? w.XS + pc * td.Cp * 16 : nullptr;      // the piece's start row
            if constexpr (HERMITE) {      // evaluate: the knot's row, then the value image
                const float* src = (evaluate && j == 0) ? start : img;
                for (int e = tid; e < a.C * 16; e += GEN_THREADS) UC[e] = src[e];
            } else {
                if (evaluate) stream_field_value(a, UC, start, img, w.STEP, j, n_pieces, pc, tid);      // (j > 0: img is the piece's own)
                else
                    for (int e = tid; e < a.C * 16; e += GEN_THREADS) UC[e] = img[e];
            }
            __syncthreads();
        }
        // (RU, RG, XB: the gru field's, which the host refuses -- valid addresses all the same, never touched)
        vr_stage_forward(a, w.YS, w.ACT0, w.ACT0, w.ACT0, w.ACT0, img, w.KO, nullptr, nullptr, nullptr, lds, td.Hp, td.Cp, td.DS, tid);
    }
};

extern "C" __global__ __launch_bounds__(GEN_THREADS) void ncde_stream_step_field_kernel(KArgs a, StreamArgs q) { stream_body<StreamFieldStage<false>, false>(&a, &q, 1); }
extern "C" __global__ __launch_bounds__(GEN_THREADS) void ncde_stream_step_field_hermite_kernel(KArgs a, StreamArgs q) { stream_body<StreamFieldStage<true>, true>(&a, &q, 1); }
extern "C" __global__ __launch_bounds__(GEN_THREADS) void ncde_stream_step_field_hybrid_kernel(KArgs a, StreamArgs q) { stream_body<StreamFieldStage<false>, false, true>(&a, &q, 1); }

// The low-rank step (ncde_stream_step_lowrank, ncde_stream_step_lowrank_hermite): the phases and the stage loop of stream_body
// around the stage of ncde_fwd_lowrank (ncde_lowrank_stage.h) -- the inner layers on dense_relu, ping-pong in ACT0 / ACT1, then
// lr_heads into PQ, a barrier, and lr_contract of PQ with the stage's dX/dt image into KO.  The image is the one stream_stages hands
// the original field: the left-piece rule on a linear or rectilinear stream, b and the rebuilt slope image in the DXB slot on the
// Hermite path.  The heads are streamed (wl = NULL, wres_o = -1: one step per launch does not repay a resident copy), so the sums
// run in the order of a batch ncde_fwd_lowrank solve WITHOUT residency.
//
// LDS, in floats (HS = ru16(H) 16, DS = 16 max(ru16(H), ru16(layer widths)), CS = ru4(C) 16, NTp = ru16((H + C) R)):
//   YS, K1, K2, KO 4 HS | ACT0, ACT1 2 DS | DXL, DXA, DXB 3 CS | STEP, EVER 32 | state HS + 2 CS + 16 | PQ 16 NTp     = 5 HS + 2 DS + 5 CS + 48 + 16 NTp
// What is read is inside what the launch cleared or a phase wrote, area by area:
//   YS rows < Hp      from Y0 at load and by every combine; rows H .. Hp - 1 stay zero (Y0's pad rows are zero from the clear, KO's
//                     are written as 0 by lr_contract), pad samples >= B never step and stay 0.  The first layer reads rows < ru4(H).
//   ACT0 / ACT1       rows < ru16(dout) by dense_relu (rows >= dout as 0) before the next layer or lr_heads reads rows < ru4(dout).
//   PQ rows < NTp     by lr_heads in every stage (rows NT .. NTp - 1 as 0), all 16 samples, before lr_contract reads rows < NT.
//   KO rows < Hp      by lr_contract in every stage; K1 / K2 by stage 1 / 2 of a step before stage 2 / 3 reads them.
//   DXL, DXA, DXB     all 16 Cp entries by every fill, zeros where c >= C, the sample is beyond B or the stream does not step;
//                     lr_contract reads channels < C.  Hermite: DXB all 16 Cp entries again by every rebuild.
// Every barrier sits in uniform control flow: the only branch around stages is the tile-wide any_step.
struct StreamLowrankStage {
    static constexpr int kFamily = kFamLowrank;
    const KArgs& a;
    const StreamScratch& w;
    const LrDims d;      // (wres_o = -1: d.wl = NULL)
    float* PQ;           // [NTp][16]
    int tid;
    __device__ __forceinline__ StreamLowrankStage(const KArgs& a_, const StreamScratch& w_, float* lds, float* PQ_, int tid_)
        : a(a_), w(w_), d(lr_dims(a_, lds)), PQ(PQ_), tid(tid_) {}
    static __device__ __forceinline__ int tail_rows(const KArgs& a) { return lr_dims(a, nullptr).NTp; }
    __device__ __forceinline__ float* starts() const { return nullptr; }
    __device__ __forceinline__ void stage(int, int, int, const float* dx) const {
        const int lane = tid & 63, wave = tid >> 6;
        const float* in = w.YS;
        for (int l = 0; l < a.n_layers; ++l) {
            float* outb = (l & 1) ? w.ACT1 : w.ACT0;
            dense_relu(a.W[l], a.b[l], a.dout[l], a.din[l], in, outb, wave, lane);
            __syncthreads();
            in = outb;
        }
        lr_heads(a, d, in, PQ, wave, lane);
        __syncthreads();
        lr_contract(d, PQ, dx, w.KO, ru16(a.H) * 16, tid);
        __syncthreads();
    }
};

// HYBRID (ncde_stream_step_lowrank_hybrid; "The hybrid step" above): the same body, 16 flags more (HASB, behind EVER).
extern "C" __global__ __launch_bounds__(GEN_THREADS) void ncde_stream_step_lowrank_kernel(KArgs a, StreamArgs q) { stream_body<StreamLowrankStage, false>(&a, &q, 1); }
extern "C" __global__ __launch_bounds__(GEN_THREADS) void ncde_stream_step_lowrank_hermite_kernel(KArgs a, StreamArgs q) { stream_body<StreamLowrankStage, true>(&a, &q, 1); }
extern "C" __global__ __launch_bounds__(GEN_THREADS) void ncde_stream_step_lowrank_hybrid_kernel(KArgs a, StreamArgs q) { stream_body<StreamLowrankStage, false, true>(&a, &q, 1); }

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
// stream_problem_head: the copy and the checks every step shares, up to the range of the field's two enums.
int stream_problem_head(const NcdeProblem* in, NcdeProblem* p, bool hermite) {
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
    return NCDE_OK;
}

// hybrid (the *_hybrid entry points): the linear path only -- the Hermite cubic has no hybrid form --, 16 flags more of LDS.
int stream_hybrid_head(const NcdeProblem* in, NcdeProblem* p) {
    if (in && in->abi_version >= 1 && in->abi_version <= NCDE_ABI_VERSION && in->interp == NCDE_INTERP_CUBIC)
        return sfail(NCDE_ERR_UNSUPPORTED, "online hybrid step: the Hermite path has no hybrid form (interp must be NCDE_INTERP_LINEAR)");
    return stream_problem_head(in, p, false);
}

// THE STEP KINDS: one row per (family, path) that has an entry point -- which kernel runs it under which name, and which of
// KArgs' wres* are set to -1 (no resident copy: one step per launch does not repay filling one).
enum StreamPath { kPathLinear, kPathHermite, kPathInterp, kPathHybrid };      // kPathInterp: linear or Hermite, as the problem's interp says
enum StreamStreamed { kStreamNone, kStreamHeads, kStreamAll };
struct StreamKind {
    int family, path;
    void (*kernel[2])(KArgs, StreamArgs);      // [1], name[1]: a kPathInterp kind on the Hermite path
    const char* name[2];
    int streamed;
};
const StreamKind kStep = {kFamStep, kPathLinear, {ncde_stream_step_kernel}, {"ncde_stream_step"}, kStreamNone};
const StreamKind kStepHermite = {kFamStep, kPathHermite, {ncde_stream_step_hermite_kernel}, {"ncde_stream_step_hermite"}, kStreamNone};
const StreamKind kStepHybrid = {kFamStep, kPathHybrid, {ncde_stream_step_hybrid_kernel}, {"ncde_stream_step_hybrid"}, kStreamNone};
const StreamKind kField = {kFamField, kPathLinear, {ncde_stream_step_field_kernel}, {"ncde_stream_step_field"}, kStreamAll};
const StreamKind kFieldHermite = {kFamField, kPathHermite, {ncde_stream_step_field_hermite_kernel}, {"ncde_stream_step_field_hermite"}, kStreamAll};
const StreamKind kFieldHybrid = {kFamField, kPathHybrid, {ncde_stream_step_field_hybrid_kernel}, {"ncde_stream_step_field_hybrid"}, kStreamAll};
const StreamKind kLowrank = {kFamLowrank, kPathInterp, {ncde_stream_step_lowrank_kernel, ncde_stream_step_lowrank_hermite_kernel},
                             {"ncde_stream_step_lowrank", "ncde_stream_step_lowrank_hermite"}, kStreamHeads};
const StreamKind kLowrankHybrid = {kFamLowrank, kPathHybrid, {ncde_stream_step_lowrank_hybrid_kernel}, {"ncde_stream_step_lowrank_hybrid"}, kStreamHeads};

// the inner layers chain from d0 and have their weights
int stream_layer_chain(const NcdeProblem* p, int d) {
    for (int l = 0; l < p->n_layers; ++l) {
        if (p->layer_in[l] != d) return sfail(NCDE_ERR_INVALID, "layer %d: in=%d does not chain from %d", l, p->layer_in[l], d);
        if (p->layer_out[l] < 1) return sfail(NCDE_ERR_INVALID, "layer %d: out=%d", l, p->layer_out[l]);
        if (!p->layer_W[l] || !p->layer_b[l]) return sfail(NCDE_ERR_INVALID, "layer %d: NULL weight/bias", l);
        d = p->layer_out[l];
    }
    return NCDE_OK;
}

// The problem as a step of kind k reads it (p), its layout and the bytes of its LDS plan.  By family:
//   step      the original field with the matmul input.
//   field     plus the gate head of a gated field, and a layer chain that starts at the width of the field input, d0 = hidden (matmul)
//             or hidden + channels; the hybrid path takes the matmul and derivative inputs only.
//   low-rank  the rank in the top byte of flags and the second head (Wo / bo = M_h [H R, dlast], Wg / bg = M_o [R C, dlast]).
int stream_problem(const StreamKind& k, const NcdeProblem* in, NcdeProblem* p, Layout* y, size_t* lds) {
    const bool hybrid = k.path == kPathHybrid;
    const bool hermite = k.path == kPathHermite || (k.path == kPathInterp && in && in->interp == NCDE_INTERP_CUBIC);
    int rc = hybrid ? stream_hybrid_head(in, p) : stream_problem_head(in, p, hermite);
    if (rc != NCDE_OK) return rc;
    int d0 = p->hidden;
    long long ntp = 0;      // rows of PQ (the low-rank step)
    const char* what = "online step";
    if (k.family == kFamStep) {
        if (p->field_kind != NCDE_FIELD_ORIGINAL || p->field_input != NCDE_INPUT_MATMUL)
            return sfail(NCDE_ERR_UNSUPPORTED, "online step: the original field with the matmul input only (field_kind %d, field_input %d)", p->field_kind,
                         p->field_input);
    } else if (k.family == kFamField) {
        what = "online field step";
        if (hybrid && p->field_input == NCDE_INPUT_EVALUATE)
            return sfail(NCDE_ERR_UNSUPPORTED, "online hybrid field step: the evaluate input is not covered (its stage offset is the stream's knot index, which the state does not carry)");
        if (p->field_kind == NCDE_FIELD_GRU)
            return sfail(NCDE_ERR_UNSUPPORTED, "online field step: the GRU-gated field is not covered (its stage runs the inner net twice plus a reset gate)");
        if (p->field_kind == NCDE_FIELD_LOWRANK) return sfail(NCDE_ERR_UNSUPPORTED, "online field step: the low-rank field is not covered");
        if (p->field_kind == NCDE_FIELD_ORIGINAL && p->field_input == NCDE_INPUT_MATMUL)
            return sfail(NCDE_ERR_UNSUPPORTED, "online field step: the original field with the matmul input is %s's",
                         (hybrid ? kStepHybrid : (hermite ? kStepHermite : kStep)).name[0]);
        if (p->field_kind != NCDE_FIELD_ORIGINAL && (!p->Wg || !p->bg)) return sfail(NCDE_ERR_INVALID, "gated field: NULL Wg/bg");
        if (p->field_input != NCDE_INPUT_MATMUL) d0 = p->hidden + p->channels;
    } else {
        what = "online low-rank step";
        if (p->field_kind != NCDE_FIELD_LOWRANK) return sfail(NCDE_ERR_UNSUPPORTED, "online low-rank step: the low-rank field only (field_kind %d)", p->field_kind);
        if (p->field_input != NCDE_INPUT_MATMUL)
            return sfail(NCDE_ERR_UNSUPPORTED, "online low-rank step: the low-rank field takes the matmul input only (field_input %d)", p->field_input);
        const int rank = ncde_field_rank(p);
        if (rank < 1 || rank > p->channels)
            return sfail(NCDE_ERR_INVALID, "low-rank field: rank %d (NCDE_FLAG_FIELD_RANK) outside [1, channels = %d]", rank, p->channels);
        if (p->n_layers < 1) return sfail(NCDE_ERR_INVALID, "online low-rank step: the low-rank kernels need at least one inner layer");
        ntp = ((long long)(p->hidden + p->channels) * rank + 15) & ~15LL;
    }
    rc = stream_layer_chain(p, d0);
    if (rc != NCDE_OK) return rc;
    if (k.family == kFamLowrank) {
        if (!p->Wo || !p->bo || !p->Wg || !p->bg) return sfail(NCDE_ERR_INVALID, "low-rank field: NULL Wo/bo (M_h) or Wg/bg (M_o)");
    } else if (!p->Wo || !p->bo) return sfail(NCDE_ERR_INVALID, "NULL Wo/bo");
    *y = make_layout(p);
    if (k.family == kFamStep && y->lds_fwd > (size_t)kLdsLimit)
        return sfail(NCDE_ERR_UNSUPPORTED, "generic forward needs %zu B of LDS (> %d)", y->lds_fwd, kLdsLimit);
    *lds = sizeof(float) * (size_t)stream_plan(k.family, hybrid, y->HS, y->DS, y->Cp * 16, ntp, stream_state_floats(y->HS, y->Cp * 16)).total;
    if (*lds > (size_t)kLdsLimit) return sfail(NCDE_ERR_UNSUPPORTED, "%s needs %zu B of LDS (> %d)", what, *lds, kLdsLimit);
    return NCDE_OK;
}

// the two queries of a kind: the status of its problem, and the name of the kernel that would run it
int stream_query(const StreamKind& k, const NcdeProblem* p, int* interp = nullptr) {
    NcdeProblem q;
    Layout y;
    size_t lds;
    const int rc = stream_problem(k, p, &q, &y, &lds);
    if (rc == NCDE_OK && interp) *interp = q.interp;
    return rc;
}
const char* stream_name(const StreamKind& k, const NcdeProblem* p) {
    int interp = 0;
    return stream_query(k, p, &interp) == NCDE_OK ? k.name[k.path == kPathInterp && interp == NCDE_INTERP_CUBIC] : nullptr;
}

// NcdeStream -> StreamArgs.  rows: whose x, mask and fill value (a stack: layer 0's); s: whose state and readout.
StreamArgs stream_args(const NcdeStream* rows, const NcdeStream* s, int rect, int ti, const unsigned char* rmask) {
    StreamArgs k{};
    k.m = rows->n_rows; k.rect = rect; k.ti = ti; k.n_out = s->Wf ? s->n_out : 0;
    k.x = rows->x; k.xs_m = rows->x_stride_m; k.xs_b = rows->x_stride_b;
    k.active = rows->active; k.init = rows->initial_value_if_nan;
    k.rmask = rmask;
    k.z = s->z; k.last = s->last_row; k.pdx = s->prev_dx; k.count = s->count;
    k.Wf = s->Wf; k.bf = s->bf; k.out = s->out; k.z_out = s->z_out;
    return k;
}

// rect_mask: the hybrid kinds' per-channel mask (a DEVICE pointer, never read here); NULL on every other kind.
int stream_launch(const StreamKind& kind, const NcdeProblem* p, const NcdeStream* s, void* stream, const unsigned char* rect_mask = nullptr) {
    NcdeProblem q;
    Layout y;
    size_t lds;
    const int rc = stream_problem(kind, p, &q, &y, &lds);
    if (rc != NCDE_OK) return rc;
    const bool hermite = q.interp == NCDE_INTERP_CUBIC;
    const bool hybrid = kind.path == kPathHybrid;
    if (!s) return sfail(NCDE_ERR_INVALID, "stream is NULL");
    if (hybrid && !rect_mask) return sfail(NCDE_ERR_INVALID, "online hybrid step: rectilinear_mask is NULL (uint8 [channels] on the device)");
    if (hybrid && s->rectilinear) return sfail(NCDE_ERR_INVALID, "online hybrid step: rectilinear must be 0 (the mask says which channels step)");
    if (hybrid && s->time_index != 0) return sfail(NCDE_ERR_INVALID, "online hybrid step: time is channel 0 (time_index %d)", s->time_index);
    if (s->n_rows < 1) return sfail(NCDE_ERR_INVALID, "n_rows %d: at least one new row", s->n_rows);
    if (!s->x || !s->z || !s->last_row || !s->prev_dx || !s->count) return sfail(NCDE_ERR_INVALID, "NULL x / z / last_row / prev_dx / count");
    if (s->x_stride_b < q.channels || s->x_stride_m < 0) return sfail(NCDE_ERR_INVALID, "x strides (%lld, %lld): rows of %d channels", (long long)s->x_stride_m, (long long)s->x_stride_b, q.channels);
    if (s->rectilinear && (s->time_index < 0 || s->time_index >= q.channels))
        return sfail(NCDE_ERR_INVALID, "Time index must be in [0, %d], was given %d.", q.channels - 1, s->time_index);
    if (hermite && s->rectilinear) return sfail(NCDE_ERR_INVALID, "online Hermite step: rectilinear must be 0 (the scheme has no rectilinear form)");
    if (s->Wf ? (s->n_out < 1 || !s->out) : !s->z_out) return sfail(NCDE_ERR_INVALID, "readout: Wf needs n_out >= 1 and out; without Wf pass z_out");
    KArgs a;
    fill_kargs(&q, y, &a);
    if (kind.streamed == kStreamAll) {
        for (int l = 0; l < NCDE_MAX_LAYERS; ++l) a.wres[l] = -1;
        a.wres_g = a.wres_r = -1;
    }
    if (kind.streamed != kStreamNone) a.wres_o = -1;
    const StreamArgs k = stream_args(s, s, s->rectilinear != 0, s->time_index, hybrid ? rect_mask : nullptr);
    const int which = kind.path == kPathInterp && hermite;
    if (ncde_lds_optin((const void*)kind.kernel[which], lds) != hipSuccess) return sfail(NCDE_ERR_HIP, "LDS opt-in of %zu B failed", lds);
    hipLaunchKernelGGL(kind.kernel[which], dim3(y.n_wg), dim3(GEN_THREADS), lds, (hipStream_t)stream, a, k);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return sfail(NCDE_ERR_HIP, "%s launch failed: %s", kind.name[which], hipGetErrorString(e));
    return NCDE_OK;
}

// Every layer of a stack as the plain step reads it, the chain between the layers and the LDS plan of the whole stack: the scratch
// of the widest layer, every layer's state.
int stream_stack_problems(const NcdeProblem* const* p, int n_stack, NcdeProblem* q, Layout* y, size_t* lds) {
    if (n_stack < 1 || n_stack > NCDE_STREAM_MAX_STACK) return sfail(NCDE_ERR_INVALID, "n_stack %d outside [1, %d]", n_stack, NCDE_STREAM_MAX_STACK);
    if (!p) return sfail(NCDE_ERR_INVALID, "the list of problems is NULL");
    for (int i = 0; i < n_stack; ++i)
        if (!p[i]) return sfail(NCDE_ERR_INVALID, "stacked online step: problem %d is NULL", i);
    int HS = 0, DS = 0, CS = 0, states = 0;
    for (int i = 0; i < n_stack; ++i) {
        size_t own;
        const int rc = stream_problem(kStep, p[i], &q[i], &y[i], &own);
        if (rc != NCDE_OK) return rc;
        if (i > 0 && q[i].channels != q[i - 1].hidden)
            return sfail(NCDE_ERR_INVALID, "stacked online step: layer %d reads %d channels, layer %d has %d hidden units", i, q[i].channels, i - 1, q[i - 1].hidden);
        if (q[i].batch != q[0].batch) return sfail(NCDE_ERR_INVALID, "stacked online step: layer %d has batch %d, layer 0 has %d", i, q[i].batch, q[0].batch);
        HS = std::max(HS, y[i].HS);
        DS = std::max(DS, y[i].DS);
        CS = std::max(CS, y[i].Cp * 16);
        states += stream_state_floats(y[i].HS, y[i].Cp * 16);
    }
    *lds = sizeof(float) * (size_t)stream_plan(kFamStep, false, HS, DS, CS, 0, states).total;
    if (*lds > (size_t)kLdsLimit) return sfail(NCDE_ERR_UNSUPPORTED, "stacked online step of %d layers needs %zu B of LDS (> %d)", n_stack, *lds, kLdsLimit);
    return NCDE_OK;
}
int stream_stack_query(const NcdeProblem* const* p, int n_stack) {
    NcdeProblem q[NCDE_STREAM_MAX_STACK];
    Layout y[NCDE_STREAM_MAX_STACK];
    size_t lds;
    return stream_stack_problems(p, n_stack, q, y, &lds);
}

}  // namespace

extern "C" int64_t ncde_stream_workspace_bytes(const NcdeProblem* p) { return stream_query(kStep, p); }
extern "C" const char* ncde_stream_kernel_name(const NcdeProblem* p) { return stream_name(kStep, p); }
extern "C" int ncde_stream_step(const NcdeProblem* p, const NcdeStream* s, void* stream) { return stream_launch(kStep, p, s, stream); }

extern "C" int64_t ncde_stream_hermite_workspace_bytes(const NcdeProblem* p) { return stream_query(kStepHermite, p); }
extern "C" const char* ncde_stream_hermite_kernel_name(const NcdeProblem* p) { return stream_name(kStepHermite, p); }
extern "C" int ncde_stream_step_hermite(const NcdeProblem* p, const NcdeStream* s, void* stream) { return stream_launch(kStepHermite, p, s, stream); }

extern "C" int64_t ncde_stream_field_workspace_bytes(const NcdeProblem* p) { return stream_query(kField, p); }
extern "C" const char* ncde_stream_field_kernel_name(const NcdeProblem* p) { return stream_name(kField, p); }
extern "C" int ncde_stream_step_field(const NcdeProblem* p, const NcdeStream* s, void* stream) { return stream_launch(kField, p, s, stream); }

extern "C" int64_t ncde_stream_field_hermite_workspace_bytes(const NcdeProblem* p) { return stream_query(kFieldHermite, p); }
extern "C" const char* ncde_stream_field_hermite_kernel_name(const NcdeProblem* p) { return stream_name(kFieldHermite, p); }
extern "C" int ncde_stream_step_field_hermite(const NcdeProblem* p, const NcdeStream* s, void* stream) { return stream_launch(kFieldHermite, p, s, stream); }

extern "C" int64_t ncde_stream_lowrank_workspace_bytes(const NcdeProblem* p) { return stream_query(kLowrank, p); }
extern "C" const char* ncde_stream_lowrank_kernel_name(const NcdeProblem* p) { return stream_name(kLowrank, p); }
extern "C" int ncde_stream_step_lowrank(const NcdeProblem* p, const NcdeStream* s, void* stream) { return stream_launch(kLowrank, p, s, stream); }

// the hybrid steps: the per-channel mask as an extra argument; NcdeProblem and NcdeStream as they are
extern "C" int64_t ncde_stream_hybrid_workspace_bytes(const NcdeProblem* p) { return stream_query(kStepHybrid, p); }
extern "C" const char* ncde_stream_hybrid_kernel_name(const NcdeProblem* p) { return stream_name(kStepHybrid, p); }
extern "C" int ncde_stream_step_hybrid(const NcdeProblem* p, const NcdeStream* s, const unsigned char* rectilinear_mask, void* stream) {
    return stream_launch(kStepHybrid, p, s, stream, rectilinear_mask);
}
extern "C" int64_t ncde_stream_field_hybrid_workspace_bytes(const NcdeProblem* p) { return stream_query(kFieldHybrid, p); }
extern "C" const char* ncde_stream_field_hybrid_kernel_name(const NcdeProblem* p) { return stream_name(kFieldHybrid, p); }
extern "C" int ncde_stream_step_field_hybrid(const NcdeProblem* p, const NcdeStream* s, const unsigned char* rectilinear_mask, void* stream) {
    return stream_launch(kFieldHybrid, p, s, stream, rectilinear_mask);
}
extern "C" int64_t ncde_stream_lowrank_hybrid_workspace_bytes(const NcdeProblem* p) { return stream_query(kLowrankHybrid, p); }
extern "C" const char* ncde_stream_lowrank_hybrid_kernel_name(const NcdeProblem* p) { return stream_name(kLowrankHybrid, p); }
extern "C" int ncde_stream_step_lowrank_hybrid(const NcdeProblem* p, const NcdeStream* s, const unsigned char* rectilinear_mask, void* stream) {
    return stream_launch(kLowrankHybrid, p, s, stream, rectilinear_mask);
}

// the stacked step
extern "C" int64_t ncde_stream_stack_workspace_bytes(const NcdeProblem* const* p, int n_stack) { return stream_stack_query(p, n_stack); }
extern "C" const char* ncde_stream_stack_kernel_name(const NcdeProblem* const* p, int n_stack) {
    return stream_stack_query(p, n_stack) == NCDE_OK ? "ncde_stream_stack_step" : nullptr;
}
extern "C" int ncde_stream_stack_step(const NcdeProblem* const* p, const NcdeStream* const* s, int n_stack, void* stream) {
    NcdeProblem q[NCDE_STREAM_MAX_STACK];
    Layout y[NCDE_STREAM_MAX_STACK];
    size_t lds;
    const int rc = stream_stack_problems(p, n_stack, q, y, &lds);
    if (rc != NCDE_OK) return rc;
    if (!s) return sfail(NCDE_ERR_INVALID, "the list of streams is NULL");
    for (int i = 0; i < n_stack; ++i)
        if (!s[i]) return sfail(NCDE_ERR_INVALID, "stacked online step: stream %d is NULL", i);
    const NcdeStream* s0 = s[0];
    if (s0->n_rows < 1) return sfail(NCDE_ERR_INVALID, "n_rows %d: at least one new row", s0->n_rows);
    if (s0->rectilinear) return sfail(NCDE_ERR_INVALID, "stacked online step: rectilinear must be 0 (a layer's hidden sequence is a linear path)");
    if (!s0->x) return sfail(NCDE_ERR_INVALID, "NULL x");
    if (s0->x_stride_b < q[0].channels || s0->x_stride_m < 0)
        return sfail(NCDE_ERR_INVALID, "x strides (%lld, %lld): rows of %d channels", (long long)s0->x_stride_m, (long long)s0->x_stride_b, q[0].channels);
    StreamStackArgs k;
    memset(&k, 0, sizeof(k));
    k.n_stack = n_stack;
    for (int i = 0; i < n_stack; ++i) {
        const NcdeStream* si = s[i];
        if (!si->z || !si->last_row || !si->prev_dx || !si->count) return sfail(NCDE_ERR_INVALID, "layer %d: NULL z / last_row / prev_dx / count", i);
        const bool last = i == n_stack - 1;
        if (si->Wf ? (si->n_out < 1 || !si->out) : (last && !si->z_out))
            return sfail(NCDE_ERR_INVALID, "layer %d readout: Wf needs n_out >= 1 and out; the last layer without Wf needs z_out", i);
        fill_kargs(&q[i], y[i], &k.a[i]);
        k.q[i] = stream_args(s0, si, 0, 0, nullptr);
    }
    if (ncde_lds_optin((const void*)ncde_stream_stack_step_kernel, lds) != hipSuccess) return sfail(NCDE_ERR_HIP, "LDS opt-in of %zu B failed", lds);
    hipLaunchKernelGGL(ncde_stream_stack_step_kernel, dim3(y[0].n_wg), dim3(GEN_THREADS), lds, (hipStream_t)stream, k);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return sfail(NCDE_ERR_HIP, "ncde_stream_stack_step launch failed: %s", hipGetErrorString(e));
    return NCDE_OK;
}
