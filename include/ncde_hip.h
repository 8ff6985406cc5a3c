/*
 * ncde_hip.h -- C-ABI of libncde_hip.so, the MI355X (gfx950) Neural-CDE fixed-step integrator.
 *
 * The reference (jambo6/online-neural-cdes) has no FFI layer: its hot path is two Python callables,
 *   torchcde.cdeint(X, func, z0, t, adjoint=True, ...)        modules/torchcde/torchcde/solver.py:140-238
 *   NeuralCDE.forward(inputs)                                  src/ncde/ncde.py:214-243
 * which expand to the Python time loop of torchdiffeq's FixedGridODESolver.integrate
 * (modules/torchdiffeq/torchdiffeq/_impl/solvers.py:94-119) and, for the backward pass,
 * OdeintAdjointMethod.backward (modules/torchdiffeq/torchdiffeq/_impl/adjoint.py:37-145).
 * The entry points below are what a maintainer of the reference would bind (ctypes, see
 * INTEGRATION.md) to replace exactly those two loops.
 *
 * Conventions
 *   - every pointer inside NcdeProblem is a DEVICE pointer to fp32 data owned by the caller;
 *   - the library is stateless and re-entrant; work is enqueued on `stream` (a hipStream_t, NULL =
 *     default stream) and the calls never synchronise and never allocate;
 *   - scratch memory is passed in: ask ncde_workspace_bytes(), hand over `workspace` (per-workgroup gradient partials; for the
 *     specialised kernels also one range-fault word per 16-sample tile -- they multiply in 2-way split-fp16 and re-execute a tile
 *     in 3-way split-bf16, with a second launch on the same stream, when its operands leave the fp16 range: NCDE_FLAG_SPLIT_BF16);
 *   - return value 0 = success, negative = NcdeStatus; ncde_last_error_string() describes the last
 *     failure of the calling thread.  Nothing throws across the boundary.
 */
#ifndef NCDE_HIP_H
#define NCDE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NCDE_ABI_VERSION 4 /* version-1 structs (no trailing field_kind .. br members) and version-2 structs (no trailing
                              time_plan .. members) are still accepted */
#define NCDE_MAX_LAYERS 8

typedef enum NcdeStatus {
    NCDE_OK = 0,
    NCDE_ERR_INVALID = -1,      /* malformed problem (maps to ValueError / AssertionError in Python)    */
    NCDE_ERR_UNSUPPORTED = -2,  /* well-formed but outside what the kernels cover                      */
    NCDE_ERR_WORKSPACE = -3,    /* workspace too small                                                 */
    NCDE_ERR_HIP = -4           /* a HIP runtime call failed (launch error, no device, ...)            */
} NcdeStatus;

/* control-path evaluator: replaces LinearInterpolation.derivative (interpolation_linear.py:212-234)
 * and NaturalCubicSpline.derivative (interpolation_cubic.py:315-336) on the default integer grid.
 * NCDE_INTERP_QUINTIC is a general piecewise-quintic control (any knot grid through the time plan): the representation of
 * SmoothLinearInterpolation with match_second_derivatives=True (src/ncde/interpolation.py:6-123) on its refined knot grid
 * (ncde_prepare_smooth).  It runs on the batch-tiled, generic and variant families only: NCDE_FLAG_FORCE_FAST and the
 * ncde_dopri5_* entry points answer NCDE_ERR_UNSUPPORTED for it. */
typedef enum NcdeInterp { NCDE_INTERP_LINEAR = 0, NCDE_INTERP_CUBIC = 1, NCDE_INTERP_QUINTIC = 2 } NcdeInterp;

/* fixed-step solver: replaces Euler / Midpoint / RK4 (3/8 rule) of fixed_grid.py:6-29,
 * rk_common.py:106-114 with options={'step_size': 1}. */
typedef enum NcdeMethod { NCDE_EULER = 0, NCDE_MIDPOINT = 1, NCDE_RK4_38 = 2 } NcdeMethod;

/* which times the solution is reported at: t = X.interval (2 outputs: z(0), z(T-1)) or
 * t = X.grid_points (every knot), the two cases src/ncde/ncde.py:219-225 uses on the default grid with step_size 1;
 * NCDE_OUT_TIMES = the general time axis (any increasing t, any step_size, user knot grids): needs a time plan. */
typedef enum NcdeOutput { NCDE_OUT_INTERVAL = 0, NCDE_OUT_KNOTS = 1, NCDE_OUT_TIMES = 2 } NcdeOutput;

/* kernel family selection (ncde_forward/ncde_adjoint `flags`) */
#define NCDE_FLAG_AUTO 0u
#define NCDE_FLAG_FORCE_GENERIC 1u  /* never use a shape-specialised kernel */
#define NCDE_FLAG_FORCE_FAST 2u     /* fail with NCDE_ERR_UNSUPPORTED if no specialised kernel fits */
#define NCDE_FLAG_FP32_MFMA 4u      /* specialised and batch-tiled kernels: plain fp32-input MFMA (and fp32 records) instead of the
                                       (default, fp32-equivalent) 3-way split-bf16 MFMA GEMMs */
#define NCDE_FLAG_ADJOINT_V1 8u     /* specialised adjoint: single-role kernel instead of the (default) chain+gradient
                                       wave-specialised one */
#define NCDE_FLAG_ADJOINT_V2 16u    /* specialised adjoint: chain+gradient kernel with an fp32-MFMA chain (default: split-bf16 chain) */
#define NCDE_FLAG_ADJOINT_V4 32u    /* specialised adjoint: decoupled y / cotangent waves (ncde_adj_fast4: y re-integration one stage ahead of
                                       the cotangent chain, split-bf16 dL/dx_L) instead of the (default, faster) chain+gradient kernel */
#define NCDE_FLAG_SPLIT_BF16 64u    /* specialised forward kernels: 3-way split-bf16 GEMMs (6 MFMAs per product, any operand magnitude) instead of
                                       the default 2-way split-fp16 ones (3 MFMAs per product; sample tiles whose operands leave the fp16 range
                                       are re-executed by the split-bf16 kernel, so results do not depend on this flag beyond fp32 round-off) */
#define NCDE_FLAG_ADJOINT_SPLIT_FP16 128u /* development builds (-DNCDE_DEV_KNOBS) only, ignored otherwise: split-fp16 GEMMs on the cotangent
                                       side of the specialised adjoint too (not reproducible run to run) */
#define NCDE_FLAG_DEBUG_PROFILE 0x100u /* development: instrumented kernel variant, cycle counters land in the workspace */
#define NCDE_FLAG_DENSE_CHANNELS 0x300u /* BOTH bits 0x100 and 0x200 (0x200 alone is an internal development switch; no single bit of `flags` is
                                          free): the register-resident adjoint (ncde_adj_fast3) runs every channel quad of the output layer on every stage.
                                          Default: a stage whose dX is zero in all channels >= 4 for the whole 16-sample tile -- the
                                          time-only pieces of a rectilinear path -- runs quad 0 only.  Same results up to the sign of a
                                          zero; the in-process reference of tests/test_zero_quad_skip.py.  Test it with
                                          (flags & NCDE_FLAG_DENSE_CHANNELS) == NCDE_FLAG_DENSE_CHANNELS; it is not NCDE_FLAG_DEBUG_PROFILE */
#define NCDE_FLAG_NO_COOP 0x400u       /* batch-tiled forward and backward: do not use the XCD-cooperative, weight-stationary output phase (round 5, large
                                          hidden sizes: workgroups of one launch exchange activations through L2 and spin on each other --
                                          it needs every workgroup resident, i.e. the GPU's CUs not held by another process's persistent kernel) */
#define NCDE_FLAG_COOP_FAULT_INJECT 0x800u /* verification (like the dopri5 replay): ONE workgroup of the first cooperative launch withholds its first
                                          arrival and the spin limit is shortened, so that launch gives up after ~1 ms: exercises the status word
                                          and the re-execution by the per-workgroup kernels (tests/test_gpu_parity.py); results must not change */
#define NCDE_FLAG_TILED_NS1 0x1000u    /* batch-tiled forward: force 1 / 2 / 4 sixteen-sample tiles per workgroup     */
#define NCDE_FLAG_TILED_NS2 0x2000u    /*   (default: the largest that still gives >= 256 workgroups)                 */
#define NCDE_FLAG_TILED_NS4 0x4000u
#define NCDE_FLAG_FORCE_TILED 0x8000u  /* use the batch-tiled family also where a shape-specialised kernel exists (default order:
                                          specialised, then batch-tiled wherever its shape constraints hold, then generic).
                                          Its backward keeps per-stage records for a WINDOW of steps only (sweep W steps, fold
                                          them into the output-layer gradient, reuse the record): workspace O(B H W), W sized to
                                          a 192 MB record budget (NCDE_FLAG_TILED_WINDOW_STEPS(n) overrides) */

#define NCDE_FLAG_TILED_WINDOW_STEPS(n) (((uint32_t)(n) & 0xFFu) << 16) /* batch-tiled backward: n (1..255) solver steps per time window
                                          instead of what the record budget allows (0 = budget).  The library reads no environment
                                          variable on any call path; development switches exist only in builds with -DNCDE_DEV_KNOBS */
#define NCDE_FLAG_FIELD_RANK(r) (((uint32_t)(r) & 0xFFu) << 24) /* NCDE_FIELD_LOWRANK: the rank R (1..channels) of the field, carried in the
                                          top byte of `flags`; ignored for every other field kind (existing callers pass 0) */

typedef struct NcdeProblem {
    int32_t abi_version;  /* = NCDE_ABI_VERSION */
    int32_t batch;        /* B */
    int32_t n_knots;      /* T: knots of the control path (linear: coeffs rows; cubic: rows + 1) */
    int32_t channels;     /* C: control channels incl. time */
    int32_t hidden;       /* H: state size */
    int32_t interp;       /* NcdeInterp */
    int32_t method;       /* NcdeMethod */
    int32_t output;       /* NcdeOutput */
    uint32_t flags;       /* NCDE_FLAG_* */

    /* vector field f_theta (src/ncde/vector_fields/base.py:64-69, 83-104):
     *   x_0 = z;  x_l = relu(W_l x_{l-1} + b_l), l = 1..n_layers;  M = tanh(Wo x_n + bo) viewed [H, C]
     * layer_W[l] is [layer_out[l], layer_in[l]] row-major (torch Linear layout); the same pointer may
     * appear in several slots (the reference shares ONE inner layer nl-1 times, base.py:66-68).
     * Wo is [H*C, layer_out[n_layers-1]] with row index h*C + c. */
    int32_t n_layers;
    int32_t layer_in[NCDE_MAX_LAYERS];
    int32_t layer_out[NCDE_MAX_LAYERS];
    const float* layer_W[NCDE_MAX_LAYERS];
    const float* layer_b[NCDE_MAX_LAYERS];
    const float* Wo;
    const float* bo;

    /* control-path coefficients, row-major, element strides:
     *   linear/rectilinear: coeffs[b][t][c], t < T           (linear_interpolation_coeffs output)
     *   cubic:              coeffs[b][p][4C] = a|b|2c|3d, p < T-1 (natural_cubic_coeffs output)
     *   quintic:            coeffs[b][p][6C] = a|b|2c|3d|4e|5f, p < T-1; with f = t - knot[p]:
     *                       dX/dt = b + f(2c + f(3d + f(4e + f 5f))),  X = a + f(b + f(2c/2 + f(3d/3 + f(4e/4 + f 5f/5))))
     * Stride contract (tests/test_strided_coeffs_gpu.py runs every kernel family on it): both strides count ELEMENTS (floats), the
     * channel stride is 1.  coeffs_stride_b is any value >= 0 -- 0 (one path shared by the batch) and values smaller than one sample
     * (overlapping samples) included; coeffs_stride_t is at least the row width (C, 4C, 6C), anything smaller is NCDE_ERR_INVALID.
     * The pointer needs the alignment of a float (4 bytes) only, rows need not be 16-byte aligned, and b * coeffs_stride_b +
     * t * coeffs_stride_t is formed in 64 bits: offsets up to 2^63 bytes.  Only rows t < T (p < T-1) of a sample are read.      */
    const float* coeffs;
    int64_t coeffs_stride_b;
    int64_t coeffs_stride_t;

    const float* z0; /* [B, H] contiguous */

    /* ---- ABI version 2: vector-field variants (read only when abi_version >= 2; version 1 = original / matmul) ----
     * field_kind  (src/ncde/vector_fields/gating.py:7-61)
     *   NCDE_FIELD_ORIGINAL  M = tanh(Wo hh + bo)
     *   NCDE_FIELD_MINIMAL   M = sigmoid(Wg hh + bg) * tanh(Wo hh + bo)
     *   NCDE_FIELD_GRU       M = sigmoid(Wg net(u) + bg) * tanh(Wo net(sigmoid(Wr u + br) * u) + bo)
     *   NCDE_FIELD_LOWRANK   M = tanh(P Q),  P = (Wo hh + bo) viewed [H, R],  Q = (Wg hh + bg) viewed [R, C]
     *                        (src/ncde/vector_fields/sparsity.py:33-55: Wo, bo = M_h, [H*R, last width] with row index h*R + r;
     *                        Wg, bg = M_o, [R*C, last width] with row index r*C + c; Wr, br unused).  The rank R travels in
     *                        flags (NCDE_FLAG_FIELD_RANK(R), 1 <= R <= channels); matmul input only.  Fixed-step solves only:
     *                        ncde_dopri5_* and ncde_backward_control answer NCDE_ERR_UNSUPPORTED, as do NCDE_FLAG_FORCE_FAST
     *                        and NCDE_FLAG_FORCE_TILED (the field has its own kernels, ncde_fwd_lowrank / ncde_adj_lowrank).
     * field_input (vector_field_type of cdeint, modules/torchcde/torchcde/solver.py:112-137)
     *   NCDE_INPUT_MATMUL      u = z;             heads have H*C rows, dz/dt = M[H,C] . dX/dt
     *   NCDE_INPUT_EVALUATE    u = [z, X(t)];     heads have H rows,   dz/dt = M        (layer_in[0] = H + C)
     *   NCDE_INPUT_DERIVATIVE  u = [z, dX/dt(t)]; heads have H rows,   dz/dt = M
     * Wg, bg: the sigmoid head (same shape as Wo, bo; low-rank: M_o, see above); Wr [d0, d0], br [d0]: the GRU reset net,
     * d0 = layer_in[0]. */
    int32_t field_kind;
    int32_t field_input;
    const float* Wg;
    const float* bg;
    const float* Wr;
    const float* br;

    /* ---- ABI version 3: general time axis (read only when abi_version >= 3 and output == NCDE_OUT_TIMES) ----
     * time_plan: DEVICE copy of the buffer ncde_time_plan_build() filled on the host; the three counts are the ones it
     * returned in NcdeTimePlanInfo.  The solution then has n_t_out rows per sample (row 0 = z0 = z(t[0])). */
    const void* time_plan;
    int32_t n_t_out;
    int32_t n_steps_fwd;
    int32_t n_steps_adj;
    int32_t reserved_;      /* padding; NOT an input -- the library ignores whatever the caller leaves here (it is zeroed on entry) */
} NcdeProblem;

typedef enum NcdeFieldKind { NCDE_FIELD_ORIGINAL = 0, NCDE_FIELD_MINIMAL = 1, NCDE_FIELD_GRU = 2, NCDE_FIELD_LOWRANK = 3 } NcdeFieldKind;
typedef enum NcdeFieldInput { NCDE_INPUT_MATMUL = 0, NCDE_INPUT_EVALUATE = 1, NCDE_INPUT_DERIVATIVE = 2 } NcdeFieldInput;

/* gradient outputs of the adjoint sweep; aliasing must mirror NcdeProblem.layer_W/layer_b
 * (a shared layer receives the SUM over its uses).  Buffers are overwritten, not accumulated. */
typedef struct NcdeGrads {
    float* grad_z0;                      /* [B, H] */
    float* grad_layer_W[NCDE_MAX_LAYERS];
    float* grad_layer_b[NCDE_MAX_LAYERS];
    float* grad_Wo;
    float* grad_bo;
    /* read only when the problem's abi_version >= 2 and the field kind has these parameters */
    float* grad_Wg;
    float* grad_bg;
    float* grad_Wr;
    float* grad_br;
} NcdeGrads;

/* General time axis of torchdiffeq's fixed-grid solvers, replacing
 *   the grid built from options['step_size']                     torchdiffeq/_impl/solvers.py:78-87
 *   the output pick / linear interpolation between grid states    solvers.py:103-117, 166-172
 *   user knot grids of the control path                           torchcde/interpolation_linear.py:186-202, interpolation_cubic.py:283-305
 *   one reverse solve per output interval on its own grid         torchdiffeq/_impl/adjoint.py:116-133
 * The caller describes the axis with HOST arrays; ncde_time_plan_build() (pure CPU code, exact torch arithmetic in the
 * dtype of t) turns it into a small table the kernels walk.  Copy the table to the device, point NcdeProblem.time_plan
 * at it, set output = NCDE_OUT_TIMES and the three counts from NcdeTimePlanInfo. */
typedef struct NcdeTimeSpec {
    int32_t n_t;          /* number of output times (>= 2); t[0] is where the solve starts (z0 = z(t[0])) */
    int32_t time_is_f64;  /* 0: the caller's t tensor is fp32 (grid arithmetic in fp32, as torch does); 1: fp64 */
    const double* t;      /* HOST, n_t strictly increasing values */
    double step_size;     /* options['step_size'] > 0 */
    const double* knots;  /* HOST, the n_knots knot times X was built on, or NULL = default integer grid 0..T-1 */
} NcdeTimeSpec;

typedef struct NcdeTimePlanInfo {
    int32_t n_t_out;      /* = n_t */
    int32_t n_steps_fwd;  /* solver steps of the forward solve */
    int32_t n_steps_adj;  /* solver steps of all reverse solves of the continuous adjoint */
    int32_t stages;       /* stages per step of the method */
    int64_t bytes;        /* size of the plan */
} NcdeTimePlanInfo;

/* host_buffer == NULL: only fills *info (sizes).  Uses p->method, p->n_knots. */
int ncde_time_plan_build(const NcdeProblem* p, const NcdeTimeSpec* ts, void* host_buffer, size_t bytes, NcdeTimePlanInfo* info);

/* ---- adaptive Dormand-Prince 5(4): method='dopri5' of torchdiffeq (the default method of cdeint; NeuralCDE(solver="dopri5")
 * passes options {'min_step': 0.5}, src/ncde/ncde.py:130-134).  Replaces Dopri5Solver / RKAdaptiveStepsizeODESolver
 * (torchdiffeq/_impl/dopri5.py:5-36, rk_common.py:117-313, misc.py:33-103, interp.py) and, for the backward pass, the
 * per-interval adaptive solves of OdeintAdjointMethod.backward over (vjp_t, y, a, g_theta) with the mixed error norm
 * (adjoint.py:37-145, 235-247).  The error norm is over the WHOLE batch (one accept / reject per attempt), the time is kept
 * in fp64 on the device.  These two calls DO synchronise the stream (the number of attempts is data dependent).
 * p->method and p->output are ignored; the solution has ts->n_t rows per sample (row 0 = z0 = z(t[0])); ts->step_size is
 * ignored.  Original field with the matmul input only. */
typedef struct NcdeAdaptiveOptions {
    double rtol, atol;      /* cdeint defaults: 1e-4, 1e-6 (torchcde/solver.py:193-196) */
    double min_step;        /* options['min_step'], default 0 */
    double max_step;        /* options['max_step'], 0 = infinity */
    double first_step;      /* options['first_step'], 0 = select automatically (misc.py:33-74) */
    double safety, ifactor, dfactor; /* 0 = the reference's defaults 0.9, 10, 0.2 */
    int32_t max_num_steps;  /* 0 = 2^31 - 1 */
    int32_t trace_capacity; /* diagnostics: number of attempts `trace` has room for (0 = none) */
    double* trace;          /* HOST buffer of trace_capacity x 4 doubles, filled after the solve with one row per attempt:
                               t0, dt, accepted (0/1), error ratio -- the step sequence, for comparison with the reference's */
    /* ---- read only when the problem's abi_version >= 4 ----
     * Replay of a recorded step sequence (verification): attempt i (counted over the whole call, all output intervals of an adjoint
     * solve included) takes dt = replay[2 i] and is accepted iff replay[2 i + 1] != 0 instead of what the controller would decide;
     * attempts beyond replay_count run free.  With the reference's own sequence (tests/golden/g10, g12: `trace_fwd` / `trace_bwd`)
     * the solve does the reference's arithmetic step for step, so the comparison with its outputs is tight instead of
     * solver-tolerance level. */
    int32_t replay_count;
    int32_t reserved_;
    const double* replay;   /* HOST, replay_count x 2 doubles */
} NcdeAdaptiveOptions;

typedef struct NcdeAdaptiveStats {
    int32_t nfe;            /* vector-field evaluations, as the reference's func.nfe counts them (base.py:90) */
    int32_t n_accepted, n_rejected;
    int32_t reserved_;
} NcdeAdaptiveStats;

int64_t ncde_dopri5_workspace_bytes(const NcdeProblem* p, const NcdeTimeSpec* ts, int pass /* 0 forward, 1 adjoint, 2 taped backward */);
/* Which kernels a dopri5 call of this problem runs (static string; NULL + last error if the problem is not supported): the fused
 * attempt kernels of round 4 -- one launch per attempt for the forward solve ("ncde_dpf_fwd<...>": hidden, hidden_hidden <= 32 with
 * C <= 20, or <= 64 with C <= 4), an attempt + a reduce launch for the adjoint ("ncde_dpf_adj<...> + ncde_dpf_reduce") and the persistent
 * reverse sweep of a taped solve ("ncde_dpf_tape<...>"; both: the (32, 32, 20) set, <= 3 layers -- a fourth layer's LDS images do
 * not fit 160 KB, so the library caps n_layers at 3 there) -- or the per-launch kernels
 * ("ncde_dp_stage x 6 + ncde_dp_control + ncde_dp_commit", "ncde_dp_tape_backward") for every other shape and under
 * NCDE_FLAG_FORCE_GENERIC. */
const char* ncde_dopri5_kernel_name(const NcdeProblem* p, int pass /* 0 forward, 1 adjoint, 2 taped backward */);
int ncde_dopri5_forward(const NcdeProblem* p, const NcdeTimeSpec* ts, const NcdeAdaptiveOptions* opt, float* out, void* workspace,
                        size_t workspace_bytes, void* stream, NcdeAdaptiveStats* stats);
int ncde_dopri5_adjoint(const NcdeProblem* p, const NcdeTimeSpec* ts, const NcdeAdaptiveOptions* opt, const float* z_out,
                        const float* grad_out, const NcdeGrads* grads, void* workspace, size_t workspace_bytes, void* stream,
                        NcdeAdaptiveStats* stats);

/* dopri5 with adjoint=False -- how the reference's shipped "interpolation" experiments run it (experiments/configurations/
 * configurations.json5:187-191 -> torchdiffeq.odeint under autograd, torchcde/solver.py:224-225).  Replaces the autograd tape of
 * RKAdaptiveStepsizeODESolver (rk_common.py:216-305): ncde_dopri5_forward_record is ncde_dopri5_forward that also keeps, per ACCEPTED
 * step, (t0, dt, the state at its start, the outputs interpolated in it) in a caller-owned device record; ncde_dopri5_backward is the
 * exact reverse-mode sweep over that record -- six stage VJPs per step with FSAL, the transpose of the 4th-order dense output
 * (interp.py:4-61), and the gradient of the FIRST step size through _select_initial_step (misc.py:33-74; every later step size is a
 * constant because _optimal_step_size is @torch.no_grad(), misc.py:84-97).  The backward first reads the record's 64-byte header back
 * (step count, overflow flag: one small copy + stream synchronisation; a second one uploads a user knot grid), then enqueues one
 * persistent launch + two small ones + the partial reduction; the forward synchronises like ncde_dopri5_forward.
 * Limits of the taped path (checked by ncde_dopri5_record_bytes / _forward_record, NCDE_ERR_UNSUPPORTED): hidden <= 128, last
 * hidden width <= 128, the reverse sweep's 7 [H][16] LDS arrays within 160 KB.
 * Record size: ncde_dopri5_record_bytes() is enough for every solve with options.min_step > 0 (never more than max_num_steps per
 * output interval); without a minimum step it is an estimate (about two steps per knot) that a solve can exceed: it then returns
 * NCDE_ERR_WORKSPACE ("pass a larger record") and may simply be repeated with a larger one (the Python host doubles it).  Workspace of the backward:
 * ncde_dopri5_workspace_bytes(p, ts, 2). */
int64_t ncde_dopri5_record_bytes(const NcdeProblem* p, const NcdeTimeSpec* ts, const NcdeAdaptiveOptions* opt);
int ncde_dopri5_forward_record(const NcdeProblem* p, const NcdeTimeSpec* ts, const NcdeAdaptiveOptions* opt, float* out, void* record,
                               size_t record_bytes, void* workspace, size_t workspace_bytes, void* stream, NcdeAdaptiveStats* stats);
int ncde_dopri5_backward(const NcdeProblem* p, const NcdeTimeSpec* ts, const NcdeAdaptiveOptions* opt, const void* record,
                         size_t record_bytes, const float* grad_out, const NcdeGrads* grads, void* workspace, size_t workspace_bytes,
                         void* stream);

int ncde_version(void);
const char* ncde_last_error_string(void);

/* number of solution rows per sample: 2 (interval) or T (knots) */
int ncde_num_outputs(const NcdeProblem* p);

/* scratch bytes needed by ncde_forward[_record] (pass = 0) / ncde_adjoint (pass = 1) / ncde_backward (pass = 2);
 * negative = NcdeStatus */
int64_t ncde_workspace_bytes(const NcdeProblem* p, int pass);

/* The XCD-cooperative kernels of the batch-tiled family (large hidden sizes) spin on each other and therefore carry a bounded wait: a
 * launch whose workgroups never all became resident (another process's persistent kernel, a CU mask) GIVES UP, and the per-workgroup
 * kernels the library always enqueues behind it re-execute the pass -- the caller's outputs are correct either way, only late.  That it
 * happened is recorded in a STATUS WORD inside the caller's workspace: uint32 at byte offset ncde_coop_status_offset(p, pass), zeroed
 * by the call, 1 after a cooperative launch of that call gave up.  Read it after the stream has finished the call (it is the caller's
 * memory; the library never synchronises); a caller that sees 1 should pass NCDE_FLAG_NO_COOP from then on (the Python host does).
 * Returns NCDE_ERR_UNSUPPORTED (-2) when the problem / pass launches nothing cooperative. */
int64_t ncde_coop_status_offset(const NcdeProblem* p, int pass);

/* name of the kernel family the call would dispatch to ("generic", "fast_h32_c20", ...); NULL on error */
const char* ncde_kernel_name(const NcdeProblem* p, int pass);

/* Forward solve.  out: [B, n_out, H]; row 0 is z0, then the solution at the requested times.
 * Replaces odeint(...)/FixedGridODESolver.integrate under torch.no_grad (adjoint.py:24-33). */
int ncde_forward(const NcdeProblem* p, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* Continuous-adjoint reverse sweep (adjoint.py:37-145): given the forward outputs z_out [B,n_out,H]
 * and dL/dz_out grad_out [B,n_out,H], writes dL/dz0 and dL/dtheta. */
int ncde_adjoint(const NcdeProblem* p, const float* z_out, const float* grad_out, const NcdeGrads* grads,
                 void* workspace, size_t workspace_bytes, void* stream);

/* ---- exact backward of the DISCRETISED solve: what cdeint(..., adjoint=False) + autograd computes in the reference
 * (modules/torchcde/torchcde/solver.py:224 picks torchdiffeq.odeint; autograd then tapes solvers.py:94-119 and
 * fixed_grid.py:6-29 / rk_common.py:106-114).  Instead of a tape, the forward records every stage input
 * ("stage record", [(T-1)*stages][B][H] fp32, caller-owned, ncde_stage_record_bytes() bytes) and the backward
 * transposes the solve stage by stage, re-evaluating f_theta at the recorded inputs.
 *   ncde_forward_record  = ncde_forward + the stage record
 *   ncde_backward        : stage record + dL/dz_out -> dL/dz0, dL/dtheta   (workspace: ncde_workspace_bytes(p, 2)) */
int64_t ncde_stage_record_bytes(const NcdeProblem* p);
int ncde_forward_record(const NcdeProblem* p, float* out, float* stages, void* workspace, size_t workspace_bytes, void* stream);
int ncde_backward(const NcdeProblem* p, const float* stages, const float* grad_out, const NcdeGrads* grads, void* workspace,
                  size_t workspace_bytes, void* stream);

/* ---- gradient of the control path: what adjoint=False + autograd hands to a coefficient tensor that requires grad (a stacked CDE
 * feeds layer i's hidden sequence to layer i+1 as linear coefficients, src/ncde/stacked.py:7-131).  ncde_backward_control is
 * ncde_backward that ALSO writes dL/dcoeffs: per recorded stage g[b, c] = sum_h cot[b, h] M[b, h, c] (M = tanh(Wo x_L + bo), cot = the
 * stage cotangent the sweep already forms) is computed from the sweep's records by ncde_dctl_tiled -- fp32-input MFMA, one workgroup per
 * stage and 16-sample tile -- and folded by ncde_dctl_fold onto the coefficient rows the stage read (linear: +-g / knot spacing into rows
 * idx + 1 / idx;  cubic: g, g frac, g frac^2 into b, 2c, 3d).  No float atomics: grad_coeffs is bit-reproducible.
 *   stages      the record of ncde_forward_record (its layout does not depend on the kernel family: the forward keeps its usual route)
 *   grad_coeffs dense, shaped like the coefficients ([B, T, C] linear, [B, T-1, 4C] cubic), fully written
 *   grads       receives what ncde_backward writes
 * The call always runs the batch-tiled family's per-workgroup kernels over fp32 records, zero-padded like any shape -- exactly
 * ncde_backward with flags = NCDE_FLAG_FORCE_TILED | NCDE_FLAG_FP32_MFMA | NCDE_FLAG_NO_COOP (of the caller's flags only
 * NCDE_FLAG_TILED_WINDOW_STEPS(n) is kept), then pass C per time window.  Supported: original field, matmul input, NCDE_INTERP_LINEAR /
 * _CUBIC, every method / output mode / time plan.  Gated fields, evaluate / derivative inputs, the quintic kind and shapes beyond the
 * batch-tiled backward answer NCDE_ERR_UNSUPPORTED. */
int64_t ncde_control_workspace_bytes(const NcdeProblem* p);   /* < 0: status code */
const char* ncde_control_kernel_name(const NcdeProblem* p);   /* NULL on error */
int ncde_backward_control(const NcdeProblem* p, const float* stages, const float* grad_out, const NcdeGrads* grads, float* grad_coeffs,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Timing helper for benchmarks: runs `iters` back-to-back launches of the dominant kernel of the given
 * pass on `stream`, bracketed by HIP events on that same stream, and returns the mean milliseconds per
 * launch in *ms_per_launch (this call DOES synchronise).  pass = 1: `out` is z_out; pass = 2: `out` is the stage record. */
int ncde_time_kernel(const NcdeProblem* p, int pass, float* out, const float* grad_out, const NcdeGrads* grads,
                     void* workspace, size_t workspace_bytes, void* stream, int iters, float* ms_per_launch);

/* ---- control-path coefficient construction on the GPU (the step right before the hot path) ----------------
 * Default integer time grid, fp32.  x: [B, L, C] raw series (NaN = missing), device pointers.
 * ncde_prepare_linear   replaces torchcde.linear_interpolation_coeffs (interpolation_linear.py:131-180):
 *                       rectilinear_time_index >= 0 -> rectilinear preparation (out [B, 2L-1, C]), else plain
 *                       NaN-filled linear knots (out [B, L, C]).
 * ncde_prepare_cubic    replaces torchcde.natural_cubic_coeffs (interpolation_cubic.py:7-165, 170-190; NaN = missing:
 *                       ends filled from the first/last observation, spline through the observed knots):
 *                       out [B, L-1, 4C] = a|b|2c|3d.
 * kind = NcdeInterp for the workspace query. */
int64_t ncde_prepare_workspace_bytes(int kind, int B, int L, int C);
int ncde_prepare_linear(const float* x, int B, int L, int C, int rectilinear_time_index, float* out, void* stream);
int ncde_prepare_cubic(const float* x, int B, int L, int C, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* The same builders with the observations on a USER time grid (the t= argument of torchcde.linear_interpolation_coeffs /
 * natural_cubic_coeffs: interpolation_linear.py:131-180, interpolation_cubic.py:56-165): t = DEVICE pointer to L strictly
 * increasing fp32 times, NULL = the integer grid.  Linear: the grid enters the interior-gap fill only (ignored by the rectilinear
 * preparation, whose output the caller pairs with a grid of 2L-1 times).  Cubic: non-uniform natural spline. */
int ncde_prepare_linear_grid(const float* x, const float* t, int B, int L, int C, int rectilinear_time_index, float* out, void* stream);
int ncde_prepare_cubic_grid(const float* x, const float* t, int B, int L, int C, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* Which kernel a builder call with these arguments launches (host-side query, no GPU work; the launch reads the same decision):
 * kind = NCDE_INTERP_LINEAR -> "ncde_linear_coeffs_lds" (one workgroup per sample, the series staged in LDS) or "ncde_linear_coeffs"
 * (one thread per series on global memory);  NCDE_INTERP_CUBIC -> "ncde_cubic_coeffs_lds<nsmp=N>" (N samples per workgroup in LDS;
 * a workgroup that meets a NaN runs the per-series routine) or "ncde_cubic_coeffs" (one thread per series on global memory).
 * has_grid != 0: a user time grid is passed.  rectilinear_time_index: as for ncde_prepare_linear (ignored for the spline).
 * NULL for arguments the builders refuse.  The string lives in thread-local storage until the next call. */
const char* ncde_prepare_kernel_name(int kind, int B, int L, int C, int has_grid, int rectilinear_time_index);

/* Hermite cubic with backward differences (upstream torchcde's hermite_cubic_coefficients_with_backward_differences): a smooth path
 * whose piece on [t_i, t_i+1] reads knots i-1, i, i+1 only.  knots [B, L, C]: the LINEAR knots (ncde_prepare_linear_grid's output:
 * no NaN left; built with both causal options, knot k sees x[:k+1] only).  t: DEVICE pointer to L strictly increasing fp32 times,
 * NULL = the integer grid (h = 1).  out [B, L-1, 4C] = a|b|2c|3d, an NCDE_INTERP_CUBIC tensor.  Per piece i and channel, in fp32 and
 * in this operation order, with h = t[i+1] - t[i], d_i = (knots[i+1] - knots[i]) / h and dprev = d_{i-1} (d_0 for i = 0):
 *   a = knots[i];  b = dprev;  2c = 2 * (3 * ((knots[i+1] - knots[i]) / h - b) - d_i + dprev) / h;  3d = (1 / h^2) * (d_i - b) - 2c / h
 * The first piece is linear: its 2c and 3d are exactly zero.  One launch on `stream`, one thread per (piece, channel) looping over the
 * four parts, every element of `out` written; no workspace, no atomics, bit-reproducible.  Bad arguments NCDE_ERR_INVALID.
 * ncde_prepare_hermite_kernel_name: "ncde_hermite_coeffs", or NULL for arguments the builder refuses. */
int ncde_prepare_hermite(const float* knots, const float* t, int B, int L, int C, float* out, void* stream);
const char* ncde_prepare_hermite_kernel_name(int B, int L, int C);


/* Smoothed-linear control paths (SmoothLinearInterpolation, src/ncde/interpolation.py:6-123: cubic / quintic matching of the
 * slopes in (k, k + eps) after every interior knot k of the integer grid) as a piecewise polynomial on the REFINED knot grid
 * 0, 1, 1+eps, 2, 2+eps, ..., T-2, T-2+eps, T-1  (eps < 1: P = 2T-3 pieces;  eps == 1: the integer grid, P = T-1 pieces).
 * x: linear coefficients [B, T, C] (device, contiguous), order 3 -> out [B, P, 4C] = a|b|2c|3d (an NCDE_INTERP_CUBIC tensor),
 * order 5 -> out [B, P, 6C] = a|b|2c|3d|4e|5f (NCDE_INTERP_QUINTIC).  One launch on `stream`, no workspace; the matching
 * coefficients are evaluated in fp32 in the operation order of _setup_cubic / _setup_quintic_matching_coefficients.
 * Pieces outside a matching region are the linear piece (higher parts zero).  ncde_smooth_pieces: P, or < 0 for bad arguments. */
int ncde_smooth_pieces(int T, double eps);
int ncde_prepare_smooth(const float* x, int B, int T, int C, double eps, int order, float* out, void* stream);

/* Transpose of ncde_prepare_smooth for cubic matching: what autograd hands back to the linear coefficients through
 * _setup_cubic_matching_coefficients (src/ncde/interpolation.py:146-158) when a SmoothLinearInterpolation is built on a tensor that
 * requires grad and the solve is taped (adjoint=False).  The builder is linear in x with weights that depend on eps only
 * (2c = (4 / eps) jump, 3d = (-3 / eps^2) jump, jump = x[k+1] - 2 x[k] + x[k-1]; the linear rest starts at x[k] + eps (x[k+1] - x[k])).
 *   grad_rows [B, P, 4C], P = ncde_smooth_pieces(T, eps): dL/d(a | b | 2c | 3d) of every piece (e.g. grad_coeffs of ncde_backward_control)
 *   grad_x    [B, T, C], written completely
 * One launch on `stream`, one thread per element of grad_x summing the at most 5 pieces that read that knot in a fixed order: no
 * atomics, no workspace, bit-reproducible.  order 3 only: order 5 answers NCDE_ERR_UNSUPPORTED (ncde_last_error_string() says so);
 * other bad arguments NCDE_ERR_INVALID, as for ncde_prepare_smooth. */
int ncde_prepare_smooth_backward(const float* grad_rows, int B, int T, int C, double eps, int order, float* grad_x, void* stream);

/* ---- causal (online) control paths: a prediction at t_k may only see observations up to t_k ---------------------------------
 * ncde_prepare_fill: the two fill arguments of the reference's torchcde.linear_interpolation_coeffs (interpolation_linear.py:159-173)
 * and misc.forward_fill (misc.py:103-126).  x, out: [B, L, C] fp32 device, contiguous, x != out; L >= 1.
 *   has_initial != 0  NaNs of the first time row become (float)initial_value           (initial_value_if_nan)
 *   forward_fill != 0 then every channel is filled forward along time; NaNs in front of a channel's first observation stay NaN
 * Values are copied, never computed.  One workgroup per sample, one launch on `stream`, `out` written completely. */
int ncde_prepare_fill(const float* x, int B, int L, int C, int has_initial, double initial_value, int forward_fill, float* out, void* stream);

/* The linear / rectilinear hybrid scheme (src/ncde/interpolation.py:191-253; time is channel 0): linear channels move with time,
 * rectilinear channels step, and a knot is added only where a rectilinear channel changes.  The full table of a sample has 2L-1
 * rows,  row 2i = (t_i, lin_i, rect_i),  row 2i+1 = (t_{i+1}, lin_{i+1}, rect_i);  row 0 is kept, any other row iff its time or
 * one of its rectilinear values differs (!=) from the row before it; kept rows are packed to the front; a sample shorter than T
 * repeats its last kept row.
 *   x_filled   [B, L, C]: time in channel 0 and the rectilinear channels after ncde_prepare_fill(has_initial, 0.0, forward_fill)
 *              (no NaN left in them; the other channels are not read)
 *   x_linear   [B, L, NL], NL = C - 1 - n_rect: the linear channels in ascending channel order, NaN filled (ncde_prepare_fill with
 *              initial value 0.0, then ncde_prepare_linear on the gathered channels); not read (may be NULL) when NL == 0
 *   rect_idx   DEVICE pointer to n_rect distinct int32 channel indices in [1, C) (NULL when n_rect == 0); the caller validates
 *              them, an index outside [1, C) is ignored by the kernels
 * ncde_prepare_hybrid_count (pass 1): keep flag of every row, exclusive prefix sum per sample (wave scan, carried across the waves
 *   and across chunks of 256 rows) -> row positions in `workspace`, lengths[b] = kept rows of sample b (int32 device, [B]), and
 *   *max_len = max_b lengths[b] (int32 device): the ONE value the host has to read to size the output (T = *max_len).
 * ncde_prepare_hybrid_write (pass 2): out [B, T, C], every element written (kept rows scattered to their positions, rows
 *   lengths[b] .. T-1 = the last kept row).  `workspace` and `lengths` as pass 1 left them, lengths[b] <= T <= 2L-1.
 * Both: launches on `stream` only, no atomics, bit-reproducible.  Workspace: ncde_prepare_hybrid_workspace_bytes(B, L, C).
 * Bad arguments NCDE_ERR_INVALID (also a sample of 2^31 elements or more), a workspace too small NCDE_ERR_WORKSPACE. */
int64_t ncde_prepare_hybrid_workspace_bytes(int B, int L, int C);
int ncde_prepare_hybrid_count(const float* x_filled, int B, int L, int C, const int* rect_idx, int n_rect, void* workspace,
                              size_t workspace_bytes, int* lengths, int* max_len, void* stream);
int ncde_prepare_hybrid_write(const float* x_filled, const float* x_linear, int B, int L, int C, int n_rect, const void* workspace,
                              size_t workspace_bytes, const int* lengths, int T, float* out, void* stream);

/* ---- online inference: carry the CDE state of B independent streams from one observation to the next --------------------------
 * What a served model needs instead of NeuralCDE(return_sequences=True) on the whole prefix (src/ncde/ncde.py:214-243): after the
 * k-th observation the state z equals row 2k (rectilinear) / row k (linear) of the batch solve on t = X.grid_points with
 * step_size 1, at the cost of the one or two solver steps the new observation adds.
 *   fill       NaN = not observed.  NaNs of a stream's FIRST row become initial_value_if_nan, later NaNs the stream's last filled
 *              value: linear_interpolation_coeffs(x, rectilinear=time_index, initial_value_if_nan=v) for a rectilinear stream,
 *              linear_interpolation_coeffs(x, initial_value_if_nan=v, forward_fill=True) for a linear one
 *              (interpolation_linear.py:159-173).  Values are copied, never computed; the time channel is never NaN.
 *   pieces     linear: one piece per observation;  rectilinear: two (first only the time channel moves, then only the values).
 *   solve      one step of p->method per piece; stage 1 of a step reads the piece to the LEFT of its knot -- the previous piece, or
 *              the step's own piece at a stream's very first step (interpolation_linear.py:212-219) -- every later stage its own.
 *   state      z [B, H], last_row [B, C] (the last filled row), prev_dx [B, C] (dX/dt of the last piece), count [B] int32
 *              (observations received).  A stream's first row (count == 0) initialises it: the row is filled and kept, count
 *              becomes 1, z is left as the caller set it (z(t0): the read-in layer of the model) and no solver step is taken.
 *   active     uint8 [n_rows, B] or NULL = every stream receives every row.  A stream whose entry is 0 keeps its state untouched;
 *              its output row is the readout of its unchanged z.
 *   readout    out [n_rows, B, n_out] = Wf z + bf after each row (Wf [n_out, H] row-major, bf [n_out] or NULL);  Wf == NULL: no
 *              readout, z_out is then required.  z_out (optional) [n_rows, B, H]: z after each row.
 * The step reads of the problem: batch, channels, hidden, method and the vector field (original field, matmul input; interp must be
 * NCDE_INTERP_LINEAR) -- coeffs, z0, n_knots, output and the time plan are ignored.  ONE launch on `stream`, one workgroup per
 * 16 streams, no workspace, no atomics, no synchronisation; rows of one call are processed in order.  The caller owns every buffer.
 * ncde_stream_workspace_bytes: 0, or the status the step would answer for this problem (NCDE_ERR_UNSUPPORTED for a gated / low-rank
 * field, the evaluate / derivative inputs and shapes beyond the generic forward's LDS plan; NCDE_ERR_INVALID for a malformed
 * problem).  ncde_stream_kernel_name: "ncde_stream_step", or NULL on such a problem. */
typedef struct NcdeStream {
    int32_t n_rows;             /* m >= 1 new observation rows */
    int32_t rectilinear;        /* 0: linear stream, else rectilinear */
    int32_t time_index;         /* rectilinear: the time channel */
    int32_t n_out;              /* rows of Wf */
    const float* x;             /* x[r * x_stride_m + b * x_stride_b + c], element strides, channel stride 1 */
    int64_t x_stride_m;
    int64_t x_stride_b;         /* >= channels */
    const uint8_t* active;      /* [n_rows, B] or NULL */
    float initial_value_if_nan;
    int32_t reserved_;
    float* z;                   /* [B, H]  in / out */
    float* last_row;            /* [B, C]  in / out */
    float* prev_dx;             /* [B, C]  in / out */
    int32_t* count;             /* [B]     in / out */
    const float* Wf;
    const float* bf;
    float* out;
    float* z_out;
} NcdeStream;
int64_t ncde_stream_workspace_bytes(const NcdeProblem* p);   /* < 0: status code */
const char* ncde_stream_kernel_name(const NcdeProblem* p);   /* NULL on error */
int ncde_stream_step(const NcdeProblem* p, const NcdeStream* s, void* stream);

/* The same step on the Hermite cubic with backward differences (ncde_prepare_hermite on the integer grid, built with
 * initial_value_if_nan = v and forward_fill): the one cubic that is causal.  Same structs, same state; prev_dx holds the backward
 * difference of the last piece.  Per new row of a stream with count >= 1, elementwise per channel and in this operation order:
 *   dn = fill - last_row;  b = count == 1 ? dn : prev_dx;  two_c = 2 * (3 * (dn - b) - dn + b);  three_d = (dn - b) - two_c
 *   stage 1 sits on the knot and reads the piece to its left at frac = 1, which in exact arithmetic is b: the step reads b
 *   stage j > 1 reads b + (two_c + three_d * s_j) * s_j, s_j the stage's offset in the piece (the cubic branch of the batch kernels)
 *   then prev_dx = dn, last_row = fill, count += 1.  A stream's first row initialises it, as for ncde_stream_step.
 * The problem must say interp = NCDE_INTERP_CUBIC (the layout of the path's coefficients) and s->rectilinear must be 0.  The LDS
 * plan is that of ncde_stream_step (dn, b and ONE stage image rebuilt per stage take its three dX/dt slots), so the two queries
 * accept the same shapes; everything else stated for ncde_stream_step holds.  The kernel name is "ncde_stream_step_hermite". */
int64_t ncde_stream_hermite_workspace_bytes(const NcdeProblem* p);   /* < 0: status code */
const char* ncde_stream_hermite_kernel_name(const NcdeProblem* p);   /* NULL on error */
int ncde_stream_step_hermite(const NcdeProblem* p, const NcdeStream* s, void* stream);

/* The field step: the same step, same structs and same state for five further (field, input) pairs on linear and rectilinear
 * streams, with euler, midpoint or rk4 -- NCDE_FIELD_ORIGINAL with the evaluate / derivative input, NCDE_FIELD_MINIMAL with the
 * matmul / evaluate / derivative input.  The problem carries field_kind, field_input, Wg / bg for the gate, and for the direct
 * inputs a layer chain that starts at d0 = hidden + channels (layer_in[0], or the columns of Wo / Wg when n_layers == 0).
 *   matmul, derivative   the control input of a stage is the dX/dt of the left-piece rule above.
 *   evaluate             X at the stage time: stage 1 reads the row at the piece's first knot itself (the stream's last row before
 *                        this fill; the lagged row for the second rectilinear piece), stage j > 1 that row + frac_j * the piece's own
 *                        dX/dt, frac_j = (n + offset_j) - n in fp32 at the stream's own step index n = count - 1 (linear),
 *                        2 (count - 1) and 2 (count - 1) + 1 (rectilinear) -- the batch kernels' arithmetic.
 * Every weight is streamed from L2; results agree with a batch solve to rounding, not bit for bit (a batch solve that keeps
 * weights resident in LDS sums in another order).  NCDE_ERR_INVALID: what ncde_stream_step answers it for (a non-linear interp
 * among it), a NULL Wg / bg on a gated field, a layer chain that does not start at d0.  NCDE_ERR_UNSUPPORTED, each with a message:
 * the GRU-gated field, the low-rank field, the original field with the matmul input (ncde_stream_step's) and a shape whose LDS
 * plan, 4 (3 DS + 4 HS + 7 CS + 48) bytes with HS = 16 ru16(hidden), DS = 16 max(ru16(d0), ru16(hidden), ru16(layer widths)),
 * CS = 16 ru4(channels), exceeds 160 KiB (the message carries the bytes).  A refusal launches nothing and leaves every state
 * buffer untouched.  The kernel name is "ncde_stream_step_field". */
int64_t ncde_stream_field_workspace_bytes(const NcdeProblem* p);   /* 0, or < 0: status code */
const char* ncde_stream_field_kernel_name(const NcdeProblem* p);   /* NULL on error */
int ncde_stream_step_field(const NcdeProblem* p, const NcdeStream* s, void* stream);

/* The field step on the Hermite cubic with backward differences: the five pairs of ncde_stream_step_field on the path of
 * ncde_stream_step_hermite (same structs, same state; the problem says interp = NCDE_INTERP_CUBIC, s->rectilinear must be 0).
 * With dn, b, two_c and three_d as stated for ncde_stream_step_hermite and s_j the stage's offset in the piece, per stage j:
 *   matmul, derivative   stage 1 reads b, stage j > 1 reads b + (two_c + three_d * s_j) * s_j.
 *   evaluate             stage 1 reads the row at the knot itself (the stream's last row before this fill), stage j > 1 reads
 *                        that row + (b + (0.5 * two_c + three_d * s_j / 3) * s_j) * s_j -- the cubic branch of the batch kernels.
 * The LDS plan is that of ncde_stream_step_field (the stage image takes the slot of the second rectilinear piece), so the query
 * accepts exactly the shapes ncde_stream_field_workspace_bytes accepts; every weight is streamed.  NCDE_ERR_UNSUPPORTED: the GRU-gated
 * field, the low-rank field, the original field with the matmul input (the message points to ncde_stream_step_hermite) and a plan
 * above 160 KiB (the message carries the bytes).  NCDE_ERR_INVALID: what ncde_stream_step_field answers it for, interp other than
 * NCDE_INTERP_CUBIC, s->rectilinear != 0.  A refusal launches nothing and leaves every state buffer untouched.  The kernel name is
 * "ncde_stream_step_field_hermite". */
int64_t ncde_stream_field_hermite_workspace_bytes(const NcdeProblem* p);   /* 0, or < 0: status code */
const char* ncde_stream_field_hermite_kernel_name(const NcdeProblem* p);   /* NULL on error */
int ncde_stream_step_field_hermite(const NcdeProblem* p, const NcdeStream* s, void* stream);

/* The low-rank step: the same step, same structs and same state for NCDE_FIELD_LOWRANK (matmul input) with euler, midpoint or rk4.
 * The problem carries the rank in flags (NCDE_FLAG_FIELD_RANK(R), 1 <= R <= channels), Wo / bo = M_h [H*R, last width],
 * Wg / bg = M_o [R*C, last width] and at least one inner layer whose chain starts at hidden.  p->interp says the path:
 *   NCDE_INTERP_LINEAR   a linear or rectilinear stream (s->rectilinear), the pieces and the left-piece rule of ncde_stream_step;
 *   NCDE_INTERP_CUBIC    the Hermite cubic of ncde_stream_step_hermite (s->rectilinear must be 0): stage 1 reads b, stage j > 1
 *                        b + (two_c + three_d * s_j) * s_j.
 * The stage is that of the batch kernel ncde_fwd_lowrank with the heads streamed from L2 (the same sums in the same order).  ONE
 * launch, one workgroup per 16 streams, no workspace.  NCDE_ERR_UNSUPPORTED, each with a message: any other field kind, an input
 * other than matmul, and a shape whose LDS plan, 4 (5 HS + 2 DS + 5 CS + 48 + 16 ru16((hidden + channels) R)) bytes with
 * HS = 16 ru16(hidden), DS = 16 max(ru16(hidden), ru16(layer widths)), CS = 16 ru4(channels), exceeds 160 KiB (the message carries
 * the bytes).  NCDE_ERR_INVALID: a rank outside [1, channels], n_layers == 0, a layer chain that does not start at hidden or does
 * not chain, a NULL Wo / bo / Wg / bg, and what ncde_stream_step answers it for about NcdeStream.  A refusal launches nothing and
 * leaves every state buffer untouched.  The kernel name is "ncde_stream_step_lowrank" or "ncde_stream_step_lowrank_hermite". */
int64_t ncde_stream_lowrank_workspace_bytes(const NcdeProblem* p);   /* 0, or < 0: status code */
const char* ncde_stream_lowrank_kernel_name(const NcdeProblem* p);   /* NULL on error */
int ncde_stream_step_lowrank(const NcdeProblem* p, const NcdeStream* s, void* stream);

/* The hybrid steps: the online half of the linear / rectilinear hybrid scheme (ncde_prepare_hybrid_*).  The same structs and the
 * same state; the extra argument rectilinear_mask is a DEVICE pointer to uint8 [channels], 1 = the channel steps rectilinearly (the
 * sparse channels R), 0 = it is interpolated linearly.  Time is channel 0 and rectilinear_mask[0] is 0.  The host never reads the
 * mask.  A new row of a stream with count >= 1 is filled as for ncde_stream_step (every channel) and adds, in this order,
 *   piece A   time and the linear channels move: da[c] = fill[c] - last[c] for c not in R, 0 for c in R.  Stage 1 reads prev_dx (da
 *             itself at count == 1), every later stage da.
 *   piece B   the sparse channels move: db[c] = fill[c] - last[c] for c in R, 0 elsewhere.  Stage 1 reads da, every later stage db.
 *             Taken by a stream if and only if db[c] != 0 for some c -- the builder's kept knot; a re-observed unchanged value adds
 *             no piece -- and skipped by the whole workgroup where none of its 16 streams takes it.
 *   then      prev_dx = db where piece B was taken, da otherwise; last_row = fill, count += 1.
 * Precondition, not checked (as "time is never NaN" is not): a stream's time strictly increases, so piece A always exists.
 *   ncde_stream_step_hybrid          the fields of ncde_stream_step (the original field, matmul input)
 *   ncde_stream_step_field_hybrid    those of ncde_stream_step_field with the matmul or derivative input
 *   ncde_stream_step_lowrank_hybrid  that of ncde_stream_step_lowrank
 * LDS plans in bytes, with the HS / DS / CS of the plain steps: 4 (5 HS + 2 DS + 5 CS + 64), 4 (3 DS + 4 HS + 5 CS + 64) and
 * 4 (5 HS + 2 DS + 5 CS + 64 + 16 ru16((hidden + channels) R)).  NCDE_ERR_UNSUPPORTED, each with a message: what the plain step of
 * the same family refuses, the evaluate input (its stage offset is the stream's knot index, which the state does not carry),
 * interp = NCDE_INTERP_CUBIC (the Hermite path has no hybrid form) and a plan above 160 KiB.  NCDE_ERR_INVALID: what the plain step
 * answers it for, a NULL rectilinear_mask, s->rectilinear != 0 (the mask replaces it) and s->time_index != 0.  There is no hybrid
 * form of the stacked step.  A refusal launches nothing and leaves every state buffer untouched.  The kernel names are those of the
 * entry points. */
int64_t ncde_stream_hybrid_workspace_bytes(const NcdeProblem* p);   /* 0, or < 0: status code */
const char* ncde_stream_hybrid_kernel_name(const NcdeProblem* p);   /* NULL on error */
int ncde_stream_step_hybrid(const NcdeProblem* p, const NcdeStream* s, const unsigned char* rectilinear_mask, void* stream);
int64_t ncde_stream_field_hybrid_workspace_bytes(const NcdeProblem* p);   /* 0, or < 0: status code */
const char* ncde_stream_field_hybrid_kernel_name(const NcdeProblem* p);   /* NULL on error */
int ncde_stream_step_field_hybrid(const NcdeProblem* p, const NcdeStream* s, const unsigned char* rectilinear_mask, void* stream);
int64_t ncde_stream_lowrank_hybrid_workspace_bytes(const NcdeProblem* p);   /* 0, or < 0: status code */
const char* ncde_stream_lowrank_hybrid_kernel_name(const NcdeProblem* p);   /* NULL on error */
int ncde_stream_step_lowrank_hybrid(const NcdeProblem* p, const NcdeStream* s, const unsigned char* rectilinear_mask, void* stream);

/* The stacked step: n_stack chained linear CDE layers (StackedNeuralCDE: layer i + 1 reads layer i's hidden sequence as the linear
 * coefficients of its control) advance by s[0]->n_rows rows in ONE launch, one workgroup per 16 streams walking the layers of a row.
 *   layer 0    fills its row from s[0]->x exactly as ncde_stream_step does.
 *   layer i>0  takes as its new row z of layer i - 1 after that layer's step for this row (a stream's first row: layer i - 1's z as
 *              the caller set it), so p[i]->channels == p[i - 1]->hidden.  It never passes through global memory.
 *   per layer  its own problem p[i] (shape, field, method) and its own state s[i]->z / last_row / prev_dx / count; pieces, the
 *              left-piece rule from the stream's own count, stages and bookkeeping are those of ncde_stream_step.  A first row
 *              (count == 0) takes no step at any layer: the caller sets z(t0) of EVERY layer beforehand.
 *   s[0]       carries x and its strides, active, initial_value_if_nan and n_rows for the whole stack; those fields of s[i], i > 0,
 *              are ignored.  rectilinear must be 0 and every interp NCDE_INTERP_LINEAR.
 *   readout    Wf / bf / out / n_out and z_out of s[i] are honoured per layer as in the single step; they are optional for inner
 *              layers, the last layer needs Wf + out or z_out.
 * NCDE_ERR_INVALID: n_stack outside [1, NCDE_STREAM_MAX_STACK], a NULL entry, p[i]->channels != p[i - 1]->hidden, differing batch,
 * rectilinear, a non-linear interp.  NCDE_ERR_UNSUPPORTED: what ncde_stream_step refuses at any layer, and a stack whose LDS plan (the
 * stage scratch of the widest layer + z, last_row, prev_dx, count of every layer) exceeds the limit; the message says the bytes
 * needed.  A refusal leaves every state buffer untouched.  n_stack == 1 is ncde_stream_step, bit for bit.  The two queries answer as
 * those of the single step do; the kernel name is "ncde_stream_stack_step". */
#define NCDE_STREAM_MAX_STACK 4
int64_t ncde_stream_stack_workspace_bytes(const NcdeProblem* const* p, int n_stack);   /* 0, or < 0: status code */
const char* ncde_stream_stack_kernel_name(const NcdeProblem* const* p, int n_stack);   /* NULL on error */
int ncde_stream_stack_step(const NcdeProblem* const* p, const NcdeStream* const* s, int n_stack, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NCDE_HIP_H */
