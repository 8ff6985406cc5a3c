// Shape-specialised (register-resident) kernel family: the plan of one pass, read by every query and by the one launch routine.
#pragma once
#include <hip/hip_runtime.h>

#include "ncde_common.h"
#include "ncde_hip.h"

struct FastLaunch {
    NcdeKernel fn;       // nullptr: no such launch
    int block;
    size_t lds;          // dynamic LDS bytes
};

// "this problem, this pass -> these launches".  pass 0 = forward, 1 = continuous adjoint, 2 = exact discrete backward.
struct FastPlan {
    bool ok;             // the family covers (problem, pass).  ok with main.fn == nullptr: the flags ask for a development variant that
                         // is not instantiated for this problem -- the queries answer, the launch returns NCDE_ERR_UNSUPPORTED
    const char* name;    // reported kernel name (an instrumented variant reports the name of the kernel it instruments)
    int grid;            // workgroups = partials the reduce sums
    FastLaunch main;
    FastLaunch redo;     // re-execution of range-faulted workgroups (KArgs.only_faulted = 1) by the instance without fp16 inputs
    int64_t ws_bytes;    // workspace: [adjoint: partials, 256 B | development tail | range-fault words]
    int64_t fault_off;   // byte offset of the range-fault words, one per workgroup; -1: the main kernel writes none
    int64_t tail_off;    // byte offset of the development tail (profile counters / chain dump); -1: none
    bool reduce;         // ncde_reduce_partials follows (unless the caller asks for the main kernel only)
};
FastPlan ncde_fast_plan(const NcdeProblem* p, int pass);

// Ends a plan's workspace: `body` bytes, then one range-fault word per workgroup of P->grid (the words are always reserved).
inline void ncde_fast_plan_workspace(FastPlan* P, int64_t body, bool faults) {
    P->ws_bytes = body + ((((int64_t)P->grid * 4) + 255) & ~(int64_t)255);
    P->fault_off = faults ? body : -1;
}

inline bool ncde_fast_supported(const NcdeProblem* p, int pass) { return ncde_fast_plan(p, pass).ok; }
inline const char* ncde_fast_kernel_name(const NcdeProblem* p, int pass) { return ncde_fast_plan(p, pass).name; }
inline int64_t ncde_fast_workspace_bytes(const NcdeProblem* p, int pass) { const FastPlan P = ncde_fast_plan(p, pass); return P.ok ? P.ws_bytes : (int64_t)NCDE_ERR_UNSUPPORTED; }

// Runs the plan of `pass`.  Forward: out (+ stages to record them); adjoint: src = z_out (pass 1) / the stage record (pass 2).
int ncde_fast_launch(const NcdeProblem* p, int pass, float* out, float* stages, const float* src, const float* grad_out,
                     const NcdeGrads* g, void* ws, size_t ws_bytes, hipStream_t st, bool main_kernel_only);
