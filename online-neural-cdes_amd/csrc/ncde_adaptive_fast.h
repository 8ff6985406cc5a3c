// Fused dopri5 attempt kernels (csrc/ncde_adaptive_fast.hip); driven by ncde_dp_solve (ncde_adaptive.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "ncde_hip.h"

namespace {
struct DpArgs;      // ncde_dp_defs.h: the argument block of every dopri5 kernel, filled by ncde_dp_solve / ncde_dp_tape_backward_run
}

bool ncde_dpf_supported(const NcdeProblem* p, int adj);
const char* ncde_dpf_kernel_name(const NcdeProblem* p, int adj);
size_t ncde_dpf_pack_floats(const NcdeProblem* p, int adj);      // workspace floats of the per-lane weight image (0: not supported)
size_t ncde_dpf_partial_floats(const NcdeProblem* p, int theta1);
int ncde_dpf_reduce_blocks(const NcdeProblem* p, int theta1);
// reverse sweep of a taped solve (adjoint=False) on the fused stage machinery; workspace: ncde_dpf_pack_floats(p, 1) floats at DpArgs.WP
bool ncde_dpf_tape_supported(const NcdeProblem* p);
const char* ncde_dpf_tape_kernel_name(const NcdeProblem* p);
// The launchers.  DpArgs lives in an unnamed namespace (its name is part of every kernel's symbol), and a C++ function over such a type
// is local to its unit: these three have C linkage so that ncde_adaptive.hip can call them.  Both units read ncde_dp_defs.h.
extern "C" {
int ncde_dpf_prepare(const NcdeProblem* p, const DpArgs& d, int adj, hipStream_t st);      // once per solve: the per-lane weight image
// enqueue `rounds` attempt launches (launches of a finished solve exit at once)
int ncde_dpf_launch(const NcdeProblem* p, const DpArgs& d, int adj, int rounds, hipStream_t st);
int ncde_dpf_tape_launch(const NcdeProblem* p, const DpArgs& d, hipStream_t st);
}
