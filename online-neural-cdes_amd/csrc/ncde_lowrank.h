// Low-rank vector field (NCDE_FIELD_LOWRANK): host-side hooks used by ncde_abi.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "ncde_hip.h"

// pass 0 forward, 1 continuous adjoint, 2 exact discrete backward; `why` (may be NULL) receives the reason of a refusal
bool ncde_lowrank_supported(const NcdeProblem* p, int pass, char* why = nullptr, size_t n = 0);
int64_t ncde_lowrank_workspace_bytes(const NcdeProblem* p, int pass);
int ncde_lowrank_forward(const NcdeProblem* p, float* out, float* stages, hipStream_t st);
int ncde_lowrank_adjoint(const NcdeProblem* p, const float* src, const float* grad_out, const NcdeGrads* g, void* ws, hipStream_t st,
                         bool main_kernel_only, bool discrete);
