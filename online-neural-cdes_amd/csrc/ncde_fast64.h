// In-sweep adjoint of the register-resident family for H = HH = 64, C <= 4 (BASELINE cfg4): host-side hook used by ncde_fast.hip.
#pragma once
#include "ncde_fast.h"
#include "ncde_host.h"

// pass 1 = continuous adjoint (adjoint.py:37-145), pass 2 = exact discrete backward (ncde_backward): fills *P (its own grid of
// 16 * NS samples per workgroup, names, LDS size) and returns true, or returns false where these kernels do not cover the problem
bool ncde_fast64_plan(const NcdeProblem* p, int pass, const Layout& y, FastPlan* P);
