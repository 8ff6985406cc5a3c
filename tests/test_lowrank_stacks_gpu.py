"""The low-rank kernels (ncde_fwd_lowrank / ncde_adj_lowrank) where tests/test_lowrank_gpu.py does not take them: un-shared, tied and
uneven layer stacks, the regimes of the LDS plan, general time axes and the edges of the head arithmetic (tests/lowrank_cases.py).

Every case: the fused fp32 solve through ncde_amd.cdeint with warnings as errors, the library naming the low-rank kernels for the
captured problem, against the package's unfused torch-op solver in fp64 on the same inputs (which must emit its one warning).  The
reference of every case runs the UNTIED stack -- each layer its own equal-valued tensors -- and a tied tensor's gradient is compared
with the fp64 sum over its uses.  Tolerances are the project's: forward <= 2e-5, dL/dz0 and every parameter gradient <= 2e-4, as
|delta| relative to max |ref|; every gradient of the reference, heads and inner layers, has a maximum >= 1e3 x the tolerance
(validated without a GPU in tests/test_lowrank_plan_cpu.py)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import lowrank_cases as lc
from ncde_amd import _lib

pytestmark = pytest.mark.gpu

NAMES = ["ncde_fwd_lowrank", "ncde_adj_lowrank", "ncde_adj_lowrank<discrete>"]


def _runs(prefix):
    return [(n, m) for n in sorted(lc.CASES) if n.startswith(prefix) for m in lc.CASES[n]["modes"]]


def _ids(runs):
    return ["%s-%s" % r for r in runs]


@functools.lru_cache(maxsize=None)
def _reference(name, mode):
    """The unfused solver in fp64 on the untied stack: computed once, shared, never modified."""
    probe = {}
    ref = lc.solve(name, mode, torch.float64, "cuda", untie=True, field_probe=lambda f, z: probe.update(share=lc.saturated_share(f, z)))
    ref["saturated_share"] = probe["share"]
    return ref


def _kernel_names(lib, p):
    return [(lib.ncde_kernel_name(ctypes.byref(p), ps) or b"?").decode() for ps in (0, 1, 2)]


def _fused(name, mode, lib):
    """-> (result, the problem handed to the library); asserts it is a low-rank problem that the low-rank kernels take."""
    probs = []
    res = lc.solve(name, mode, torch.float32, "cuda", capture=probs)
    p, c = probs[-1], lc.CASES[name]
    assert _kernel_names(lib, p) == NAMES
    assert p.flags >> 24 == c["R"] and p.field_kind == 3 and p.n_layers == len(lc.arrays(name)["layers"])
    assert [int(p.layer_out[l]) for l in range(p.n_layers)] == [d[0] for d in lc.arrays(name)["dims"]]
    return res, p


def _compare(name, mode, lib):
    res, p = _fused(name, mode, lib)
    lc.check("%s %s" % (name, mode), res, _reference(name, mode), lc.arrays(name)["names"])
    return res, p


@pytest.mark.parametrize("name,mode", _runs("stack_"), ids=_ids(_runs("stack_")))
def test_lowrank_layer_stacks(name, mode, gpu_lib):
    """Un-shared, tied (the shared tensor's gradient = the fp64 sum over its uses), weight-tied with own biases, bias-shared, eight
    layers, one layer, and uneven widths -- a 128-wide layer in front of a 16-wide one (the ping-pong buffers keep its rows), widths
    above H and a last width of 15; rk4 on the linear path, midpoint on the cubic one."""
    res, p = _compare(name, mode, gpu_lib)
    a = lc.arrays(name)
    tensors = set(n for wb in a["layers"] for n in wb)
    assert len(a["names"]) == len(tensors) + 4 and set(res["grads"]) == set(a["names"])


@pytest.mark.parametrize("name,mode", _runs("regime_"), ids=_ids(_runs("regime_")))
def test_lowrank_lds_plan_regimes(name, mode, gpu_lib):
    """One case per regime of the LDS plan that the everything-resident and the everything-streamed tests do not reach (the regime is
    asserted through the restated plan, so a change of the plan cannot silently move the case); two runs give the same bits."""
    assert lc.plan_of(name) == (True, True) + lc.REGIMES[name], lc.plan_of(name)
    res, _ = _compare(name, mode, gpu_lib)
    again, _ = _fused(name, mode, gpu_lib)
    assert np.array_equal(res["z_out"], again["z_out"]) and np.array_equal(res["dz0"], again["dz0"])
    for k in lc.arrays(name)["names"]:
        assert np.array_equal(res["grads"][k].view(np.int32), again["grads"][k].view(np.int32)), k


@pytest.mark.parametrize("mode", ["adjoint", "discrete"])
def test_lowrank_first_refused_shape_runs_unfused(mode, gpu_lib):
    """H 64, C 24, HH 64, two layers at R = 10, the first rank whose backward plan passes 160 KB: cdeint takes the unfused route
    behind exactly one warning, within the same tolerances of the fp64 solve."""
    name = "refused_rank10"
    assert lc.plan_of(name)[:2] == (True, False)
    c = lc.CASES[name]
    assert dict(H=c["H"], C=c["C"], R=c["R"], HH=c["spec"][0], nl=len(c["spec"])) == lc.REFUSED
    probs = []
    res = lc.solve(name, mode, torch.float32, "cuda", capture=probs, refused=True)
    assert gpu_lib.ncde_workspace_bytes(ctypes.byref(probs[-1]), 1 if mode == "adjoint" else 2) == -2
    lc.check("%s %s (unfused fp32)" % (name, mode), res, _reference(name, mode), lc.arrays(name)["names"])


@pytest.mark.parametrize("name,mode", _runs("time_"), ids=_ids(_runs("time_")))
def test_lowrank_on_general_time_axes(name, mode, gpu_lib):
    """Off-grid output times (interpolated outputs, their cotangents in the discrete backward, the per-interval reverse grids of the
    continuous adjoint), rk4 at step 0.5, midpoint at 0.4 (its first stage has weight 0), euler at 1.3 (does not divide the knot
    spacing), linear and cubic paths, and a user knot grid."""
    _, p = _compare(name, mode, gpu_lib)
    assert p.output == _lib.OUT_TIMES and p.time_plan and p.n_steps_fwd >= 3


@pytest.mark.parametrize("name,mode", _runs("edge_"), ids=_ids(_runs("edge_")))
def test_lowrank_head_arithmetic_edges(name, mode, gpu_lib):
    """C = R = 1; R = 4 (the register ranks exactly) and R = 5 at C = 7; (H + C) R a multiple of 16 and not; a last width of 15; a
    single step with final-only output and B = 1; heads scaled by 4 so that more than a quarter of |M| is above 0.99."""
    res, p = _compare(name, mode, gpu_lib)
    if name == "edge_T2_B1_final":
        assert (p.batch, p.n_knots, p.output) == (1, 2, _lib.OUT_INTERVAL) and res["z_out"].shape == (1, 2, 10)
    if name == "edge_saturated_heads":
        share = _reference(name, mode)["saturated_share"]
        print("share of |M| > 0.99: %.3f" % share)
        assert share >= lc.SATURATED_SHARE
