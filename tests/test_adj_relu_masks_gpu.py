"""ReLU gating of the chain + gradient-wave adjoint (ncde_adj_fast3) on inputs where the gates decide the result.

The kernel keeps `x > 0` of every hidden activation of a stage as a wave lane mask and gates the cotangent with it on the way back.
A wrong, stale or mis-indexed mask moves a gradient by O(1), so the comparison is the one test_gpu_parity.py makes for the adjoint
kernel in isolation: the kernel is fed the oracle's own forward solution (adjoint=True) or stage record (adjoint=False) and must
match the oracle's gradients at that file's TIGHT_G.  Shapes are the smallest that take every path: B = 17 (one full 16-sample tile
and a one-sample tile), raw length 3 (5 rectilinear knots) / a 4-knot cubic, H = HH = 32, C in {4, 20}, 1 to 4 layers, every solver.

Every case asserts that ncde_adj_fast3 is the kernel that ran, with ONE exception: C = 20, nl = 4 on a cubic path does not fit the
kernel's LDS plan and runs on the batch-tiled family, which has no lane-mask code.  Those cases are kept because the shape list asks
for them; they check the gating semantics of that family, not the code this file was written for.

The dead layer is made through the sample's z0 (W0 z0 = -50 in every unit), not through a large negative bias: a bias is shared by
all samples and would kill the layer for the whole tile, while the point is one dead sample between live neighbours.
"""
import functools

import numpy as np
import pytest

import golden_util as gu
from test_gpu_parity import TIGHT_G, _grad_errors

pytestmark = pytest.mark.gpu

B, H, HH = 17, 32, 32
DEAD = 5      # the sample whose first hidden layer is dead (tile 0, next to live samples)


@functools.lru_cache(maxsize=None)
def _case(interp, method, C, nl, kind):
    """kind "half": random weights and biases (about half of the pre-activations negative) and one sample whose whole first layer is
    dead.  kind "zero": all biases 0 and sample 0 started at z0 = 0, so that sample stays at 0 and every pre-activation of it is
    exactly 0.  The oracle's results are computed once per case and shared."""
    import ncde_oracle as orc
    seed = 4000 + 100 * C + 10 * nl + (1 if interp == "cubic" else 0)
    if interp == "cubic":
        coeffs = gu.data.make_cubic_coeffs(B, 4, C - 1, seed=seed)
        x0 = coeffs[:, 0, :C]
    else:
        coeffs = gu.data.make_rectilinear_coeffs(B, 3, C - 1, missing=0.3, seed=seed)
        assert coeffs.shape[1] == 5
        x0 = coeffs[:, 0]
    p = dict(gu.data.make_field_weights(H, HH, C, seed=seed + 1))
    rw = gu.data.make_readin_weights(H, C, 1, seed=seed + 1)
    z0 = (x0 @ rw["Wi"].T + rw["bi"]).astype(np.float32)
    if kind == "zero":
        for b in ("b0", "b1", "bo"):
            p[b] = np.zeros_like(p[b])
        z0[0] = 0.0
    else:
        # W0 z0 = -50 in every unit: no step of the short path (|f| <= 1) brings a unit of that layer back above 0
        z0[DEAD] = np.linalg.solve(p["W0"].astype(np.float64), np.full(HH, -50.0)).astype(np.float32)
        assert (p["W0"] @ z0[DEAD] + p["b0"] < -40.0).all()
    if nl == 1:
        p = {k: v for k, v in p.items() if k not in ("W1", "b1")}
    names = ["W0", "b0"] + (["W1", "b1"] if nl > 1 else []) + ["Wo", "bo"]
    case = {"meta": {"kind": interp, "method": method, "sequence": False, "param_names": names, "field_kind": "original", "field_mode": "matmul",
                     "dims": {"C": C, "H": H, "HH": HH, "nl": nl}, "field": "original"},
            "coeffs": coeffs, "z0": z0, "params": p, "layers": [("W0", "b0")] + [("W1", "b1")] * (nl - 1), "H": H, "C": C}
    field = gu.oracle_field(case)
    ctl = orc.Control(coeffs, interp)
    z = orc.solve_forward(ctl, field, z0, method, False)
    gout = (gu.data.normal(seed + 2, z.numel(), stream=1).reshape(z.shape) / np.sqrt(z.shape[1])).astype(np.float32)
    dz0, gp = orc.solve_adjoint(ctl, field, z, gout, method, False)
    ex = {"z_out": z.numpy(), "grad_out": gout, "dz0": dz0.numpy()}
    for n_, g_ in zip(names, gp):
        ex["d" + n_] = g_.numpy()
    bdz0, bgp = orc.solve_discrete_backward(ctl, field, z0, gout, method, False)
    ex["bp_dz0"] = bdz0.numpy()
    for n_, g_ in zip(names, bgp):
        ex["bp_d" + n_] = g_.numpy()
    case["expect"] = ex
    case["stage_record"] = orc.stage_record(ctl, field, z0, method).numpy()
    # the inputs do what they are meant to: the first layer's pre-activations at the start are about half negative
    pre = z0 @ p["W0"].T + p["b0"]
    live = np.delete(pre, DEAD, axis=0) if kind == "half" else pre[1:]
    assert 0.3 < float((live < 0).mean()) < 0.7
    if kind == "zero":
        assert not np.any(ex["z_out"][0]) and not np.any(case["stage_record"][:, 0])
    return case


def _differing(a, b):
    """Names of the results that are not bitwise equal between two launches, with the largest difference."""
    pairs = [("dz0", a["dz0"], b["dz0"])] + [(k, a["grads"][k], b["grads"][k]) for k in a["grads"]]
    return {k: float(np.abs(x.astype(np.float64) - y).max()) for k, x, y in pairs if not np.array_equal(x, y)}


def _check(case, adjoint):
    import gpu_util
    m = case["meta"]
    C, nl = m["dims"]["C"], m["dims"]["nl"]
    names = gpu_util.kernel_names(case)
    ran = names[1 if adjoint else 2]
    if C == 20 and nl == 4 and m["kind"] == "cubic":      # the LDS plan does not fit (module docstring)
        assert names[1].startswith("ncde_adj_tiled") and not ran.startswith("ncde_adj_fast3"), names
    else:
        assert ran.startswith("ncde_adj_fast3<H32,HH32,C%d,NL%d" % (C, nl)) and ("discrete" in ran) == (not adjoint), names
    z = case["expect"]["z_out"]
    stages = None if adjoint else case["stage_record"]
    first = gpu_util.run_adjoint_direct(case, z, stages=stages)
    errs = _grad_errors(case, first, "" if adjoint else "bp_")
    print(m["kind"], m["method"], "C", C, "nl", nl, "adjoint" if adjoint else "discrete", {k: "%.2e" % e for k, e in errs.items()})
    for k, e in errs.items():
        assert e <= TIGHT_G, (names, k, e)
    again = gpu_util.run_adjoint_direct(case, z, stages=stages)
    assert not _differing(first, again), (names, _differing(first, again))
    return first


@pytest.mark.parametrize("adjoint", [True, False])
@pytest.mark.parametrize("method", ["rk4", "midpoint", "euler"])
@pytest.mark.parametrize("interp", ["linear", "cubic"])
@pytest.mark.parametrize("nl", [1, 2, 3, 4])
@pytest.mark.parametrize("C", [4, 20])
def test_half_negative_activations_and_a_dead_layer(C, nl, interp, method, adjoint, gpu_lib):
    """About half of all gates closed, and one sample of the full tile with its first layer dead while its neighbours are live: that
    sample's vector field has no dependence on z, so its dL/dz0 is exactly the dL/dz it was handed (the two output rows added up)."""
    case = _case(interp, method, C, nl, "half")
    res = _check(case, adjoint)
    assert np.array_equal(res["dz0"][DEAD], case["expect"]["grad_out"][DEAD].sum(0))


@pytest.mark.parametrize("adjoint", [True, False])
@pytest.mark.parametrize("interp", ["linear", "cubic"])
@pytest.mark.parametrize("nl", [1, 2, 3, 4])
@pytest.mark.parametrize("C", [4, 20])
def test_activations_of_exactly_zero_block_the_gradient(C, nl, interp, adjoint, gpu_lib):
    """Sample 0 sits at z = 0 with all biases 0: every pre-activation of it is exactly 0.  Its dP is not (dbo shows it), so only the
    strict `x > 0` gate keeps it out of the hidden layers: with dL/dz of every other sample set to 0 the hidden-weight gradients
    are exactly 0."""
    import gpu_util
    case = _case(interp, "rk4", C, nl, "zero")
    _check(case, adjoint)
    one = dict(case)
    one["expect"] = dict(case["expect"])
    g = np.zeros_like(case["expect"]["grad_out"])
    g[0] = case["expect"]["grad_out"][0]
    one["expect"]["grad_out"] = g
    res = gpu_util.run_adjoint_direct(one, case["expect"]["z_out"], stages=None if adjoint else case["stage_record"])
    assert np.any(res["grads"]["bo"] != 0)
    for k in ("W0", "b0") + (("W1", "b1") if nl > 1 else ()):
        assert not np.any(res["grads"][k]), k
    assert not np.any(res["grads"]["Wo"])      # x_L = 0
