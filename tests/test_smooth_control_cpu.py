"""CPU side of the fused control-path gradient of cubic-smoothed paths: the fp64 transpose of the smoothing operator (the reference the
GPU test of ncde_prepare_smooth_backward is held to) is the adjoint of coeff_ref64.smooth, the new entry point's argument checks, the
routing predicate, and the g17 fixtures mean what their manifest claims (tools/gen_golden_smooth_control.py)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import coeff_ref64
import golden_util as gu
import ncde_amd
from ncde_amd import _lib, solver, unfused

TIGHT_Z, E2E_G = 2e-5, 2e-4
CASES = ["g17_a_eps1_rk4_knots", "g17_b_eps05_midpoint_half_interval", "g17_c_eps02_euler_quarter_times", "g17_d_eps05_rk4_interval_T2"]
SHAPES = [(T, eps) for T in (2, 3, 7) for eps in (1, 0.5, 0.2)]


def smooth_transpose(g, T, eps, absolute=False):
    """S^T g in float64, S = coeff_ref64.smooth(., eps, 3): g [B, P, 4C] = dL/d(a | b | 2c | 3d) of every piece -> [B, T, C].
    Gather form, in the kernel's order (ncde_smooth_coeffs_bwd_kernel): per knot t the pieces that read x[t], ascending --
    piece 0 (t <= 1), M(t-1), R(t-1), M(t), R(t), M(t+1), with M(k) the matching piece of interior knot k and R(k) the linear rest
    behind it (eps < 1 only).  absolute: the same sum over |weight| |g| -- the sum of the magnitudes of every term, which the
    rounding-error bound of the GPU test is stated in."""
    g = np.asarray(g, dtype=np.float64)
    B, P, C4 = g.shape
    C = C4 // 4
    assert P == coeff_ref64.smooth_pieces(T, eps) and C * 4 == C4
    split = eps < 1
    w2, w3 = 4.0 / eps, -3.0 / eps ** 2
    if absolute:
        g = np.abs(g)
    term = (lambda w, v: abs(w) * v) if absolute else (lambda w, v: w * v)
    part = lambda p, q: g[:, p, q * C:(q + 1) * C]      # noqa: E731
    piece = lambda k: 1 + 2 * (k - 1) if split else k      # noqa: E731  M(k); R(k) is the next row
    interior = lambda k: 1 <= k <= T - 2      # noqa: E731
    out = np.zeros((B, T, C))
    for t in range(T):
        acc = np.zeros((B, C))
        if t == 0:
            acc = part(0, 0) + term(-1.0, part(0, 1))
        elif t == 1:
            acc = part(0, 1).copy()
        if interior(t - 1):
            p = piece(t - 1)
            acc = acc + (term(w2, part(p, 2)) + term(w3, part(p, 3)))
            if split:
                acc = acc + (term(eps, part(p + 1, 0)) + part(p + 1, 1))
        if interior(t):
            p = piece(t)
            s = term(w2, part(p, 2)) + term(w3, part(p, 3))
            acc = acc + ((part(p, 0) + part(p, 1)) + term(-2.0, s))
            if split:
                acc = acc + (term(1.0 - eps, part(p + 1, 0)) + term(-1.0, part(p + 1, 1)))
        if interior(t + 1):
            p = piece(t + 1)
            acc = acc + ((term(w2, part(p, 2)) + term(w3, part(p, 3))) + term(-1.0, part(p, 1)))
        out[:, t] = acc
    return out


@pytest.mark.parametrize("T,eps", SHAPES)
def test_fp64_transpose_is_the_adjoint_of_the_fp64_builder(T, eps):
    """<S x, g> == <x, S^T g> for random x, g, within 1e-12 relative to the inner product itself (fp64: a few hundred terms of unit
    size with weights up to 3 / eps^2 = 75 leave ~1e-14 of it)."""
    rng = np.random.default_rng(100 * T + int(10 * eps))
    B, C = 3, 4
    x = rng.standard_normal((B, T, C))
    g = rng.standard_normal((B, coeff_ref64.smooth_pieces(T, eps), 4 * C))
    Sx = coeff_ref64.smooth(x, eps, 3)
    lhs, rhs = float((Sx * g).sum()), float((x * smooth_transpose(g, T, eps)).sum())
    scale = max(abs(lhs), abs(rhs))
    assert scale >= 1e-2 * float((np.abs(Sx) * np.abs(g)).sum()) / np.sqrt(g.size)      # (not a cancelled-out product)
    print("T %d eps %s: <Sx, g> %.15e  <x, S^T g> %.15e  rel %.2e" % (T, eps, lhs, rhs, abs(lhs - rhs) / scale))
    assert abs(lhs - rhs) <= 1e-12 * scale
    # the `absolute` form bounds the plain one element by element, and is the plain one for non-negative weights' worth of input
    assert (np.abs(smooth_transpose(g, T, eps)) <= smooth_transpose(g, T, eps, absolute=True) * (1 + 1e-15)).all()
    # every element of S^T is exercised: the transpose of a unit gradient on each row part reaches a knot
    assert (smooth_transpose(np.ones_like(g), T, eps, absolute=True) > 0).all()


def test_backward_entry_point_checks_its_arguments():
    """Bad arguments answer NCDE_ERR_INVALID as ncde_prepare_smooth does; order 5 answers NCDE_ERR_UNSUPPORTED with a message.  (All
    refused before anything is launched: dummy pointers.)"""
    lib = ncde_amd.lib()
    assert "ncde_prepare_smooth_backward" in _lib.EXPORTS
    fn = lib.ncde_prepare_smooth_backward
    ok = dict(g=0x1000, B=2, T=5, C=3, eps=0.5, order=3, gx=0x2000)
    for bad in (dict(g=None), dict(gx=None), dict(B=0), dict(T=1), dict(C=0), dict(eps=0.0), dict(eps=1.5), dict(eps=float("nan")),
                dict(order=4)):
        a = dict(ok, **bad)
        assert fn(a["g"], a["B"], a["T"], a["C"], a["eps"], a["order"], a["gx"], None) == -1, bad
        assert lib.ncde_prepare_smooth(a["g"], a["B"], a["T"], a["C"], a["eps"], a["order"], a["gx"], None) == -1, bad
    assert fn(ok["g"], 2, 5, 3, 0.5, 5, ok["gx"], None) == -2
    assert b"order 5" in lib.ncde_last_error_string() and b"ncde_prepare_smooth_backward" in lib.ncde_last_error_string()
    with pytest.raises(NotImplementedError, match="order 5"):
        _lib.check(-2, "ncde_prepare_smooth_backward")


def test_route_predicate_reads_a_smoothed_control():
    """Cubic smoothing on the integer grid is a control the fused control-gradient route takes; quintic matching, no smoothing
    (gradient_matching_eps=None), a user `t` and knots that require grad are not.  _unfused_reason's answer is the same for all of
    them.  (CPU tensors: _control_route_ok itself is false for every one -- `cuda_fp32` --, so each case is paired with the values
    the reader hands to the decision; tests/test_smooth_control_gpu.py asks _control_route_ok on the GPU.)"""
    c = torch.zeros(2, 5, 3, requires_grad=True)
    f = ncde_amd.OriginalVectorField(3, 4, 8, 2)
    z0 = torch.zeros(2, 4)
    S = ncde_amd.SmoothLinearInterpolation
    cubic, cubic1 = S(c, gradient_matching_eps=0.5), S(c, gradient_matching_eps=1)
    quintic = S(c, gradient_matching_eps=0.5, match_second_derivatives=True)
    plain, user_t = S(c), S(c, t=torch.tensor([0.0, 0.5, 1.5, 2.0, 4.0]))
    for X in (cubic, cubic1, quintic, plain, user_t):
        assert solver._unfused_reason(X, f, z0, X.interval, False, None, "rk4") == solver._CONTROL_REASON
        assert not solver._control_route_ok(solver._CONTROL_REASON, X, z0, X.interval, False, "rk4")      # CPU tensors
    assert solver._cubic_smoothed(cubic) and solver._cubic_smoothed(cubic1)
    assert not solver._cubic_smoothed(quintic) and not solver._cubic_smoothed(plain) and not solver._cubic_smoothed(user_t)
    assert not solver._cubic_smoothed(ncde_amd.LinearInterpolation(c))

    class Sub(S):      # (an exact type, as for the plain controls: a subclass may evaluate anything)
        pass
    assert not solver._cubic_smoothed(Sub(c, gradient_matching_eps=0.5))
    # knots that require grad: `other_grad`, which refuses the route whatever the control
    Xk = S(c, gradient_matching_eps=0.5)
    Xk._t = Xk._t.clone().requires_grad_(True)
    assert solver._cubic_smoothed(Xk) and any(b.requires_grad for b in Xk.buffers() if b is not Xk._coeffs)
    reason = solver._CONTROL_REASON
    assert solver._control_route(reason, False, "rk4", True, True, True, False, False)
    assert not solver._control_route(reason, False, "rk4", True, True, True, True, False)       # knots with grad
    assert not solver._control_route(reason, False, "dopri5", True, True, True, False, False)   # dopri5 keeps its own reason anyway:
    assert solver._unfused_reason(cubic, f, z0, cubic.interval, False, None, "dopri5") == "method='dopri5' on a smoothed-linear control path"
    assert not solver._control_route(reason, True, "rk4", True, True, True, False, False)       # adjoint=True


def _load(name):
    f = dict(np.load(os.path.join(gu.GOLD, name + ".npz")))
    return f, json.loads(str(f["meta"]))


@pytest.mark.parametrize("name", CASES)
def test_fixture_meets_the_manifest_conditions_and_the_unfused_solver_reproduces_it(name):
    """What the generator enforced, re-read from the committed files: ref_drift <= a quarter of each bound, vs_linear >= 100 x each
    bound (case d, T = 2, is one linear piece: there the smoothed solve IS the linear one and vs_linear must be below the drift bar),
    a gradient far above the tolerance with no (nearly) zero knot row.  And the fixture means what it claims: the package's own
    SmoothLinearInterpolation under autograd through the unfused torch-op solver on the CPU (fp32) reproduces every quantity to 1e-6
    -- twice the largest fp32-vs-fp64 drift of the reference itself (<= 4.6e-7), the level test_control_grad_cpu.py holds g16 to."""
    f, m = _load(name)
    with open(os.path.join(gu.GOLD, "MANIFEST_smooth_control.json")) as fh:
        assert {e["name"]: e for e in json.load(fh)}[name] == m
    d = m["dims"]
    bound = lambda k: TIGHT_Z if k == "z" else E2E_G      # noqa: E731
    assert set(m["ref_drift"]) == set(m["vs_linear"]) == {"z", "dcoeffs", "dz0", "dtheta"}
    assert all(v <= bound(k) / 4 for k, v in m["ref_drift"].items())
    if m["single_piece"]:
        assert d["T"] == 2 and all(v <= bound(k) / 4 for k, v in m["vs_linear"].items())
    else:
        assert d["T"] > 2 and all(v >= 100 * bound(k) for k, v in m["vs_linear"].items())
    dc = f["dcoeffs"]
    assert dc.shape == f["coeffs"].shape == (d["B"], d["T"], d["C"])
    assert m["max_dcoeffs"] == float(np.abs(dc).max()) >= 1e3 * E2E_G and (np.abs(dc).max(axis=(0, 2)) >= 1e-2 * np.abs(dc).max()).all()
    func = ncde_amd.OriginalVectorField(d["C"], d["H"], d["HH"], d["nl"])
    sp = func.fused_spec()
    pp = {"W0": sp.layers[0][0], "b0": sp.layers[0][1], "Wo": sp.Wo, "bo": sp.bo}
    if d["nl"] > 1:
        pp.update(W1=sp.layers[1][0], b1=sp.layers[1][1])
    assert sorted(pp) == sorted(m["param_names"])
    with torch.no_grad():
        for k, q in pp.items():
            q.copy_(torch.from_numpy(f["p_" + k]).reshape(q.shape))
    x = torch.from_numpy(f["coeffs"]).requires_grad_(True)
    X = ncde_amd.SmoothLinearInterpolation(x, gradient_matching_eps=m["eps"])
    z0 = torch.from_numpy(f["z0"]).requires_grad_(True)
    out = unfused.cdeint_unfused(X, func, z0, torch.from_numpy(f["t_out"]), False, "matmul", m["method"], m["step_size"])
    (out * torch.from_numpy(f["grad_out"])).sum().backward()
    errs = {"z": gu.relerr(out.detach().numpy(), f["z_out"]), "dcoeffs": gu.relerr(x.grad.numpy(), dc), "dz0": gu.relerr(z0.grad.numpy(), f["dz0"])}
    for n in m["param_names"]:
        errs["d" + n] = gu.relerr(pp[n].grad.numpy().reshape(f["d" + n].shape), f["d" + n])
    print(name, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert all(v <= 1e-6 for v in errs.values()), errs
