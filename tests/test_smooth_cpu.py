"""Smoothed-linear control paths, the part that needs no GPU: the torch restatement of the class against recorded reference values
(tests/golden/g14_i_probe.npz), its assertions, the NeuralCDE constructor, the NCDE_INTERP_QUINTIC constant across header / binding,
and the time plan on the refined knot grid against the reference's region rule (goldens g14_a .. g14_f give the cases)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import golden_util as gu

TIGHT_Z = 2e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _probe():
    f = dict(np.load(os.path.join(gu.GOLD, "g14_i_probe.npz")))
    return f, json.loads(str(f["meta"]))


@pytest.mark.parametrize("dn,dtype", [("f32", torch.float32), ("f64", torch.float64)])
def test_class_reproduces_the_reference_at_the_probe_times(dn, dtype):
    """evaluate / derivative / matching coefficients: equal to the recorded reference values bit for bit, except at probe times within
    1 ulp of k + eps (either side of the region rule is right there up to round-off: TIGHT_Z)."""
    import ncde_amd
    f, meta = _probe()
    coeffs = torch.from_numpy(f["coeffs"]).to(dtype)
    for c in meta["combos"]:
        tag, eps = c["tag"], c["eps"]
        X = ncde_amd.SmoothLinearInterpolation(coeffs, gradient_matching_eps=eps, match_second_derivatives=c["quintic"])
        assert np.array_equal(X.gradient_matching_coeffs.numpy(), f["m_%s_%s" % (tag, dn)])
        times = f["t_" + tag]
        assert len(times) >= 25
        n_edge = 0
        for i, t in enumerate(times):
            ev, dv = X.evaluate(float(t)).numpy(), X.derivative(float(t)).numpy()
            k = np.floor(t - eps)
            edge = k >= 1 and abs(np.float32(t) - np.float32(k + eps)) <= np.spacing(np.float32(k + eps))
            if edge:
                n_edge += 1
                assert gu.relerr(ev, f["ev_%s_%s" % (tag, dn)][i]) <= TIGHT_Z and gu.relerr(dv, f["dv_%s_%s" % (tag, dn)][i]) <= TIGHT_Z, (tag, t)
            else:
                assert np.array_equal(ev, f["ev_%s_%s" % (tag, dn)][i]), (tag, t)
                assert np.array_equal(dv, f["dv_%s_%s" % (tag, dn)][i]), (tag, t)
        assert n_edge >= 8


def test_constructor_and_grids():
    import ncde_amd
    from ncde_amd import solver
    c = torch.randn(3, 6, 4)
    with pytest.raises(AssertionError, match="times not implemented"):
        ncde_amd.SmoothLinearInterpolation(c, t=torch.arange(6.0), gradient_matching_eps=0.5)
    for bad in (0, -0.1, 1.5):
        with pytest.raises(AssertionError):
            ncde_amd.SmoothLinearInterpolation(c, gradient_matching_eps=bad)
    X = ncde_amd.SmoothLinearInterpolation(c, gradient_matching_eps=0.25, match_second_derivatives=True)
    assert X.interp_name == "quintic" and len(X) == 6 and X.n_knots == 6
    assert torch.equal(X.grid_points, torch.arange(6.0)) and torch.equal(X.interval, torch.tensor([0.0, 5.0]))
    assert solver._is_tagged_time(X, X.grid_points) and solver._is_tagged_time(X, X.interval)
    kn, n = X._plan_grid()      # the refined grid feeds the time plan; n_knots as seen by the tagged-time shortcut stays T
    assert n == 10 and kn.tolist() == [0, 1, 1.25, 2, 2.25, 3, 3.25, 4, 4.25, 5]
    assert solver._time_mode(X, X.interval) is None                 # eps < 1: always the time plan
    X1 = ncde_amd.SmoothLinearInterpolation(c, gradient_matching_eps=1)
    assert X1.interp_name == "cubic" and X1._plan_grid() == (None, 6)
    assert solver._time_mode(X1, X1.interval) == ncde_amd._lib.OUT_INTERVAL and solver._time_mode(X1, X1.grid_points) == ncde_amd._lib.OUT_KNOTS
    X0 = ncde_amd.SmoothLinearInterpolation(c)                      # no smoothing: LinearInterpolation
    L = ncde_amd.LinearInterpolation(c)
    assert X0.interp_name == "linear" and X0.fused_coeffs is c
    for t in (0, 0.3, 2.0, 4.75):
        assert torch.equal(X0.evaluate(t), L.evaluate(t)) and torch.equal(X0.derivative(t), L.derivative(t))
    assert torch.equal(X.evaluate(0), c[:, 0])


def test_neural_cde_accepts_the_smoothed_schemes():
    import ncde_amd
    for name in ("linear_cubic_smoothing", "linear_quintic_smoothing"):
        m = ncde_amd.NeuralCDE(4, 8, 2, interpolation=name, interpolation_eps=0.5)
        X = m.spline(torch.randn(2, 5, 4))
        assert isinstance(X, ncde_amd.SmoothLinearInterpolation) and X.match_second_derivatives == ("quintic" in name)
        assert sorted(m.state_dict()) == sorted(ncde_amd.NeuralCDE(4, 8, 2).state_dict())
        ncde_amd.NeuralCDE(4, 8, 2, interpolation=name)             # eps None: plain linear
        with pytest.raises(AssertionError):
            ncde_amd.NeuralCDE(4, 8, 2, interpolation=name, interpolation_eps=1.5)
    with pytest.raises(NotImplementedError):
        ncde_amd.NeuralCDE(4, 8, 2, interpolation="rectilinear_cubic_smoothing")
    with pytest.raises(AssertionError):
        ncde_amd.NeuralCDE(4, 8, 2, interpolation="linear", interpolation_eps=0.5)


def test_quintic_constant_agrees_across_header_and_binding():
    from ncde_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ncde_hip.h")).read()
    assert int(re.search(r"NCDE_INTERP_QUINTIC\s*=\s*(\d+)", hdr).group(1)) == _lib.INTERP["quintic"] == 2
    assert _lib.INTERP_PARTS == {"linear": 1, "cubic": 4, "quintic": 6}
    assert int(re.search(r"#define\s+NCDE_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.NCDE_ABI_VERSION == 4
    for name in ("ncde_prepare_smooth", "ncde_smooth_pieces"):
        assert name in _lib.EXPORTS and re.search(r"\b%s\(" % name, hdr)
    lib = _lib.lib()
    assert lib.ncde_smooth_pieces(9, 0.5) == 15 and lib.ncde_smooth_pieces(9, 1.0) == 8
    assert lib.ncde_smooth_pieces(9, 0.0) == -1 and lib.ncde_smooth_pieces(9, 1.25) == -1 and lib.ncde_smooth_pieces(1, 0.5) == -1


@pytest.mark.parametrize("name", ["g14_a_cubic_eps1_rk4", "g14_b_cubic_eps05_rk4", "g14_c_cubic_eps02_rk4_quarter",
                                  "g14_d_quintic_eps1_midpoint", "g14_e_quintic_eps05_rk4", "g14_f_quintic_eps03_euler_tenth"])
def test_time_plan_on_the_refined_grid_follows_the_region_rule(name):
    """ncde_time_plan_build on the refined knots: at every forward stage time the piece index / frac are those the reference's rule
    gives (index = bucketize(t) - 1 on the integer grid, matching region iff 0 < index and frac < eps).  The stage time is recovered
    from the plan itself (refined knot + frac); a stage that hits k + eps exactly may sit on either side."""
    import ncde_amd
    from ncde_amd import _lib
    f = dict(np.load(os.path.join(gu.GOLD, name + ".npz")))
    m = json.loads(str(f["meta"]))
    eps, T = m["eps"], f["coeffs"].shape[1]
    X = ncde_amd.SmoothLinearInterpolation(torch.from_numpy(f["coeffs"]), gradient_matching_eps=eps, match_second_derivatives=m["scheme"] == "quintic")
    kn, n_knots = X._plan_grid()
    kn_np = np.arange(T, dtype=np.float64) if kn is None else kn.numpy()
    tv = np.ascontiguousarray(f["t_out"].astype(np.float64))
    p = _lib.NcdeProblem()
    p.abi_version, p.n_knots, p.method = _lib.NCDE_ABI_VERSION, n_knots, _lib.METHOD[m["method"]]
    dp = ctypes.POINTER(ctypes.c_double)
    ts = _lib.NcdeTimeSpec(n_t=len(tv), time_is_f64=0, t=tv.ctypes.data_as(dp), step_size=float(m["step_size"]),
                           knots=None if kn is None else np.ascontiguousarray(kn_np).ctypes.data_as(dp))
    info = _lib.NcdeTimePlanInfo()
    lib = _lib.lib()
    assert lib.ncde_time_plan_build(ctypes.byref(p), ctypes.byref(ts), None, 0, ctypes.byref(info)) == 0
    buf = np.zeros(info.bytes // 4, dtype=np.int32)
    assert lib.ncde_time_plan_build(ctypes.byref(p), ctypes.byref(ts), buf.ctypes.data, buf.nbytes, ctypes.byref(info)) == 0
    S = {"euler": 1, "midpoint": 2, "rk4": 4}[m["method"]]
    assert S * (info.n_steps_fwd + info.n_steps_adj) == m["nfe"]          # the forward grid + the adjoint's (one reverse solve per output interval)
    header = (buf.size - info.n_steps_fwd * (3 + 3 * S) - 2 * info.n_t_out - info.n_steps_adj * (3 + 3 * S))
    assert header >= 5 and buf[1] == S and buf[2] == info.n_steps_fwd
    n_match = 0
    for n in range(info.n_steps_fwd):
        step = buf[header + n * (3 + 3 * S):]
        for j in range(S):
            idx, frac = int(step[3 + 3 * j]), float(step[4 + 3 * j:5 + 3 * j].view(np.float32)[0])
            t = kn_np[idx] + frac
            if abs(t - round(t)) < 1e-6:      # (frac is an fp32 number: a stage on an integer knot comes back a rounding error off it)
                t = float(round(t))
            k = min(max(int(np.ceil(t)) - 1, 0), T - 2)            # the reference's index: the left piece at an exact knot
            fr = t - k
            on_edge = abs(fr - eps) <= 1e-6
            matching = k > 0 and fr < eps
            if eps == 1:
                want = [k]
            else:
                want = [0] if k == 0 else ([2 * k - 1] if matching else [2 * k])
                if on_edge and k > 0:
                    want = [2 * k - 1, 2 * k]
            assert idx in want, (n, j, t, idx, want)
            assert 0.0 <= frac <= (kn_np[idx + 1] - kn_np[idx]) + 1e-6
            n_match += matching
    assert n_match > 0


def test_module_pickles_and_derived_tensors_follow_the_coefficients():
    """The smoothed schemes keep NeuralCDE picklable (torch.save(model)); the class's derived tensors are rebuilt when the
    coefficient tensor is replaced (X.double()) or edited in place."""
    import pickle
    import ncde_amd
    m = ncde_amd.NeuralCDE(4, 8, 2, interpolation="linear_quintic_smoothing", interpolation_eps=0.5)
    m2 = pickle.loads(pickle.dumps(m))
    X = m2.spline(torch.randn(2, 5, 4))
    assert X.gradient_matching_eps == 0.5 and X.match_second_derivatives
    assert X._matching[1] is None                                   # nothing built until a matching region is evaluated
    a = X.derivative(1.25)
    assert X._matching[1] is not None and X.gradient_matching_coeffs.dtype == torch.float32
    X = X.double()
    assert X.gradient_matching_coeffs.dtype == torch.float64 and X.derivative(1.25).dtype == torch.float64
    assert torch.allclose(X.derivative(1.25).float(), a, atol=1e-5)
    with torch.no_grad():
        X._coeffs.mul_(2.0)
    assert torch.allclose(X.derivative(1.25).float(), 2 * a, atol=1e-5)
