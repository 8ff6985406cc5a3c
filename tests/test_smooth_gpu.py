"""Smoothed-linear control paths (ncde_amd.SmoothLinearInterpolation: cubic / quintic matching) on the fused kernels, against golden
vectors produced by the imported reference (tools/gen_golden_smooth.py -> tests/golden/g14_*.npz, MANIFEST_smooth.json).

Tolerances: the project's own for reference goldens on a general time axis (tests/test_gpu_parity.py:20-21).  The manifest records, per
case, that the reference's smoothed solve differs from its linear one by >= 100 x TIGHT_Z (``vs_linear``) -- a silent fall-back to
linear interpolation cannot pass -- and that the fp32 reference sits within a quarter of each tolerance of its fp64 self (``ref_drift``).

dopri5 on a smoothed path runs on the unfused solver through the class's torch restatement: cases j1 (the module in fp64, the reference's
own configuration) and j2 (pinned step, fp32)."""
import ctypes
import json
import os
import warnings

import numpy as np
import pytest
import torch

import golden_util as gu

pytestmark = pytest.mark.gpu

TIGHT_Z, E2E_G = 2e-5, 2e-4
CASES = ["g14_a_cubic_eps1_rk4", "g14_b_cubic_eps05_rk4", "g14_c_cubic_eps02_rk4_quarter", "g14_d_quintic_eps1_midpoint",
         "g14_e_quintic_eps05_rk4", "g14_f_quintic_eps03_euler_tenth", "g14_g_quintic_eps1_gru_evaluate", "g14_h_quintic_eps05_rk4_half_c20"]
FORCE_GENERIC, FORCE_FAST, FORCE_TILED = 1, 2, 0x8000


def _load(name):
    f = dict(np.load(os.path.join(gu.GOLD, name + ".npz")))
    return f, json.loads(str(f["meta"]))


def _control(f, m, device="cuda"):
    import ncde_amd
    return ncde_amd.SmoothLinearInterpolation(torch.from_numpy(f["coeffs"]).to(device), gradient_matching_eps=m["eps"],
                                              match_second_derivatives=m["scheme"] == "quintic")


def _run(f, m, adjoint, flags=0, X=None, params=None, capture=None):
    """The case through cdeint; capture (a list) receives the NcdeProblem structs the solver built."""
    import gpu_util
    import ncde_amd
    from ncde_amd import solver
    X = X if X is not None else _control(f, m)
    params = params if params is not None else {k[2:]: f[k] for k in f if k.startswith("p_")}
    func = gpu_util.CaseField(params, [("W0", "b0")] + [("W1", "b1")] * (m["dims"]["nl"] - 1), "cuda", m["field_kind"], m["field_mode"])
    z0 = torch.from_numpy(f["z0"]).cuda().requires_grad_(True)
    t = {"interval": lambda: X.interval, "knots": lambda: X.grid_points, "times": lambda: torch.from_numpy(f["t_out"]).cuda()}[m["outputs"]]()
    real = solver.build_problem

    def spy(*a, **k):
        p = real(*a, **k)
        if capture is not None:
            capture.append(p)
        return p
    solver.build_problem = spy
    try:
        with warnings.catch_warnings():      # (a call routed to the unfused solver warns: not here)
            warnings.filterwarnings("error", message=".*unfused.*")
            out = ncde_amd.cdeint(X, func, z0, t, adjoint=adjoint, vector_field_type=m["field_mode"], method=m["method"],
                                  options={"step_size": m["step_size"]}, kernel_flags=flags)
            nfe_fwd = func.nfe
            (out * torch.from_numpy(f["grad_out"]).cuda()).sum().backward()
        torch.cuda.synchronize()
    finally:
        solver.build_problem = real
    return {"z_out": out.detach().cpu().numpy(), "dz0": z0.grad.cpu().numpy(), "nfe": func.nfe, "nfe_fwd": nfe_fwd,
            "grads": {k: v.grad.cpu().numpy() for k, v in func.p.items() if v.grad is not None}}


def _check(f, m, flags, label):
    res = _run(f, m, True, flags)
    assert res["z_out"].shape == f["z_out"].shape
    errs = {"z": gu.relerr(res["z_out"], f["z_out"]), "dz0": gu.relerr(res["dz0"], f["dz0"])}
    for n in m["param_names"]:
        errs["d" + n] = gu.relerr(res["grads"][n], f["d" + n])
    resd = _run(f, m, False, flags)
    errs["bp_dz0"] = gu.relerr(resd["dz0"], f["bp_dz0"])
    for n in m["param_names"]:
        errs["bp_d" + n] = gu.relerr(resd["grads"][n], f["bp_d" + n])
    print(m["name"], label, "vs_linear %.2e" % m["vs_linear"], " ".join("%s %.2e" % kv for kv in errs.items()))
    assert errs["z"] <= TIGHT_Z, errs
    assert all(v <= E2E_G for k, v in errs.items() if k != "z"), errs
    assert res["nfe"] == m["nfe"]                            # the reference's own counter (forward + adjoint sweep)
    assert np.array_equal(resd["z_out"], res["z_out"])       # the recording forward is the same forward


@pytest.mark.parametrize("name", CASES)
def test_smoothed_path_matches_reference_golden(name, gpu_lib):
    """Cases a - h: z_out, dz0 and every parameter gradient with adjoint=True and adjoint=False; nfe equal to the reference's."""
    f, m = _load(name)
    assert m["vs_linear"] >= 100 * TIGHT_Z
    assert m["ref_drift"]["z"] <= TIGHT_Z / 4 and max(v for k, v in m["ref_drift"].items() if k != "z") <= E2E_G / 4
    _check(f, m, 0, "default")
    if m["scheme"] == "quintic":
        _check(f, m, FORCE_GENERIC, "generic")


def test_quintic_dispatch_never_takes_a_register_resident_set(gpu_lib):
    """Case h, (C, H, HH) = (20, 32, 32): a shape with a register-resident kernel set.  A piecewise-quintic control runs batch-tiled
    under default flags, NCDE_FLAG_FORCE_FAST is NCDE_ERR_UNSUPPORTED, and the dopri5 entry points refuse the kind."""
    from ncde_amd import _lib
    lib = _lib.lib()
    f, m = _load("g14_h_quintic_eps05_rk4_half_c20")
    probs = []
    _run(f, m, True, 0, capture=probs)
    p = probs[-1]
    assert p.interp == _lib.INTERP["quintic"] == 2
    for ps in (0, 1, 2):
        name = (lib.ncde_kernel_name(ctypes.byref(p), ps) or b"?").decode()
        assert "tiled" in name, (ps, name)
    p.flags = FORCE_FAST
    for ps in (0, 1, 2):
        assert lib.ncde_workspace_bytes(ctypes.byref(p), ps) == -2
        assert lib.ncde_kernel_name(ctypes.byref(p), ps) is None
    p.flags = 0
    # the same shape as a cubic control does have its register-resident set: the refusal above is the quintic kind's
    p.interp = _lib.INTERP["cubic"]
    assert "tiled" not in (lib.ncde_kernel_name(ctypes.byref(p), 0) or b"?").decode()
    p.interp = _lib.INTERP["quintic"]
    tv = (ctypes.c_double * 2)(0.0, 8.0)
    ts = _lib.NcdeTimeSpec(n_t=2, time_is_f64=1, t=ctypes.cast(tv, ctypes.POINTER(ctypes.c_double)), step_size=1.0, knots=None)
    assert lib.ncde_dopri5_workspace_bytes(ctypes.byref(p), ctypes.byref(ts), 0) == -2
    # a coefficient row narrower than 6C is refused
    p.coeffs_stride_t = 6 * p.channels - 1
    assert lib.ncde_workspace_bytes(ctypes.byref(p), 0) == -1


def test_cubic_smoothing_eps1_runs_on_the_default_axis_kernels(gpu_lib):
    """Case a (eps = 1: the refined grid is the integer grid again): the same kernel a NaturalCubicSpline of that shape gets."""
    import gpu_util
    import ncde_amd
    from ncde_amd import _lib, solver
    lib = _lib.lib()
    f, m = _load("g14_a_cubic_eps1_rk4")
    probs = []
    _run(f, m, True, 0, capture=probs)
    p = probs[-1]
    assert p.output == _lib.OUT_INTERVAL and not p.time_plan
    X = _control(f, m)
    spline = ncde_amd.NaturalCubicSpline(X.fused_coeffs)
    func = gpu_util.CaseField({k[2:]: f[k] for k in f if k.startswith("p_")}, [("W0", "b0"), ("W1", "b1"), ("W1", "b1")], "cuda")
    q = solver.build_problem(spline.fused_coeffs, "cubic", torch.from_numpy(f["z0"]).cuda(), func.fused_spec(), "rk4", _lib.OUT_INTERVAL, 0)
    for ps in (0, 1, 2):
        assert lib.ncde_kernel_name(ctypes.byref(p), ps) == lib.ncde_kernel_name(ctypes.byref(q), ps) is not None


@pytest.mark.parametrize("name", CASES)
def test_prepare_smooth_matches_the_reference_coefficients(name, gpu_lib):
    """ncde_prepare_smooth against the fp32 golden matching coefficients: <= 4 x the case's recorded coeff_drift (two fp32
    evaluations of one formula with different contraction: their errors add, x 2 slack); linear pieces exactly."""
    f, m = _load(name)
    X = _control(f, m)
    C, T = f["coeffs"].shape[2], f["coeffs"].shape[1]
    order = 5 if m["scheme"] == "quintic" else 3
    got = X.fused_coeffs.cpu().numpy()
    P = 2 * T - 3 if m["eps"] < 1 else T - 1
    assert got.shape == (f["coeffs"].shape[0], P, (order + 1) * C)
    got = got.reshape(got.shape[0], P, order + 1, C)
    mc = f["matching_coeffs"]                                   # [B, T-2, C, order+1], highest power first
    match = got[:, 1::2] if m["eps"] < 1 else got[:, 1:]
    want = np.stack([mc[..., order - q] * np.float32(max(q, 1)) for q in range(order + 1)], axis=2)      # a | b | 2c | 3d | ...
    err = float(np.abs(match.astype(np.float64) - want.astype(np.float64)).max())
    print(m["name"], "coeff err %.3e" % err, "coeff_drift %.3e" % m["coeff_drift"])
    assert err <= 4 * m["coeff_drift"], (err, m["coeff_drift"])
    x = f["coeffs"]
    assert np.array_equal(got[:, 0, 0], x[:, 0]) and np.array_equal(got[:, 0, 1], x[:, 1] - x[:, 0]) and not got[:, 0, 2:].any()
    if m["eps"] < 1:
        lin = got[:, 2::2]
        assert np.array_equal(lin[:, :, 1], x[:, 2:] - x[:, 1:-1]) and not lin[:, :, 2:].any()
        assert np.array_equal(lin[:, :, 0], x[:, 1:-1] + np.float32(m["eps"]) * (x[:, 2:] - x[:, 1:-1]))


def test_quintic_on_a_wide_shape_batch_tiled_vs_generic(gpu_lib):
    """(C 7, H 256, HH 196): no golden; quintic on the batch-tiled family (zero-padded) against quintic on the generic family at the
    TIGHT_Z test_general_time_axis_on_the_wide_sweeps_vs_oracle applies to this shape.  The generic family has a forward for this shape
    but no backward (last hidden width > 128), so the independent reference for the gradients -- at E2E_G, continuous adjoint and exact
    discrete backward -- is the unfused solver in fp64 on the class's torch restatement; one and several time windows."""
    import ncde_amd
    from ncde_amd import _lib, solver, unfused
    lib = _lib.lib()
    B, L, C, H, HH, nl = 21, 7, 7, 256, 196, 2
    x = (gu.data.normal(51, B * L * C, stream=3).reshape(B, L, C) * 0.5).astype(np.float32)
    x[:, :, 0] = np.arange(L, dtype=np.float32)[None, :]
    p = gu.data.make_field_weights(H, HH, C, seed=29)
    f = {"coeffs": x, "z0": (gu.data.normal(53, B * H, stream=2).reshape(B, H) * 0.5).astype(np.float32),
         "t_out": np.array([0.0, 1.5, 3.0, 4.05, 5.875], np.float32)}
    f["grad_out"] = (gu.data.normal(27, B * 5 * H, stream=1).reshape(B, 5, H) / 2.0).astype(np.float32)
    f.update({"p_" + k: v for k, v in p.items()})
    m = {"eps": 0.5, "scheme": "quintic", "outputs": "times", "method": "rk4", "step_size": 0.75, "field_kind": "original",
         "field_mode": "matmul", "dims": {"C": C, "H": H, "HH": HH, "nl": nl}}
    probs = []
    tiled = {True: _run(f, m, True, 0, params=p, capture=probs), False: _run(f, m, False, 0, params=p)}
    for ps in (0, 1):
        assert "tiled" in (lib.ncde_kernel_name(ctypes.byref(probs[-1]), ps) or b"?").decode()
    generic = _run_forward_only(f, m, FORCE_GENERIC, p)
    assert gu.relerr(tiled[True]["z_out"], generic) <= TIGHT_Z, gu.relerr(tiled[True]["z_out"], generic)
    windows = {True: _run(f, m, True, 3 << 16, params=p), False: _run(f, m, False, 3 << 16, params=p)}
    func, pp = _original_field(f, m, torch.float64)
    X = ncde_amd.SmoothLinearInterpolation(torch.from_numpy(x).double().cuda(), gradient_matching_eps=0.5, match_second_derivatives=True)
    for adjoint in (True, False):
        for q in func.parameters():
            q.grad = None
        z0 = torch.from_numpy(f["z0"]).double().cuda().requires_grad_(True)
        unfused._WARNED.clear()
        with pytest.warns(UserWarning, match="not fp32"):
            out = ncde_amd.cdeint(X, func, z0, torch.from_numpy(f["t_out"]).double().cuda(), adjoint=adjoint, method="rk4", options={"step_size": 0.75})
        (out * torch.from_numpy(f["grad_out"]).double().cuda()).sum().backward()
        for label, res in (("default", tiled[adjoint]), ("windows", windows[adjoint])):
            errs = {"z": gu.relerr(res["z_out"], out.detach().cpu().numpy()), "dz0": gu.relerr(res["dz0"], z0.grad.cpu().numpy())}
            for n, q in pp.items():
                errs["d" + n] = gu.relerr(res["grads"][n], q.grad.cpu().numpy().reshape(res["grads"][n].shape))
            print("wide quintic adjoint=%s %s" % (adjoint, label), " ".join("%s %.2e" % kv for kv in errs.items()))
            assert errs["z"] <= TIGHT_Z, errs
            assert all(v <= E2E_G for k, v in errs.items() if k != "z"), errs


def _run_forward_only(f, m, flags, params):
    import gpu_util
    import ncde_amd
    X = _control(f, m)
    func = gpu_util.CaseField(params, [("W0", "b0")] + [("W1", "b1")] * (m["dims"]["nl"] - 1), "cuda", m["field_kind"], m["field_mode"])
    with torch.no_grad():
        out = ncde_amd.cdeint(X, func, torch.from_numpy(f["z0"]).cuda(), torch.from_numpy(f["t_out"]).cuda(), adjoint=True,
                              method=m["method"], options={"step_size": m["step_size"]}, kernel_flags=flags)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_eps_none_is_linear_interpolation(gpu_lib):
    """gradient_matching_eps=None: bit-equal to LinearInterpolation on the same input, forward and gradients."""
    import ncde_amd
    f, m = _load("g14_b_cubic_eps05_rk4")
    m = dict(m, eps=None)
    a = _run(f, m, True, 0)
    b = _run(f, m, True, 0, X=ncde_amd.LinearInterpolation(torch.from_numpy(f["coeffs"]).cuda()))
    assert np.array_equal(a["z_out"], b["z_out"]) and np.array_equal(a["dz0"], b["dz0"])
    for n in a["grads"]:
        assert np.array_equal(a["grads"][n], b["grads"][n]), n
    assert gu.relerr(a["z_out"], f["z_out"]) >= 100 * TIGHT_Z      # (and NOT the smoothed solve)


def test_neural_cde_module_with_a_smoothed_scheme(gpu_lib):
    """NeuralCDE(interpolation='linear_quintic_smoothing', interpolation_eps=0.5): forward and backward run fused (no unfused warning),
    differ from the plain linear model, and dopri5 on a smoothed path goes to the unfused solver with its warning."""
    import ncde_amd
    from ncde_amd import unfused
    f, _ = _load("g14_e_quintic_eps05_rk4")
    x = torch.from_numpy(f["coeffs"]).cuda()
    torch.manual_seed(3)
    model = ncde_amd.NeuralCDE(5, 16, 2, hidden_hidden_dim=24, num_layers=3, interpolation="linear_quintic_smoothing", interpolation_eps=0.5).cuda()
    lin = ncde_amd.NeuralCDE(5, 16, 2, hidden_hidden_dim=24, num_layers=3, interpolation="linear").cuda()
    lin.load_state_dict(model.state_dict())
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*unfused.*")
        out = model(x)
        out.square().sum().backward()
    assert all(torch.isfinite(q.grad).all() for q in model.parameters())
    assert float((out - lin(x)).abs().max()) > 1e-4
    unfused._WARNED.clear()
    dp = ncde_amd.NeuralCDE(5, 16, 2, hidden_hidden_dim=24, num_layers=3, interpolation="linear_cubic_smoothing", interpolation_eps=1,
                            solver="dopri5").cuda()
    with pytest.warns(UserWarning, match="smoothed-linear"):
        assert torch.isfinite(dp(x)).all()


def _original_field(f, m, dtype=torch.float32):
    """ncde_amd.OriginalVectorField carrying a case's p_* weights (a callable module: what the unfused solver needs)."""
    import ncde_amd
    d = m["dims"]
    func = ncde_amd.OriginalVectorField(d["C"], d["H"], d["HH"], d["nl"]).to(dtype).cuda()
    sp = func.fused_spec()
    p = {"W0": sp.layers[0][0], "b0": sp.layers[0][1], "Wo": sp.Wo, "bo": sp.bo}
    if d["nl"] > 1:
        p["W1"], p["b1"] = sp.layers[1]
    with torch.no_grad():
        for k, q in p.items():
            q.copy_(torch.from_numpy(f["p_" + k]).to(dtype).reshape(q.shape))
    return func, p


def test_j1_module_dopri5_fp64_takes_the_reference_step_sequence(gpu_lib):
    """Case j1, the reference's own configuration: NeuralCDE(interpolation='linear_cubic_smoothing', interpolation_eps=1, solver='dopri5',
    adjoint=False) -- min_step 0.5 -- as a module in fp64 with the reference's state_dict.  Unfused dopri5 (warning expected).  As in
    test_unfused_dopri5_taped_gradient_includes_the_first_step_size both sides take the same free-running step sequence in fp64: the
    accepted / rejected counts equal the recorded ones (asserted first), then output and every gradient at 1e-10."""
    import ncde_amd
    from ncde_amd import unfused
    f, m = _load("g14_j1_module_dopri5_f64")
    d = m["dims"]
    model = ncde_amd.NeuralCDE(d["C"], d["H"], d["OUT"], hidden_hidden_dim=d["HH"], num_layers=d["nl"], interpolation="linear_cubic_smoothing",
                               interpolation_eps=1, solver="dopri5", adjoint=False).double()
    model.load_state_dict({k[3:]: torch.from_numpy(f[k]) for k in f if k.startswith("sd_")})      # the reference's, unchanged
    model = model.cuda()
    unfused._WARNED.clear()
    with pytest.warns(UserWarning, match="smoothed-linear"):
        out = model(torch.from_numpy(f["coeffs"]).cuda())
    st = model.func.dopri5_stats
    print("j1 steps", st["accepted"], st["rejected"], "recorded", m["steps_fwd"])
    assert [st["accepted"], st["rejected"]] == m["steps_fwd"] and m["steps_fwd"][1] >= 1
    assert out.dtype == torch.float64
    (out * torch.from_numpy(f["grad_out"]).cuda()).sum().backward()
    errs = {"out": gu.relerr(out.detach().cpu().numpy(), f["out"])}
    for k, q in model.named_parameters():
        errs[k] = gu.relerr(q.grad.cpu().numpy(), f["g_" + k])
    print("j1", " ".join("%s %.2e" % kv for kv in errs.items()))
    assert sorted(k for k, _ in model.named_parameters()) == sorted(m["param_names"])
    assert all(v <= 1e-10 for v in errs.values()), errs


def test_j2_cdeint_dopri5_pinned_step_matches_reference_golden(gpu_lib):
    """Case j2: cdeint(method='dopri5') in fp32 on the cubic-smoothed path with a pinned step (first_step = min_step = max_step = 0.75),
    adjoint=True and adjoint=False, at the pinned-step bounds of tests/test_unfused_gpu.py:188-200: 1e-5 forward, 1e-4 gradients
    (adjoint=False against the reference's own adjoint=False gradients, which the golden holds)."""
    import ncde_amd
    from ncde_amd import unfused
    f, m = _load("g14_j2_cdeint_dopri5_pinned")
    assert m["vs_linear"] >= 100 * 1e-5 and m["ref_drift"]["z"] <= 1e-5 / 4 and max(v for k, v in m["ref_drift"].items() if k != "z") <= 1e-4 / 4
    func, p = _original_field(f, m)
    X = _control(f, m)
    for adjoint, pre in ((True, ""), (False, "bp_")):
        for q in func.parameters():
            q.grad = None
        z0 = torch.from_numpy(f["z0"]).cuda().requires_grad_(True)
        unfused._WARNED.clear()
        with pytest.warns(UserWarning, match="smoothed-linear"):
            out = ncde_amd.cdeint(X, func, z0, X.grid_points, adjoint=adjoint, method="dopri5", rtol=m["rtol"], atol=m["atol"], options=dict(m["options"]))
        st = func.dopri5_stats
        assert [st["accepted"], st["rejected"]] == m["steps_fwd"]
        (out * torch.from_numpy(f["grad_out"]).cuda()).sum().backward()
        errs = {"z": gu.relerr(out.detach().cpu().numpy(), f["z_out"]), "dz0": gu.relerr(z0.grad.cpu().numpy(), f[pre + "dz0"])}
        for n in m["param_names"]:
            errs["d" + n] = gu.relerr(p[n].grad.cpu().numpy().reshape(f[pre + "d" + n].shape), f[pre + "d" + n])
        print("j2 adjoint=%s" % adjoint, " ".join("%s %.2e" % kv for kv in errs.items()))
        assert errs["z"] <= 1e-5, errs
        assert all(v <= 1e-4 for k, v in errs.items() if k != "z"), errs
