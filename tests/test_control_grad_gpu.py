"""Fused control-path gradients (ncde_backward_control: dL/dcoeffs of an adjoint=False solve) and StackedNeuralCDE, against golden
vectors produced by the imported reference (tools/gen_golden_control.py -> tests/golden/g16_*.npz, MANIFEST_control.json).

Tolerances: the project's own for reference goldens (tests/test_smooth_gpu.py:23): forward <= 2e-5, dL/dcoeffs,
dL/dz0 and every parameter gradient <= 2e-4, as |delta| relative to max |ref|.  The manifest records per case that max |dL/dcoeffs| is
>= 1e3 x that tolerance, that no interior row is zero, and that the fp32 reference sits within a quarter of each tolerance of its
fp64 self."""
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
CASES = ["g16_a_rect_rk4_interval", "g16_b_linear_midpoint_knots", "g16_c_cubic_rk4_knots", "g16_d_linear_userknots_euler_half",
         "g16_e_linear_rk4_interval_c24"]
FORCE_TILED, FP32_MFMA, NO_COOP = 0x8000, 4, 0x400
CONTROL_FLAGS = FORCE_TILED | FP32_MFMA | NO_COOP      # what ncde_backward_control applies internally (include/ncde_hip.h)
_CACHE = {}


def _load(name):
    if name not in _CACHE:      # read once, shared by the tests below, never modified
        f = dict(np.load(os.path.join(gu.GOLD, name + ".npz")))
        _CACHE[name] = (f, json.loads(str(f["meta"])))
    return _CACHE[name]


def _control(f, m, coeffs):
    import ncde_amd
    kn = torch.from_numpy(f["knots"]).cuda() if "knots" in f else None
    return (ncde_amd.NaturalCubicSpline if m["interp"] == "cubic" else ncde_amd.LinearInterpolation)(coeffs, kn)


def _times(f, m, X):
    return {"interval": lambda: X.interval, "knots": lambda: X.grid_points, "times": lambda: torch.from_numpy(f["t_out"]).cuda()}[m["outputs"]]()


def _run(f, m, flags=0, capture=None):
    """The case through cdeint(adjoint=False) with a coefficient leaf that requires grad.  ANY warning is an error here: the fused
    route emits none, and a call sent to the unfused solver warns."""
    import gpu_util
    import ncde_amd
    from ncde_amd import solver, unfused
    unfused._WARNED.clear()
    coeffs = torch.from_numpy(f["coeffs"]).cuda().requires_grad_(True)
    X = _control(f, m, coeffs)
    func = gpu_util.CaseField({k[2:]: f[k] for k in f if k.startswith("p_")}, [("W0", "b0")] + [("W1", "b1")] * (m["dims"]["nl"] - 1), "cuda")
    z0 = torch.from_numpy(f["z0"]).cuda().requires_grad_(True)
    real = solver.build_problem

    def spy(*a, **k):
        p = real(*a, **k)
        if capture is not None:
            capture.append(p)
        return p
    solver.build_problem = spy
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            out = ncde_amd.cdeint(X, func, z0, _times(f, m, X), adjoint=False, method=m["method"], options={"step_size": m["step_size"]},
                                  kernel_flags=flags)
            (out * torch.from_numpy(f["grad_out"]).cuda()).sum().backward()
        torch.cuda.synchronize()
    finally:
        solver.build_problem = real
    assert not unfused._WARNED, unfused._WARNED
    return {"z_out": out.detach().cpu().numpy(), "dcoeffs": coeffs.grad.cpu().numpy(), "dz0": z0.grad.cpu().numpy(),
            "grads": {k: v.grad.cpu().numpy() for k, v in func.p.items()}}


def _errors(res, f, m):
    errs = {"z": gu.relerr(res["z_out"], f["z_out"]), "dcoeffs": gu.relerr(res["dcoeffs"], f["dcoeffs"]), "dz0": gu.relerr(res["dz0"], f["dz0"])}
    for n in m["param_names"]:
        errs["d" + n] = gu.relerr(res["grads"][n], f["d" + n])
    return errs


@pytest.mark.parametrize("name", CASES)
def test_control_gradient_matches_reference_golden(name, gpu_lib):
    """Cases a - e through cdeint: solution, dL/dcoeffs, dL/dz0 and every parameter gradient.  Case e twice against ONE golden: the
    default window and windows of 3 steps (the fold across windows, a partial last window).  No warning, nothing unfused, and the
    control route names a batch-tiled kernel -- on the parent commit the symbol is missing and the call warns."""
    from ncde_amd import _lib
    f, m = _load(name)
    assert m["max_dcoeffs"] >= 1e3 * E2E_G
    assert m["ref_drift"]["z"] <= TIGHT_Z / 4 and max(v for k, v in m["ref_drift"].items() if k != "z") <= E2E_G / 4
    runs = [("default", 0)] + ([("windows of 3", 3 << 16)] if name.startswith("g16_e") else [])
    for label, flags in runs:
        probs = []
        res = _run(f, m, flags, capture=probs)
        kname = (gpu_lib.ncde_control_kernel_name(ctypes.byref(probs[-1])) or b"?").decode()
        assert "ncde_adj_tiled" in kname and "ncde_dctl_tiled" in kname and "ncde_dctl_fold" in kname, kname
        assert gpu_lib.ncde_control_workspace_bytes(ctypes.byref(probs[-1])) > 0
        assert res["z_out"].shape == f["z_out"].shape and res["dcoeffs"].shape == f["dcoeffs"].shape
        errs = _errors(res, f, m)
        print(m["name"], label, " ".join("%s %.2e" % kv for kv in errs.items()))
        assert errs["z"] <= TIGHT_Z, errs
        assert all(v <= E2E_G for k, v in errs.items() if k != "z"), errs
        if m["interp"] == "cubic":
            assert not res["dcoeffs"][..., :m["dims"]["C"]].any()      # the a columns: written, exactly zero
    assert _lib.FLAG_FORCE_TILED == FORCE_TILED and _lib.FLAG_FP32_MFMA == FP32_MFMA and _lib.FLAG_NO_COOP == NO_COOP


def _abi_backward(lib, f, m, control, flags=0):
    """forward_record + ncde_backward (control=False, with `flags`) or ncde_backward_control, straight on the C-ABI.
    -> (every buffer of NcdeGrads as one dict, grad_coeffs or None)"""
    import gpu_util
    from ncde_amd import _lib, solver
    coeffs = torch.from_numpy(f["coeffs"]).cuda()
    X = _control(f, m, coeffs)
    func = gpu_util.CaseField({k[2:]: f[k] for k in f if k.startswith("p_")}, [("W0", "b0")] + [("W1", "b1")] * (m["dims"]["nl"] - 1), "cuda")
    spec = func.fused_spec()
    z0 = torch.from_numpy(f["z0"]).cuda()
    plan = None
    output = {"interval": _lib.OUT_INTERVAL, "knots": _lib.OUT_KNOTS, "times": _lib.OUT_TIMES}[m["outputs"]]
    if output == _lib.OUT_TIMES or "knots" in f or m["step_size"] != 1:
        plan = solver._time_plan(X, _times(f, m, X), m["method"], m["step_size"], z0.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def ws_for(n):
        assert n > 0, lib.ncde_last_error_string()
        return torch.empty(int(n), dtype=torch.uint8, device="cuda")
    p = solver.build_problem(coeffs, m["interp"], z0, spec, m["method"], output, 0, plan)
    out = torch.empty(f["z_out"].shape, dtype=torch.float32, device="cuda")
    stages = torch.empty(int(lib.ncde_stage_record_bytes(ctypes.byref(p))) // 4, dtype=torch.float32, device="cuda")
    ws = ws_for(lib.ncde_workspace_bytes(ctypes.byref(p), 0))
    assert lib.ncde_forward_record(ctypes.byref(p), out.data_ptr(), stages.data_ptr(), ws.data_ptr(), ws.numel(), stream) == 0
    p = solver.build_problem(coeffs, m["interp"], z0, spec, m["method"], output, flags, plan)
    bound = solver.bind_grads(spec, z0.shape, z0.device, fill=float("nan"))
    g = bound.g
    bufs = {"z0": bound.grad_z0}
    bufs.update({k: bound.of(v) for k, v in func.p.items()})
    gout = torch.from_numpy(f["grad_out"]).cuda()
    gc = None
    if control:
        gc = torch.full_like(coeffs, float("nan"))
        ws = ws_for(lib.ncde_control_workspace_bytes(ctypes.byref(p)))
        rc = lib.ncde_backward_control(ctypes.byref(p), stages.data_ptr(), gout.data_ptr(), ctypes.byref(g), gc.data_ptr(), ws.data_ptr(),
                                       ws.numel(), stream)
    else:
        assert "tiled" in (lib.ncde_kernel_name(ctypes.byref(p), 2) or b"?").decode()
        ws = ws_for(lib.ncde_workspace_bytes(ctypes.byref(p), 2))
        rc = lib.ncde_backward(ctypes.byref(p), stages.data_ptr(), gout.data_ptr(), ctypes.byref(g), ws.data_ptr(), ws.numel(), stream)
    assert rc == 0, lib.ncde_last_error_string()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in bufs.items()}, (None if gc is None else gc.cpu().numpy())


@pytest.mark.parametrize("name,window", [("g16_a_rect_rk4_interval", 0), ("g16_d_linear_userknots_euler_half", 0), ("g16_e_linear_rk4_interval_c24", 3 << 16)])
def test_control_backward_is_ncde_backward_plus_grad_coeffs(name, window, gpu_lib):
    """`grads` of ncde_backward_control are bit-identical to ncde_backward called with the flags the control route applies internally
    (a zero-padded shape, a time plan, an aligned shape over several windows); grad_coeffs is fully written, matches the golden, and
    two consecutive calls give the same bits."""
    f, m = _load(name)
    base, _ = _abi_backward(gpu_lib, f, m, False, CONTROL_FLAGS | window)
    one, gc1 = _abi_backward(gpu_lib, f, m, True, window)
    two, gc2 = _abi_backward(gpu_lib, f, m, True, window)
    for k in base:
        assert np.isfinite(base[k]).all() and np.array_equal(base[k], one[k]) and np.array_equal(one[k], two[k]), k
    assert np.isfinite(gc1).all() and np.array_equal(gc1, gc2)
    assert gu.relerr(gc1, f["dcoeffs"]) <= E2E_G


def test_control_route_under_no_grad_keeps_no_stage_record(gpu_lib):
    """Case a through cdeint under torch.no_grad(): the same bits as with grad enabled, on the fused route (no warning), and the
    stage record is never sized -- ncde_stage_record_bytes is counted for the duration of the two calls: 0 queries, then 1."""
    import gpu_util
    import ncde_amd
    from ncde_amd import unfused
    f, m = _load("g16_a_rect_rk4_interval")
    unfused._WARNED.clear()
    coeffs = torch.from_numpy(f["coeffs"]).cuda().requires_grad_(True)
    X = _control(f, m, coeffs)
    func = gpu_util.CaseField({k[2:]: f[k] for k in f if k.startswith("p_")}, [("W0", "b0")] + [("W1", "b1")] * (m["dims"]["nl"] - 1), "cuda")
    z0 = torch.from_numpy(f["z0"]).cuda().requires_grad_(True)
    real, queries = gpu_lib.ncde_stage_record_bytes, []

    def counted(p):
        queries.append(1)
        return real(p)

    def solve():
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            return ncde_amd.cdeint(X, func, z0, _times(f, m, X), adjoint=False, method=m["method"], options={"step_size": m["step_size"]})
    gpu_lib.ncde_stage_record_bytes = counted
    try:
        with torch.no_grad():
            quiet = solve()
        n_quiet = len(queries)
        taped = solve()
    finally:
        gpu_lib.ncde_stage_record_bytes = real
    assert n_quiet == 0 and len(queries) == 1, (n_quiet, len(queries))
    assert not unfused._WARNED, unfused._WARNED
    assert not quiet.requires_grad and taped.requires_grad
    assert quiet.shape == f["z_out"].shape and torch.equal(quiet.view(torch.int32), taped.detach().view(torch.int32))
    assert gu.relerr(quiet.cpu().numpy(), f["z_out"]) <= TIGHT_Z


@pytest.mark.parametrize("seq", [True, False])
def test_stacked_module_matches_reference_golden(seq, gpu_lib):
    """Case f: ncde_amd.StackedNeuralCDE(3, [8, 6], 2, adjoint=False) with the reference's state_dict: output, every parameter gradient
    of both layers and the gradient of the input coefficients; both layers on the fused route (no warning at all)."""
    import ncde_amd
    from ncde_amd import unfused
    f, m = _load("g16_f_stacked")
    tag = "seq" if seq else "final"
    model = ncde_amd.StackedNeuralCDE(adjoint=False, return_sequences=seq, **m["ctor"])
    model.load_state_dict({k[3:]: torch.from_numpy(f[k]) for k in f if k.startswith("sd_")})      # the reference's, unchanged
    model = model.cuda()
    coeffs = torch.from_numpy(f["coeffs"]).cuda().requires_grad_(True)
    unfused._WARNED.clear()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = model(coeffs)
        (out * torch.from_numpy(f["grad_out_" + tag]).cuda()).sum().backward()
    assert not unfused._WARNED
    errs = {"out": gu.relerr(out.detach().cpu().numpy(), f["out_" + tag]), "dcoeffs": gu.relerr(coeffs.grad.cpu().numpy(), f["dcoeffs_" + tag])}
    for k, q in model.named_parameters():
        if k.startswith("fc_output"):
            assert q.grad is None      # exists, unused: as in the reference
            continue
        errs[k] = gu.relerr(q.grad.cpu().numpy(), f["g_%s__%s" % (tag, k)])
    print("g16_f_stacked", tag, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert sorted(k for k, _ in model.named_parameters()) == sorted(m["param_names"])
    assert errs["out"] <= TIGHT_Z, errs
    assert all(v <= E2E_G for k, v in errs.items() if k != "out"), errs


@pytest.mark.parametrize("what", ["quintic", "gru", "evaluate", "knots", "adjoint_params"])
def test_requests_outside_the_control_route_stay_unfused(what, gpu_lib):
    """A quintic control, the GRU field, the evaluate input, knots that require grad, adjoint=True with the coefficients in
    adjoint_params: each still runs on the unfused solver with its warning, and the control still receives a gradient."""
    import ncde_amd
    from ncde_amd import unfused
    f, m = _load("g16_d_linear_userknots_euler_half")
    d = m["dims"]
    torch.manual_seed(5)
    coeffs = torch.from_numpy(f["coeffs"]).cuda().requires_grad_(True)
    mode, adjoint, extra = "matmul", False, {}
    func = ncde_amd.OriginalVectorField(d["C"], d["H"], d["HH"], d["nl"]).cuda()
    X = ncde_amd.LinearInterpolation(coeffs)
    if what == "quintic":
        X = ncde_amd.SmoothLinearInterpolation(coeffs, gradient_matching_eps=0.5, match_second_derivatives=True)
    elif what == "gru":
        func = ncde_amd.GRUGatedVectorField(d["C"], d["H"], d["HH"], d["nl"]).cuda()
    elif what == "evaluate":
        mode = "evaluate"
        func = ncde_amd.OriginalVectorField(d["C"], d["H"], d["HH"], d["nl"], vector_field_type="evaluate").cuda()
    elif what == "knots":
        X = ncde_amd.LinearInterpolation(coeffs, torch.from_numpy(f["knots"]).cuda().requires_grad_(True))
    else:
        adjoint, extra = True, {"adjoint_params": tuple(func.parameters()) + (coeffs,)}
    z0 = torch.from_numpy(f["z0"]).cuda()
    t = torch.tensor([0.0, 2.5, 5.0], device="cuda")
    unfused._WARNED.clear()
    with pytest.warns(UserWarning, match="unfused torch-op solver .the control path requires gradients"):
        out = ncde_amd.cdeint(X, func, z0, t, adjoint=adjoint, vector_field_type=mode, method="rk4", options={"step_size": 0.5}, **extra)
    out.square().sum().backward()
    assert coeffs.grad is not None and torch.isfinite(coeffs.grad).all() and float(coeffs.grad.abs().max()) > 0


def test_control_gradient_on_a_wide_shape_vs_fp64_unfused(gpu_lib):
    """(C 7, H 256, HH 196, B 18, T 6): no golden -- the wide instantiation of the sweep, zero-padded C and HH, 16 row tiles of Wo per
    channel quad.  Reference: the unfused solver in fp64 on the GPU, as test_quintic_on_a_wide_shape_batch_tiled_vs_generic does."""
    import ncde_amd
    from ncde_amd import unfused
    B, L, C, H, HH, nl = 18, 6, 7, 256, 196, 2
    x = (gu.data.normal(51, B * L * C, stream=3).reshape(B, L, C) * 0.5).astype(np.float32)
    x[:, :, 0] = np.arange(L, dtype=np.float32)[None, :]
    p = gu.data.make_field_weights(H, HH, C, seed=29)
    f = {"coeffs": x, "z0": (gu.data.normal(53, B * H, stream=2).reshape(B, H) * 0.5).astype(np.float32)}
    f["grad_out"] = (gu.data.normal(27, B * L * H, stream=1).reshape(B, L, H) / 2.0).astype(np.float32)
    f.update({"p_" + k: v for k, v in p.items()})
    m = {"interp": "linear", "outputs": "knots", "method": "rk4", "step_size": 1, "dims": {"C": C, "H": H, "HH": HH, "nl": nl},
         "param_names": ["W0", "b0", "W1", "b1", "Wo", "bo"]}
    res = _run(f, m)
    func = ncde_amd.OriginalVectorField(C, H, HH, nl).double().cuda()
    sp = func.fused_spec()
    pp = {"W0": sp.layers[0][0], "b0": sp.layers[0][1], "W1": sp.layers[1][0], "b1": sp.layers[1][1], "Wo": sp.Wo, "bo": sp.bo}
    with torch.no_grad():
        for k, q in pp.items():
            q.copy_(torch.from_numpy(p[k]).double().reshape(q.shape))
    coeffs = torch.from_numpy(x).double().cuda().requires_grad_(True)
    X = ncde_amd.LinearInterpolation(coeffs)
    z0 = torch.from_numpy(f["z0"]).double().cuda().requires_grad_(True)
    unfused._WARNED.clear()
    with pytest.warns(UserWarning, match="unfused"):
        out = ncde_amd.cdeint(X, func, z0, X.grid_points, adjoint=False, method="rk4", options={"step_size": 1})
    (out * torch.from_numpy(f["grad_out"]).double().cuda()).sum().backward()
    ref = {"z_out": out.detach().cpu().numpy(), "dcoeffs": coeffs.grad.cpu().numpy(), "dz0": z0.grad.cpu().numpy()}
    ref.update({"d" + k: q.grad.cpu().numpy().reshape(res["grads"][k].shape) for k, q in pp.items()})
    errs = _errors(res, ref, m)
    print("wide control gradient", " ".join("%s %.2e" % kv for kv in errs.items()))
    assert float(np.abs(ref["dcoeffs"]).max()) >= 1e3 * E2E_G
    assert errs["z"] <= TIGHT_Z, errs
    assert all(v <= E2E_G for k, v in errs.items() if k != "z"), errs


@pytest.mark.parametrize("method", ["midpoint", "rk4"])
def test_control_gradient_under_a_time_plan_with_several_stages(method, gpu_lib):
    """The fold's stage order under a time plan with S > 1 (the goldens walk a plan with euler only): case d's inputs -- non-uniform
    user knots, output times between knots, step 0.5 -- with midpoint / rk4, against the unfused solver in fp64 on the GPU.  Same bounds."""
    import ncde_amd
    from ncde_amd import unfused
    f0, m0 = _load("g16_d_linear_userknots_euler_half")
    d = m0["dims"]
    for interp in ("linear",):
        f = dict(f0)
        if interp == "cubic":      # the same path as spline rows on the user grid: a = x_k, b = slope, and nonzero 2c / 3d so that frac matters
            x, kn = f0["coeffs"], f0["knots"]
            slope = (x[:, 1:] - x[:, :-1]) / (kn[1:] - kn[:-1])[None, :, None]
            f["coeffs"] = np.ascontiguousarray(np.concatenate([x[:, :-1], slope, 0.3 * slope, -0.2 * x[:, :-1]], axis=2), dtype=np.float32)
        m = dict(m0, interp=interp, method=method)
        func = ncde_amd.OriginalVectorField(d["C"], d["H"], d["HH"], d["nl"]).double().cuda()
        sp = func.fused_spec()
        pp = {"W0": sp.layers[0][0], "b0": sp.layers[0][1], "W1": sp.layers[1][0], "b1": sp.layers[1][1], "Wo": sp.Wo, "bo": sp.bo}
        with torch.no_grad():
            for k, q in pp.items():
                q.copy_(torch.from_numpy(f["p_" + k]).double().reshape(q.shape))
        coeffs = torch.from_numpy(f["coeffs"]).double().cuda().requires_grad_(True)
        kn64 = torch.from_numpy(f["knots"]).double().cuda()
        X = (ncde_amd.NaturalCubicSpline if interp == "cubic" else ncde_amd.LinearInterpolation)(coeffs, kn64)
        z0 = torch.from_numpy(f["z0"]).double().cuda().requires_grad_(True)
        unfused._WARNED.clear()
        with pytest.warns(UserWarning, match="unfused"):
            out = ncde_amd.cdeint(X, func, z0, torch.from_numpy(f["t_out"]).double().cuda(), adjoint=False, method=method, options={"step_size": 0.5})
        (out * torch.from_numpy(f["grad_out"]).double().cuda()).sum().backward()
        ref = {"z_out": out.detach().cpu().numpy(), "dcoeffs": coeffs.grad.cpu().numpy(), "dz0": z0.grad.cpu().numpy()}
        ref.update({"d" + k: q.grad.cpu().numpy().reshape(f["p_" + k].shape) for k, q in pp.items()})
        res = _run(f, m)
        errs = _errors(res, ref, m)
        print("planned", method, interp, " ".join("%s %.2e" % kv for kv in errs.items()))
        assert float(np.abs(ref["dcoeffs"]).max()) >= 1e3 * E2E_G
        assert errs["z"] <= TIGHT_Z, errs
        assert all(v <= E2E_G for k, v in errs.items() if k != "z"), errs
