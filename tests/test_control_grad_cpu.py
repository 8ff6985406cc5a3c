"""CPU side of the fused control-path gradients: the g16 fixtures mean what they claim (the unfused torch-op solver, plain torch on
the CPU, reproduces them), the new C-ABI queries, the routing predicate, and the StackedNeuralCDE module's surface."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import golden_util as gu
import ncde_amd
from ncde_amd import _lib, solver, unfused

CASES = ["g16_a_rect_rk4_interval", "g16_b_linear_midpoint_knots", "g16_c_cubic_rk4_knots", "g16_d_linear_userknots_euler_half",
         "g16_e_linear_rk4_interval_c24"]


def _load(name):
    f = dict(np.load(os.path.join(gu.GOLD, name + ".npz")))
    return f, json.loads(str(f["meta"]))


def _manifest():
    with open(os.path.join(gu.GOLD, "MANIFEST_control.json")) as fh:
        return {m["name"]: m for m in json.load(fh)}


@pytest.mark.parametrize("name", CASES)
def test_unfused_solver_reproduces_the_golden_control_gradient(name):
    """cdeint_unfused (adjoint=False, autograd through the torch-op solve) on the CPU against the reference's dL/dcoeffs, solution,
    dL/dz0 and parameter gradients, at the 1e-6 level the unfused solver is pinned at on reference goldens.  Measured here, fp32,
    max over the five cases: z 0 (bit-equal), dcoeffs 2.0e-7, dz0 1.8e-7, parameters 3.5e-7."""
    f, m = _load(name)
    assert _manifest()[name] == m
    d = m["dims"]
    func = ncde_amd.OriginalVectorField(d["C"], d["H"], d["HH"], d["nl"])
    sp = func.fused_spec()
    pp = {"W0": sp.layers[0][0], "b0": sp.layers[0][1], "W1": sp.layers[1][0], "b1": sp.layers[1][1], "Wo": sp.Wo, "bo": sp.bo}
    with torch.no_grad():
        for k, q in pp.items():
            q.copy_(torch.from_numpy(f["p_" + k]).reshape(q.shape))
    coeffs = torch.from_numpy(f["coeffs"]).requires_grad_(True)
    kn = torch.from_numpy(f["knots"]) if "knots" in f else None
    X = (ncde_amd.NaturalCubicSpline if m["interp"] == "cubic" else ncde_amd.LinearInterpolation)(coeffs, kn)
    z0 = torch.from_numpy(f["z0"]).requires_grad_(True)
    out = unfused.cdeint_unfused(X, func, z0, torch.from_numpy(f["t_out"]), False, "matmul", m["method"], m["step_size"])
    (out * torch.from_numpy(f["grad_out"])).sum().backward()
    errs = {"z": gu.relerr(out.detach().numpy(), f["z_out"]), "dcoeffs": gu.relerr(coeffs.grad.numpy(), f["dcoeffs"]),
            "dz0": gu.relerr(z0.grad.numpy(), f["dz0"])}
    for n in m["param_names"]:
        errs["d" + n] = gu.relerr(pp[n].grad.numpy().reshape(f["d" + n].shape), f["d" + n])
    print(name, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert all(v <= 1e-6 for v in errs.values()), errs
    # what the generator enforced: a gradient far above the GPU tests' tolerance, no zero interior row, zero `a` columns
    dc = f["dcoeffs"]
    assert np.abs(dc).max() >= 1e3 * 2e-4 and (np.abs(dc).max(axis=(0, 2))[1:-1] >= 1e-2 * np.abs(dc).max()).all()
    if m["interp"] == "cubic":
        assert not dc[..., :d["C"]].any()


@pytest.mark.parametrize("seq", [True, False])
def test_unfused_chain_reproduces_the_golden_stacked_model(seq):
    """Case f: the package's StackedNeuralCDE with the reference's state_dict, its layers chained by hand over the unfused solver
    (cdeint itself refuses CPU tensors): output, dL/dcoeffs and every parameter gradient.  Measured here: <= 4.3e-7."""
    f, m = _load("g16_f_stacked")
    tag = "seq" if seq else "final"
    model = ncde_amd.StackedNeuralCDE(adjoint=False, return_sequences=seq, **m["ctor"])
    model.load_state_dict({k[3:]: torch.from_numpy(f[k]) for k in f if k.startswith("sd_")})
    coeffs = torch.from_numpy(f["coeffs"]).requires_grad_(True)
    h = coeffs
    for layer in model.ncdes:
        X, z0 = layer._control_and_start(h)
        t = X.grid_points if layer.return_sequences else X.interval
        h = layer._readout(unfused.cdeint_unfused(X, layer.func, z0, t, False, "matmul", "rk4", 1))
    (h * torch.from_numpy(f["grad_out_" + tag])).sum().backward()
    errs = {"out": gu.relerr(h.detach().numpy(), f["out_" + tag]), "dcoeffs": gu.relerr(coeffs.grad.numpy(), f["dcoeffs_" + tag])}
    for k, q in model.named_parameters():
        if not k.startswith("fc_output"):
            errs[k] = gu.relerr(q.grad.numpy(), f["g_%s__%s" % (tag, k)])
    print("g16_f_stacked", tag, "max %.2e" % max(errs.values()))
    assert all(v <= 1e-6 for v in errs.values()), errs


def _problem(B=32, T=49, C=20, H=32, HH=32, nl=3, interp=0, method=2, output=0, flags=0):
    """A structurally valid problem with dummy (never dereferenced) device pointers."""
    p = _lib.NcdeProblem()
    p.abi_version = _lib.NCDE_ABI_VERSION
    p.batch, p.n_knots, p.channels, p.hidden = B, T, C, H
    p.interp, p.method, p.output, p.flags = interp, method, output, flags
    p.n_layers = nl
    for l in range(nl):
        p.layer_in[l], p.layer_out[l] = (H if l == 0 else HH), HH
        p.layer_W[l] = 0x1000 if l == 0 else 0x2000
        p.layer_b[l] = 0x1100 if l == 0 else 0x2100
    p.Wo, p.bo, p.coeffs, p.z0 = 0x3000, 0x3100, 0x4000, 0x5000
    parts = {0: 1, 1: 4, 2: 6}[interp]
    p.coeffs_stride_b, p.coeffs_stride_t = T * parts * C, parts * C
    return p


def test_control_queries_name_the_tiled_kernels_or_refuse():
    lib = ncde_amd.lib()
    for kw in (dict(), dict(interp=1), dict(method=0, output=1), dict(C=5, H=8, HH=12, nl=2), dict(C=7, H=256, HH=196, nl=2, B=18, T=6),
               dict(flags=_lib.FLAG_FORCE_FAST)):      # (of the caller's flags only the window override is read)
        p = _problem(**kw)
        name = lib.ncde_control_kernel_name(ctypes.byref(p))
        assert name is not None and b"ncde_adj_tiled" in name and name.endswith(b"+ncde_dctl_tiled+ncde_dctl_fold"), (kw, name)
        assert lib.ncde_control_workspace_bytes(ctypes.byref(p)) > 0
    # (32, 32, 20) has a register-resident kernel set; the control route does not take it, ncde_backward still does
    p = _problem()
    assert b"fast" in lib.ncde_kernel_name(ctypes.byref(p), 2) and b"wide" not in lib.ncde_control_kernel_name(ctypes.byref(p))
    assert b"wide" in lib.ncde_control_kernel_name(ctypes.byref(_problem(C=7, H=256, HH=196, nl=2)))
    # the window buffer grows with the window: more steps per window, more workspace
    small = lib.ncde_control_workspace_bytes(ctypes.byref(_problem(flags=_lib.FLAG_TILED_WINDOW_STEPS(2))))
    assert 0 < small < lib.ncde_control_workspace_bytes(ctypes.byref(_problem(flags=_lib.FLAG_TILED_WINDOW_STEPS(8))))
    refused = []
    p = _problem(interp=2)
    refused.append(("quintic", p))
    p = _problem()
    p.field_kind, p.Wg, p.bg = 1, 0x6000, 0x6100
    refused.append(("gated", p))
    p = _problem()
    p.field_input = 1
    p.layer_in[0] = p.hidden + p.channels
    refused.append(("evaluate", p))
    refused.append(("beyond the tiled backward", _problem(H=512, HH=512)))
    for what, p in refused:
        assert lib.ncde_control_workspace_bytes(ctypes.byref(p)) == -2, what
        assert b"control-path gradients" in lib.ncde_last_error_string(), what
        assert lib.ncde_control_kernel_name(ctypes.byref(p)) is None, what
        assert lib.ncde_backward_control(ctypes.byref(p), 0x7000, 0x7100, ctypes.byref(_lib.NcdeGrads(grad_z0=0x7200)), 0x7300, 0x7400, 1 << 40, None) == -2, what
    p = _problem()
    assert lib.ncde_backward_control(ctypes.byref(p), 0x7000, 0x7100, ctypes.byref(_lib.NcdeGrads(grad_z0=0x7200)), None, 0x7400, 1 << 40, None) == -1
    assert lib.ncde_backward_control(ctypes.byref(p), 0x7000, 0x7100, ctypes.byref(_lib.NcdeGrads(grad_z0=0x7200)), 0x7300, 0x7400, 16, None) == -3
    p.n_knots = 1
    assert lib.ncde_control_workspace_bytes(ctypes.byref(p)) == -1


def test_route_decision_is_a_pure_predicate():
    """_unfused_reason keeps its pinned answers; _control_route_ok decides from the arguments alone and is false for CPU tensors
    (they keep the "no CPU fallback" refusal), for adjoint=True, dopri5, a smoothed path, another reason."""
    c = torch.zeros(2, 5, 3, requires_grad=True)
    X = ncde_amd.LinearInterpolation(c)
    f = ncde_amd.OriginalVectorField(3, 4, 8, 2)
    z0 = torch.zeros(2, 4)
    reason = solver._unfused_reason(X, f, z0, X.interval, False, None)
    assert reason == "the control path requires gradients" == solver._CONTROL_REASON
    assert solver._unfused_reason(X, f, z0, X.interval, True, tuple(f.parameters()) + (c,)) == reason
    assert solver._unfused_reason(X, f, z0, X.interval, True, None) is None
    assert not solver._control_route_ok(reason, X, z0, X.interval, False, "rk4")            # CPU tensors
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        ncde_amd.cdeint(X, f, z0, X.interval, adjoint=False, method="rk4", options={"step_size": 1})

    # the decision itself, on plain values: (reason, adjoint, method, plain_control, cuda_fp32, coeffs_grad, other_grad, t_grad)
    ok = (reason, False, "rk4", True, True, True, False, False)
    assert solver._control_route(*ok) and solver._control_route(reason, False, "euler", True, True, True, False, False)
    flips = {1: True, 2: "dopri5", 3: False, 4: False, 5: False, 6: True, 7: True}      # adjoint=True, dopri5, a smoothed path, CPU / fp64
    flips[0] = "decreasing output times"                                              # tensors, no grad, knots with grad, t with grad
    for k, v in flips.items():
        args = list(ok)
        args[k] = v
        assert not solver._control_route(*args), k
    # and how the arguments are read: a smoothed path, fp64 coefficients, knots that require grad (all on the CPU: false anyway,
    # so each is paired with the value the reader hands to the decision)
    assert not solver._control_route_ok(reason, ncde_amd.SmoothLinearInterpolation(c), z0, X.interval, False, "rk4")
    Xk = ncde_amd.LinearInterpolation(c, torch.arange(5.0, requires_grad=True))
    assert any(b.requires_grad for b in Xk.buffers() if b is not Xk._coeffs) and not solver._control_route_ok(reason, Xk, z0, torch.tensor([0.0, 4.0]), False, "rk4")


def test_stacked_module_surface_equals_the_reference():
    """Constructor attributes and state_dict keys of StackedNeuralCDE against the lists the generator took from the reference module."""
    m = _manifest()["g16_f_stacked"]
    model = ncde_amd.StackedNeuralCDE(adjoint=False, return_sequences=True, **m["ctor"])
    assert list(model.state_dict().keys()) == m["state_dict_keys"]
    assert [k for k, _ in model.named_parameters()] == m["param_names"]
    for k, v in m["attributes"].items():
        assert getattr(model, k) == v, k
    assert model.return_sequences is True and len(model.ncdes) == 2
    assert [n.apply_final_linear for n in model.ncdes] == [False, True] and [n.return_sequences for n in model.ncdes] == [True, True]
    last = ncde_amd.StackedNeuralCDE(3, [8, 6], 2).ncdes
    assert last[0].return_sequences and not last[1].return_sequences and last[0].adjoint
    with pytest.raises(AssertionError, match="hidden_dims must be a list"):
        ncde_amd.StackedNeuralCDE(3, (8, 6), 2)
    static = ncde_amd.StackedNeuralCDE(3, [8, 6], 2, static_dim=4, static_in_all_layers=True)
    assert static.ncdes[1].initial_linear.in_features == 8 + 4 and static._handle_hidden_static_features(["s", "x"], "h") == ["s", "h"]
