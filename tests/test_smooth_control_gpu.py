"""Fused dL/dcoeffs of cubic-smoothed control paths (adjoint=False): the transpose kernel ncde_prepare_smooth_backward against its fp64
definition, and the route through cdeint / NeuralCDE against golden vectors of the imported reference
(tools/gen_golden_smooth_control.py -> tests/golden/g17_*.npz, MANIFEST_smooth_control.json).

Tolerances of the golden cases: the project's own for reference goldens (tests/test_smooth_gpu.py:23):
forward <= 2e-5, dL/dcoeffs, dL/dz0 and every parameter gradient <= 2e-4, as |delta| relative to max |ref|."""
import ctypes
import json
import os
import warnings

import numpy as np
import pytest
import torch

import coeff_ref64
import golden_util as gu
from test_smooth_control_cpu import CASES, SHAPES, smooth_transpose

pytestmark = pytest.mark.gpu

TIGHT_Z, E2E_G = 2e-5, 2e-4
_CACHE = {}


def _load(name):
    if name not in _CACHE:      # read once, shared by the tests below, never modified
        f = dict(np.load(os.path.join(gu.GOLD, name + ".npz")))
        _CACHE[name] = (f, json.loads(str(f["meta"])))
    return _CACHE[name]


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _kernel_backward(lib, g, T, eps):
    """ncde_prepare_smooth_backward of g [B, P, 4C] (device) into a NaN-filled buffer -> numpy [B, T, C]."""
    B, C = g.shape[0], g.shape[2] // 4
    gx = torch.full((B, T, C), float("nan"), dtype=torch.float32, device="cuda")
    assert lib.ncde_prepare_smooth_backward(g.data_ptr(), B, T, C, float(eps), 3, gx.data_ptr(), _stream()) == 0, lib.ncde_last_error_string()
    torch.cuda.synchronize()
    return gx.cpu().numpy()


def _forward_error_tree(x, eps):
    """The builder's formulas (ncde_smooth_coeffs_kernel, order 3) with every operand replaced by its magnitude and every
    subtraction by an addition, in fp64, laid out like coeff_ref64.smooth: the quantity a running error analysis multiplies by
    (number of roundings on the longest path) x 2^-24."""
    a = np.abs(np.asarray(x, dtype=np.float64))
    B, T, C = a.shape
    P = coeff_ref64.smooth_pieces(T, eps)
    out = np.zeros((B, P, 4, C))
    out[:, 0, 0], out[:, 0, 1] = a[:, 0], a[:, 1] + a[:, 0]
    if T > 2:
        xp, xk, xn = a[:, :-2], a[:, 1:-1], a[:, 2:]
        d_prev, d_next = xk + xp, xn + xk
        x_eps = xk + eps * d_next
        Bq = (1 / eps ** 2) * (3 * (x_eps + d_prev * eps + xk) + eps * (d_next + d_prev))
        Aq = (1 / (3 * eps ** 2)) * (d_next + d_prev + 2 * Bq * eps)
        m = np.stack([xk, d_prev, 2 * Bq, 3 * Aq], axis=2)
        if eps < 1:
            out[:, 1::2] = m
            out[:, 2::2, 0], out[:, 2::2, 1] = x_eps, d_next
        else:
            out[:, 1:] = m
    return out.reshape(B, P, 4 * C)


@pytest.mark.parametrize("T,eps", SHAPES)
def test_transpose_kernel_against_its_fp64_definition(T, eps, gpu_lib):
    """ncde_prepare_smooth_backward for every (T, eps) of the CPU test, C in {1, 5}, B in {1, 18}.

    Bound, from the kernel (ncde_smooth_coeffs_bwd_kernel): an element of grad_x sums the contributions of the pieces that read that
    knot -- M(t-1), R(t-1), M(t), R(t), M(t+1) (piece 0 takes the place of the missing M(0) at t = 1): N = 5 pieces for eps < 1,
    N = 3 for eps == 1 (no rest pieces).  A term w g of a piece goes through at most: rounding of w to fp32 (1), the product (1), the
    sum inside the piece (2: s = w2 g2c + w3 g3d, then its combination with the a / b terms; the factor 2 is exact) and the N - 1
    additions of the running sum plus its own: <= 4 + N <= 2 N roundings for N = 5 (for eps == 1 the weights 4 and -3 are exact:
    <= 2 + N <= 2 N).  So |kernel - S^T g| <= 2 N 2^-24 sum |terms| = N 2^-23 sum |terms|, the sums over |w| |g| in fp64 by the same
    transpose.  Two runs are bit-identical (no atomics); every element is written (the buffer starts as NaN).
    Inner product against the FORWARD kernel: <ncde_prepare_smooth(x), g> and <x, backward(g)>, accumulated in fp64, differ by at
    most sum |g| E_fwd + sum |x| E_bwd: E_bwd the bound above, E_fwd = 16 x 2^-24 x (the builder's formulas over magnitudes) -- 16
    roundings on the longest path of the 3d row (x_eps 4, the bracket 4, the two scalings by rounded constants 2 + 2, the product
    with eps 2, the last difference and the factor 3: 2)."""
    N = 5 if eps < 1 else 3
    worst = 0.0
    for C in (1, 5):
        for B in (1, 18):
            rng = np.random.default_rng(1000 * T + 100 * C + B + int(10 * eps))
            P = coeff_ref64.smooth_pieces(T, eps)
            g = rng.standard_normal((B, P, 4 * C)).astype(np.float32)
            x = rng.standard_normal((B, T, C)).astype(np.float32)
            gd, xd = torch.from_numpy(g).cuda(), torch.from_numpy(x).cuda()
            one, two = _kernel_backward(gpu_lib, gd, T, eps), _kernel_backward(gpu_lib, gd, T, eps)
            assert np.isfinite(one).all() and np.array_equal(one.view(np.int32), two.view(np.int32)), (T, eps, C, B)
            ref, mag = smooth_transpose(g, T, eps), smooth_transpose(g, T, eps, absolute=True)
            bound = N * 2.0 ** -23 * mag
            err = np.abs(one.astype(np.float64) - ref)
            ratio = float((err / bound).max())
            worst = max(worst, ratio)
            print("T %d eps %s C %d B %d: max err %.3e, max err / bound %.3f" % (T, eps, C, B, err.max(), ratio))
            assert (err <= bound).all(), (T, eps, C, B, ratio)
            # inner-product identity against the forward kernel
            rows = torch.full((B, P, 4 * C), float("nan"), dtype=torch.float32, device="cuda")
            assert gpu_lib.ncde_prepare_smooth(xd.data_ptr(), B, T, C, float(eps), 3, rows.data_ptr(), _stream()) == 0
            torch.cuda.synchronize()
            lhs = float((rows.cpu().numpy().astype(np.float64) * g).sum())
            rhs = float((x.astype(np.float64) * one).sum())
            tol = float((np.abs(g) * 16 * 2.0 ** -24 * _forward_error_tree(x, eps)).sum() + (np.abs(x) * bound).sum())
            print("    <S x, g> %.9e  <x, S^T g> %.9e  |diff| %.3e  tol %.3e" % (lhs, rhs, abs(lhs - rhs), tol))
            assert abs(lhs - rhs) <= tol, (T, eps, C, B)
    print("T %d eps %s: worst err / bound %.3f" % (T, eps, worst))


def _field(f, m):
    import gpu_util
    return gpu_util.CaseField({k[2:]: f[k] for k in f if k.startswith("p_")}, [("W0", "b0")] + [("W1", "b1")] * (m["dims"]["nl"] - 1), "cuda")


def _times(f, m, X):
    return {"interval": lambda: X.interval, "knots": lambda: X.grid_points, "times": lambda: torch.from_numpy(f["t_out"]).cuda()}[m["outputs"]]()


class _Spy:
    """Counts the calls of some entry points of the loaded library for the duration of a `with` block."""

    def __init__(self, lib, *names):
        self.lib, self.names, self.calls = lib, names, {n: 0 for n in names}

    def __enter__(self):
        self.real = {n: getattr(self.lib, n) for n in self.names}
        for n in self.names:
            setattr(self.lib, n, self._counted(n))
        return self

    def _counted(self, n):
        def call(*a):
            self.calls[n] += 1
            return self.real[n](*a)
        return call

    def __exit__(self, *exc):
        for n in self.names:
            setattr(self.lib, n, self.real[n])


def _run(f, m, lib):
    """The case through cdeint(adjoint=False) on a SmoothLinearInterpolation whose coefficient leaf requires grad.  ANY warning is an
    error: the fused route emits none, and a call sent to the unfused solver warns."""
    import ncde_amd
    from ncde_amd import unfused
    unfused._WARNED.clear()
    x = torch.from_numpy(f["coeffs"]).cuda().requires_grad_(True)
    X = ncde_amd.SmoothLinearInterpolation(x, gradient_matching_eps=m["eps"])
    func = _field(f, m)
    z0 = torch.from_numpy(f["z0"]).cuda().requires_grad_(True)
    with _Spy(lib, "ncde_backward_control", "ncde_prepare_smooth_backward", "ncde_prepare_smooth") as spy:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            out = ncde_amd.cdeint(X, func, z0, _times(f, m, X), adjoint=False, method=m["method"], options={"step_size": m["step_size"]})
            (out * torch.from_numpy(f["grad_out"]).cuda()).sum().backward()
        torch.cuda.synchronize()
    assert not unfused._WARNED, unfused._WARNED
    return {"z_out": out.detach().cpu().numpy(), "dcoeffs": x.grad.cpu().numpy(), "dz0": z0.grad.cpu().numpy(),
            "grads": {k: v.grad.cpu().numpy() for k, v in func.p.items()}, "calls": spy.calls}


@pytest.mark.parametrize("name", CASES)
def test_smoothed_control_gradient_matches_reference_golden(name, gpu_lib):
    """Cases a - d through cdeint: solution, dL/dcoeffs (with respect to the LINEAR coefficients), dL/dz0 and every parameter gradient
    against the reference; no warning, nothing unfused, and ncde_backward_control and ncde_prepare_smooth_backward each ran once (the
    rows were built once by ncde_prepare_smooth).  On the parent commit the call warns and runs unfused.
    Measured (MI355X): see DESIGN.md section 5.11."""
    f, m = _load(name)
    res = _run(f, m, gpu_lib)
    assert res["calls"] == {"ncde_backward_control": 1, "ncde_prepare_smooth_backward": 1, "ncde_prepare_smooth": 1}, res["calls"]
    assert res["z_out"].shape == f["z_out"].shape and res["dcoeffs"].shape == f["dcoeffs"].shape == f["coeffs"].shape
    errs = {"z": gu.relerr(res["z_out"], f["z_out"]), "dcoeffs": gu.relerr(res["dcoeffs"], f["dcoeffs"]), "dz0": gu.relerr(res["dz0"], f["dz0"])}
    for n in m["param_names"]:
        errs["d" + n] = gu.relerr(res["grads"][n], f["d" + n])
    print(m["name"], " ".join("%s %.2e" % kv for kv in errs.items()))
    assert errs["z"] <= TIGHT_Z, errs
    assert all(v <= E2E_G for k, v in errs.items() if k != "z"), errs


def test_parameter_gradients_are_those_of_backward_control_on_the_built_rows(gpu_lib):
    """Case b: the new step only post-processes grad_coeffs.  forward_record + ncde_backward_control straight on the C-ABI, on the rows
    ncde_prepare_smooth builds and the time plan of the refined grid, give the bits cdeint's dL/dz0 and parameter gradients have; and
    ncde_prepare_smooth_backward of that call's grad_coeffs gives the bits of cdeint's dL/dcoeffs."""
    import ncde_amd
    from ncde_amd import _lib, solver
    lib = gpu_lib
    f, m = _load("g17_b_eps05_midpoint_half_interval")
    res = _run(f, m, lib)
    x = torch.from_numpy(f["coeffs"]).cuda()
    X = ncde_amd.SmoothLinearInterpolation(x, gradient_matching_eps=m["eps"])
    rows = X.fused_coeffs
    func = _field(f, m)
    spec = func.fused_spec()
    z0 = torch.from_numpy(f["z0"]).cuda()
    plan = solver._time_plan(X, X.interval, m["method"], m["step_size"], z0.device)
    p = solver.build_problem(rows, "cubic", z0, spec, m["method"], _lib.OUT_TIMES, 0, plan)
    out = torch.empty(f["z_out"].shape, dtype=torch.float32, device="cuda")
    stages = torch.empty(int(lib.ncde_stage_record_bytes(ctypes.byref(p))) // 4, dtype=torch.float32, device="cuda")

    def ws_for(n):
        assert n > 0, lib.ncde_last_error_string()
        return torch.empty(int(n), dtype=torch.uint8, device="cuda")
    ws = ws_for(lib.ncde_workspace_bytes(ctypes.byref(p), 0))
    assert lib.ncde_forward_record(ctypes.byref(p), out.data_ptr(), stages.data_ptr(), ws.data_ptr(), ws.numel(), _stream()) == 0
    bound = solver.bind_grads(spec, z0.shape, z0.device, fill=float("nan"))
    gout = torch.from_numpy(f["grad_out"]).cuda()
    gc = torch.full_like(rows, float("nan"))
    ws = ws_for(lib.ncde_control_workspace_bytes(ctypes.byref(p)))
    rc = lib.ncde_backward_control(ctypes.byref(p), stages.data_ptr(), gout.data_ptr(), ctypes.byref(bound.g), gc.data_ptr(), ws.data_ptr(),
                                   ws.numel(), _stream())
    assert rc == 0, lib.ncde_last_error_string()
    torch.cuda.synchronize()
    same = lambda a, b: a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))      # noqa: E731
    assert same(out.cpu().numpy(), res["z_out"]) and same(bound.grad_z0.cpu().numpy(), res["dz0"])
    for k, q in func.p.items():
        assert same(bound.of(q).cpu().numpy(), res["grads"][k]), k
    d = m["dims"]
    assert torch.isfinite(gc).all() and not gc[..., :d["C"]].any()      # (the a columns: written, zero)
    assert same(_kernel_backward(lib, gc, d["T"], m["eps"]), res["dcoeffs"])


def test_route_predicate_on_the_gpu(gpu_lib):
    """_control_route_ok on CUDA tensors: cubic smoothing accepted; quintic matching, no smoothing, a user `t`, knots that require
    grad, adjoint=True and dopri5 refused."""
    import ncde_amd
    from ncde_amd import solver
    c = torch.zeros(2, 5, 3, device="cuda", requires_grad=True)
    z0 = torch.zeros(2, 4, device="cuda")
    S, reason = ncde_amd.SmoothLinearInterpolation, solver._CONTROL_REASON
    ok = lambda X, adjoint=False, method="rk4": solver._control_route_ok(reason, X, z0, X.interval, adjoint, method)      # noqa: E731
    cubic = S(c, gradient_matching_eps=0.5)
    assert ok(cubic) and ok(S(c, gradient_matching_eps=1)) and ok(cubic, method="euler")
    assert not ok(cubic, adjoint=True) and not ok(cubic, method="dopri5")
    assert not ok(S(c, gradient_matching_eps=0.5, match_second_derivatives=True))
    assert not ok(S(c)) and not ok(S(c, t=torch.tensor([0.0, 0.5, 1.5, 2.0, 4.0], device="cuda")))
    Xk = S(c, gradient_matching_eps=0.5)
    Xk._t = Xk._t.clone().requires_grad_(True)
    assert not ok(Xk)
    assert not ok(S(c.detach().double().requires_grad_(True), gradient_matching_eps=0.5))


def test_module_trains_fused_behind_a_learned_embedding(gpu_lib):
    """NeuralCDE(interpolation="linear_cubic_smoothing", interpolation_eps=0.5, adjoint=False) behind an nn.Linear on the raw series:
    no warning, and the Linear's weight gradient within 2e-4 (relative to its maximum) of the same model run in fp64 on the unfused
    solver -- which warns, as the fp32 model did before."""
    import ncde_amd
    from ncde_amd import unfused
    B, T, RAW, C, H, HH, nl = 18, 5, 3, 5, 12, 10, 2
    torch.manual_seed(7)
    embed = torch.nn.Linear(RAW, C).cuda()
    model = ncde_amd.NeuralCDE(C, H, 2, hidden_hidden_dim=HH, num_layers=nl, interpolation="linear_cubic_smoothing", interpolation_eps=0.5,
                               adjoint=False).cuda()
    raw = torch.from_numpy((gu.data.normal(61, B * T * RAW, stream=3).reshape(B, T, RAW) * 1.5).astype(np.float32)).cuda()
    gout = torch.from_numpy(gu.data.normal(62, B * 2, stream=1).reshape(B, 2).astype(np.float32)).cuda()
    unfused._WARNED.clear()
    with _Spy(gpu_lib, "ncde_backward_control", "ncde_prepare_smooth_backward") as spy:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            out = model(embed(raw))
            (out * gout).sum().backward()
        torch.cuda.synchronize()
    assert not unfused._WARNED and spy.calls == {"ncde_backward_control": 1, "ncde_prepare_smooth_backward": 1}
    got = {"out": out.detach().cpu().numpy(), "embed.weight": embed.weight.grad.cpu().numpy(), "embed.bias": embed.bias.grad.cpu().numpy()}
    got.update({k: q.grad.cpu().numpy() for k, q in model.named_parameters()})
    embed64, model64 = embed.double(), model.double()
    for q in list(embed64.parameters()) + list(model64.parameters()):
        q.grad = None
    with pytest.warns(UserWarning, match="unfused torch-op solver .the control path requires gradients"):
        out64 = model64(embed64(raw.double()))
    (out64 * gout.double()).sum().backward()
    ref = {"out": out64.detach().cpu().numpy(), "embed.weight": embed64.weight.grad.cpu().numpy(), "embed.bias": embed64.bias.grad.cpu().numpy()}
    ref.update({k: q.grad.cpu().numpy() for k, q in model64.named_parameters()})
    errs = {k: gu.relerr(got[k], ref[k]) for k in ref}
    print("module behind an embedding", " ".join("%s %.2e" % kv for kv in errs.items()))
    assert float(np.abs(ref["embed.weight"]).max()) >= 1e3 * E2E_G
    assert errs["out"] <= TIGHT_Z, errs
    assert all(v <= E2E_G for k, v in errs.items() if k != "out"), errs


@pytest.mark.parametrize("what", ["quintic", "adjoint_params"])
def test_requests_outside_the_route_keep_their_warning(what, gpu_lib):
    """Quintic matching with coefficients that require grad, and adjoint=True with the coefficients in adjoint_params, still run on the
    unfused solver behind "the control path requires gradients"; the coefficients still receive a gradient."""
    import ncde_amd
    from ncde_amd import unfused
    f, m = _load("g17_b_eps05_midpoint_half_interval")
    d = m["dims"]
    torch.manual_seed(5)
    x = torch.from_numpy(f["coeffs"]).cuda().requires_grad_(True)
    func = ncde_amd.OriginalVectorField(d["C"], d["H"], d["HH"], d["nl"]).cuda()
    X = ncde_amd.SmoothLinearInterpolation(x, gradient_matching_eps=0.5, match_second_derivatives=what == "quintic")
    adjoint, extra = (False, {}) if what == "quintic" else (True, {"adjoint_params": tuple(func.parameters()) + (x,)})
    z0 = torch.from_numpy(f["z0"]).cuda()
    unfused._WARNED.clear()
    with _Spy(gpu_lib, "ncde_backward_control", "ncde_prepare_smooth_backward") as spy:
        with pytest.warns(UserWarning, match="unfused torch-op solver .the control path requires gradients"):
            out = ncde_amd.cdeint(X, func, z0, X.interval, adjoint=adjoint, method="rk4", options={"step_size": 0.5}, **extra)
        out.square().sum().backward()
    assert spy.calls == {"ncde_backward_control": 0, "ncde_prepare_smooth_backward": 0}
    assert x.grad is not None and torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0
