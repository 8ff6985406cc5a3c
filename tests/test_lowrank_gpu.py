"""The low-rank vector field on its fused kernels (ncde_fwd_lowrank / ncde_adj_lowrank) against golden vectors produced by the imported
reference solver (tools/gen_golden_lowrank.py -> tests/golden/g17_*.npz, MANIFEST_lowrank.json) and, where no golden exists, against
the package's unfused torch-op solver in fp64 on the GPU.

Tolerances: the project's own for reference goldens (tests/test_smooth_gpu.py:23): forward <= 2e-5, dL/dz0 and every parameter gradient
<= 2e-4, as |delta| relative to max |ref|.  The manifest records per case that the fp32 reference sits within a quarter of each of its
fp64 self and that every gradient of M_h / M_o has a maximum >= 1e3 x the tolerance."""
import ctypes
import json
import os
import warnings

import numpy as np
import pytest
import torch

import golden_util as gu
import lowrank_util as lu
import strided_views as sv

pytestmark = pytest.mark.gpu

TIGHT_Z, E2E_G = 2e-5, 2e-4
CASES = ["g17_a_rect_rk4_interval", "g17_b_linear_midpoint_knots", "g17_c_cubic_rk4_knots", "g17_d_linear_userknots_euler_half",
         "g17_e_linear_rk4_interval_c24"]
_CACHE = {}


def _load(name):
    if name not in _CACHE:      # read once, shared by the tests below, never modified
        f = dict(np.load(os.path.join(gu.GOLD, name + ".npz")))
        _CACHE[name] = (f, json.loads(str(f["meta"])))
    return _CACHE[name]


def _params(f):
    return {k[2:]: f[k] for k in f if k.startswith("p_")}


def _control(f, m, coeffs, smooth=None):
    import ncde_amd
    if smooth is not None:
        return ncde_amd.SmoothLinearInterpolation(coeffs, gradient_matching_eps=smooth, match_second_derivatives=True)
    kn = torch.from_numpy(f["knots"]).to(coeffs) if "knots" in f else None
    return (ncde_amd.NaturalCubicSpline if m["interp"] == "cubic" else ncde_amd.LinearInterpolation)(coeffs, kn)


def _times(f, m, X):
    return {"interval": lambda: X.interval, "knots": lambda: X.grid_points, "times": lambda: torch.from_numpy(f["t_out"]).to(X.interval)}[m["outputs"]]()


def _solve(f, m, adjoint, dtype=torch.float32, coeffs=None, smooth=None, capture=None, method=None, options=None, **kw):
    """The case through ncde_amd.cdeint -> {z_out, dz0, grads}.  fp32: ANY warning is an error (the fused route emits none, a call sent
    to the unfused solver warns) and `capture` collects the problems handed to the library; fp64: the unfused solver, which must warn."""
    import ncde_amd
    from ncde_amd import solver, unfused
    d = m["dims"]
    unfused._WARNED.clear()
    if coeffs is None:
        coeffs = torch.from_numpy(f["coeffs"]).cuda()
    coeffs = coeffs.to(dtype)
    X = _control(f, m, coeffs, smooth)
    func, named = lu.make_field(ncde_amd, _params(f), d["C"], d["H"], d["HH"], d["nl"], m["sparsity"], "cuda", dtype)
    z0 = torch.from_numpy(f["z0"]).cuda().to(dtype).requires_grad_(True)
    gout = torch.from_numpy(f["grad_out"]).cuda().to(dtype)
    real = solver.build_problem

    def spy(*a, **k):
        p = real(*a, **k)
        if capture is not None:
            capture.append(p)
        return p
    solver.build_problem = spy
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("error" if dtype == torch.float32 and method is None else "always")
            out = ncde_amd.cdeint(X, func, z0, _times(f, m, X), adjoint=adjoint, method=method or m["method"],
                                  options=options or {"step_size": m["step_size"]}, **kw)
            (out * gout).sum().backward()
        torch.cuda.synchronize()
    finally:
        solver.build_problem = real
    if dtype == torch.float32 and method is None:
        assert not unfused._WARNED, unfused._WARNED
    else:
        assert sum("unfused" in str(w.message) for w in rec) == 1, [str(w.message) for w in rec]
    return {"z_out": out.detach().cpu().numpy(), "dz0": z0.grad.cpu().numpy(), "grads": {k: v.grad.cpu().numpy() for k, v in named.items()}}


def _errors(res, ref, names):
    errs = {"z": gu.relerr(res["z_out"], ref["z_out"]), "dz0": gu.relerr(res["dz0"], ref["dz0"])}
    for n in names:
        errs["d" + n] = gu.relerr(res["grads"][n], ref["grads"][n])
    return errs


def _check(label, res, ref, names):
    errs = _errors(res, ref, names)
    print(label, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert res["z_out"].shape == ref["z_out"].shape
    assert errs["z"] <= TIGHT_Z, (label, errs)
    assert all(v <= E2E_G for k, v in errs.items() if k != "z"), (label, errs)
    for n in ("Wh", "bh", "Wq", "bq"):      # the head gradients are far above the tolerance: a wrong kernel cannot hide in them
        assert float(np.abs(ref["grads"][n]).max()) >= 1e3 * E2E_G, (label, n)
    return errs


def _golden(f, m, adjoint):
    tag = "adj" if adjoint else "disc"
    return {"z_out": f["z_out"], "dz0": f["dz0_" + tag], "grads": {k: f["d%s_%s" % (k, tag)] for k in m["param_names"]}}


def _kernel_names(lib, p):
    return [(lib.ncde_kernel_name(ctypes.byref(p), ps) or b"?").decode() for ps in (0, 1, 2)]


@pytest.mark.parametrize("adjoint", [True, False], ids=["adjoint", "discrete"])
@pytest.mark.parametrize("name", CASES)
def test_lowrank_matches_reference_golden(name, adjoint, gpu_lib):
    """Cases a - e through cdeint: the solution, dL/dz0 and every parameter gradient, continuous adjoint and exact discrete backward;
    no warning, nothing unfused, and the library names the low-rank kernels for the problem it was handed."""
    f, m = _load(name)
    probs = []
    res = _solve(f, m, adjoint, capture=probs)
    assert _kernel_names(gpu_lib, probs[-1]) == ["ncde_fwd_lowrank", "ncde_adj_lowrank", "ncde_adj_lowrank<discrete>"]
    assert probs[-1].flags >> 24 == m["dims"]["R"] and probs[-1].field_kind == 3
    _check(name + (" adjoint" if adjoint else " discrete"), res, _golden(f, m, adjoint), m["param_names"])


@pytest.mark.parametrize("adjoint", [True, False], ids=["adjoint", "discrete"])
def test_lowrank_on_strided_coefficients(adjoint, gpu_lib):
    """Case a with the coefficients as strided views carved out of NaN-filled buffers: rows C + 3 floats apart (against the golden, and
    the same bits as the contiguous run), and ONE path shared by the batch with batch stride 0 and that row stride (the same bits as a
    contiguous copy of those values, and within the tolerances of the unfused solver in fp64)."""
    f, m = _load(CASES[0])
    C = m["dims"]["C"]
    base = _solve(f, m, adjoint)
    probs = []
    view = sv.make_view(f["coeffs"], "row_padded", "cuda")
    assert view.stride(1) == C + 3
    res = _solve(f, m, adjoint, coeffs=view, capture=probs)
    assert probs[-1].coeffs_stride_t == C + 3 and probs[-1].coeffs == view.data_ptr()
    _check("row stride C + 3", res, _golden(f, m, adjoint), m["param_names"])
    B, T, _ = f["coeffs"].shape
    buf = torch.full((sv.PAD + T * (C + 3) + sv.PAD,), float("nan"), device="cuda")
    shared = buf.as_strided((B, T, C), (0, C + 3, 1), sv.PAD)
    shared[0] = torch.from_numpy(f["coeffs"][0]).cuda()
    probs = []
    res0 = _solve(f, m, adjoint, coeffs=shared, capture=probs)
    assert probs[-1].coeffs_stride_b == 0 and probs[-1].coeffs_stride_t == C + 3
    logical = sv.logical(f["coeffs"], "broadcast")
    same = _solve(f, m, adjoint, coeffs=torch.from_numpy(logical).cuda())
    ref = _solve(f, m, adjoint, torch.float64, coeffs=torch.from_numpy(logical).cuda())
    _check("shared path, stride 0", res0, ref, m["param_names"])
    for a, b in ((res, base), (res0, same)):
        assert np.array_equal(a["z_out"], b["z_out"]) and np.array_equal(a["dz0"], b["dz0"])
        assert all(np.array_equal(a["grads"][k], b["grads"][k]) for k in m["param_names"])


@pytest.mark.parametrize("adjoint", [True, False], ids=["adjoint", "discrete"])
def test_lowrank_on_a_quintic_smoothed_path(adjoint, gpu_lib):
    """Case a's coefficients as a quintic-smoothed path (eps 0.5: piecewise-quintic pieces on the refined knot grid, a time plan),
    against the unfused solver in fp64."""
    f, m = _load(CASES[0])
    probs = []
    res = _solve(f, m, adjoint, smooth=0.5, capture=probs)
    assert probs[-1].interp == 2 and _kernel_names(gpu_lib, probs[-1])[0] == "ncde_fwd_lowrank"
    _check("quintic", res, _solve(f, m, adjoint, torch.float64, smooth=0.5), m["param_names"])


def test_lowrank_discrete_backward_is_autograd_through_the_solve(gpu_lib):
    """adjoint=False on case e's shape (C 24, R 3, H 32, three layers, a partial third tile) against torch autograd through the
    unfused solver in fp64."""
    f, m = _load(CASES[4])
    _check("case e vs autograd", _solve(f, m, False), _solve(f, m, False, torch.float64), m["param_names"])


@pytest.mark.parametrize("adjoint", [True, False], ids=["adjoint", "discrete"])
def test_lowrank_several_tiles_and_a_one_sample_tail(adjoint, gpu_lib):
    """Case e's field with B = 16 * 5 + 1: six workgroups, the last with one live sample; against the unfused solver in fp64."""
    f0, m = _load(CASES[4])
    d = m["dims"]
    B, T, C, H = 16 * 5 + 1, d["T"], d["C"], d["H"]
    f = dict(f0)
    f["coeffs"] = np.ascontiguousarray(gu.data.make_linear_coeffs(B, T, C - 1, seed=61), dtype=np.float32)
    f["z0"] = (gu.data.normal(63, B * H, stream=2).reshape(B, H) * 0.5).astype(np.float32)
    f["grad_out"] = (gu.data.normal(67, B * 2 * H, stream=1).reshape(B, 2, H) / 2.0).astype(np.float32)
    res = _solve(f, m, adjoint)
    assert np.isfinite(res["z_out"]).all() and res["z_out"].shape == (B, 2, H)
    _check("B = 81", res, _solve(f, m, adjoint, torch.float64), m["param_names"])


@pytest.mark.parametrize("adjoint", [True, False], ids=["adjoint", "discrete"])
@pytest.mark.parametrize("C,sparsity,H,HH,B", [(6, 0.0, 10, 12, 5), (24, 0.67, 64, 64, 17)], ids=["rank6", "rank8_streamed"])
def test_lowrank_beyond_the_register_ranks_and_the_resident_heads(C, sparsity, H, HH, B, adjoint, gpu_lib):
    """The paths the goldens (R <= 4, everything LDS-resident) do not take, against the unfused solver in fp64:
    rank6: R = 6 -- ranks 4 and 5 of the contraction and of gP / gQ go through LDS instead of registers; H = 10 is no multiple of 4.
    rank8_streamed: R = 8, (H + C) R = 704 stacked head rows of 64 columns: the resident copy (704 x 65 floats = 183 KB) does not fit
    the 160 KB of LDS, so the heads stream from L2, and the gradient partial (> 45,000 floats) lives in global memory."""
    R, nl, T = lu.rank_of(C, sparsity), 2, 6
    assert R == (6 if C == 6 else 8)
    f = {"coeffs": np.ascontiguousarray(gu.data.make_linear_coeffs(B, T, C - 1, seed=81), dtype=np.float32),
         "z0": (gu.data.normal(83, B * H, stream=2).reshape(B, H) * 0.5).astype(np.float32),
         "grad_out": (gu.data.normal(87, B * T * H, stream=1).reshape(B, T, H) / 2.0).astype(np.float32)}
    f.update({"p_" + k: v for k, v in lu.make_weights(gu.data, H, HH, C, R, nl, seed=19).items()})
    m = {"interp": "linear", "outputs": "knots", "method": "rk4", "step_size": 1, "sparsity": sparsity,
         "dims": {"C": C, "H": H, "HH": HH, "nl": nl, "R": R}, "param_names": lu.param_names(nl)}
    probs = []
    res = _solve(f, m, adjoint, capture=probs)
    assert probs[-1].flags >> 24 == R and _kernel_names(gpu_lib, probs[-1])[1] == "ncde_adj_lowrank"
    _check("R = %d" % R, res, _solve(f, m, adjoint, torch.float64), m["param_names"])


def test_lowrank_model_trains_on_the_fused_kernels_reproducibly(gpu_lib):
    """NeuralCDE(vector_field="low-rank", sparsity=0.9, return_sequences=True) on the reference's default widths: the training step
    runs ncde_fwd_lowrank / ncde_adj_lowrank (hidden_hidden_dim = 15: no multiple of anything), and two runs give the same bits."""
    import ncde_amd
    from ncde_amd import solver, unfused
    B, T, C, H = 20, 10, 4, 32
    torch.manual_seed(3)
    model = ncde_amd.NeuralCDE(C, H, 2, hidden_hidden_dim=15, num_layers=3, vector_field="low-rank", sparsity=0.9, return_sequences=True).cuda()
    assert model.func.rank == 1
    coeffs = torch.from_numpy(np.ascontiguousarray(gu.data.make_linear_coeffs(B, T, C - 1, seed=71), dtype=np.float32)).cuda()
    target = torch.from_numpy(gu.data.normal(73, B * T * 2, stream=1).reshape(B, T, 2).astype(np.float32)).cuda()
    probs, real = [], solver.build_problem

    def spy(*a, **k):
        probs.append(real(*a, **k))
        return probs[-1]
    runs = []
    solver.build_problem = spy
    unfused._WARNED.clear()
    try:
        for _ in range(2):
            model.zero_grad(set_to_none=True)
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                out = model(coeffs)
                (out - target).square().mean().backward()
            torch.cuda.synchronize()
            runs.append({k: q.grad.clone() for k, q in model.named_parameters()})
    finally:
        solver.build_problem = real
    assert not unfused._WARNED and out.shape == (B, T, 2)
    for p in probs:
        assert _kernel_names(gpu_lib, p)[:2] == ["ncde_fwd_lowrank", "ncde_adj_lowrank"]
    for k, g in runs[0].items():
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0, k
        assert torch.equal(g.view(torch.int32), runs[1][k].view(torch.int32)), k


def test_lowrank_with_dopri5_runs_unfused(gpu_lib):
    """solver='dopri5' has no fused low-rank kernel: one UserWarning, the unfused adaptive solver, and -- on a forced step sequence on
    case c's cubic control, so that fp32 and fp64 take the same steps -- the same numbers as in fp64."""
    f, m = _load(CASES[2])
    opts = {"first_step": 0.5, "min_step": 0.5, "max_step": 0.5}
    res = _solve(f, m, True, method="dopri5", options=opts, rtol=1e-3, atol=1e-5)
    ref = _solve(f, m, True, torch.float64, method="dopri5", options=opts, rtol=1e-3, atol=1e-5)
    _check("dopri5 unfused", res, ref, m["param_names"])
