"""Every kernel family on un-shared, tied and uneven layer stacks (tests/layer_topologies.py; expectations pinned on the CPU by
tests/test_layer_topologies_cpu.py): forward, continuous adjoint and exact discrete backward against the oracle, at the constants of
tests/test_gpu_parity.py.  Shapes are the smallest that still pick each family: B = 21 (two sample tiles, one ragged), L = 7.

Which kernel served which stack is collected in DISPATCH and printed by the last test ("Layer topologies", holds the
table as measured); a family name is asserted only where a guard in the C code states it."""
import ctypes

import numpy as np
import pytest
import torch

import golden_util as gu
import layer_topologies as lt
from test_gpu_parity import E2E_G, TIGHT_G, TIGHT_Z, TOL_DTHETA, TOL_DZ0, _grad_errors

pytestmark = pytest.mark.gpu

B, L = 21, 7
SETTINGS = [("linear", "rk4", True), ("cubic", "midpoint", False)]
_SID = lambda s: "%s_%s_%s" % (s[0], s[1], "seq" if s[2] else "final")      # noqa: E731
SQUARE_SHAPES = [(20, 32, 32),      # register-resident cfg2 set
                 (8, 32, 32),       # ncde_fast_c set
                 (4, 64, 64),       # ncde_adj_h64
                 (5, 16, 16),       # pads onto a register-resident set
                 (8, 48, 48)]       # batch-tiled for stacks not tied to layer 0 (a tied 48 x 48 matrix cannot be zero-padded as both
#                                     the H -> HH and an HH -> HH layer, so tied stacks train on the generic adjoint here; they reach the
#                                     batch-tiled backward at the (20, 32, 32), (8, 32, 32), (4, 64, 64) and (5, 16, 16) anchors)
ODD_SHAPE = (6, 10, 15)             # zero-padded into the batch-tiled family; no square layer
MAIN = [t for t in lt.TOPOLOGIES if t not in lt.DEEP]
GRID = [(t, s) for t in MAIN for s in SQUARE_SHAPES] + [(t, ODD_SHAPE) for t in MAIN if t not in lt.NEEDS_SQUARE] + \
    [(tuple(w[1]), (5 if w[0] % 2 else 8, w[0], None)) for w in lt.WIDTHS]


def _gid(g):
    spec, (C, H, HH) = g
    return "%s-C%d_H%d%s" % (spec if isinstance(spec, str) else "x".join(map(str, spec)), C, H, "" if HH is None else "_HH%d" % HH)


# a stack that is NOT "layer 0, then one other shared layer, nothing aliased between them" (csrc/ncde_host.h:
# ncde_one_shared_inner_layer) must not be served by the shape-specialised sets whose adjoints keep two accumulators
_SPECIALISED = ("ncde_fwd_fast", "ncde_adj_fast", "ncde_adj_h64", "ncde_dpf_")
DISPATCH = {}


def _reference_shaped(case):
    ly = case["layers"]
    if len(ly) < 2:
        return True
    shared = all(wb == ly[1] for wb in ly[2:])
    return shared and ly[1][0] != ly[0][0] and ly[1][1] != ly[0][1]


def _note(case, shape, kernels, tag=""):
    for pass_, k in zip(("forward", "adjoint", "backward"), kernels):
        assert k != "?", (pass_, "ncde_kernel_name is NULL")
        DISPATCH[(case["meta"]["topology"] + tag, "C%d H%d" % (shape[0], shape[1]), pass_)] = k
        if not _reference_shaped(case):
            assert not k.startswith(_SPECIALISED), (case["meta"]["topology"], pass_, k)


def _case(spec, shape, setting, kind="original"):
    C, H, HH = shape
    interp, method, seq = setting
    return lt.cached_case(spec, C, H, HH, interp, method, seq, B, L, 900 + 11 * SETTINGS.index(setting) + C, kind)


def _rows(got, want):
    """the three largest per-sample errors of dL/dz0 (relative to its max norm): one row apart = one sample's ReLU mask flipped"""
    per = np.abs(got - want).max(axis=1) / np.abs(want).max()
    return "worst dz0 rows " + " ".join("%.1e" % v for v in np.sort(per)[-3:])


def _check_all_passes(case, shape, tag=""):
    import gpu_util
    from ncde_amd import _lib
    ex = case["expect"]
    # each backward kernel in isolation, on the oracle's forward solution / stage record: tight, fully written, reproducible
    _note(case, shape, gpu_util.kernel_names(case), tag)
    for prefix, stages in (("", None), ("bp_", case["stage_record"])):
        iso = gpu_util.run_adjoint_direct(case, ex["z_out"], stages=stages)
        assert set(iso["grads"]) == set(case["meta"]["param_names"])
        bad = [k for k, v in iso["grads"].items() if not np.isfinite(v).all()] + ([] if np.isfinite(iso["dz0"]).all() else ["dz0"])
        assert not bad, ("gradient buffers left unwritten (NaN-filled before the call)", prefix, bad, iso["kernel"])
        for k, e in _grad_errors(case, iso, prefix).items():
            assert e <= TIGHT_G, ("isolated " + (prefix or "adjoint"), k, e, iso["kernel"])
        again = gpu_util.run_adjoint_direct(case, ex["z_out"], stages=stages)
        assert np.array_equal(again["dz0"], iso["dz0"]) and all(np.array_equal(again["grads"][k], iso["grads"][k]) for k in iso["grads"]), \
            ("not bit-reproducible", prefix, iso["kernel"])
    # forward (default arithmetic and split-bf16) + continuous adjoint, end to end
    res = gpu_util.run_case(case)
    ez = gu.relerr(res["z_out"], ex["z_out"])
    assert res["z_out"].shape == ex["z_out"].shape and ez <= TIGHT_Z, ("z", ez, res["kernels"])
    rb = gpu_util.run_case(case, flags=_lib.FLAG_SPLIT_BF16, need_grads=False)
    ez = gu.relerr(rb["z_out"], ex["z_out"])
    assert ez <= TIGHT_Z, ("z, split-bf16", ez, rb["kernels"])
    for k, e in _grad_errors(case, res).items():
        assert e <= (TOL_DZ0 if k == "dz0" else TOL_DTHETA), ("adjoint end to end", k, e, res["kernels"], _rows(res["dz0"], ex["dz0"]))
    # exact discrete backward, end to end: the recording forward returns the same bits
    resd = gpu_util.run_case(case, adjoint=False)
    assert np.array_equal(resd["z_out"], res["z_out"]), "recording forward differs from the plain forward"
    for k, e in _grad_errors(case, resd, "bp_").items():
        assert e <= (TOL_DZ0 if k == "dz0" else TOL_DTHETA), ("discrete backward end to end", k, e, resd["kernels"], _rows(resd["dz0"], ex["bp_dz0"]))


@pytest.mark.parametrize("setting", SETTINGS, ids=_SID)
@pytest.mark.parametrize("grid", GRID, ids=_gid)
def test_every_pass_on_every_stack(grid, setting, gpu_lib):
    """Forward (default and split-bf16) at TIGHT_Z; continuous adjoint and exact discrete backward end to end at TOL_DZ0 /
    TOL_DTHETA and in isolation at TIGHT_G; every gradient buffer of the isolated calls finite (they are NaN-filled before the
    call, so each parameter is written once and in full); a second isolated call bit-identical; a kernel name for every pass.

    The inputs are the first seed on which every ReLU mask of the oracle's own runs is decided in fp32 (lt.ReluMargin)."""
    spec, shape = grid
    _check_all_passes(_case(spec, shape, setting), shape)


DEEP_GRID = [(t, "original", sh, st) for t in lt.DEEP for sh in (ODD_SHAPE, (8, 48, 48)) for st in SETTINGS] + \
    [("deep8_distinct", "minimal", ODD_SHAPE, SETTINGS[0])]      # the gated eight-layer stack once


@pytest.mark.parametrize("spec,kind,shape,setting", DEEP_GRID, ids=lambda v: v if isinstance(v, str) else ("C%d_H%d_HH%d" % v if len(v) == 3 and isinstance(v[0], int) else _SID(v)))
def test_deep_stacks(spec, kind, shape, setting, gpu_lib):
    """Six layers (five shared) and the ABI maximum of eight distinct layers: 18 (gated: 20) distinct parameter tensors, more
    than the 12 segments of a zero-padding plan -- the odd shape cannot be padded and runs where its real widths are supported."""
    _check_all_passes(_case(spec, shape, setting, kind), shape, "" if kind == "original" else " (minimal-gated)")


@pytest.mark.parametrize("setting", SETTINGS, ids=_SID)
@pytest.mark.parametrize("shape", [(8, 32, 32), (3, 16, 16)], ids=lambda s: "C%d_H%d_HH%d" % s)
@pytest.mark.parametrize("kind", ["minimal", "gru"])
@pytest.mark.parametrize("spec", ["distinct3", "tied_first_last", "w_shared_b_own"])
def test_field_variants(spec, kind, shape, setting, gpu_lib):
    """The minimal-gated field (batch-tiled family) and the GRU field (variant kernels, LDS residency of shared matrices) on
    stacks with shared pointers."""
    _check_all_passes(_case(spec, shape, setting, kind), shape, " (%s)" % kind)


def _run_times(case, tout, step, adjoint, gout):
    import gpu_util
    import ncde_amd
    m = case["meta"]
    X = (ncde_amd.LinearInterpolation if m["kind"] == "linear" else ncde_amd.NaturalCubicSpline)(torch.from_numpy(case["coeffs"]).cuda())
    func = gpu_util.case_field(case, "cuda")
    z0 = torch.from_numpy(case["z0"]).cuda().requires_grad_(True)
    out = ncde_amd.cdeint(X, func, z0, torch.from_numpy(tout).cuda(), adjoint=adjoint, method=m["method"], options={"step_size": step})
    (out * torch.from_numpy(gout).cuda()).sum().backward()
    torch.cuda.synchronize()
    return {"z_out": out.detach().cpu().numpy(), "dz0": z0.grad.cpu().numpy(), "grads": {k: v.grad.cpu().numpy() for k, v in func.p.items()}}


@pytest.mark.parametrize("interp,method,step", [("linear", "rk4", 0.5), ("cubic", "midpoint", 0.4)])
@pytest.mark.parametrize("shape", [(20, 32, 32), (8, 48, 48)], ids=lambda s: "C%d_H%d_HH%d" % s)
@pytest.mark.parametrize("spec", ["tied_all3", "distinct3", "tied_first_last", (16, 32, 16)], ids=lambda s: s if isinstance(s, str) else "16x32x16")
def test_general_time_axis(spec, shape, interp, method, step, gpu_lib):
    """Output times between the knots and a step size that does not divide them (the plan-driven kernels), against the oracle's
    general-time functions: forward, continuous adjoint and exact discrete backward, end to end."""
    import ncde_oracle as orc
    C, H, HH = shape
    def build(seed):      # (inputs on which every ReLU mask of the oracle's runs is decided in fp32: lt.ReluMargin)
        case = lt.bare_case(spec if isinstance(spec, str) else list(spec), C, H, HH, interp, method, True, B, L, seed)
        field, ctl = gu.oracle_field(case), orc.Control(case["coeffs"], interp)
        tout = np.array([0.0, 1.5, 2.0, 3.25, ctl.n_knots - 1.125], np.float32)
        with lt.ReluMargin(field) as rm:
            z = orc.solve_forward_times(ctl, field, case["z0"], tout, method, step)
            gout = (gu.data.normal(23, z.numel(), stream=1).reshape(z.shape) / 2.0).astype(np.float32)
            dz0, gp = orc.solve_adjoint_times(ctl, field, tout, z, gout, method, step)
            bdz0, bgp = orc.solve_discrete_backward_times(ctl, field, case["z0"], tout, gout, method, step)
        return (case, tout, z, gout, dz0, gp, bdz0, bgp), rm.worst
    case, tout, z, gout, dz0, gp, bdz0, bgp = lt.well_posed(build, 950 + C)
    m, names = case["meta"], case["meta"]["param_names"]
    for adjoint, want_dz0, want_gp in ((True, dz0, gp), (False, bdz0, bgp)):
        res = _run_times(case, tout, step, adjoint, gout)
        assert gu.relerr(res["z_out"], z) <= TIGHT_Z, (adjoint, gu.relerr(res["z_out"], z))
        assert gu.relerr(res["dz0"], want_dz0) <= TOL_DZ0, (adjoint, gu.relerr(res["dz0"], want_dz0))
        for n_, g_ in zip(names, want_gp):
            assert gu.relerr(res["grads"][n_], g_) <= TOL_DTHETA, (adjoint, n_, gu.relerr(res["grads"][n_], g_))
    assert m["dims"]["nl"] == len(case["layers"])


@pytest.mark.parametrize("shape,interp", [((20, 32, 32), "linear"), ((4, 64, 64), "cubic")], ids=["C20_H32_linear", "C4_H64_cubic"])
@pytest.mark.parametrize("spec", ["tied_all3", "w_tied_b_own", "distinct3"])
def test_dopri5_forced_step_sequence(spec, shape, interp, gpu_lib):
    """first_step = min_step = max_step = 0.75 (GPU and oracle walk the same steps), as
    test_dopri5_every_kernel_set_forced_sequence_vs_oracle does for the reference's stack: forward at TIGHT_Z, adaptive adjoint and
    the taped `adjoint=False` backward at E2E_G.  None of these stacks may run on the fused attempt kernels (dpf_shape)."""
    import gpu_util
    import ncde_amd
    import ncde_oracle as orc
    from ncde_amd import _lib, solver
    C, H, HH = shape
    opts = {"first_step": 0.75, "min_step": 0.75, "max_step": 0.75}

    def build(seed):      # (inputs on which every ReLU mask of the oracle's runs is decided in fp32: lt.ReluMargin)
        case = lt.bare_case(spec, C, H, HH, interp, "rk4", True, B, 12 if interp == "cubic" else 6, seed)
        field, ctl = gu.oracle_field(case), orc.Control(case["coeffs"], interp)
        tt = torch.arange(ctl.n_knots, dtype=torch.float32)
        with lt.ReluMargin(field) as rm:
            z = orc.dopri5_forward(ctl, field, case["z0"], tt, 1e-3, 1e-5, opts)
            gout = (gu.data.normal(31, z.numel(), stream=1).reshape(z.shape) / np.sqrt(z.shape[1])).astype(np.float32)
            dz0, gp = orc.dopri5_adjoint(ctl, field, tt, z, gout, 1e-3, 1e-5, opts)
            _zb, bdz0, bgp = orc.dopri5_discrete_backward(ctl, field, case["z0"], tt, gout, 1e-3, 1e-5, opts)
        return (case, z, gout, dz0, gp, bdz0, bgp), rm.worst
    case, z, gout, dz0, gp, bdz0, bgp = lt.well_posed(build, 960 + C)
    names, p, z0n, coeffs = case["meta"]["param_names"], case["params"], case["z0"], case["coeffs"]
    X = (ncde_amd.LinearInterpolation if interp == "linear" else ncde_amd.NaturalCubicSpline)(torch.from_numpy(coeffs).cuda())
    func = gpu_util.case_field(case, "cuda")
    prob = solver.build_problem(torch.from_numpy(coeffs).cuda(), interp, torch.from_numpy(z0n).cuda(), func.fused_spec(), "rk4", _lib.OUT_INTERVAL, 0)
    kn = [(_lib.lib().ncde_dopri5_kernel_name(ctypes.byref(prob), k) or b"?").decode() for k in (0, 1, 2)]
    for pass_, k in zip(("dopri5 forward", "dopri5 adjoint", "dopri5 taped backward"), kn):
        DISPATCH[(spec, "C%d H%d" % (C, H), pass_)] = k
        assert k != "?" and not k.startswith("ncde_dpf_"), (pass_, k)
    for adjoint, want_dz0, want_gp in ((True, dz0, gp), (False, bdz0, bgp)):
        func = gpu_util.case_field(case, "cuda")
        z0 = torch.from_numpy(z0n).cuda().requires_grad_(True)
        out = ncde_amd.cdeint(X, func, z0, X.grid_points, adjoint=adjoint, method="dopri5", rtol=1e-3, atol=1e-5, options=dict(opts))
        assert gu.relerr(out.detach().cpu().numpy(), z) <= TIGHT_Z, (adjoint, gu.relerr(out.detach().cpu().numpy(), z))
        (out * torch.from_numpy(gout).cuda()).sum().backward()
        assert gu.relerr(z0.grad.cpu().numpy(), want_dz0) <= E2E_G, (adjoint, gu.relerr(z0.grad.cpu().numpy(), want_dz0), _rows(z0.grad.cpu().numpy(), want_dz0.numpy()), kn)
        for n_, g_ in zip(names, want_gp):
            assert gu.relerr(func.p[n_].grad.cpu().numpy(), g_) <= E2E_G, (adjoint, n_, gu.relerr(func.p[n_].grad.cpu().numpy(), g_))


@pytest.mark.parametrize("adjoint", [True, False])
@pytest.mark.parametrize("C,H,widths", [(8, 48, (64, 32)), (20, 32, (32, 32, 32))], ids=["C8_H48_64x32", "C20_H32_32x32x32"])
def test_mlpfield_trains_through_neuralcde(C, H, widths, adjoint, gpu_lib):
    """One training step of NeuralCDE with func = ncde_amd.MLPField (an un-shared stack): the output and every .grad -- the
    field's, the read-in's and the read-out's -- against the oracle on the module's own parameters; nfe as the reference counts it."""
    import ncde_amd
    import ncde_oracle as orc
    OUT, Lr = 2, 5
    coeffs = gu.data.make_rectilinear_coeffs(B, Lr, C - 1, missing=0.3, seed=970 + C)
    case = lt.bare_case(list(widths), C, H, None, "linear", "rk4", False, B, Lr, 970 + C)
    torch.manual_seed(7)
    model = ncde_amd.NeuralCDE(C, H, OUT, interpolation="rectilinear", adjoint=adjoint, solver="rk4").cuda()
    model.func = lt.mlp_field(case, "cuda")
    out = model(torch.from_numpy(coeffs).cuda())
    w = torch.from_numpy(gu.data.normal(5, out.numel(), stream=2).reshape(out.shape).astype(np.float32)).cuda()
    (out * w).sum().backward()
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    field, ctl = gu.oracle_field(case), orc.Control(coeffs, "linear")
    z0 = torch.from_numpy(coeffs[:, 0]) @ sd["initial_linear.weight"].t() + sd["initial_linear.bias"]
    z = orc.solve_forward(ctl, field, z0, "rk4", False)
    ref = z[:, -1] @ sd["final_linear.weight"].t() + sd["final_linear.bias"]
    assert out.shape == ref.shape and gu.relerr(out.detach().cpu(), ref) <= TIGHT_Z
    gz = torch.zeros_like(z)
    gz[:, -1] = w.cpu() @ sd["final_linear.weight"]
    dz0, gp = orc.solve_adjoint(ctl, field, z, gz, "rk4", False) if adjoint else orc.solve_discrete_backward(ctl, field, z0, gz, "rk4", False)
    got = lt.mlp_grads(model.func, case)
    for n_, g_ in zip(case["meta"]["param_names"], gp):
        assert gu.relerr(got[n_], g_) <= E2E_G, (n_, gu.relerr(got[n_], g_))
    assert gu.relerr(model.initial_linear.weight.grad.cpu(), dz0.t() @ torch.from_numpy(coeffs[:, 0])) <= E2E_G
    assert gu.relerr(model.final_linear.weight.grad.cpu(), w.cpu().t() @ z[:, -1]) <= E2E_G
    steps = 2 * Lr - 2        # rectilinear data of Lr observations: 2 Lr - 1 knots
    assert model.nfe == (2 if adjoint else 1) * 4 * steps


@pytest.mark.parametrize("setting", SETTINGS, ids=_SID)
@pytest.mark.parametrize("spec", ["distinct3", "tied_first_last", (64, 32)], ids=lambda s: s if isinstance(s, str) else "H48_64x32")
def test_control_path_gradient(spec, setting, gpu_lib):
    """`adjoint=False` with coefficients that require grad at (C, H, HH) = (8, 48, 48): dL/dcoeffs, dL/dz0 and every parameter
    gradient against the reference tests/test_control_grad_gpu.py uses where it has no golden -- the unfused solver in fp64 on the
    GPU -- at that file's bounds.  The fused control route (ncde_backward_control) runs on the batch-tiled backward alone: the
    uneven two-layer stack is served by it without a warning; `distinct3` (three matrices) and `tied_first_last` (a 48 x 48 matrix
    that would have to be zero-padded as layer 0 AND as an inner layer) are refused by tiled_adj_ok, and cdeint must then say so
    and run the unfused solver -- same reference, same bounds."""
    import warnings
    import ncde_amd
    from ncde_amd import unfused
    from test_control_grad_gpu import E2E_G as CTL_G, TIGHT_Z as CTL_Z
    interp, method, seq = setting
    case = _case(spec, (8, 48, None if not isinstance(spec, str) else 48), setting)
    m, ex = case["meta"], case["expect"]
    spline = ncde_amd.LinearInterpolation if interp == "linear" else ncde_amd.NaturalCubicSpline

    def solve(func, dtype, expect_unfused):
        coeffs = torch.from_numpy(case["coeffs"]).to(device="cuda", dtype=dtype).requires_grad_(True)
        X = spline(coeffs)
        z0 = torch.from_numpy(case["z0"]).to(device="cuda", dtype=dtype).requires_grad_(True)
        unfused._WARNED.clear()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore" if expect_unfused else "error")
            out = ncde_amd.cdeint(X, func, z0, X.grid_points if seq else X.interval, adjoint=False, method=method, options={"step_size": 1})
            (out * torch.from_numpy(ex["grad_out"]).to(device="cuda", dtype=dtype)).sum().backward()
        torch.cuda.synchronize()
        assert bool(unfused._WARNED) == expect_unfused, unfused._WARNED
        if expect_unfused and dtype == torch.float32:
            assert any("the control path requires gradients" in r for r in unfused._WARNED), unfused._WARNED
        return out.detach().cpu().numpy(), coeffs.grad.cpu().numpy(), z0.grad.cpu().numpy()
    f64, p64 = lt.torch_field(case, "cuda", torch.float64)
    z64, dc64, dz64 = solve(f64, torch.float64, True)
    fused = not isinstance(spec, str)
    func, p32 = lt.torch_field(case, "cuda", torch.float32)
    z, dc, dz0 = solve(func, torch.float32, not fused)
    errs = {"z": gu.relerr(z, z64), "dcoeffs": gu.relerr(dc, dc64), "dz0": gu.relerr(dz0, dz64)}
    errs.update({"d" + n: gu.relerr(p32[n].grad.cpu().numpy(), p64[n].grad.cpu().numpy()) for n in m["param_names"]})
    DISPATCH[(m["topology"], "C8 H48", "control gradient")] = "ncde_backward_control" if fused else "unfused solver (warned)"
    print("control gradient", m["topology"], setting, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert float(np.abs(dc64).max()) >= 1e3 * CTL_G and np.isfinite(dc).all()
    assert gu.relerr(ex["z_out"], z64) <= CTL_Z       # (the fp32 oracle of the case agrees with this reference)
    assert errs["z"] <= CTL_Z, errs
    assert all(v <= CTL_G for k, v in errs.items() if k != "z"), errs


def test_print_dispatch_table(gpu_lib):
    """Not a check of its own: prints which kernel served each (stack, shape, pass) of the tests above (run the whole file)."""
    rows = sorted(DISPATCH.items())
    print("\n(stack | shape | pass | kernel)")
    for (topo, shape, pass_), k in rows:
        print("| %s | %s | %s | `%s` |" % (topo, shape, pass_, k))
    assert all(k and k != "?" for _, k in rows)
