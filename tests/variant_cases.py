"""Seeded cases for the variant kernels (ncde_fwd_variant / ncde_adj_variant): one per regime of their LDS plan (gradient partial in
LDS or in global memory, every weight matrix resident or streamed, per pass), of the register weight-gradient rule (in registers at
its 16-tile bound, refused by size, refused by topology), the VR_MAXJT bound, widths that are no multiple of 16, one- and 17-sample
tail tiles and general time axes.  Each case states the regime it is there for; tests/test_variant_plan_cpu.py asserts it through
variant_util.vr_plan and validates the case on the CPU (the unfused solver in fp32 against itself in fp64, the gradient-magnitude
condition, ReLU masks away from a knife edge), tests/test_variant_regimes_gpu.py runs the fused kernels against the unfused solver
in fp64.  Helper only: no test functions."""
import ctypes
import functools
import warnings

import numpy as np
import torch

import golden_util as gu
import layer_topologies as lt
import variant_util as vu

TIGHT_Z, E2E_G = 2e-5, 2e-4
MIN_GRAD = 1e3 * E2E_G      # every gradient tensor's maximum in the fp64 reference: a wrong gradient cannot hide in a near-zero tensor
OFF_GRID = (0.35, 1.6, 2.85, 4.0)      # output times between the knots 0 .. 4 (the solve starts at 0.35), the last on the last knot
VARIANT_NAMES = ["ncde_fwd_variant", "ncde_adj_variant", "ncde_adj_variant<discrete>"]

CASES = {}
N, Y = False, True


def _case(name, kind, mode, C, H, HH, nl, B, regime=None, widths=None, T=5, interp="linear", method="rk4", step=1.0, out="knots", seed=1,
          gain=1.0, scale=1.0, reset_scale=1.0, gout=1.0, backward=True):
    """C, H, HH, nl: the reference's stack (layer 0, then one shared layer) unless `widths` lists distinct layers.  out: "knots",
    "interval" or a tuple of output times.  regime: (gacc_in_lds, dw_why, backward residency {r, layers, o, g}) as vr_plan must
    give it; backward=False: a forward-only case, the backward's plan is refused.  gain multiplies the inner matrices, scale the heads,
    reset_scale the reset gate, gout the cotangent dL/dz."""
    assert name not in CASES
    CASES[name] = dict(name=name, kind=kind, mode=mode, C=C, H=H, HH=HH, nl=nl, B=B, regime=regime, widths=widths, T=T, interp=interp,
                       method=method, step=step, out=out, seed=seed, gain=gain, scale=scale, reset_scale=reset_scale, gout=gout,
                       modes=("adjoint", "discrete") if backward else ())


def _res(r, layers, o, g):
    return {"r": r, "layers": list(layers), "o": o, "g": g}


# ---- cases with a backward: (partial in LDS, register weight gradients, backward residency) --------------------------------------------
# A: nothing resident in the backward, partial in global memory, dw_reg refused by size (reset gate 5 x 5 tiles, layer 0 4 x 5);
#    forward: both heads streamed.  B = 17: a one-sample tail tile.
_case("A_gru_matmul_H80", "gru", "matmul", 4, 80, 64, 2, 17, (N, "size", _res(N, (N, N), N, N)), seed=11, gout=5.0)
# B: d0 = 72: the reset gate (5 x 5 tiles) streamed with layer 0 resident behind it, the shared layer streamed; dw_reg refused by the
#    reset gate ALONE (layer 0 has 3 x 5 = 15 tiles, the shared layer 9).  HH = 48, not 64: at 64 layer 0 has 20 tiles of its own.
_case("B_gru_evaluate_d72", "gru", "evaluate", 8, 64, 48, 2, 33, (N, "size", _res(N, (Y, N), N, N)), interp="cubic", method="midpoint", seed=112)
# C: exactly 16 tiles per matrix (64 x 64): dw_reg true at its bound, partial in global memory, the shared layer streamed
_case("C_gru_matmul_16tiles", "gru", "matmul", 4, 64, 64, 2, 17, (N, "registers", _res(Y, (Y, N), N, N)), out="interval", seed=13, gout=6.0)
# D: dlast = 128, eight column tiles (VR_MAXJT); register gradients; the backward's plan at 38,272 of 40,960 floats
_case("D_gru_matmul_dlast128", "gru", "matmul", 2, 16, 128, 1, 17, (N, "registers", _res(Y, (Y,), N, N)), method="euler", seed=14, gout=5.0)
# E: odd everything; the partial in LDS with only layer 0 resident
_case("E_minimal_evaluate_odd", "minimal", "evaluate", 7, 33, 50, 2, 19, (Y, "registers", _res(None, (Y, N), N, N)), method="midpoint", seed=15)
# F: forward all resident, backward nothing resident (40,384 floats); the cubic path
_case("F_original_derivative_odd", "original", "derivative", 5, 47, 93, 3, 21, (N, "size", _res(None, (N, N, N), N, None)), interp="cubic",
      seed=16)
# G: d0 = 37; the backward at 39,872 floats, nothing resident
_case("G_gru_derivative_d37", "gru", "derivative", 7, 30, 100, 2, 17, (N, "size", _res(N, (N, N), N, N)), method="midpoint", out="interval",
      seed=17, gout=3.0)
# H: H < 16, one layer, one sample, one step with final-only output: everything resident, the partial in LDS
_case("H_gru_matmul_tiny", "gru", "matmul", 3, 7, 15, 1, 1, (Y, "registers", _res(Y, (Y,), Y, Y)), T=2, out="interval", seed=18, gout=20.0)
# I: dw_reg false (layer 0 is 6 x 3, the shared layer 6 x 6 tiles), only the reset gate resident in the backward
_case("I_gru_matmul_odd", "gru", "matmul", 5, 47, 93, 2, 33, (N, "size", _res(Y, (N, N), N, N)), interp="cubic", method="euler", seed=19, gout=2.5)
# J: three distinct 64-wide layers at H 48 (every matrix <= 16 tiles): dw_reg refused by topology WITH the partial in global memory
_case("J_gru_matmul_distinct3", "gru", "matmul", 4, 48, 64, 3, 17, (N, "topology", _res(Y, (Y, Y, N), N, N)), widths=(64, 64, 64), interp="cubic",
      seed=20, gout=8.0)
# K: A and E on a general time axis (off-grid outputs; the plan-walking paths of both kernels)
_case("K_A_times_rk4", "gru", "matmul", 4, 80, 64, 2, 17, (N, "size", _res(N, (N, N), N, N)), step=0.5, out=OFF_GRID, seed=21, gout=6.0)
_case("K_E_times_midpoint", "minimal", "evaluate", 7, 33, 50, 2, 19, (Y, "registers", _res(None, (Y, N), N, N)), method="midpoint", step=0.4,
      out=OFF_GRID, seed=22, gout=2.0)
# ---- forward-only cases: the backward's plan passes 160 KB -> cdeint takes the unfused route ------------------------------------------
# forward residency {r, layers, o, g}: the shared layer streamed; only the reset gate resident
FORWARD_ONLY = {"fwd_shared_streamed": _res(Y, (Y, N), N, N), "fwd_only_reset_resident": _res(Y, (N, N), N, N)}
_case("fwd_shared_streamed", "gru", "matmul", 6, 96, 96, 2, 17, T=4, seed=31, gout=5.0, backward=False)
_case("fwd_only_reset_resident", "gru", "matmul", 6, 112, 96, 2, 17, T=4, seed=32, gout=4.0, backward=False)
WITH_BACKWARD = sorted(n for n, c in CASES.items() if c["modes"])
ALL_MODES = ("adjoint", "discrete")


def stack_of(c):
    if c["widths"] is None:
        return vu.ref_stack(c["mode"], c["C"], c["H"], c["HH"], c["nl"])
    d0 = vu.field_dims(c["mode"], c["C"], c["H"])[0]
    w = [d0] + list(c["widths"])
    return [("W%d" % i, "b%d" % i) for i in range(len(c["widths"]))], [(w[i + 1], w[i]) for i in range(len(c["widths"]))]


@functools.lru_cache(maxsize=None)
def arrays(name):
    """The case's inputs as fp32 arrays (built once; callers do not modify them)."""
    c = CASES[name]
    H, C, B, T = c["H"], c["C"], c["B"], c["T"]
    layers, dims = stack_of(c)
    p = vu.make_weights(layers, dims, c["kind"], c["mode"], C, H, c["seed"], c["gain"], c["scale"], c["reset_scale"])
    make = gu.data.make_cubic_coeffs if c["interp"] == "cubic" else gu.data.make_linear_coeffs
    n_out = {"knots": T, "interval": 2}.get(c["out"], len(c["out"]))
    return {"layers": layers, "dims": dims, "params": p, "names": vu.param_names(layers, c["kind"]),
            "coeffs": np.ascontiguousarray(make(B, T, C - 1, seed=c["seed"] + 1), dtype=np.float32),
            "z0": (gu.data.normal(c["seed"] + 2, B * H, stream=2).reshape(B, H) * 0.5).astype(np.float32),
            "grad_out": (gu.data.normal(c["seed"] + 3, B * n_out * H, stream=1).reshape(B, n_out, H) * (c["gout"] / 2.0)).astype(np.float32)}


def plan_of(name):
    c, a = CASES[name], arrays(name)
    return vu.vr_plan(c["kind"], c["mode"], c["C"], c["H"], a["dims"], a["layers"])


def regime_of(name):
    p = plan_of(name)
    return (p.gacc_in_lds, p.dw_why, p.res_adj)


def untied(a):
    """Every layer with its OWN equal-valued tensors -> (params, layers, {copy name: original name}): dL/d(tied tensor) is the sum of
    dL/d(its copies), so the reference of a tied stack never shares a tensor."""
    p = {k: v for k, v in a["params"].items() if k in ("Wo", "bo", "Wg", "bg", "Wr", "br")}
    layers, origin = [], {}
    for l, (w, b) in enumerate(a["layers"]):
        wn, bn = "W%d_%d" % (l, l), "b%d_%d" % (l, l)
        p[wn], p[bn] = a["params"][w].copy(), a["params"][b].copy()
        origin[wn], origin[bn] = w, b
        layers.append((wn, bn))
    return p, layers, origin


def setup(name, dtype, device, untie=False, samples=None):
    """-> dict(X, func, z0, t, gout, origin): the case's control, field, start state (requires grad), output times and cotangent on
    `device` in `dtype`.  samples: the first so many samples of the batch only."""
    import ncde_amd
    c, a = CASES[name], arrays(name)
    params, layers, origin = untied(a) if untie else (a["params"], a["layers"], None)
    func = vu.StackField(params, layers, c["H"], c["C"], c["kind"], c["mode"], device, dtype)
    cut = slice(0, samples if samples is not None else c["B"])
    coeffs = torch.from_numpy(np.ascontiguousarray(a["coeffs"][cut])).to(device=device, dtype=dtype)
    X = (ncde_amd.NaturalCubicSpline if c["interp"] == "cubic" else ncde_amd.LinearInterpolation)(coeffs)
    t = X.grid_points if c["out"] == "knots" else (X.interval if c["out"] == "interval" else torch.tensor(c["out"], device=device, dtype=dtype))
    z0 = torch.from_numpy(np.ascontiguousarray(a["z0"][cut])).to(device=device, dtype=dtype).requires_grad_(True)
    gout = torch.from_numpy(np.ascontiguousarray(a["grad_out"][cut])).to(device=device, dtype=dtype)
    return {"X": X, "func": func, "z0": z0, "t": t, "gout": gout, "origin": origin}


def solve(name, mode, dtype, device, untie=False, capture=None, refused=False, flags=0, observe=False):
    """The case -> {z_out, dz0, grads{name: array}} for L = sum(z * grad_out); mode "adjoint" / "discrete".
    device "cuda": through ncde_amd.cdeint.  fp32: ANY warning is an error (the fused route emits none) and `capture` collects the
    problems handed to the library; fp64: the unfused solver, which must emit its one warning.
    device "cpu": the unfused solver called directly (cdeint has no CPU route).
    untie: the stack of untied(), gradients summed over the copies of each tensor.  refused: the fp32 call is expected on the unfused
    route behind exactly one warning.  observe: -> also "relu_margin", the worst layer_topologies.ReluMargin ratio over every
    evaluation of the inner net, forward and backward."""
    import ncde_amd
    from ncde_amd import solver, unfused
    c, a = CASES[name], arrays(name)
    adjoint = {"adjoint": True, "discrete": False}[mode]
    s = setup(name, dtype, device, untie)
    X, func, z0, t = s["X"], s["func"], s["z0"], s["t"]
    rm = lt.ReluMargin(func)
    if observe:
        rm.__enter__()
    if device == "cpu":
        out = unfused.cdeint_unfused(X, func, z0, t, adjoint, c["mode"], c["method"], c["step"])
    else:
        fused = dtype == torch.float32 and not refused
        unfused._WARNED.clear()
        real = solver.build_problem

        def spy(*args, **kw):
            p = real(*args, **kw)
            if capture is not None:
                capture.append(p)
            return p
        solver.build_problem = spy
        try:
            with warnings.catch_warnings(record=True) as rec:
                warnings.simplefilter("error" if fused else "always")
                out = ncde_amd.cdeint(X, func, z0, t, adjoint=adjoint, vector_field_type=c["mode"], method=c["method"],
                                      options={"step_size": c["step"]}, kernel_flags=flags)
        finally:
            solver.build_problem = real
        if fused:
            assert not unfused._WARNED, unfused._WARNED
        else:
            assert sum("unfused" in str(w.message) for w in rec) == 1, [str(w.message) for w in rec]
    (out * s["gout"]).sum().backward()
    if device != "cpu":
        torch.cuda.synchronize()
    if observe:
        rm.__exit__()
    grads = {k: v.grad.detach().cpu().numpy() for k, v in func.p.items()}
    if untie:
        grads = lt.sum_over_copies(grads, s["origin"], a["names"])
    res = {"z_out": out.detach().cpu().numpy(), "dz0": z0.grad.cpu().numpy(), "grads": grads}
    if observe:
        res["relu_margin"] = rm.worst
    return res


class Direct:
    """The case's problem handed to the C ABI directly, one call at a time (fp32, the GPU): forward() / forward(record=True), and
    backward() into NaN-filled gradient buffers -- so that a test can look at one launch in isolation, bit for bit."""

    def __init__(self, name, flags=0, samples=None):
        from ncde_amd import _lib, solver
        c = CASES[name]
        self.s = s = setup(name, torch.float32, "cuda", samples=samples)
        self.c, self.lib, self.dev = c, _lib.lib(), s["z0"].device
        self.spec = s["func"].fused_spec()
        self.coeffs = s["X"].fused_coeffs
        self.z0 = s["z0"].detach().contiguous()
        self.output, self.plan, _, _ = solver._fixed_axis(s["X"], s["t"], c["method"], c["step"], self.dev)
        self.p = solver.build_problem(self.coeffs, s["X"].interp_name, self.z0, self.spec, c["method"], self.output,
                                      solver._coop_flags(flags, self.dev), self.plan)

    def kernel_names(self):
        return [(self.lib.ncde_kernel_name(ctypes.byref(self.p), ps) or b"?").decode() for ps in (0, 1, 2)]

    def forward(self, record=False):
        """-> (solution [B, n_out, H], stage record or None), device tensors."""
        from ncde_amd import solver
        out = solver._alloc_out(self.z0, solver._num_outputs(self.coeffs, self.s["X"].interp_name, self.output, self.plan))
        out.fill_(float("nan"))
        stages = solver._launch_forward(self.p, out, record, self.dev)
        torch.cuda.synchronize()
        return out, stages

    def backward(self, out, stages=None):
        """ncde_adjoint on the solution `out`, or with `stages` ncde_backward on the stage record -> {dz0, grads{name: array}}; every
        destination holds NaN before the call."""
        from ncde_amd import _lib, solver
        bound = solver.bind_grads(self.spec, self.z0.shape, self.dev, fill=float("nan"))
        gout = self.s["gout"].contiguous()
        with torch.cuda.device(self.dev):
            ws = solver._workspace(self.p, 1 if stages is None else 2, self.dev)
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            if stages is None:
                rc = self.lib.ncde_adjoint(ctypes.byref(self.p), out.data_ptr(), gout.data_ptr(), ctypes.byref(bound.g), ws.data_ptr(), ws.numel(), stream)
            else:
                rc = self.lib.ncde_backward(ctypes.byref(self.p), stages.data_ptr(), gout.data_ptr(), ctypes.byref(bound.g), ws.data_ptr(), ws.numel(),
                                            stream)
        _lib.check(rc, "ncde_adjoint" if stages is None else "ncde_backward")
        torch.cuda.synchronize()
        return {"dz0": bound.grad_z0.cpu().numpy(), "grads": {k: bound.of(v).cpu().numpy() for k, v in self.s["func"].p.items()}}


def errors(res, ref, names):
    errs = {"z": gu.relerr(res["z_out"], ref["z_out"]), "dz0": gu.relerr(res["dz0"], ref["dz0"])}
    for n in names:
        errs["d" + n] = gu.relerr(res["grads"][n], ref["grads"][n])
    return errs


def check(label, res, ref, names):
    """The project's tolerances, |delta| relative to max |ref|, and the gradient-magnitude condition on EVERY gradient of the
    reference (reset gate, both heads and every inner layer).  Prints the errors before asserting."""
    errs = errors(res, ref, names)
    print(label, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert res["z_out"].shape == ref["z_out"].shape
    for n in names:
        assert res["grads"][n].shape == ref["grads"][n].shape, (label, n)
        assert float(np.abs(ref["grads"][n]).max()) >= MIN_GRAD, (label, n, float(np.abs(ref["grads"][n]).max()))
    assert float(np.abs(ref["dz0"]).max()) >= MIN_GRAD, (label, "dz0")
    assert errs["z"] <= TIGHT_Z, (label, errs)
    assert all(v <= E2E_G for k, v in errs.items() if k != "z"), (label, errs)
    return errs
