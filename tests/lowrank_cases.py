"""Seeded cases for the low-rank kernels (ncde_fwd_lowrank / ncde_adj_lowrank) beyond the reference's stack: layer stacks of
tests/layer_topologies.py, the regimes of the kernels' LDS plan, general time axes and the edges of the head arithmetic.  Shared by
tests/test_lowrank_plan_cpu.py (which validates every case on the CPU: the unfused solver in fp32 against itself in fp64, and the
gradient-magnitude condition) and tests/test_lowrank_stacks_gpu.py (the fused kernels against the unfused solver in fp64).
Helper only: no test functions."""
import functools
import warnings

import numpy as np
import torch

import golden_util as gu
import layer_topologies as lt
import lowrank_util as lu

TIGHT_Z, E2E_G = 2e-5, 2e-4
MIN_GRAD = 1e3 * E2E_G      # every gradient tensor's maximum in the fp64 reference: a wrong gradient cannot hide in a near-zero tensor
OFF_GRID = (0.35, 1.6, 2.85, 4.0)      # output times between the knots 0 .. 4 (the solve starts at 0.35), the last on the last knot
USER_KNOTS = (0.0, 0.7, 1.1, 2.4, 3.0)

CASES = {}


def _case(name, spec, C, R, H, HH=None, B=21, T=5, interp="linear", method="rk4", step=1.0, out="knots", knots=None, seed=1, scale=1.0,
          both=True, gain=1.0, gout=1.0):
    """spec: a layer_topologies.TOPOLOGIES name or a tuple of widths.  out: "knots", "interval" or a tuple of output times.
    both: run on the exact discrete backward as well as on the continuous adjoint.  scale multiplies the head matrices and their biases,
    gain the inner layers' matrices (a deep ReLU stack at torch's Linear scale passes almost nothing on), gout the cotangent dL/dz."""
    assert name not in CASES
    CASES[name] = dict(name=name, spec=spec, C=C, R=R, H=H, HH=HH or H, B=B, T=T, interp=interp, method=method, step=step, out=out,
                       knots=knots, seed=seed, scale=scale, gain=gain, gout=gout, modes=("adjoint", "discrete") if both else ("adjoint",))


# ---- layer stacks: rk4 on the linear path, midpoint on the cubic one ------------------------------------------------------------
STACKS = [("distinct3", 6, 5, 10, 20), ("tied_all3", 5, 2, 10, 10), ("tied_first_last", 5, 2, 12, 12), ("w_tied_b_own", 5, 2, 10, 10),
          ("w_shared_b_own", 5, 2, 10, 14), ("b_shared_w_own", 5, 2, 10, 14), ("deep8_distinct", 5, 2, 10, 12), ((14,), 5, 2, 10, None),
          ((128, 16), 5, 2, 16, None), ((93, 15, 47), 5, 2, 47, None), ((64, 32), 5, 2, 48, None)]
ON_DISCRETE = ("distinct3", "tied_all3", "tied_first_last", "w_tied_b_own", (14,), (128, 16))


def spec_id(spec):
    return spec if isinstance(spec, str) else "H_" + "x".join(str(n) for n in spec)


for _i, (_spec, _C, _R, _H, _HH) in enumerate(STACKS):
    for _interp, _method in (("linear", "rk4"), ("cubic", "midpoint")):
        _case("stack_%s_%s" % (spec_id(_spec), _interp), _spec, _C, _R, _H, _HH, B=37 if _i % 2 else 21, interp=_interp, method=_method,
              seed=100 + _i, both=_spec in ON_DISCRETE, gain=2.0 if _spec == "deep8_distinct" else 1.0,
              gout=2.0 if _spec == "w_shared_b_own" else 1.0)

# ---- LDS plan regimes (tests assert the regime through lowrank_util.lr_plan) ----------------------------------------------------
# name -> (gacc_in_lds, heads resident in the forward, heads resident in the backward)
REGIMES = {"regime_lds_partial_streamed_bwd": (True, True, False), "regime_global_partial_resident": (False, True, True),
           "regime_global_partial_resident_fwd_only": (False, True, False)}
_case("regime_lds_partial_streamed_bwd", (48, 48), 16, 4, 48, B=17, T=3, seed=201)
_case("regime_global_partial_resident", (128, 128, 128), 4, 2, 16, B=17, T=3, seed=202, gout=16.0)
_case("regime_global_partial_resident_fwd_only", (64, 64), 8, 8, 32, B=17, T=3, seed=203)

# ---- time axes: off-grid outputs, steps that do / do not divide the knot spacing, a user knot grid ---------------------------------
for _method, _step in (("rk4", 0.5), ("midpoint", 0.4), ("euler", 1.3)):
    for _interp in ("linear", "cubic"):
        _case("time_%s_%s" % (_method, _interp), "ref_shared3", 5, 2, 10, 12, B=19, interp=_interp, method=_method, step=_step, out=OFF_GRID,
              seed=301, gout=2.0)
_case("time_userknots_rk4", "ref_shared3", 5, 2, 10, 12, B=19, method="rk4", step=0.5, knots=USER_KNOTS, seed=302)
_case("time_userknots_rk4_offgrid", "ref_shared3", 5, 2, 10, 12, B=19, method="rk4", step=0.45, out=(0.2, 0.7, 1.9, 3.0), knots=USER_KNOTS,
      seed=303, gout=2.0)

# ---- edges of the head arithmetic ---------------------------------------------------------------------------------------------------
_case("edge_C1_R1", (12, 12), 1, 1, 10, seed=401, gout=4.0)                                   # Cp = 4 with one live channel
_case("edge_R4_C7", (12, 12), 7, 4, 10, seed=402)                                   # R = LR_RREG; (H + C) R = 68: rows 68 .. 79 are zero
_case("edge_R5_C7", (12, 12), 7, 5, 10, seed=403)                                   # odd, above LR_RREG; (H + C) R = 85
_case("edge_rows_multiple_of_16", (12, 12), 6, 4, 10, seed=404)                     # (H + C) R = 64
_case("edge_dlast_15", (20, 15), 5, 3, 10, seed=405)                                # dlast no multiple of 4
_case("edge_T2_B1_final", (12, 12), 5, 2, 10, B=1, T=2, out="interval", seed=406, gout=32.0)   # one step: n == T - 2 and n == 1 at once
# |M| -> 1: 1 - M^2 cancels.  (gain 1.5, not more: at gain 2 the share is 0.56, but the rk4 steps of size 1 through the saturated field
# make the discrete backward ill-conditioned -- fp32 torch ops on the CPU with tanh as 1 - 2 / (exp(2x) + 1), 2e-7 absolute, move the
# solution by 4.5e-6 and with it every gradient by 4e-4; at gain 1.5 the same arithmetic stays below 4e-6 on every tensor.)
_case("edge_saturated_heads", (12, 12), 5, 3, 10, scale=4.0, gain=1.5, seed=407)
# ---- the accepted documented point's nearest refused neighbour in the rank: the backward's plan passes 160 KB -> the unfused route ---
REFUSED = dict(H=64, C=24, R=10, HH=64, nl=2)
_case("refused_rank10", (64, 64), 24, 10, 64, B=5, T=3, seed=501)
SATURATED_SHARE = 0.25     # at least this share of |M| above 0.99 along the fp64 solution of edge_saturated_heads


@functools.lru_cache(maxsize=None)
def arrays(name):
    """The case's inputs as fp32 arrays (built once; callers do not modify them)."""
    c = CASES[name]
    H, C, R, B, T = c["H"], c["C"], c["R"], c["B"], c["T"]
    layers, dims = lt.stack_of(c["spec"] if isinstance(c["spec"], str) else list(c["spec"]), H, c["HH"])
    p = {k: v for k, v in lt.make_weights(layers, dims, C, H, c["seed"]).items() if k not in ("Wo", "bo")}
    p = {k: (v * np.float32(c["gain"])).astype(np.float32) if k.startswith("W") else v for k, v in p.items()}
    p.update(lu.head_weights(gu.data, H, C, R, dims[-1][0], c["seed"], c["scale"]))
    make = gu.data.make_cubic_coeffs if c["interp"] == "cubic" else gu.data.make_linear_coeffs
    n_out = {"knots": T, "interval": 2}.get(c["out"], len(c["out"]))
    return {"layers": layers, "dims": dims, "params": p, "names": lt.param_names(layers)[:-2] + ["Wh", "bh", "Wq", "bq"],
            "coeffs": np.ascontiguousarray(make(B, T, C - 1, seed=c["seed"] + 1), dtype=np.float32),
            "z0": (gu.data.normal(c["seed"] + 2, B * H, stream=2).reshape(B, H) * 0.5).astype(np.float32),
            "grad_out": (gu.data.normal(c["seed"] + 3, B * n_out * H, stream=1).reshape(B, n_out, H) * (c["gout"] / 2.0)).astype(np.float32)}


def plan_of(name):
    c, a = CASES[name], arrays(name)
    return lu.lr_plan(c["H"], c["C"], c["R"], a["dims"], a["layers"])


def untied(a):
    """Every layer with its OWN equal-valued tensors -> (params, layers, {copy name: original name}): dL/d(tied tensor) is the sum of
    dL/d(its copies), so the reference of a tied stack never shares a tensor."""
    p = {k: a["params"][k] for k in ("Wh", "bh", "Wq", "bq")}
    layers, origin = [], {}
    for l, (w, b) in enumerate(a["layers"]):
        wn, bn = "W%d_%d" % (l, l), "b%d_%d" % (l, l)
        p[wn], p[bn] = a["params"][w].copy(), a["params"][b].copy()
        origin[wn], origin[bn] = w, b
        layers.append((wn, bn))
    return p, layers, origin


def solve(name, mode, dtype, device, untie=False, capture=None, field_probe=None, refused=False):
    """The case -> {z_out, dz0, grads{name: array}} for L = sum(z * grad_out).
    device "cuda": through ncde_amd.cdeint.  fp32: ANY warning is an error (the fused route emits none) and `capture` collects the
    problems handed to the library; fp64: the unfused solver, which must emit its one warning.
    device "cpu": the unfused solver called directly (cdeint has no CPU route).
    untie: the stack of untied(), gradients summed over the copies of each tensor.  field_probe(field, z): called with the field
    module and the solution before the backward.  refused: the fp32 call is expected on the unfused route behind exactly one warning."""
    import ncde_amd
    from ncde_amd import solver, unfused
    c, a = CASES[name], arrays(name)
    adjoint = {"adjoint": True, "discrete": False}[mode]
    params, layers, origin = untied(a) if untie else (a["params"], a["layers"], None)
    func = lu.StackField(params, layers, c["H"], c["C"], c["R"], device, dtype)
    coeffs = torch.from_numpy(a["coeffs"]).to(device=device, dtype=dtype)
    kn = torch.tensor(c["knots"], device=device, dtype=dtype) if c["knots"] is not None else None
    X = (ncde_amd.NaturalCubicSpline if c["interp"] == "cubic" else ncde_amd.LinearInterpolation)(coeffs, kn)
    t = X.grid_points if c["out"] == "knots" else (X.interval if c["out"] == "interval" else torch.tensor(c["out"], device=device, dtype=dtype))
    z0 = torch.from_numpy(a["z0"]).to(device=device, dtype=dtype).requires_grad_(True)
    gout = torch.from_numpy(a["grad_out"]).to(device=device, dtype=dtype)
    if device == "cpu":
        out = unfused.cdeint_unfused(X, func, z0, t, adjoint, "matmul", c["method"], c["step"])
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
                out = ncde_amd.cdeint(X, func, z0, t, adjoint=adjoint, method=c["method"], options={"step_size": c["step"]})
        finally:
            solver.build_problem = real
        if fused:
            assert not unfused._WARNED, unfused._WARNED
        else:
            assert sum("unfused" in str(w.message) for w in rec) == 1, [str(w.message) for w in rec]
    if field_probe is not None:
        field_probe(func, out.detach())
    (out * gout).sum().backward()
    if device != "cpu":
        torch.cuda.synchronize()
    grads = {k: v.grad.detach().cpu().numpy() for k, v in func.p.items()}
    if untie:
        grads = lt.sum_over_copies(grads, origin, a["names"])
    return {"z_out": out.detach().cpu().numpy(), "dz0": z0.grad.cpu().numpy(), "grads": grads}


def errors(res, ref, names):
    errs = {"z": gu.relerr(res["z_out"], ref["z_out"]), "dz0": gu.relerr(res["dz0"], ref["dz0"])}
    for n in names:
        errs["d" + n] = gu.relerr(res["grads"][n], ref["grads"][n])
    return errs


def check(label, res, ref, names):
    """The project's tolerances, |delta| relative to max |ref|, and the gradient-magnitude condition on EVERY gradient of the
    reference (heads and inner layers).  Prints the errors before asserting."""
    errs = errors(res, ref, names)
    print(label, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert res["z_out"].shape == ref["z_out"].shape
    for n in names:
        assert res["grads"][n].shape == ref["grads"][n].shape, (label, n)
        assert float(np.abs(ref["grads"][n]).max()) >= MIN_GRAD, (label, n, float(np.abs(ref["grads"][n]).max()))
    assert errs["z"] <= TIGHT_Z, (label, errs)
    assert all(v <= E2E_G for k, v in errs.items() if k != "z"), (label, errs)
    return errs


def saturated_share(func, z):
    """Share of |M| above 0.99 over the field evaluated at every output state of the solution z [B, n_out, H]."""
    with torch.no_grad():
        M = func(0.0, z.reshape(-1, z.shape[-1]))
    return float((M.abs() > 0.99).double().mean())
