"""Seeded cases for the batch-tiled kernel family (csrc/ncde_tiled.hip: ncde_fwd_tiled, ncde_adj_tiled, ncde_dwo_tiled, ncde_dwo_pair and
their reductions) at the edges of its bookkeeping: one live lane / one exact sample tile / one exact tile pair / a one-sample unpaired
tile / a pass-B wave that owns two sample tiles (and one that owns one) / two part-groups; one- and two-step solves; the planned
instantiations on the degenerate plans of resident_cases.PLANS, with time-window hand-overs on and beside the step where a reverse
solve ends; range faults of the split-fp16 forward late in the solve and in a one-sample tail tile.  Shared by
tests/test_tiled_edges_cpu.py (validates every case without a GPU) and tests/test_tiled_edges_gpu.py (the kernels against the fp64
expectations).  Helper only: no test functions.

Reference, screening and bounds are those of tests/resident_cases.py (its docstring: conditions (i) - (iii), the sample pool), on the
oracle's Field of the set's kind ("original" / "minimal") and input mode ("matmul" / "evaluate" / "derivative"); for the gated field
the sigmoid head's gradients dWg, dbg are held to (i) and (iii) like every other tensor.  The cap on left-out rows and cases is zero.
"""
import ctypes
import functools

import numpy as np
import torch

import golden_util as gu
import resident_cases as rc
import variant_util as vu
from resident_cases import (E2E_G, FAULT_DX, FAULT_Z0, MIN_GRAD, PLANS, POISON, POOL, RELU_MARGIN, STAGES, TIGHT_G, TIGHT_Z,      # noqa: F401
                            Margins, check, errors, is_planned, kind_of, name_matches, t_out)

FORCE_TILED = 0x8000      # NCDE_FLAG_FORCE_TILED: ahead of a shape-specialised kernel set and of the zero-padding onto one
FP32_MFMA = 4             # NCDE_FLAG_FP32_MFMA
LDS_LIMIT = 160 * 1024
WINDOW_BUDGET = 192 << 20      # bytes of per-stage records one time window may hold (per-workgroup sequence)

# set -> (C, H, HH, nl, field kind, input mode, flags): the smallest shapes that select each instantiation
SETS = {"T16": (8, 16, 16, 2, "original", "matmul", FORCE_TILED),      # PK 1, RES 1 sweep, fp32 records, ncde_dwo_tiled<1>; fp32-input forward
        "T32r1": (8, 32, 32, 2, "original", "matmul", FORCE_TILED),    # RES 1 at its limit (H C / 16 = 16); forward: resident hidden fragments
        "T32r2": (12, 32, 32, 2, "original", "matmul", FORCE_TILED),   # RES 2, split-bf16 records, ncde_dwo_pair<2>
        "T48": (8, 48, 64, 2, "original", "matmul", FORCE_TILED),      # streamed weights, pair records PK 4 (no kernel set to pad onto: the flag changes nothing)
        "T1L": (4, 16, 32, 1, "original", "matmul", FORCE_TILED),      # one layer, streamed, pair PK 2
        "G32": (8, 32, 32, 2, "minimal", "matmul", 0),                 # gated sweep + ncde_dwo_pair<2, 3> (both heads in one pass)
        "G16": (4, 16, 16, 2, "minimal", "matmul", 0),                 # gated, fp32 records: ncde_dwo_tiled head pass + the gate head's own
        "D32": (8, 32, 32, 2, "original", "evaluate", 0),              # direct sweep, no records, LDS-resident matrices
        "DG32": (8, 32, 32, 2, "minimal", "derivative", 0),            # gated direct
        "W160": (4, 160, 32, 1, "original", "matmul", FORCE_TILED),    # BIGH sweep (4 waves), pair records
        "W256": (4, 32, 256, 1, "original", "matmul", FORCE_TILED)}    # W16 mode, ncde_dwo_tiled<16, 0, 1>
# kernel names (forward, continuous adjoint, discrete backward), on either time axis; "+" joins required substrings
_A, _AD = "ncde_adj_tiled", "ncde_adj_tiled<discrete"
NAMES = {"T16": ("ncde_fwd_tiled<NS1>", _A + "+ncde_dwo_tiled", _AD + ">+ncde_dwo_tiled"),
         "T32r1": ("ncde_fwd_tiled<NS1,fp16x2>", _A + "+ncde_dwo_tiled", _AD + ">+ncde_dwo_tiled"),
         "T32r2": ("ncde_fwd_tiled<NS1,fp16x2>", _A + "<bf16>+ncde_dwo_pair", _AD + ",bf16>+ncde_dwo_pair"),
         "T48": ("ncde_fwd_tiled<NS1,fp16x2>", _A + "<bf16>+ncde_dwo_pair", _AD + ",bf16>+ncde_dwo_pair"),
         "T1L": ("ncde_fwd_tiled<NS1,fp16x2>", _A + "<bf16>+ncde_dwo_pair", _AD + ",bf16>+ncde_dwo_pair"),
         "G32": ("ncde_fwd_tiled<NS1,gated,fp16x2>", _A + "<gated,bf16>+ncde_dwo_pair", _A + "<gated,discrete,bf16>+ncde_dwo_pair"),
         "G16": ("ncde_fwd_tiled<NS1,gated>", _A + "<gated>+ncde_dwo_tiled", _A + "<gated,discrete>+ncde_dwo_tiled"),
         "D32": ("ncde_fwd_tiled<NS1,direct>", _A + "<direct>", _A + "<direct,discrete>"),
         "DG32": ("ncde_fwd_tiled<NS1,gated,direct>", _A + "<gated,direct>", _A + "<gated,direct,discrete>"),
         "W160": ("ncde_fwd_tiled<NS1,fp16x2>", _A + "<wide,bf16>+ncde_dwo_pair", _A + "<wide,discrete,bf16>+ncde_dwo_pair"),
         "W256": ("ncde_fwd_tiled<NS1>", _A + "<wide>+ncde_dwo_tiled", _A + "<wide,discrete>+ncde_dwo_tiled")}

CASES = {}


def _case(name, kset, B, T, path, method, out, seed, group, step=1.0, knots=None, t64=False, gout=8.0, base=None, rows=None, outlier=None):
    """The layout of resident_cases._case (so that its _walk / _control / t_out read a case of this table as one of their own)."""
    assert name not in CASES and kset in SETS
    CASES[name] = dict(name=name, set=kset, B=B, T=T, path=path, method=method, out=out, seed=seed, group=group, step=step, knots=knots,
                       t64=t64, gout=gout, base=base, rows=rows, outlier=outlier, bump=None)


# ---- 1. batch edges: T = 4, linear, rk4, every knot.  B = 129: nine sample tiles = four pairs + a ONE-sample unpaired tile, two
# part-groups of pass B.  Its row subsets: one live lane, one exact tile, tile + one sample, one exact pair, pair + a one-sample unpaired
# tile, and seven tiles = one part-group whose four fp32 pass-B waves own 2, 2, 2, 1 sample tiles.
BATCH_SETS = ("T16", "T32r2", "T48", "G32")
BATCH_ROWS = {1: (128, 129), 16: (0, 16), 17: (0, 17), 32: (0, 32), 33: (0, 33), 97: (0, 97)}
BATCH_SIZES = (129,) + tuple(sorted(BATCH_ROWS))
_GOUT = {"G32": 16.0, "G16": 24.0, "DG32": 16.0}      # the gated fields' gradients are about half the original field's
for _i, _set in enumerate(BATCH_SETS):
    _b129 = "batch_%s_B129" % _set
    _case(_b129, _set, 129, 4, "linear", "rk4", "knots", 2000 + 10 * _i, "batch", gout=_GOUT.get(_set, 8.0))
    for _B, _rows in sorted(BATCH_ROWS.items()):
        _case("batch_%s_B%d" % (_set, _B), _set, _B, 4, "linear", "rk4", "knots", None, "batch", base=_b129, rows=_rows,
              gout=_GOUT.get(_set, 8.0) * (4.0 if _B == 1 else 1.0))
# ncde_dwo_tiled fetches one (stage, sample tile) fragment ahead and steps two per iteration: the fragment "past the end" (the last
# one again, zero cotangent) is CONSUMED only where stages x tiles of a wave is odd -- never with the two or four stages of midpoint /
# rk4.  Euler over three steps on the fp32-record set: odd for the waves owning one tile (B = 97: the fourth; B = 129: seven of eight).
_case("batch_T16_euler_B129", "T16", 129, 4, "linear", "euler", "knots", 2100, "batch")
_case("batch_T16_euler_B97", "T16", 97, 4, "linear", "euler", "knots", None, "batch", base="batch_T16_euler_B129", rows=(0, 97))
EULER_SIZES = (129, 97)

# ---- 2. short solves: one and two steps on every set -------------------------------------------------------------------------------------
for _i, _set in enumerate(SETS):
    for _T in (2, 3):
        _case("steps_%s_T%d_linear_rk4_interval" % (_set, _T), _set, 17, _T, "linear", "rk4", "interval", 2200 + 10 * _i + _T, "steps",
              gout=_GOUT.get(_set, 8.0))
        _case("steps_%s_T%d_cubic_midpoint_knots" % (_set, _T), _set, 17, _T, "cubic", "midpoint", "knots", 2400 + 10 * _i + _T, "steps",
              gout=_GOUT.get(_set, 8.0))

# ---- 3. plan edges: resident_cases.PLANS (a) - (g) --------------------------------------------------------------------------------------------
PLAN_SETS = ("T32r2", "T48", "G32", "D32", "W160")
for _i, _set in enumerate(PLAN_SETS):
    for _j, (_k, (_T, _step, _t, _kn, _f64)) in enumerate(sorted(PLANS.items())):
        for _path, _m in (("linear", "rk4"), ("cubic", "midpoint")):
            if _kn is not None and _path == "cubic":
                continue
            _case("plan_%s_%s_%s_%s" % (_k, _set, _path, _m), _set, 19, _T, _path, _m, _t, 2600 + 100 * _i + 10 * _j, "plan", step=_step,
                  knots=_kn, t64=_f64, gout=_GOUT.get(_set, 8.0))
# Forced time windows of 1 and 2 reverse steps (NCDE_FLAG_TILED_WINDOW_STEPS) on the continuous adjoint of each plan: (reverse steps,
# forward steps, {window: does a window boundary fall on a step that ends a reverse solve (y := z(t[i-1]), a += dL/dz)?}).  Two steps
# per window put the boundary ON that step in (a), (c), (e), (f) and just beside it in (b), (d), (g).  (e) and (g): more reverse than
# forward steps, so the default window (the larger count) is longer than the discrete backward's whole solve.
PLAN_WINDOWS = {"a": (3, 1, {1: True, 2: True}), "b": (6, 6, {1: True, 2: False}), "c": (3, 3, {1: True, 2: True}),
                "d": (3, 3, {1: True, 2: False}), "e": (9, 8, {1: True, 2: True}), "f": (3, 3, {1: True, 2: True}),
                "g": (7, 5, {1: True, 2: False})}

# ---- 4. range faults of the split-fp16 forward (OUT_KNOTS; the backward of this family does not speculate on range) -----------------------------
for _i, (_set, _seed) in enumerate((("T48", 3252), ("G32", 3209))):      # (seeds 3200, 3201: the outlier sample misses (ii))
    _case("fault_late_%s" % _set, _set, 37, 5, "linear", "rk4", "knots", _seed, "fault", outlier=(21, "dx", FAULT_DX), gout=_GOUT.get(_set, 8.0))
    _case("fault_tail_%s" % _set, _set, 33, 2, "linear", "rk4", "knots", 3210 + _i, "fault", outlier=(32, "z0", FAULT_Z0), gout=_GOUT.get(_set, 8.0))

BY_GROUP = {g: sorted(n for n, c in CASES.items() if c["group"] == g) for g in ("batch", "steps", "plan", "fault")}


def dims_of(name):
    return SETS[CASES[name]["set"]]


def stack_of(kset):
    """-> (layers [(Wname, bname)], dims [(out, in)]): the reference's stack, layer 0 then one shared layer."""
    C, H, HH, nl, _, mode, _ = SETS[kset]
    return vu.ref_stack(mode, C, H, HH, nl)


def names_of(name):
    kset = CASES[name]["set"]
    return vu.param_names(stack_of(kset)[0], SETS[kset][4])


def flags_of(name):
    return SETS[CASES[name]["set"]][6]


def want_names(name):
    return NAMES[CASES[name]["set"]]


def _weights(kset, seed):
    C, H, HH, nl, kind, mode, _ = SETS[kset]
    if (kind, mode) == ("original", "matmul"):      # as resident_cases draws them
        p = dict(gu.data.make_field_weights(H, HH, C, seed=seed))
        return {k: v for k, v in p.items() if nl > 1 or k not in ("W1", "b1")}
    layers, dims = stack_of(kset)
    return vu.make_weights(layers, dims, kind, mode, C, H, seed)


def _make_paths(c, n, seed):
    C = SETS[c["set"]][0]
    if c["path"] == "cubic":
        x = gu.data.make_cubic_coeffs(n, c["T"], C - 1, seed=seed)
    else:
        x = gu.data.make_linear_coeffs(n, c["T"], C - 1, seed=seed).copy()
        if c["knots"] is not None:
            x[:, :, 0] = np.asarray(c["knots"], np.float32)[None, :]
    return np.ascontiguousarray(x, dtype=np.float32)


def field_of(c, params, dtype):
    """The oracle's Field of the set's kind and input mode on `params` in `dtype` (a repeated name is one tensor)."""
    import ncde_oracle as orc
    C, H, _, _, kind, mode, _ = SETS[c["set"]]
    t = {k: torch.from_numpy(v).to(dtype) for k, v in params.items()}
    return orc.Field([(t[w], t[b]) for w, b in stack_of(c["set"])[0]], t["Wo"], t["bo"], H, C, kind, mode, t.get("Wg"), t.get("bg"))


def _switch_off(W0):
    """A direction v with W0 v <= -0.1 in every row (W0 v = -1 exactly where W0 is square): a state of any size along it switches every
    unit of layer 0 off (resident_cases.arrays on why).  Rows beyond the columns (HH > H): cyclic projections onto the violated
    half-spaces, from the least-squares solution."""
    W = W0.astype(np.float64)
    v = -np.linalg.lstsq(W, np.ones(W.shape[0]), rcond=None)[0]
    for _ in range(100000):
        r = W @ v
        i = int(np.argmax(r))
        if r[i] <= -0.1:
            return v
        v -= (r[i] + 0.2) / float(W[i] @ W[i]) * W[i]
    raise AssertionError("no direction switches every unit of layer 0 off")


@functools.lru_cache(maxsize=None)
def arrays(name):
    """The case's inputs as fp32 arrays (built once; callers do not modify them): coeffs, z0, params, grad_out; for a range-fault
    case also clean_coeffs / clean_z0 (the batch without its outlier)."""
    c = CASES[name]
    C, H = SETS[c["set"]][:2]
    if c["base"] is not None:
        b = arrays(c["base"])
        lo, hi = c["rows"]
        return {"params": b["params"], "coeffs": np.ascontiguousarray(b["coeffs"][lo:hi]), "z0": np.ascontiguousarray(b["z0"][lo:hi]),
                "grad_out": np.ascontiguousarray(b["grad_out"][lo:hi] * np.float32(c["gout"] / CASES[c["base"]]["gout"]))}
    seed, B = c["seed"], c["B"]
    p = _weights(c["set"], seed)
    for pool in POOL:      # keep the first B candidates that pass (ii) against the pool-wide layer maxima
        n = pool * B
        coeffs = _make_paths(c, n, seed + 1)
        z0 = (gu.data.normal(seed + 2, n * H, stream=2).reshape(n, H) * 0.5).astype(np.float32)
        field = field_of(c, p, torch.float64)
        mg = Margins(field)
        rc._walk(c, field, rc._control(c, coeffs, torch.float64), torch.from_numpy(z0).double(), None)
        keep = np.nonzero(mg.per_sample() >= RELU_MARGIN)[0][:B]
        if len(keep) == B:
            break
    assert len(keep) == B, (name, len(keep))
    coeffs, z0 = np.ascontiguousarray(coeffs[keep]), np.ascontiguousarray(z0[keep])
    a = {"params": p}
    if c["outlier"] is not None:
        s, what, mag = c["outlier"]
        a["clean_coeffs"], a["clean_z0"] = coeffs.copy(), z0.copy()
        if what == "z0":
            v = _switch_off(p["W0"])
            z0[s] = (v * (mag / np.abs(v).max())).astype(np.float32)
        else:
            coeffs[s, 2:, min(5, C - 1)] += np.float32(mag)      # a value channel moves by `mag` on piece 1 and stays there
    n_out = len(c["out"]) if is_planned(c) else (c["T"] if c["out"] == "knots" else 2)
    a["coeffs"], a["z0"] = coeffs, z0
    a["grad_out"] = (gu.data.normal(seed + 3, B * n_out * H, stream=1).reshape(B, n_out, H) * (c["gout"] / 2.0)).astype(np.float32)
    if c["outlier"] is not None and c["outlier"][1] == "dx":
        a["grad_out"][c["outlier"][0]] = 0.0      # (resident_cases.arrays: the late outlier carries no cotangent)
    return a


def _as_np(w, names):
    dz0, gp = w
    assert len(gp) == len(names)
    return {"dz0": dz0.numpy(), "grads": {n: g.numpy() for n, g in zip(names, gp)}}


def walk(name, coeffs, z0, gout, dtype):
    """The oracle in `dtype` on the case's field -> resident_cases._walk's dict."""
    c, a = CASES[name], arrays(name)
    return rc._walk(c, field_of(c, a["params"], dtype), rc._control(c, coeffs, dtype), torch.from_numpy(z0).to(dtype),
                    torch.from_numpy(gout).to(dtype))


@functools.lru_cache(maxsize=None)
def expect(name, clean=False):
    """The fp64 oracle on the case -> dict(z_out, stages, adjoint {dz0, grads}, discrete {dz0, grads}, margin [B], layer_max);
    clean: on the batch without its outlier (range-fault cases)."""
    c, a = CASES[name], arrays(name)
    coeffs, z0 = (a["clean_coeffs"], a["clean_z0"]) if clean else (a["coeffs"], a["z0"])
    field = field_of(c, a["params"], torch.float64)
    mg = Margins(field)
    w = rc._walk(c, field, rc._control(c, coeffs, torch.float64), torch.from_numpy(z0).double(), torch.from_numpy(a["grad_out"]).double())
    names = names_of(name)
    return {"z_out": w["z"].numpy(), "stages": w["stages"].numpy(), "adjoint": _as_np(w["adjoint"], names),
            "discrete": _as_np(w["discrete"], names), "margin": mg.per_sample(), "layer_max": dict(mg.mx)}


def outlier_margin(name):
    """(ii) for the outlier sample of a range-fault case on its own (resident_cases.outlier_margin)."""
    c, a = CASES[name], arrays(name)
    s = c["outlier"][0]
    field = field_of(c, a["params"], torch.float64)
    worst = [1.0]

    def obs(li, pre):
        worst[0] = min(worst[0], float(pre.abs().min() / pre.abs().max()))
    field.on_pre = obs
    rc._walk(c, field, rc._control(c, a["coeffs"][s:s + 1], torch.float64), torch.from_numpy(a["z0"][s:s + 1]).double(), None)
    return worst[0]


@functools.lru_cache(maxsize=None)
def oracle32(name):
    """The fp32 oracle on the case: end to end (its own z) and the continuous adjoint on the fp64 z_out rounded to fp32."""
    import ncde_oracle as orc
    c, a = CASES[name], arrays(name)
    names = names_of(name)
    w = walk(name, a["coeffs"], a["z0"], a["grad_out"], torch.float32)
    res = {"z_out": w["z"].numpy(), "adjoint": _as_np(w["adjoint"], names), "discrete": _as_np(w["discrete"], names)}
    field, ctl, gout = field_of(c, a["params"], torch.float32), rc._control(c, a["coeffs"], torch.float32), torch.from_numpy(a["grad_out"])
    z64 = torch.from_numpy(expect(name)["z_out"].astype(np.float32))
    if is_planned(c):
        iso = orc.solve_adjoint_times(ctl, field, torch.from_numpy(t_out(c)), z64, gout, c["method"], c["step"])
    else:
        iso = orc.solve_adjoint(ctl, field, z64, gout, c["method"], c["out"] == "knots")
    res["adjoint_iso"] = _as_np(iso, names)
    return res


def poisoned(name):
    """resident_cases.poisoned on a case of this table: the pieces a plan (c) / (f) solve never reads, overwritten."""
    x = arrays(name)["coeffs"].copy()
    x[:, 0], x[:, -1] = POISON, -POISON
    return x


def golden_case(name, coeffs=None, z0=None):
    """The case in the layout gpu_util / cpu_lib_util take (default axis)."""
    c, a = CASES[name], arrays(name)
    C, H, HH, nl, kind, mode, _ = SETS[c["set"]]
    return {"meta": {"kind": kind_of(c), "method": c["method"], "sequence": c["out"] == "knots", "param_names": names_of(name),
                     "field_kind": kind, "field_mode": mode, "dims": {"C": C, "H": H, "HH": HH, "nl": nl}, "field": kind},
            "coeffs": a["coeffs"] if coeffs is None else coeffs, "z0": a["z0"] if z0 is None else z0, "params": a["params"],
            "layers": stack_of(c["set"])[0], "H": H, "C": C, "expect": {"grad_out": a["grad_out"]}}


def times_case(name, coeffs=None):
    """The case in the layout gpu_util.run_times_case takes (general time axis) -> (f, meta, kind, mode)."""
    c, a = CASES[name], arrays(name)
    f = {"coeffs": a["coeffs"] if coeffs is None else coeffs, "z0": a["z0"], "t_out": t_out(c), "grad_out": a["grad_out"]}
    if c["knots"] is not None:
        f["knots"] = np.asarray(c["knots"], np.float32)
    kset = SETS[c["set"]]
    return f, {"kind": kind_of(c), "method": c["method"], "step_size": c["step"], "dims": {"nl": kset[3]}}, kset[4], kset[5]


def problem_of(name, flags=None, device="cpu"):
    """-> (NcdeProblem of the case under `flags` (None: the set's own), the time plan's host words or None, the tensors it points into)."""
    import gpu_util
    import ncde_amd
    from ncde_amd import _lib, solver
    c, a = CASES[name], arrays(name)
    kset = SETS[c["set"]]
    cc = torch.from_numpy(a["coeffs"]).to(device)
    kn = None if c["knots"] is None else torch.tensor(c["knots"], dtype=torch.float32, device=device)
    X = (ncde_amd.NaturalCubicSpline if c["path"] == "cubic" else ncde_amd.LinearInterpolation)(cc, t=kn)
    func = gpu_util.CaseField(a["params"], stack_of(c["set"])[0], device, kset[4], kset[5])
    plan, output = None, (_lib.OUT_KNOTS if c["out"] == "knots" else _lib.OUT_INTERVAL)
    if is_planned(c):
        plan = solver._time_plan(X, torch.from_numpy(t_out(c)), c["method"], c["step"], torch.device(device))
        output = _lib.OUT_TIMES
    z0 = torch.from_numpy(a["z0"]).to(device)
    p = solver.build_problem(cc, kind_of(c), z0, func.fused_spec(), c["method"], output, kset[6] if flags is None else flags, plan)
    return p, (None if plan is None else plan[0].cpu().numpy()), (cc, z0, func, plan)


def kernel_names(name, flags=None, device="cpu"):
    """(forward, adjoint, discrete backward) names the library dispatches the case to: a host-side query, no GPU needed."""
    from ncde_amd import _lib
    p, _, _keep = problem_of(name, flags, device)
    return tuple((_lib.lib().ncde_kernel_name(ctypes.byref(p), k) or b"?").decode() for k in (0, 1, 2))


def workspace_bytes(name, pass_, flags=None):
    from ncde_amd import _lib
    p, _, _keep = problem_of(name, flags)
    return int(_lib.lib().ncde_workspace_bytes(ctypes.byref(p), pass_))


# ---- the backward's plan, restated (tiled_adj_plan: per-workgroup sequence, matmul input) ------------------------------------------
def adj_plan(name, flags=None, steps=None):
    """-> dict(n_st, pairs, bf, nrt, parts, window, total): sample tiles and tile pairs, split-bf16 records?, row tiles per pass-B wave,
    part-groups of pass B, steps per time window, floats of the workspace.  steps: reverse steps of the solve (default axis: T - 1)."""
    c = CASES[name]
    C, H, HH, nl, kind, mode, own = SETS[c["set"]]
    flags = own if flags is None else flags
    assert mode == "matmul"
    gated, S, n_st = kind == "minimal", STAGES[c["method"]], (c["B"] + 15) // 16
    pk = HH // 16
    square = pk in (1, 2, 4) and H == HH
    res = 0 if not square else (1 if not gated and H * C // 16 <= 16 and not is_planned(c) else 2)
    lds = 4 * (4 * H * 16 + (nl + 2) * max(16, HH) * 16 + C * 16 + (4 if H > 128 or HH == 256 else 8) * (256 * pk + 64))
    bf = not flags & FP32_MFMA and 2 <= pk <= 8 and res != 1 and lds + pk * 16 * 16 * 6 <= LDS_LIMIT
    rec_a = HH * (24 if bf else 16)
    steps = c["T"] - 1 if steps is None else steps
    window = max(1, min(steps, WINDOW_BUDGET // (S * n_st * (2 * rec_a + (H + C) * 16) * 4)))
    forced = (flags >> 16) & 0xFF
    window = min(steps, forced) if forced else window
    tiles = window * S * n_st
    row_tiles = H * C // 16
    nrt = 1 if gated or HH == 256 else (4 if row_tiles % 4 == 0 and row_tiles >= 64 and HH < 128 else (2 if row_tiles % 2 == 0 and row_tiles >= 32 else 1))
    parts = 1
    while parts < 64 and (row_tiles // nrt) * 4 * parts < 4096 and 4 * parts * 2 <= n_st:
        parts *= 2
    hidden = HH * H + HH + (HH * HH + HH if nl > 1 else 0)      # the sweep's per-workgroup partial: every distinct hidden tensor once
    theta_o = H * C * HH + H * C
    pack = H * C * HH * (2 if gated else 1)
    total = 64 + tiles * rec_a + (window * S * ((n_st + 1) // 2) * HH * 48 if bf else tiles * HH * 16) + tiles * (H + C) * 16
    total += n_st * hidden + parts * theta_o * (2 if gated else 1) + 2 * n_st * H * 16 + pack + (pack + pack // 2 if bf and not gated else 0) + 64
    return {"n_st": n_st, "pairs": (n_st + 1) // 2, "bf": bool(bf), "nrt": nrt, "parts": parts, "window": window, "total": total}


def expected_workspace_bytes(name, flags=None):
    return 4 * adj_plan(name, flags)["total"]


def window_on_reset(words, window):
    """Does a boundary between two time windows of `window` reverse steps fall on a step that ends a reverse solve (the plan's
    adjoint step words: [dt, output row or -1, 0, stages...])?  Reverse step q is the q-th of the adjoint table; the windows cut
    behind every window-th step."""
    S, n_adj, off_adj = int(words[1]), int(words[3]), int(words[7])
    rows = words[off_adj:off_adj + n_adj * (3 + 3 * S)].reshape(n_adj, 3 + 3 * S)[:, 1]
    return any(rows[q - 1] >= 0 for q in range(window, n_adj, window))
