"""Seeded cases for the register-resident kernel family (ncde_fast_kernels.h and its instantiating units, ncde_fast64.hip,
ncde_fast4.hip) at the edges of its bookkeeping: the three-slot dX/dt ring with 1 .. 6 pieces, the stage-record fetch of a one-step
solve, the zero-quad slot words on short rectilinear paths, one live lane / one full tile / a one-sample tail tile, the planned
instantiations on degenerate plans, and range faults that appear late or in a one-sample tile.  Shared by
tests/test_resident_edges_cpu.py (validates every case without a GPU) and tests/test_resident_edges_gpu.py (the kernels against
the fp64 expectations).  Helper only: no test functions.

Reference: oracle/ncde_oracle.py on float64 copies of the fp32 inputs; the output times of a planned case keep their own dtype, so
the time arithmetic stays that of the product path.

Screening (a case is accepted only if all hold; tests/test_resident_edges_cpu.py asserts them):
  (i)   the oracle in fp32 agrees with the oracle in fp64 within HALF of each bound, on z and every gradient, continuous and discrete;
  (ii)  no ReLU pre-activation along the fp64 solution (every sample, stage, layer; the forward solve, whose stages are the discrete
        backward's, and the reverse sweep of the continuous adjoint) is smaller than RELU_MARGIN x that layer's largest one;
  (iii) every gradient tensor's fp64 maximum is at least MIN_GRAD.
Random inputs of these sizes hold ten to twenty pre-activations below 1e-4 x the layer maximum (13,056 evaluations per layer at
B = 17, T = 7, rk4), so no seed of a whole batch passes (ii).  Samples do not interact along the solution: each case draws a POOL of
candidate samples from its seed and keeps the first B that pass (ii) on their own against the pool-wide layer maxima (which bound
the batch's own maxima from above: the kept samples pass with room).  The table holds the final seeds.
"""
import ctypes
import functools

import numpy as np
import torch

import golden_util as gu

TIGHT_Z, TIGHT_G, E2E_G = 2e-5, 2e-5, 2e-4
MIN_GRAD = 1e3 * E2E_G      # every gradient tensor's maximum in the fp64 reference: a wrong gradient cannot hide in a near-zero tensor
RELU_MARGIN = 1e-4
POOL = (8, 64)              # candidate samples drawn per kept sample (the second pool where the first holds too few)
STAGES = {"rk4": 4, "midpoint": 2, "euler": 1}

# (C, H, HH, nl) of every kernel set
SETS = {"R20": (20, 32, 32, 3), "R20nl1": (20, 32, 32, 1), "R20nl2": (20, 32, 32, 2), "R20nl4": (20, 32, 32, 4),
        "Rc4": (4, 32, 32, 3), "Rc8": (8, 32, 32, 3), "Rc12": (12, 32, 32, 3), "R40": (40, 32, 32, 3), "R64": (4, 64, 64, 3),
        "pad5": (5, 16, 15, 3), "pad3": (3, 47, 32, 2)}
# kernel-name prefixes (forward, continuous adjoint, discrete backward) on the default axis; "+" joins required substrings
_F32, _F64 = "ncde_fwd_fast_bf3<H32,HH32,C%d,", "ncde_fwd_fast_bf3<H64,HH64,C4,"
NAMES = {"R20": (_F32 % 20, "ncde_adj_fast3<H32,HH32,C20,NL3", "ncde_adj_fast3<H32,HH32,C20,NL3+discrete"),
         "R20nl1": (_F32 % 20, "ncde_adj_fast3<H32,HH32,C20,NL1", "ncde_adj_fast3<H32,HH32,C20,NL1+discrete"),
         "R20nl2": (_F32 % 20, "ncde_adj_fast3<H32,HH32,C20,NL2", "ncde_adj_fast3<H32,HH32,C20,NL2+discrete"),
         "R20nl4": (_F32 % 20, "ncde_adj_fast3<H32,HH32,C20,NL4", "ncde_adj_fast3<H32,HH32,C20,NL4+discrete"),
         "Rc4": (_F32 % 4, "ncde_adj_fast3<H32,HH32,C4,NL3", "ncde_adj_fast3<H32,HH32,C4,NL3+discrete"),
         "Rc8": (_F32 % 8, "ncde_adj_fast3<H32,HH32,C8,NL3", "ncde_adj_fast3<H32,HH32,C8,NL3+discrete"),
         "Rc12": (_F32 % 12, "ncde_adj_fast3<H32,HH32,C12,NL3", "ncde_adj_fast3<H32,HH32,C12,NL3+discrete"),
         "R40": (_F32 % 40, "ncde_adj_tiled", "ncde_adj_tiled"),      # forward-only set: the backward is the batch-tiled family's
         "R64": (_F64, "ncde_adj_h64", "ncde_adj_h64+discrete"),
         "pad5": (_F32 % 8, "ncde_adj_fast3<H32,HH32,C8,NL3", "ncde_adj_fast3<H32,HH32,C8,NL3+discrete"),
         "pad3": (_F64, "ncde_adj_h64", "ncde_adj_h64+discrete")}
# planned instantiations: the forward and (R20) the adjoint walk the time plan; the planned discrete backward exists on the
# batch-tiled family only (a documented limitation: the name is asserted, the numbers are compared all the same)
PLAN_NAMES = {"R20": (_F32 % 20 + "+time plan", "ncde_adj_fast3<H32,HH32,C20,NL3+time plan", "ncde_adj_tiled"),
              "R64": (_F64 + "+time plan", "ncde_adj_h64", "ncde_adj_tiled"),
              "pad5": (_F32 % 20 + "+time plan", "ncde_adj_fast3<H32,HH32,C20,NL3+time plan", "ncde_adj_tiled")}      # planned: onto C20

CASES = {}


def _case(name, kset, B, T, path, method, out, seed, group, step=1.0, knots=None, t64=False, gout=8.0, base=None, rows=None,
          outlier=None, bump=None):
    """path: "linear" / "cubic" (T knots) or "rect" (T = 2 L - 1 knots of a rectilinear path, linear evaluation).  out: "interval",
    "knots" or a tuple of output times (the planned instantiations).  base / rows: the samples `rows` of case `base` (sample
    independence across batch sizes).  outlier: (sample, "z0" | "dx", magnitude).  bump: (sample, piece, channel, delta)."""
    assert name not in CASES and kset in SETS
    CASES[name] = dict(name=name, set=kset, B=B, T=T, path=path, method=method, out=out, seed=seed, group=group, step=step, knots=knots,
                       t64=t64, gout=gout, base=base, rows=rows, outlier=outlier, bump=bump)


# ---- 1. ring phases, default axis --------------------------------------------------------------------------------------------------
RING_T = (2, 3, 4, 5, 7)
for _T in RING_T:
    for _path in ("linear", "cubic"):
        for _m in ("rk4", "midpoint", "euler"):
            for _out in ("interval", "knots"):
                _case("ring_R20_T%d_%s_%s_%s" % (_T, _path, _m, _out), "R20", 17, _T, _path, _m, _out, 1000 + 10 * _T, "ring")
for _i, _set in enumerate(s for s in SETS if s != "R20"):
    for _T in (2, 4):
        _case("ring_%s_T%d_linear_rk4_interval" % (_set, _T), _set, 17, _T, "linear", "rk4", "interval", 1200 + 10 * _i + _T, "ring")
        _case("ring_%s_T%d_cubic_midpoint_knots" % (_set, _T), _set, 17, _T, "cubic", "midpoint", "knots", 1300 + 10 * _i + _T, "ring")
# rectilinear paths of raw length 2, 3, 4: time-only pieces alternate with value pieces, the slot words change owner on every step
for _set in ("R20", "Rc8", "Rc12"):
    for _L in (2, 3, 4):
        _case("skip_%s_L%d" % (_set, _L), _set, 17, 2 * _L - 1, "rect", "rk4", "knots", 1400 + _L, "skip")
# one sample of the tile moves channel 4 on the time-only piece of a three-knot path
_case("skip_R20_L2_one_sample_channel4", "R20", 17, 3, "rect", "rk4", "knots", 1402, "skip", bump=(5, None, 4, 0.25))

# ---- 2. batch edges: one live lane, one full tile, a one-sample tail tile --------------------------------------------------------------
BATCH_SETS = ("R20", "R64", "Rc8")
for _i, _set in enumerate(BATCH_SETS):
    for _T in (2, 4):
        _b33 = "batch_%s_T%d_B33" % (_set, _T)
        _case(_b33, _set, 33, _T, "linear", "rk4", "knots", 1500 + 10 * _i + _T, "batch")
        _case("batch_%s_T%d_B16" % (_set, _T), _set, 16, _T, "linear", "rk4", "knots", None, "batch", base=_b33, rows=(0, 16))
        _case("batch_%s_T%d_B1" % (_set, _T), _set, 1, _T, "linear", "rk4", "knots", None, "batch", base=_b33, rows=(32, 33), gout=32.0)

# ---- 3. plan edges (T = 4 knots unless the plan needs more) ---------------------------------------------------------------------------------------
PLAN_SETS = ("R20", "R64", "pad5")
USER_KNOTS = (0.0, 0.7, 1.1, 2.4)
# letter -> (T, step, output times, user knots, fp64 t)
PLANS = {"a": (4, 4.0, (0.0, 0.8, 1.9, 3.0), None, False),      # ONE forward step: outputs of kind 2, 2, 1; every reverse solve one step
         "b": (4, 0.5, (0.0, 0.5, 1.5, 3.0), None, False),      # outputs on grid points (kinds 0 / 1); cnt = 0 on [1.5, 2] and [2, 2.5]
         "c": (5, 0.5, (1.25, 1.75, 2.5), None, False),         # five knots: starts in piece 1, ends in piece 2; pieces 0 and 3 never read
         "d": (7, 2.5, (0.0, 4.0, 6.0), None, False),           # the stages of one step sit in different pieces
         "e": (2, 0.125, (0.0, 0.3, 1.0), None, False),         # eight steps in the only piece
         "f": (5, 0.5, (1.25, 1.75, 2.5), None, True),          # (c) with an fp64 t (time_is_f64 = 1)
         "g": (4, 0.45, (0.2, 0.9, 1.5, 2.4), USER_KNOTS, False)}      # uneven user knots, off-grid outputs
for _i, _set in enumerate(PLAN_SETS):
    for _j, (_k, (_T, _step, _t, _kn, _f64)) in enumerate(sorted(PLANS.items())):
        for _path, _m in (("linear", "rk4"), ("cubic", "midpoint")):
            if _kn is not None and _path == "cubic":
                continue
            _case("plan_%s_%s_%s_%s" % (_k, _set, _path, _m), _set, 19, _T, _path, _m, _t, 1600 + 100 * _i + 10 * _j, "plan", step=_step,
                  knots=_kn, t64=_f64)

# ---- 4. range faults at the edges (forward kernels, OUT_KNOTS) -------------------------------------------------------------------------
FAULT_DX = 3.0e5      # increment of one value channel in piece 1: |z| passes the fp16 operand range from step 2 on
FAULT_Z0 = 1.0e5      # largest |z0| of the outlier row
for _i, _set in enumerate(("R20", "R64")):
    _case("fault_late_%s" % _set, _set, 37, 5, "linear", "rk4", "knots", 1900 + _i, "fault", outlier=(21, "dx", FAULT_DX))
    _case("fault_tail_%s" % _set, _set, 33, 2, "linear", "rk4", "knots", 1910 + _i, "fault", outlier=(32, "z0", FAULT_Z0))

BY_GROUP = {g: sorted(n for n, c in CASES.items() if c["group"] == g) for g in ("ring", "skip", "batch", "plan", "fault")}
PARAM_NAMES = {1: ["W0", "b0", "Wo", "bo"]}
for _nl in (2, 3, 4):
    PARAM_NAMES[_nl] = ["W0", "b0", "W1", "b1", "Wo", "bo"]


def names_of(name):
    return PARAM_NAMES[SETS[CASES[name]["set"]][3]]


def is_planned(c):
    return not isinstance(c["out"], str)


def t_out(c):
    return np.array(c["out"], dtype=np.float64 if c["t64"] else np.float32)


def kind_of(c):
    return "cubic" if c["path"] == "cubic" else "linear"


def _make_paths(c, n, seed):
    C = SETS[c["set"]][0]
    if c["path"] == "rect":
        x = gu.data.make_rectilinear_coeffs(n, (c["T"] + 1) // 2, C - 1, missing=0.3, seed=seed)
        assert x.shape == (n, c["T"], C)
    elif c["path"] == "cubic":
        x = gu.data.make_cubic_coeffs(n, c["T"], C - 1, seed=seed)
    else:
        x = gu.data.make_linear_coeffs(n, c["T"], C - 1, seed=seed).copy()
        if c["knots"] is not None:
            x[:, :, 0] = np.asarray(c["knots"], np.float32)[None, :]
    return np.ascontiguousarray(x, dtype=np.float32)


def _field(c, t):
    import ncde_oracle as orc
    C, H, _, nl = SETS[c["set"]]
    return orc.Field([(t["W0"], t["b0"])] + [(t["W1"], t["b1"])] * (nl - 1) if nl > 1 else [(t["W0"], t["b0"])], t["Wo"], t["bo"], H, C)


def _field64(c, params):
    return _field(c, {k: torch.from_numpy(v).double() for k, v in params.items()})


def _field32(c, params):
    return _field(c, {k: torch.from_numpy(v) for k, v in params.items()})


def _control(c, coeffs, dtype):
    import ncde_oracle as orc
    kn = None if c["knots"] is None else np.asarray(c["knots"], np.float32)
    return orc.Control(torch.from_numpy(coeffs).to(dtype), kind_of(c), t=kn)


class Margins:
    """Observer of every inner-net evaluation of an oracle field: per layer the largest |pre-activation| and per sample the
    smallest one."""

    def __init__(self, field):
        self.mx, self.mn = {}, {}
        field.on_pre = self

    def __call__(self, li, pre):
        a = pre.detach().abs()
        self.mx[li] = max(self.mx.get(li, 0.0), float(a.max()))
        m = a.min(dim=1).values
        self.mn[li] = m if li not in self.mn else torch.minimum(self.mn[li], m)

    def per_sample(self, mx=None):
        """-> [B]: the smallest |pre-activation| of each sample relative to its layer's largest (`mx`: these maxima instead)."""
        mx = mx or self.mx
        return torch.stack([self.mn[li] / mx[li] for li in sorted(self.mn)]).min(dim=0).values.numpy()


def _walk(c, field, ctl, z0, gout):
    """The fp64 / fp32 oracle on one batch -> dict(z, stages, adjoint (dz0, grads), discrete (dz0, grads))."""
    import ncde_oracle as orc
    m = c["method"]
    if is_planned(c):
        t = torch.from_numpy(t_out(c))
        z = orc.solve_forward_times(ctl, field, z0, t, m, c["step"])
        if gout is None:
            gout = torch.zeros_like(z)
        adj = orc.solve_adjoint_times(ctl, field, t, z, gout, m, c["step"])
        disc = orc.solve_discrete_backward_times(ctl, field, z0, t, gout, m, c["step"])
        rec = orc.stage_record_times(ctl, field, z0, t, m, c["step"])
    else:
        seq = c["out"] == "knots"
        z = orc.solve_forward(ctl, field, z0, m, seq)
        if gout is None:
            gout = torch.zeros_like(z)
        adj = orc.solve_adjoint(ctl, field, z, gout, m, seq)
        disc = orc.solve_discrete_backward(ctl, field, z0, gout, m, seq)
        rec = orc.stage_record(ctl, field, z0, m)
    return {"z": z, "stages": rec, "adjoint": adj, "discrete": disc}


@functools.lru_cache(maxsize=None)
def arrays(name):
    """The case's inputs as fp32 arrays (built once; callers do not modify them): coeffs, z0, params, grad_out; for a range-fault
    case also clean_coeffs / clean_z0 (the batch without its outlier)."""
    c = CASES[name]
    C, H, HH, nl = SETS[c["set"]]
    if c["base"] is not None:
        b = arrays(c["base"])
        lo, hi = c["rows"]
        a = {"params": b["params"], "coeffs": np.ascontiguousarray(b["coeffs"][lo:hi]), "z0": np.ascontiguousarray(b["z0"][lo:hi]),
             "grad_out": np.ascontiguousarray(b["grad_out"][lo:hi] * np.float32(c["gout"] / CASES[c["base"]]["gout"]))}
        return a
    seed, B = c["seed"], c["B"]
    p = dict(gu.data.make_field_weights(H, HH, C, seed=seed))
    if nl == 1:
        p = {k: v for k, v in p.items() if k not in ("W1", "b1")}
    for pool in POOL:      # keep the first B candidates that pass (ii) against the pool-wide layer maxima
        n = pool * B
        coeffs = _make_paths(c, n, seed + 1)
        z0 = (gu.data.normal(seed + 2, n * H, stream=2).reshape(n, H) * 0.5).astype(np.float32)
        field = _field64(c, p)
        mg = Margins(field)
        _walk(c, field, _control(c, coeffs, torch.float64), torch.from_numpy(z0).double(), None)
        keep = np.nonzero(mg.per_sample() >= RELU_MARGIN)[0][:B]
        if len(keep) == B:
            break
    assert len(keep) == B, (name, len(keep))
    coeffs, z0 = np.ascontiguousarray(coeffs[keep]), np.ascontiguousarray(z0[keep])
    a = {"params": p}
    if c["bump"] is not None:
        s, piece, ch, delta = c["bump"]
        d = coeffs[:, 1:, 1:] - coeffs[:, :-1, 1:]
        narrow = [q for q in range(d.shape[1]) if not np.any(d[:, q])]
        assert narrow, name
        piece = narrow[0] if piece is None else piece
        coeffs[s, piece + 1:, ch] += np.float32(delta)
        a["bump_piece"] = piece
    if c["outlier"] is not None:
        s, what, mag = c["outlier"]
        a["clean_coeffs"], a["clean_z0"] = coeffs.copy(), z0.copy()
        if what == "z0":
            # a state of size `mag` along -W0^-1 1: every unit of layer 0 is switched off (W0 z + b0 = b0 - k with k in the thousands), so
            # the layers behind it see zeros and the head stays unsaturated -- z leaves the fp16 range as an operand of the layer-0
            # GEMM, and the sample keeps an ordinary share of dW1, db1, dWo, dbo (a state of that size along a random direction
            # saturates every row of the head, and its share of every gradient is exactly 0)
            v = -np.linalg.solve(p["W0"].astype(np.float64), np.ones(HH))
            z0[s] = (v * (mag / np.abs(v).max())).astype(np.float32)
        else:
            coeffs[s, 2:, min(5, C - 1)] += np.float32(mag)      # a value channel moves by `mag` on piece 1 and stays there
    n_out = len(c["out"]) if is_planned(c) else (c["T"] if c["out"] == "knots" else 2)
    a["coeffs"], a["z0"] = coeffs, z0
    a["grad_out"] = (gu.data.normal(seed + 3, B * n_out * H, stream=1).reshape(B, n_out, H) * (c["gout"] / 2.0)).astype(np.float32)
    if c["outlier"] is not None and c["outlier"][1] == "dx":
        # The late outlier carries no cotangent: next to states of 1e5 the head's 1 - tanh^2 of its few unsaturated rows is decided
        # by fp32 round-off, and the fp32 oracle misses condition (i) on the parameter gradients.  Its tile is faulted and re-executed
        # all the same, and the partial of the tile's other fifteen samples must be counted exactly once.
        a["grad_out"][c["outlier"][0]] = 0.0
    return a


def _as_np(w, names):
    dz0, gp = w
    return {"dz0": dz0.numpy(), "grads": {n: g.numpy() for n, g in zip(names, gp)}}


@functools.lru_cache(maxsize=None)
def expect(name, clean=False):
    """The fp64 oracle on the case -> dict(z_out, stages, adjoint {dz0, grads}, discrete {dz0, grads}, margin [B], layer_max);
    clean: on the batch without its outlier (range-fault cases)."""
    c, a = CASES[name], arrays(name)
    coeffs, z0 = (a["clean_coeffs"], a["clean_z0"]) if clean else (a["coeffs"], a["z0"])
    field = _field64(c, a["params"])
    mg = Margins(field)
    w = _walk(c, field, _control(c, coeffs, torch.float64), torch.from_numpy(z0).double(), torch.from_numpy(a["grad_out"]).double())
    names = names_of(name)
    return {"z_out": w["z"].numpy(), "stages": w["stages"].numpy(), "adjoint": _as_np(w["adjoint"], names),
            "discrete": _as_np(w["discrete"], names), "margin": mg.per_sample(), "layer_max": dict(mg.mx)}


def outlier_margin(name):
    """(ii) for the outlier sample of a range-fault case on its own: the smallest |pre-activation| of each of its evaluations
    relative to the largest one of the SAME evaluation and layer (its state grows from 1 to 1e5 along the solve, so neither the
    batch's layer maximum nor its own says anything about its early stages)."""
    c, a = CASES[name], arrays(name)
    s = c["outlier"][0]
    field = _field64(c, a["params"])
    worst = [1.0]

    def obs(li, pre):
        worst[0] = min(worst[0], float(pre.abs().min() / pre.abs().max()))
    field.on_pre = obs
    _walk(c, field, _control(c, a["coeffs"][s:s + 1], torch.float64), torch.from_numpy(a["z0"][s:s + 1]).double(), None)
    return worst[0]


def outlier_share(name):
    """The outlier sample's own part of every parameter gradient (the fp64 oracle on that sample alone), relative to the batch's
    maximum of that tensor -> {pass: {name: share}}."""
    c, a, ex = CASES[name], arrays(name), expect(name)
    s = c["outlier"][0]
    w = _walk(c, _field64(c, a["params"]), _control(c, a["coeffs"][s:s + 1], torch.float64), torch.from_numpy(a["z0"][s:s + 1]).double(),
              torch.from_numpy(a["grad_out"][s:s + 1]).double())
    return {ps: {n: float(g.abs().max()) / float(np.abs(ex[ps]["grads"][n]).max()) for n, g in zip(names_of(name), w[ps][1])}
            for ps in ("adjoint", "discrete")}


POISON = 1.0e30


def poisoned(name):
    """The coefficients of a plan (c) / (f) case with the pieces its solve never reads overwritten: knots 0 and T - 1 of a linear path,
    the rows of pieces 0 and T - 2 of a cubic one."""
    x = arrays(name)["coeffs"].copy()
    x[:, 0], x[:, -1] = POISON, -POISON
    return x


@functools.lru_cache(maxsize=None)
def oracle32(name):
    """The fp32 oracle on the case: end to end (its own z) and, as the isolated backward kernels are run, on the fp64 z_out / stage
    record rounded to fp32 (the continuous adjoint only: the discrete backward of the oracle recomputes its stages)."""
    c, a = CASES[name], arrays(name)
    field = _field32(c, a["params"])
    ctl = _control(c, a["coeffs"], torch.float32)
    gout = torch.from_numpy(a["grad_out"])
    w = _walk(c, field, ctl, torch.from_numpy(a["z0"]), gout)
    names = names_of(name)
    res = {"z_out": w["z"].numpy(), "adjoint": _as_np(w["adjoint"], names), "discrete": _as_np(w["discrete"], names)}
    import ncde_oracle as orc
    z64 = torch.from_numpy(expect(name)["z_out"].astype(np.float32))
    if is_planned(c):
        iso = orc.solve_adjoint_times(ctl, field, torch.from_numpy(t_out(c)), z64, gout, c["method"], c["step"])
    else:
        iso = orc.solve_adjoint(ctl, field, z64, gout, c["method"], c["out"] == "knots")
    res["adjoint_iso"] = _as_np(iso, names)
    return res


def errors(res, ref, names, z=None):
    """relerr of dz0 and every gradient of `res` against `ref` (both {dz0, grads}); z = (got, want) adds the solution."""
    errs = {} if z is None else {"z": gu.relerr(z[0], z[1])}
    errs["dz0"] = gu.relerr(res["dz0"], ref["dz0"])
    for n in names:
        assert res["grads"][n].shape == ref["grads"][n].shape, n
        errs["d" + n] = gu.relerr(res["grads"][n], ref["grads"][n])
    return errs


def check(label, errs, bound_g):
    """Prints the errors (pytest -s shows them), asserts z <= TIGHT_Z and every gradient <= bound_g."""
    print(label, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert errs.get("z", 0.0) <= TIGHT_Z, (label, errs)
    assert all(v <= bound_g for k, v in errs.items() if k != "z"), (label, errs)
    return errs


def golden_case(name, coeffs=None, z0=None):
    """The case in the layout gpu_util / cpu_lib_util take (default axis)."""
    c, a = CASES[name], arrays(name)
    C, H, HH, nl = SETS[c["set"]]
    return {"meta": {"kind": kind_of(c), "method": c["method"], "sequence": c["out"] == "knots", "param_names": names_of(name),
                     "field_kind": "original", "field_mode": "matmul", "dims": {"C": C, "H": H, "HH": HH, "nl": nl}, "field": "original"},
            "coeffs": a["coeffs"] if coeffs is None else coeffs, "z0": a["z0"] if z0 is None else z0, "params": a["params"],
            "layers": [("W0", "b0")] + [("W1", "b1")] * (nl - 1), "H": H, "C": C, "expect": {"grad_out": a["grad_out"]}}


def times_case(name, coeffs=None):
    """The case in the layout gpu_util.run_times_case takes (general time axis) -> (f, meta)."""
    c, a = CASES[name], arrays(name)
    f = {"coeffs": a["coeffs"] if coeffs is None else coeffs, "z0": a["z0"], "t_out": t_out(c), "grad_out": a["grad_out"]}
    if c["knots"] is not None:
        f["knots"] = np.asarray(c["knots"], np.float32)
    return f, {"kind": kind_of(c), "method": c["method"], "step_size": c["step"], "dims": {"nl": SETS[c["set"]][3]}}


def control_of(name, device):
    import ncde_amd
    c, a = CASES[name], arrays(name)
    cc = torch.from_numpy(a["coeffs"]).to(device)
    kn = None if c["knots"] is None else torch.tensor(c["knots"], dtype=torch.float32, device=device)
    return (ncde_amd.NaturalCubicSpline if c["path"] == "cubic" else ncde_amd.LinearInterpolation)(cc, t=kn), cc


def kernel_names(name, flags=0, device="cpu"):
    """(forward, adjoint, discrete backward) names the library dispatches the case to: a host-side query, no GPU needed.  -> also
    the time plan's host words (None on the default axis)."""
    import gpu_util
    from ncde_amd import _lib, solver
    c, a = CASES[name], arrays(name)
    nl = SETS[c["set"]][3]
    X, cc = control_of(name, device)
    func = gpu_util.CaseField(a["params"], [("W0", "b0")] + [("W1", "b1")] * (nl - 1), device)
    plan, output = None, (_lib.OUT_KNOTS if c["out"] == "knots" else _lib.OUT_INTERVAL)
    if is_planned(c):
        plan = solver._time_plan(X, torch.from_numpy(t_out(c)), c["method"], c["step"], torch.device(device))
        output = _lib.OUT_TIMES
    p = solver.build_problem(cc, kind_of(c), torch.from_numpy(a["z0"]).to(device), func.fused_spec(), c["method"], output, flags, plan)
    got = tuple((_lib.lib().ncde_kernel_name(ctypes.byref(p), k) or b"?").decode() for k in (0, 1, 2))
    return got, (None if plan is None else plan[0].cpu().numpy())


def name_matches(got, want):
    parts = want.split("+")
    return got.startswith(parts[0]) and all(q in got for q in parts[1:])


def want_names(name):
    c = CASES[name]
    if c["set"] == "R20nl4" and c["path"] == "cubic":      # ncde_fast_nl.h: the four-layer adjoint's LDS plan on the cubic path is 224
        return (NAMES["R20nl4"][0], "ncde_adj_tiled", "ncde_adj_tiled")      # bytes over 160 KB -> the batch-tiled family
    return (PLAN_NAMES if is_planned(c) else NAMES)[c["set"]]
