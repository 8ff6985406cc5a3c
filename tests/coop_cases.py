"""Seeded cases for the XCD-cooperative kernels (csrc/ncde_coop.h, ncde_dwo2.hip, the CoopPlan code of csrc/ncde_tiled.hip:
ncde_fwd_tiled<.., COOP>, the cooperative ncde_adj_tiled, ncde_dwo_h2 and the chunked launches around them) at the edges of their
bookkeeping: every group size M = 4 .. 28 below cfg5's 32 at the smallest batch that forms one group, with H = 16 .. 128 and one to
three layers; several groups in one launch and sample independence across batch sizes; a launch of 4 tiles behind one of 256 at the
smallest width (pass-B workgroups without a pair); and the power-of-two scales -- per sample, per tile, per time window, per weight
tensor -- on inputs whose magnitudes differ by many binades, checked per row.  Shared by tests/test_coop_edges_cpu.py (validates
every case, and the plan restated below, without a GPU) and tests/test_coop_edges_gpu.py (the kernels against the fp64 expectations).
Helper only: no test functions.

Reference, screening and bounds are those of tests/resident_cases.py (its docstring: conditions (i) - (iii), the sample pool), as in
tests/tiled_cases.py.  The cap on left-out rows and cases is zero.  Where a check is per row (the scale group, the chunk tail),
condition (i) is applied per row too: PER_ROW_G below.
"""
import ctypes
import functools

import numpy as np
import torch

import golden_util as gu
import resident_cases as rc
from resident_cases import E2E_G, MIN_GRAD, POOL, RELU_MARGIN, STAGES, TIGHT_G, TIGHT_Z, Margins, check, errors, kind_of      # noqa: F401

HH = 128                  # the cooperative kernels' last hidden width (every hidden width here)
NO_COOP = 0x400           # NCDE_FLAG_NO_COOP
CUS = 256                 # tiled_device_cus() without a device, and on the MI355X
COOP_RPM = 20             # row tiles of Wo a group member keeps
LDS_LIMIT = 160 * 1024
# The per-row bound of dL/dz0 (each row relative to ITS OWN maximum).  It is TIGHT_G on the condition that the fp32 oracle, fed the
# fp64 z rounded to fp32, stays within TIGHT_G / 2 of fp64 on every row of every per-row case: tests/test_coop_edges_cpu.py asserts
# that (measured worst row of the fp32 oracle over the table: 4.2e-6, the discrete backward at Wo x 2^4; 1.0e-6 elsewhere).
PER_ROW_G = TIGHT_G

# set -> (C, H, layers); M = (H / 4) (C / 4) / 20
SETS = {"M4s": (80, 16, 1), "M4a": (20, 64, 2), "M4b": (40, 32, 2), "M12a": (80, 48, 2), "M12b": (40, 96, 3), "M16": (40, 128, 2),
        "M20": (80, 80, 2), "M24": (80, 96, 1), "M28": (80, 112, 2)}
GROUP_SIZE = {"M4s": 4, "M4a": 4, "M4b": 4, "M12a": 12, "M12b": 12, "M16": 16, "M20": 20, "M24": 24, "M28": 28}

CASES = {}
_LINEAR, _CUBIC = ("linear", "rk4"), ("cubic", "midpoint")


def _case(name, kset, B, T, pm, out, seed, group, gout=8.0, base=None, rows=None, var=None):
    """pm: (path, method).  out: "interval" / "knots".  base / rows: the samples `rows` of case `base`.  var: how the case departs
    from plain seeded inputs (the scale group; `_vary`, `_vary_gout`, `_zeros`)."""
    assert name not in CASES and kset in SETS
    CASES[name] = dict(name=name, set=kset, B=B, T=T, path=pm[0], method=pm[1], out=out, seed=seed, group=group, gout=gout, base=base,
                       rows=rows, var=var, step=1.0, knots=None, t64=False, outlier=None, bump=None)


# ---- 3. the chunk tail at the smallest width: 260 tiles = a launch of 256 (64 groups) + one of 4 (1 group; parts = 32 was sized for
# the first: n_pair = 2, thirty pass-B workgroups without a pair).  Its last 64 samples ARE the second launch: the B = 64 case of group 1.
_case("tail_M4_B4160", "M4s", 4160, 2, _LINEAR, "interval", 5002, "tail")
# ---- 2. several groups in one launch; their row subsets are cases of their own ---------------------------------------------------------------
_case("groups_M4_B384", "M4s", 384, 3, _CUBIC, "knots", 5010, "groups")      # G = 6, parts = 8: the XCD-mapped branch of ncde_dwo_h2, nrg = 5
_case("groups_M4_B64", "M4s", 64, 3, _CUBIC, "knots", None, "groups", base="groups_M4_B384", rows=(128, 192))
_case("groups_M12_B384", "M12a", 384, 3, _LINEAR, "knots", 5020, "groups")   # G = 2, parts = 8, n_pair = 12: my_n = 2, 2, 2, 2, 1, 1, 1, 1
# ---- 1. group sizes: one group each, B = 16 M (ragged by one sample where B is odd) -------------------------------------------------------------
_case("size_M4_C80_H16", "M4s", 64, 2, _LINEAR, "interval", None, "size", base="tail_M4_B4160", rows=(4096, 4160))      # the smallest cooperative problem
_case("size_M4_C20_H64", "M4a", 64, 3, _CUBIC, "knots", 5030, "size")
_case("size_M4_C40_H32", "M4b", 64, 4, _LINEAR, "interval", 5040, "size")
_case("size_M12_C80_H48", "M12a", 192, 3, _LINEAR, "knots", None, "size", base="groups_M12_B384", rows=(192, 384))      # parts = 4, n_pair = 6: my_n = 2, 2, 1, 1
_case("size_M12_C40_H96", "M12b", 191, 3, _CUBIC, "knots", 5050, "size")
_case("size_M16_C40_H128", "M16", 256, 2, _LINEAR, "interval", 5060, "size")
_case("size_M20_C80_H80", "M20", 320, 3, _CUBIC, "knots", 5070, "size")       # parts = 8, n_pair = 10
_case("size_M24_C80_H96", "M24", 384, 3, _LINEAR, "knots", 5080, "size")
_case("size_M28_C80_H112", "M28", 447, 2, _CUBIC, "interval", 5090, "size")
WINDOWED = ("size_M12_C80_H48", "size_M20_C80_H80")      # also under NCDE_FLAG_TILED_WINDOW_STEPS(1): two windows

# ---- 4. scales, on the M = 4 (C 20, H 64) and the M = 12 (C 80, H 48) shape, B = 16 M, three output times --------------------------------------
GOUT_ROWS = (-30, -17, -5, 0, 9, 20)      # sample s: grad_out x 2^GOUT_ROWS[s % 6]
GOUT_TIMES = {"up": (-20, 0, 12),         # output time i: grad_out x 2^e[i].  "up" (the issue's order): the cotangent of the LAST time leads, every window's sigma is 2^12's
              "down": (0, 12, -20)}       # "down": the first reverse window sees 2^-20 only, the second 2^12: sigma differs by 32 binades
# candidate n of a state / path case: z0 x 2^ez[n % len(ez)], its data channels x 2^ex[n % len(ex)]; kept in equal numbers per z0
# exponent (_pick).  The spreads are the widest tried that leave enough of the 64 B candidates of EVERY z0 exponent passing (ii): the
# margin is relative to the layer's largest pre-activation, which the scaled-up samples set.  Tried and short of candidates: M4a
# (-2 .. 2) x (-4 .. 2): 27 of 64; M12a (-1, 0, 1) x (-3 .. 0): 115 of 192, (-1, 0, 1) x (-4 .. -1): 168 of 192.
SPREAD = {"M4a": ((-1, 0, 1), (-2, 0, -1, 1)), "M12a": ((-1, 0), (-3, -1, -2))}
WO_DOWN = -8
# (Wo, bo) x 2^WO_UP: the largest power of two that passes the screening.  What ends it is not (iii) -- the gradients GROW with the
# weights, the solution turns chaotic before tanh saturates -- but (i) per row: at 2^5 the fp32 oracle's discrete dL/dz0 is 1.7e-5 off
# fp64 on its worst row (2^6: 7.3e-5, 2^8: 3.6e-3).  On the M = 12 shape (79 data channels) already 2^1 leaves 25 of 12288 candidates
# passing (ii) (seeds 5112, 5300, 5301: 28, 25, 12): no scaled-up case there.
WO_UP = {"M4a": 4}
ZERO_GOUT, CONST_PATH = 5, 21             # the sample without a cotangent, the sample whose path does not move
SCALE_BASE = {"M4a": "size_M4_C20_H64", "M12a": "size_M12_C80_H48"}
for _i, (_set, _b) in enumerate(sorted(SCALE_BASE.items())):
    _B, _T, _pm = CASES[_b]["B"], CASES[_b]["T"], (CASES[_b]["path"], CASES[_b]["method"])
    _case("scale_%s_gout_rows" % _set, _set, _B, _T, _pm, "knots", None, "scale", base=_b, rows=(0, _B), var=("gout_rows",))
    for _k in sorted(GOUT_TIMES):
        _case("scale_%s_gout_times_%s" % (_set, _k), _set, _B, _T, _pm, "knots", None, "scale", base=_b, rows=(0, _B), var=("gout_times", _k))
    _case("scale_%s_zeros" % _set, _set, _B, _T, _pm, "knots", None, "scale", base=_b, rows=(0, _B), var=("zeros",))
    _case("scale_%s_state_path" % _set, _set, _B, _T, _pm, "knots", 5100 + 10 * _i, "scale", var=("state_path",))
    _case("scale_%s_wo_down" % _set, _set, _B, _T, _pm, "knots", 5101 + 10 * _i, "scale", var=("weights", WO_DOWN), gout=64.0)      # (iii): the hidden layers' gradients carry the 2^-8
    if _set in WO_UP:
        _case("scale_%s_wo_up" % _set, _set, _B, _T, _pm, "knots", 5102 + 10 * _i, "scale", var=("weights", WO_UP[_set]))

# What each case is in the table for: name -> (M, parts, XCD-mapped branch of ncde_dwo_h2 (parts & 7 == 0)?, per launch (G, n_pair, my_n)).
# tests/test_coop_edges_cpu.py holds the restated plan (coop_plan) and the library's own queries to it.
FACTS = {"size_M4_C80_H16": (4, 2, False, [(1, 2, [1, 1])]),
         "size_M4_C20_H64": (4, 2, False, [(1, 2, [1, 1])]),
         "size_M4_C40_H32": (4, 2, False, [(1, 2, [1, 1])]),
         "size_M12_C80_H48": (12, 4, False, [(1, 6, [2, 2, 1, 1])]),                       # uneven my_n
         "size_M12_C40_H96": (12, 4, False, [(1, 6, [2, 2, 1, 1])]),
         "size_M16_C40_H128": (16, 8, True, [(1, 8, [1] * 8)]),
         "size_M20_C80_H80": (20, 8, True, [(1, 10, [2, 2, 1, 1, 1, 1, 1, 1])]),            # uneven my_n on the XCD-mapped branch
         "size_M24_C80_H96": (24, 8, True, [(1, 12, [2, 2, 2, 2, 1, 1, 1, 1])]),
         "size_M28_C80_H112": (28, 8, True, [(1, 14, [2, 2, 2, 2, 2, 2, 1, 1])]),
         "groups_M4_B384": (4, 8, True, [(6, 12, [2, 2, 2, 2, 1, 1, 1, 1])]),               # nrg = 5
         "groups_M4_B64": (4, 2, False, [(1, 2, [1, 1])]),
         "groups_M12_B384": (12, 8, True, [(2, 12, [2, 2, 2, 2, 1, 1, 1, 1])]),
         "tail_M4_B4160": (4, 32, True, [(64, 128, [4] * 32), (1, 2, [1, 1] + [0] * 30)])}  # the second launch: thirty idle workgroups
for _n, _c in list(CASES.items()):
    if _c["group"] == "scale":
        FACTS[_n] = FACTS[SCALE_BASE[_c["set"]]]

BY_GROUP = {g: sorted(n for n, c in CASES.items() if c["group"] == g) for g in ("size", "groups", "tail", "scale")}
PER_ROW = BY_GROUP["scale"] + BY_GROUP["tail"]


def dims_of(name):
    return SETS[CASES[name]["set"]]


def layers_of(name):
    return [("W0", "b0")] + [("W1", "b1")] * (dims_of(name)[2] - 1)


def names_of(name):
    return rc.PARAM_NAMES[dims_of(name)[2]]


def n_out_of(name):
    c = CASES[name]
    return c["T"] if c["out"] == "knots" else 2


# ---- the plan, restated (tiled_coop_plan, the `parts` rule of tiled_adj_plan, tiled_adj_run's chunks, ncde_dwo_h2's my_n) ---------------------
def coop_plan(C, H, nl, B, hh=HH, cus=CUS):
    """-> None where the problem is not cooperative, else dict(M, n_tiles, chunk, parts, nrg, xcd_mapped, launches): launches is one
    dict(tiles, G, n_pair, my_n) per chunk of the batch, my_n[by] the sample-tile pairs by, by + parts, ... pass-B workgroup `by` of a
    row group walks in every stage."""
    ncq = C // 4
    if hh != HH or H > 128 or H % 16 or C % 4 or ncq not in (5, 10, 20) or nl < 1:
        return None
    row_tiles = (H // 4) * ncq
    if row_tiles % COOP_RPM:
        return None
    M, n_tiles = row_tiles // COOP_RPM, (B + 15) // 16
    if M < 4 or M % 4 or n_tiles % M or M > cus:
        return None
    coop_lds = 2 * 10 * 2 * 64 * 4 + 2 * 8 * 64 * 4 + 2 * 80 * 16 + 2 * 256 + 2 * 64 + 2 * 4 * 64 + 2 * 16 + 8
    if 4 * (4 * H * 16 + (nl + 2) * hh * 16 + C * 16 + coop_lds) + 128 * 16 * 6 > LDS_LIMIT:
        return None
    chunk = min(n_tiles, cus // M * M)
    parts = 1
    while parts * 2 <= 32 and parts * 2 <= chunk // 2:
        parts *= 2
    launches = []
    for t0 in range(0, n_tiles, chunk):
        tiles = min(chunk, n_tiles - t0)
        n_pair = tiles >> 1
        my_n = [(n_pair - by + parts - 1) // parts if by < n_pair else 0 for by in range(parts)]
        launches.append({"tiles": tiles, "G": tiles // M, "n_pair": n_pair, "my_n": my_n})
    return {"M": M, "n_tiles": n_tiles, "chunk": chunk, "parts": parts, "nrg": H * C // 16 // 16, "xcd_mapped": parts & 7 == 0,
            "launches": launches}


def plan_of(name):
    C, H, nl = dims_of(name)
    return coop_plan(C, H, nl, CASES[name]["B"])


def pairs_walked(launch, parts):
    """The (workgroup, pair) visits of one stage of a launch, from my_n alone: every pair of the launch must come up exactly once."""
    return sorted(by + parts * k for by, n in enumerate(launch["my_n"]) for k in range(n))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def _weights(name, seed):
    C, H, nl = dims_of(name)
    p = dict(gu.data.make_field_weights(H, HH, C, seed=seed))
    return {k: v for k, v in p.items() if nl > 1 or k not in ("W1", "b1")}


def _make_paths(c, n, seed):
    C = SETS[c["set"]][0]
    make = gu.data.make_cubic_coeffs if c["path"] == "cubic" else gu.data.make_linear_coeffs
    return np.ascontiguousarray(make(n, c["T"], C - 1, seed=seed), dtype=np.float32).copy()


def _data_channels(c, coeffs):
    """A view of the data channels of every coefficient of the path (channel 0 is time): [n, ., (4,) C - 1]."""
    C = SETS[c["set"]][0]
    if c["path"] == "cubic":
        assert coeffs.shape[2] == 4 * C
        return coeffs.reshape(coeffs.shape[0], coeffs.shape[1], 4, C)[..., 1:]
    return coeffs[..., 1:]


def _vary(c, p, coeffs, z0):
    """The scale-group departures that change the solution, applied to the candidate samples BEFORE screening (ii): powers of two on
    z0 and on the data channels per candidate, or on (Wo, bo).  -> the exponents per candidate (z0, path) or None."""
    if c["var"] is None or c["var"][0] not in ("state_path", "weights"):
        return None
    if c["var"][0] == "weights":
        p["Wo"], p["bo"] = p["Wo"] * np.float32(2.0 ** c["var"][1]), p["bo"] * np.float32(2.0 ** c["var"][1])
        return None
    n = np.arange(len(z0))
    ez, ex = (np.asarray(e)[n % len(e)] for e in SPREAD[c["set"]])
    z0 *= (2.0 ** ez).astype(np.float32)[:, None]
    d = _data_channels(c, coeffs)
    d *= (2.0 ** ex).astype(np.float32).reshape((-1,) + (1,) * (d.ndim - 1))
    return np.stack([ez, ex], axis=1)


def _pick(ok, exps, B):
    """The first B passing candidates; of a state / path case the first B / n of each of the n z0 exponents (the margin is relative to
    the layer's largest pre-activation, so the scaled-up candidates pass far more often: the first B would be those alone)."""
    if exps is None:
        return ok[:B]
    classes = np.unique(exps[:, 0])
    quota = [B // len(classes) + (i < B % len(classes)) for i in range(len(classes))]
    return np.sort(np.concatenate([ok[exps[ok, 0] == e][:q] for e, q in zip(classes, quota)]))


def field_of(name, params, dtype):
    import ncde_oracle as orc
    C, H, _ = dims_of(name)
    t = {k: torch.from_numpy(v).to(dtype) for k, v in params.items()}
    return orc.Field([(t[w], t[b]) for w, b in layers_of(name)], t["Wo"], t["bo"], H, C)


@functools.lru_cache(maxsize=None)
def arrays(name):
    """The case's inputs as fp32 arrays (built once; callers do not modify them): coeffs, z0, params, grad_out; exps [B, 2] for the
    state / path scale cases."""
    c = CASES[name]
    C, H, _ = dims_of(name)
    if c["base"] is not None:
        b = arrays(c["base"])
        lo, hi = c["rows"]
        a = {"params": b["params"], "coeffs": np.ascontiguousarray(b["coeffs"][lo:hi]), "z0": np.ascontiguousarray(b["z0"][lo:hi]),
             "grad_out": np.ascontiguousarray(b["grad_out"][lo:hi])}
        if c["var"] is not None:
            a["grad_out"], a["coeffs"] = a["grad_out"].copy(), a["coeffs"].copy()
            if c["var"][0] == "gout_rows":
                k = np.asarray(GOUT_ROWS)[np.arange(c["B"]) % len(GOUT_ROWS)]
                a["grad_out"] *= (2.0 ** k).astype(np.float32)[:, None, None]
                a["exps"] = k
            elif c["var"][0] == "gout_times":
                a["grad_out"] *= (2.0 ** np.asarray(GOUT_TIMES[c["var"][1]])).astype(np.float32)[None, :, None]
            else:
                assert c["var"][0] == "zeros"
                a["grad_out"][ZERO_GOUT] = 0.0
                if c["path"] == "cubic":      # every piece: the value at knot 0, no slope, no curvature (time channel included)
                    a["coeffs"][CONST_PATH, :, :C] = a["coeffs"][CONST_PATH, :1, :C]
                    a["coeffs"][CONST_PATH, :, C:] = 0.0
                else:
                    a["coeffs"][CONST_PATH, 1:] = a["coeffs"][CONST_PATH, :1]
        return a
    seed, B = c["seed"], c["B"]
    p = _weights(name, seed)
    for pool in POOL:      # keep the first B candidates that pass (ii) against the pool-wide layer maxima
        n = pool * B
        coeffs = _make_paths(c, n, seed + 1)
        z0 = (gu.data.normal(seed + 2, n * H, stream=2).reshape(n, H) * 0.5).astype(np.float32)
        p = _weights(name, seed)
        exps = _vary(c, p, coeffs, z0)
        field = field_of(name, p, torch.float64)
        mg = Margins(field)
        rc._walk(c, field, rc._control(c, coeffs, torch.float64), torch.from_numpy(z0).double(), None)
        keep = _pick(np.nonzero(mg.per_sample() >= RELU_MARGIN)[0], exps, B)
        if len(keep) == B:
            break
    assert len(keep) == B, (name, len(keep))
    a = {"params": p, "coeffs": np.ascontiguousarray(coeffs[keep]), "z0": np.ascontiguousarray(z0[keep])}
    if exps is not None:
        a["exps"] = exps[keep]
    n_out = n_out_of(name)
    a["grad_out"] = (gu.data.normal(seed + 3, B * n_out * H, stream=1).reshape(B, n_out, H) * (c["gout"] / 2.0)).astype(np.float32)
    return a


def walk(name, dtype, a=None):
    """The oracle in `dtype` on the case -> resident_cases._walk's dict."""
    c, a = CASES[name], a or arrays(name)
    return rc._walk(c, field_of(name, a["params"], dtype), rc._control(c, a["coeffs"], dtype), torch.from_numpy(a["z0"]).to(dtype),
                    torch.from_numpy(a["grad_out"]).to(dtype))


@functools.lru_cache(maxsize=None)
def expect(name):
    """The fp64 oracle on the case -> dict(z_out, stages, adjoint {dz0, grads}, discrete {dz0, grads}, margin [B], layer_max)."""
    c, a = CASES[name], arrays(name)
    field = field_of(name, a["params"], torch.float64)
    mg = Margins(field)
    w = rc._walk(c, field, rc._control(c, a["coeffs"], torch.float64), torch.from_numpy(a["z0"]).double(), torch.from_numpy(a["grad_out"]).double())
    names = names_of(name)
    return {"z_out": w["z"].numpy(), "stages": w["stages"].numpy(), "adjoint": rc._as_np(w["adjoint"], names),
            "discrete": rc._as_np(w["discrete"], names), "margin": mg.per_sample(), "layer_max": dict(mg.mx)}


@functools.lru_cache(maxsize=None)
def oracle32(name):
    """The fp32 oracle on the case: end to end (its own z) and the continuous adjoint on the fp64 z_out rounded to fp32."""
    import ncde_oracle as orc
    c, a, names = CASES[name], arrays(name), names_of(name)
    w = walk(name, torch.float32)
    res = {"z_out": w["z"].numpy(), "adjoint": rc._as_np(w["adjoint"], names), "discrete": rc._as_np(w["discrete"], names)}
    z64 = torch.from_numpy(expect(name)["z_out"].astype(np.float32))
    iso = orc.solve_adjoint(rc._control(c, a["coeffs"], torch.float32), field_of(name, a["params"], torch.float32), z64,
                            torch.from_numpy(a["grad_out"]), c["method"], c["out"] == "knots")
    res["adjoint_iso"] = rc._as_np(iso, names)
    return res


def row_err(got, want):
    """The largest distance of a row of `got` from that row of `want`, relative to the row's OWN maximum in `want`; a row that is
    all zero in `want` must be all zero in `got`."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    mx = np.abs(want).max(axis=1)
    d = np.abs(got - want).max(axis=1)
    assert not np.any(d[mx == 0.0]), "a row that is exactly zero in the reference is not"
    return float((d[mx > 0] / mx[mx > 0]).max())


def rows_off(got, want, bound=TIGHT_G):
    """(rows of `got` further than `bound` from `want`, the largest row distance), relative to max |want|: the measure of
    test_cooperative_kernels_on_more_sample_tiles_than_cus."""
    per = np.abs(np.asarray(got, np.float64) - want).max(axis=1) / np.abs(want).max()
    return int((per > bound).sum()), float(per.max())


def golden_case(name):
    """The case in the layout gpu_util takes."""
    c, a = CASES[name], arrays(name)
    C, H, nl = dims_of(name)
    return {"meta": {"kind": kind_of(c), "method": c["method"], "sequence": c["out"] == "knots", "param_names": names_of(name),
                     "field_kind": "original", "field_mode": "matmul", "dims": {"C": C, "H": H, "HH": HH, "nl": nl}, "field": "original"},
            "coeffs": a["coeffs"], "z0": a["z0"], "params": a["params"], "layers": layers_of(name), "H": H, "C": C,
            "expect": {"grad_out": a["grad_out"]}}


def problem_of(name, flags=0, device="cpu"):
    """-> (NcdeProblem of the case under `flags`, the tensors it points into)."""
    import gpu_util
    return gpu_util.case_problem(golden_case(name), flags, device)[::2]


def kernel_names(name, flags=0, device="cpu"):
    """(forward, adjoint, discrete backward) names the library dispatches the case to: a host-side query, no GPU needed."""
    from ncde_amd import _lib
    p, _keep = problem_of(name, flags, device)
    return tuple((_lib.lib().ncde_kernel_name(ctypes.byref(p), k) or b"?").decode() for k in (0, 1, 2))


def status_window(name, pass_, flags=0):
    """-> (ncde_coop_status_offset, ncde_workspace_bytes) of the case's pass."""
    from ncde_amd import _lib
    p, _keep = problem_of(name, flags)
    return int(_lib.lib().ncde_coop_status_offset(ctypes.byref(p), pass_)), int(_lib.lib().ncde_workspace_bytes(ctypes.byref(p), pass_))


def bare_problem(C, H, nl, B, T=3, flags=0):
    """A structurally valid problem of this suite's kind (linear path, rk4, interval output, hidden widths HH) with dummy, never
    dereferenced pointers: for the host-side queries on shapes outside the table."""
    from ncde_amd import _lib
    p = _lib.NcdeProblem()
    p.abi_version = _lib.NCDE_ABI_VERSION
    p.batch, p.n_knots, p.channels, p.hidden = B, T, C, H
    p.interp, p.method, p.output, p.flags = 0, 2, 0, flags
    p.n_layers = nl
    for l in range(nl):
        p.layer_in[l], p.layer_out[l] = (H if l == 0 else HH), HH
        p.layer_W[l], p.layer_b[l] = (0x1000, 0x1100) if l == 0 else (0x2000, 0x2100)
    p.Wo, p.bo, p.coeffs, p.z0 = 0x3000, 0x3100, 0x4000, 0x5000
    p.coeffs_stride_b, p.coeffs_stride_t = T * C, C
    return p


def bare_names(p):
    from ncde_amd import _lib
    return tuple((_lib.lib().ncde_kernel_name(ctypes.byref(p), k) or b"?").decode() for k in (0, 1, 2))
