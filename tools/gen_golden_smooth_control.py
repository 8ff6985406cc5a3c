"""Golden vectors for the control-path gradients of cubic-smoothed paths (tests/golden/g17_*.npz + MANIFEST_smooth_control.json),
produced by IMPORTING the reference on the build machine -- the same way oracle/gen_golden.py does, whose import shims and helpers
are reused (cf. tools/gen_golden_control.py, tools/gen_golden_smooth.py).

    python tools/gen_golden_smooth_control.py

Every case is the reference's cdeint(SmoothLinearInterpolation(x.requires_grad_(), gradient_matching_eps=eps), ..., adjoint=False) in
fp32; the loss is a fixed random linear functional of the outputs (``grad_out``, stored).  A case holds
    coeffs (= x, the LINEAR coefficients), t_out, z0, p_*, grad_out, z_out, dcoeffs, dz0, d<param>, meta
Per case the manifest records the conditions the generator enforces, so that no test can hide behind them:
  ref_drift   the fp32 reference against itself in fp64; must be <= 1/4 of the tests' tolerance, per quantity
  vs_linear   every quantity against the same solve on plain LinearInterpolation; must be >= 100 x the tests' tolerance -- a route that
              forgot the smoothing (or its transpose) cannot pass.  Case d has T = 2: one linear piece, NO matching region, so the
              smoothed path IS the linear one; there the generator asserts the opposite (vs_linear <= the tolerance / 4) and the
              manifest says ``"single_piece": true``.
  max_dcoeffs max |dL/dx|; >= 1e3 x the tolerance, and no knot's row is (nearly) zero
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import gen_golden as gg  # noqa: E402  (sets up the reference's import path and the autots stub)
from src.ncde.interpolation import SmoothLinearInterpolation as RefSmooth  # noqa: E402

torchcde, data, GOLD = gg.torchcde, gg.data, gg.GOLD
TIGHT_Z, E2E_G = 2e-5, 2e-4      # tests/test_smooth_gpu.py:23, applied by tests/test_smooth_control_gpu.py

CASES = [
    # name, eps, method, step, outputs, (C, H, HH, nl), (B, T), seed, amplitude of the value channels
    ("a_eps1_rk4_knots", 1, "rk4", 1, "knots", (3, 8, 8, 2), (5, 6), 3, 5.0),
    ("b_eps05_midpoint_half_interval", 0.5, "midpoint", 0.5, "interval", (5, 12, 10, 3), (18, 5), 4, 3.0),
    ("c_eps02_euler_quarter_times", 0.2, "euler", 0.25, np.array([0.35, 1.6, 2.85], np.float32), (4, 16, 16, 1), (16, 4), 5, 3.0),
    ("d_eps05_rk4_interval_T2", 0.5, "rk4", 1, "interval", (2, 8, 8, 2), (3, 2), 6, 3.0),
]


def solve(x, eps, func, z0, outs, gout, method, step, dtype):
    c = torch.from_numpy(x).to(dtype).requires_grad_(True)
    X = torchcde.LinearInterpolation(c) if eps is None else RefSmooth(c, gradient_matching_eps=eps, match_second_derivatives=False)
    if isinstance(outs, str):
        tt = X.interval if outs == "interval" else X.grid_points
    else:
        tt = torch.from_numpy(outs).to(dtype)
    z0t = torch.from_numpy(z0).to(dtype).requires_grad_(True)
    for q in func.parameters():
        q.grad = None
    out = torchcde.cdeint(X, func, z0t, tt, adjoint=False, method=method, options={"step_size": step})
    (out * torch.from_numpy(gout).to(dtype)).sum().backward()
    res = {"z": out.detach(), "dcoeffs": c.grad.detach(), "dz0": z0t.grad.detach()}
    res["dtheta"] = [q.grad.detach().clone() for q in func.parameters()]
    return res, tt.detach()


def compare(a, b):
    """relerr of every quantity of `a` against `b` (parameters: the worst one)."""
    return {"z": gg.relerr(a["z"], b["z"]), "dcoeffs": gg.relerr(a["dcoeffs"], b["dcoeffs"]), "dz0": gg.relerr(a["dz0"], b["dz0"]),
            "dtheta": max(gg.relerr(p, q) for p, q in zip(a["dtheta"], b["dtheta"]))}


def bound(k):
    return TIGHT_Z if k == "z" else E2E_G


def main():
    torch.manual_seed(0)
    report = []
    for name, eps, method, step, outs, (C, H, HH, nl), (B, T), seed, amp in CASES:
        name = "g17_" + name
        x = data.synthetic_series(B, T, C - 1, missing=0.0, seed=70 + seed)
        x[:, :, 1:] *= np.float32(amp)      # (channel 0 is time)
        x = np.ascontiguousarray(torchcde.linear_interpolation_coeffs(torch.from_numpy(x)).numpy(), dtype=np.float32)
        assert x.shape == (B, T, C)
        p = data.make_field_weights(H, HH, C, seed=seed)
        if nl == 1:
            p = {k: v for k, v in p.items() if k not in ("W1", "b1")}
        rw = data.make_readin_weights(H, C, 1, seed=seed)
        z0 = gg.z0_from(x[:, 0], rw)
        names = [n for n in ("W0", "b0", "W1", "b1", "Wo", "bo") if n in p]
        n_t = 2 if isinstance(outs, str) and outs == "interval" else (T if isinstance(outs, str) else len(outs))
        gout = gg.grad_out_like((B, n_t, H), seed=13 + seed)
        res = {}
        for dtype in (torch.float32, torch.float64):
            func = gg.ref_field_original(p, C, H, HH, nl).to(dtype)
            assert [tuple(q.shape) for q in func.parameters()] == [tuple(p[n].shape) for n in names], "parameter order"
            res[dtype], tt = solve(x, eps, func, z0, outs, gout, method, step, dtype)
            if dtype == torch.float32:
                t32 = tt
                res["linear"], _ = solve(x, None, func, z0, outs, gout, method, step, dtype)
        r = res[torch.float32]
        drift, vs_linear = compare(r, res[torch.float64]), compare(res["linear"], r)
        dc = r["dcoeffs"].numpy()
        big = float(np.abs(dc).max())
        print(f"{name:40s} max|dcoeffs| {big:.3e} ref_drift " + " ".join(f"{k} {v:.2e}" for k, v in drift.items()) +
              " vs_linear " + " ".join(f"{k} {v:.2e}" for k, v in vs_linear.items()))
        assert all(v <= bound(k) / 4 for k, v in drift.items()), "reference drifts: another seed / amplitude"
        if T == 2:
            assert all(v <= bound(k) / 4 for k, v in vs_linear.items()), "T = 2 has no matching region: the path is the linear one"
        else:
            assert all(v >= 100 * bound(k) for k, v in vs_linear.items()), "too close to the linear solve to tell them apart"
        assert big >= 1e3 * E2E_G and (np.abs(dc).max(axis=(0, 2)) >= 1e-2 * big).all(), "a knot's row of dL/dx is (nearly) zero"
        rec = {"coeffs": x, "z0": z0, "t_out": t32.numpy().astype(np.float32), "grad_out": gout, "z_out": r["z"].numpy(), "dcoeffs": dc,
               "dz0": r["dz0"].numpy()}
        for n, g in zip(names, r["dtheta"]):
            rec["d" + n] = g.numpy()
        for k, v in p.items():
            rec["p_" + k] = v
        meta = {"name": name, "scheme": "cubic", "eps": eps, "method": method, "step_size": step,
                "outputs": outs if isinstance(outs, str) else "times", "dims": {"B": B, "T": T, "C": C, "H": H, "HH": HH, "nl": nl},
                "param_names": names, "max_dcoeffs": big, "single_piece": T == 2, "ref_drift": drift, "vs_linear": vs_linear}
        rec["meta"] = np.array(json.dumps(meta))
        np.savez_compressed(os.path.join(GOLD, name + ".npz"), **rec)
        report.append(meta)
    with open(os.path.join(GOLD, "MANIFEST_smooth_control.json"), "w") as f:
        json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
