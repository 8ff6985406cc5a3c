"""Golden vectors for the low-rank vector field (tests/golden/g17_*.npz + MANIFEST_lowrank.json), produced by IMPORTING the
reference's solver on the build machine -- the same way tools/gen_golden_control.py does, through oracle/gen_golden.py's shims.

    python tools/gen_golden_lowrank.py

Every case is the reference's torchcde.cdeint in fp32 with adjoint=True and with adjoint=False; the loss is a fixed random linear
functional of the outputs (``grad_out``, stored).  The field is ncde_amd.LowRankVectorField on the CPU: the reference's own module
(src/ncde/vector_fields/sparsity.py) imports the third-party ``sparselinear`` at module level and cannot be loaded.  Its forward is
pinned separately against tests/lowrank_util.restated_forward (checked here per case, and by tests/test_lowrank_cpu.py).
A case holds  coeffs, [knots], t_out, z0, p_*, grad_out, z_out, and per mode (adj = adjoint=True, disc = adjoint=False)
dz0_<mode>, d<param>_<mode>; meta carries ``ref_drift``: the fp32 reference against itself in fp64.
The generator refuses a case when that drift exceeds a quarter of either test tolerance, or when a gradient tensor of M_h or M_o
has a maximum below 1e3 x the tolerance (a wrong kernel could hide in it).
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import gen_golden as gg  # noqa: E402  (sets up the reference's import path and the autots stub)
import lowrank_util as lu  # noqa: E402
import ncde_amd  # noqa: E402

torchcde, data, GOLD = gg.torchcde, gg.data, gg.GOLD
TIGHT_Z, E2E_G = 2e-5, 2e-4      # tests/test_smooth_gpu.py:23, applied by tests/test_lowrank_gpu.py

CASES = [
    # name, control, B, T, C, sparsity, H, HH, nl, method, step, outputs, seed
    ("a_rect_rk4_interval", "rectilinear", 20, 9, 5, 0.6, 8, 12, 2, "rk4", 1, "interval", 3),
    ("b_linear_midpoint_knots", "linear", 20, 9, 5, 0.9, 8, 12, 1, "midpoint", 1, "knots", 4),
    ("c_cubic_rk4_knots", "cubic", 17, 8, 4, 0.0, 16, 16, 3, "rk4", 1, "knots", 5),
    ("d_linear_userknots_euler_half", "linear", 6, 7, 3, 0.5, 8, 8, 2, "euler", 0.5, np.array([0.0, 0.9, 2.6, 4.75, 5.0], np.float32), 6),
    ("e_linear_rk4_interval_c24", "linear", 33, 12, 24, 0.875, 32, 32, 3, "rk4", 1, "interval", 7),
]
EXPECTED_RANK = {"a": 2, "b": 1, "c": 4, "d": 2, "e": 3}


def solve(kind, coeffs, knots, func, z0, t, gout, method, step, adjoint, dtype):
    c = torch.from_numpy(coeffs).to(dtype)
    kn = None if knots is None else torch.from_numpy(knots).to(dtype)
    X = torchcde.LinearInterpolation(c, kn) if kind != "cubic" else torchcde.NaturalCubicSpline(c, kn)
    if isinstance(t, str):
        tt = X.interval if t == "interval" else X.grid_points
    else:
        tt = torch.from_numpy(t).to(dtype)
    z0t = torch.from_numpy(z0).to(dtype).requires_grad_(True)
    for q in func.parameters():
        q.grad = None
    out = torchcde.cdeint(X, func, z0t, tt, adjoint=adjoint, method=method, options={"step_size": step})
    (out * torch.from_numpy(gout).to(dtype)).sum().backward()
    return out.detach(), z0t.grad.detach(), tt.detach()


def main():
    torch.manual_seed(0)
    report = []
    for name, control, B, T, C, sparsity, H, HH, nl, method, step, outs, seed in CASES:
        R = lu.rank_of(C, sparsity)
        assert R == EXPECTED_RANK[name[0]], (name, R)
        name = "g17_" + name
        knots = None
        if control == "rectilinear":
            coeffs = data.make_rectilinear_coeffs(B, (T + 1) // 2, C - 1, missing=0.3, seed=40 + seed)
        elif control == "cubic":
            coeffs = data.make_cubic_coeffs(B, T, C - 1, seed=40 + seed)
        else:
            coeffs = data.make_linear_coeffs(B, T, C - 1, seed=40 + seed)
        if name.startswith("g17_d"):
            knots = np.array([0.0, 0.7, 1.5, 2.0, 3.1, 4.4, 5.0], np.float32)
            assert len(knots) == T
        coeffs = np.ascontiguousarray(coeffs, dtype=np.float32)
        assert coeffs.shape == ((B, T - 1, 4 * C) if control == "cubic" else (B, T, C)), coeffs.shape
        p = lu.make_weights(data, H, HH, C, R, nl, seed)
        z0 = gg.z0_from(coeffs[:, 0, :C], data.make_readin_weights(H, C, 1, seed=seed))
        names = lu.param_names(nl)
        n_t = 2 if isinstance(outs, str) and outs == "interval" else (T if isinstance(outs, str) else len(outs))
        gout = gg.grad_out_like((B, n_t, H), seed=13 + seed)
        res = {}
        for dtype in (torch.float32, torch.float64):
            func, named = lu.make_field(ncde_amd, p, C, H, HH, nl, sparsity, "cpu", dtype)
            assert func.rank == R and func.fused_spec().rank == R
            if dtype == torch.float64:      # the field's forward against the restated formula
                m = func(0.0, torch.from_numpy(z0).double())
                assert gg.relerr(m.detach(), lu.restated_forward(p, z0, H, C, R, nl)) <= 1e-12, name
            for adjoint in (True, False):
                z, dz0, tt = solve(control, coeffs, knots, func, z0, outs, gout, method, step, adjoint, dtype)
                res[dtype, adjoint] = (z, dz0, {k: named[k].grad.detach().clone() for k in names}, tt)
        rec = {"coeffs": coeffs, "z0": z0, "t_out": res[torch.float32, True][3].numpy().astype(np.float32), "grad_out": gout,
               "z_out": res[torch.float32, True][0].numpy()}
        assert torch.equal(res[torch.float32, True][0], res[torch.float32, False][0])      # one forward, whatever the backward
        if knots is not None:
            rec["knots"] = knots
        drift, big = {}, {}
        for adjoint, tag in ((True, "adj"), (False, "disc")):
            z, dz0, gp, _ = res[torch.float32, adjoint]
            z64, dz064, gp64, _ = res[torch.float64, adjoint]
            drift[tag] = {"z": gg.relerr(z, z64), "dz0": gg.relerr(dz0, dz064), "dtheta": max(gg.relerr(gp[k], gp64[k]) for k in names)}
            big[tag] = {k: float(gp[k].abs().max()) for k in ("Wh", "bh", "Wq", "bq")}
            assert drift[tag]["z"] <= TIGHT_Z / 4 and max(drift[tag]["dz0"], drift[tag]["dtheta"]) <= E2E_G / 4, (name, tag, drift[tag], "reference drifts")
            assert min(big[tag].values()) >= 1e3 * E2E_G, (name, tag, big[tag], "a head gradient is too small to test")
            rec["dz0_" + tag] = dz0.numpy()
            for k in names:
                rec["d%s_%s" % (k, tag)] = gp[k].numpy()
        print(f"{name:36s} R {R} " + " ".join(f"{t}: z {d['z']:.1e} dz0 {d['dz0']:.1e} dtheta {d['dtheta']:.1e} min max|dM| {min(big[t].values()):.2e}"
                                              for t, d in drift.items()))
        for k, v in p.items():
            rec["p_" + k] = v
        meta = {"name": name, "control": control, "interp": "cubic" if control == "cubic" else "linear", "method": method, "step_size": step,
                "outputs": outs if isinstance(outs, str) else "times", "sparsity": sparsity,
                "dims": {"B": B, "T": T, "C": C, "H": H, "HH": HH, "nl": nl, "R": R}, "param_names": names, "max_head_grads": big,
                "ref_drift": drift}
        rec["meta"] = np.array(json.dumps(meta))
        path = os.path.join(GOLD, name + ".npz")
        np.savez_compressed(path, **rec)
        assert os.path.getsize(path) < 1 << 20, (name, os.path.getsize(path))
        report.append(meta)
    with open(os.path.join(GOLD, "MANIFEST_lowrank.json"), "w") as f:
        json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
