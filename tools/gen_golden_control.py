"""Golden vectors for the control-path gradients (tests/golden/g16_*.npz + MANIFEST_control.json), produced by IMPORTING the
reference on the build machine -- the same way oracle/gen_golden.py does, whose import shims and helpers are reused.

    python tools/gen_golden_control.py

Every case is the reference's cdeint (or its StackedNeuralCDE) with adjoint=False and a coefficient LEAF that requires grad, in fp32;
the loss is a fixed random linear functional of the outputs (``grad_out``, stored).  A solve case holds
    coeffs, [knots], t_out, z0, p_*, grad_out, z_out, dcoeffs, dz0, d<param>, meta
and the stacked case  coeffs, sd_<state_dict key>, and per return_sequences setting  grad_out_*, out_*, dcoeffs_*, g_*__<parameter>.
The generator refuses a case whose dL/dcoeffs could hide a wrong kernel: max |dL/dcoeffs| must be >= 1e3 x the tests' tolerance
(2e-4, relative to that maximum: so every row is resolved far below its own size) and every interior row of every sample-independent
time index must hold a value >= 1e-2 of the maximum; a cubic case's ``a`` columns must be exactly zero.  ``ref_drift``: the fp32
reference against itself in fp64, which must stay within a quarter of each tolerance.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import gen_golden as gg  # noqa: E402  (sets up the reference's import path and the autots stub)
from src.ncde.stacked import StackedNeuralCDE as RefStacked  # noqa: E402

torchcde, data, GOLD = gg.torchcde, gg.data, gg.GOLD
TIGHT_Z, E2E_G = 2e-5, 2e-4      # tests/test_smooth_gpu.py:23, applied by tests/test_control_grad_gpu.py


def check_dcoeffs(name, dc, kind, C):
    big = float(np.abs(dc).max())
    assert big >= 1e3 * E2E_G, (name, "dL/dcoeffs too small to test", big)
    rows = np.abs(dc).max(axis=(0, 2))      # per time index
    assert (rows[1:-1] >= 1e-2 * big).all(), (name, "an interior row of dL/dcoeffs is (nearly) zero", rows / big)
    if kind == "cubic":
        assert not dc[..., :C].any(), (name, "the a columns of a cubic control receive no gradient")
        for part in (1, 2, 3):
            assert np.abs(dc[..., part * C:(part + 1) * C]).max() >= 1e-2 * big, (name, "part", part)
    return big


def solve(kind, coeffs, knots, func, z0, t, gout, method, step, dtype):
    c = torch.from_numpy(coeffs).to(dtype).requires_grad_(True)
    kn = None if knots is None else torch.from_numpy(knots).to(dtype)
    X = torchcde.LinearInterpolation(c, kn) if kind != "cubic" else torchcde.NaturalCubicSpline(c, kn)
    if isinstance(t, str):
        tt = X.interval if t == "interval" else X.grid_points
    else:
        tt = torch.from_numpy(t).to(dtype)
    z0t = torch.from_numpy(z0).to(dtype).requires_grad_(True)
    for q in func.parameters():
        q.grad = None
    out = torchcde.cdeint(X, func, z0t, tt, adjoint=False, method=method, options={"step_size": step})
    (out * torch.from_numpy(gout).to(dtype)).sum().backward()
    return out.detach(), c.grad.detach(), z0t.grad.detach(), [q.grad.detach().clone() for q in func.parameters()], tt.detach()


def gen_solves():
    cases = [
        # name, control, B, T, C, H, HH, nl, method, step, outputs, seed
        ("a_rect_rk4_interval", "rectilinear", 20, 9, 5, 8, 12, 2, "rk4", 1, "interval", 3),
        ("b_linear_midpoint_knots", "linear", 20, 9, 5, 8, 12, 2, "midpoint", 1, "knots", 4),
        ("c_cubic_rk4_knots", "cubic", 17, 8, 4, 16, 16, 3, "rk4", 1, "knots", 5),
        ("d_linear_userknots_euler_half", "linear", 6, 7, 3, 8, 8, 2, "euler", 0.5, np.array([0.0, 0.9, 2.6, 4.75, 5.0], np.float32), 6),
        ("e_linear_rk4_interval_c24", "linear", 33, 12, 24, 32, 32, 3, "rk4", 1, "interval", 7),
    ]
    report = []
    for name, control, B, T, C, H, HH, nl, method, step, outs, seed in cases:
        name = "g16_" + name
        knots = None
        if control == "rectilinear":
            coeffs = data.make_rectilinear_coeffs(B, (T + 1) // 2, C - 1, missing=0.3, seed=40 + seed)
        elif control == "cubic":
            coeffs = data.make_cubic_coeffs(B, T, C - 1, seed=40 + seed)
        else:
            coeffs = data.make_linear_coeffs(B, T, C - 1, seed=40 + seed)
        if name.startswith("g16_d"):
            knots = np.array([0.0, 0.7, 1.5, 2.0, 3.1, 4.4, 5.0], np.float32)
            assert len(knots) == T
        coeffs = np.ascontiguousarray(coeffs, dtype=np.float32)
        assert coeffs.shape == ((B, T - 1, 4 * C) if control == "cubic" else (B, T, C)), coeffs.shape
        p = data.make_field_weights(H, HH, C, seed=seed)
        rw = data.make_readin_weights(H, C, 1, seed=seed)
        z0 = gg.z0_from(coeffs[:, 0, :C], rw)
        names = ["W0", "b0", "W1", "b1", "Wo", "bo"]
        res = {}
        for dtype in (torch.float32, torch.float64):
            func = gg.ref_field_original(p, C, H, HH, nl).to(dtype)
            assert [tuple(q.shape) for q in func.parameters()] == [tuple(p[n].shape) for n in names], "parameter order"
            n_t = 2 if isinstance(outs, str) and outs == "interval" else (T if isinstance(outs, str) else len(outs))
            gout = gg.grad_out_like((B, n_t, H), seed=13 + seed)
            res[dtype] = solve(control, coeffs, knots, func, z0, outs, gout, method, step, dtype)
        z, dc, dz0, gp, tt = res[torch.float32]
        z64, dc64, dz064, gp64, _ = res[torch.float64]
        drift = {"z": gg.relerr(z, z64), "dcoeffs": gg.relerr(dc, dc64), "dz0": gg.relerr(dz0, dz064),
                 "dtheta": max(gg.relerr(a, b) for a, b in zip(gp, gp64))}
        big = check_dcoeffs(name, dc.numpy(), control, C)
        print(f"{name:36s} max|dcoeffs| {big:.3e} ref_drift " + " ".join(f"{k} {v:.2e}" for k, v in drift.items()))
        assert drift["z"] <= TIGHT_Z / 4 and max(v for k, v in drift.items() if k != "z") <= E2E_G / 4, "reference drifts: another seed"
        rec = {"coeffs": coeffs, "z0": z0, "t_out": tt.numpy().astype(np.float32), "grad_out": gout, "z_out": z.numpy(), "dcoeffs": dc.numpy(),
               "dz0": dz0.numpy()}
        if knots is not None:
            rec["knots"] = knots
        for n, g in zip(names, gp):
            rec["d" + n] = g.numpy()
        for k, v in p.items():
            rec["p_" + k] = v
        meta = {"name": name, "control": control, "interp": "cubic" if control == "cubic" else "linear", "method": method, "step_size": step,
                "outputs": outs if isinstance(outs, str) else "times", "dims": {"B": B, "T": T, "C": C, "H": H, "HH": HH, "nl": nl},
                "param_names": names, "max_dcoeffs": big, "ref_drift": drift}
        rec["meta"] = np.array(json.dumps(meta))
        np.savez_compressed(os.path.join(GOLD, name + ".npz"), **rec)
        report.append(meta)
    return report


def gen_stacked():
    """Case f: the reference's StackedNeuralCDE(3, [8, 6], 2), adjoint=False, return_sequences True and False on the same weights."""
    B, T, C = 5, 7, 3
    coeffs = np.ascontiguousarray(data.make_linear_coeffs(B, T, C - 1, seed=48), dtype=np.float32)
    torch.manual_seed(16)
    base = RefStacked(C, [8, 6], 2, adjoint=False, return_sequences=True)
    sd = {k: v.clone() for k, v in base.state_dict().items()}
    rec = {"coeffs": coeffs}
    for k, v in sd.items():
        rec["sd_" + k] = v.numpy().copy()
    meta = {"name": "g16_f_stacked", "ctor": {"input_dim": C, "hidden_dims": [8, 6], "output_dim": 2},
            "state_dict_keys": list(sd.keys()), "param_names": [k for k, _ in base.named_parameters()],
            "attributes": {k: getattr(base, k) for k in ("input_dim", "hidden_dims", "output_dim", "hidden_hidden_dim", "static_dim", "adjoint",
                                                         "static_in_all_layers", "num_stacked")},
            "ref_drift": {}, "max_dcoeffs": {}}
    for seq in (True, False):
        tag = "seq" if seq else "final"
        res = {}
        for dtype in (torch.float32, torch.float64):
            model = RefStacked(C, [8, 6], 2, adjoint=False, return_sequences=seq).to(dtype)
            model.load_state_dict({k: v.to(dtype) for k, v in sd.items()})
            c = torch.from_numpy(coeffs).to(dtype).requires_grad_(True)
            out = model(c)
            gout = gg.grad_out_like((B, T, 2), seed=29) if seq else gg.grad_out_like((B, 1, 2), seed=29)[:, 0]
            (out * torch.from_numpy(gout).to(dtype)).sum().backward()
            # (fc_output is never used: its parameters keep grad None)
            res[dtype] = (out.detach(), c.grad.detach(), {k: q.grad.detach().clone() for k, q in model.named_parameters() if q.grad is not None}, gout)
        out, dc, gp, gout = res[torch.float32]
        out64, dc64, gp64, _ = res[torch.float64]
        drift = {"out": gg.relerr(out, out64), "dcoeffs": gg.relerr(dc, dc64), "dtheta": max(gg.relerr(gp[k], gp64[k]) for k in gp)}
        big = check_dcoeffs("g16_f_stacked/" + tag, dc.numpy(), "linear", C)
        print(f"{'g16_f_stacked ' + tag:36s} max|dcoeffs| {big:.3e} ref_drift " + " ".join(f"{k} {v:.2e}" for k, v in drift.items()))
        assert drift["out"] <= TIGHT_Z / 4 and max(drift["dcoeffs"], drift["dtheta"]) <= E2E_G / 4, "reference drifts: another seed"
        assert sorted(gp) == sorted(k for k in meta["param_names"] if not k.startswith("fc_output"))
        rec["grad_out_" + tag], rec["out_" + tag], rec["dcoeffs_" + tag] = gout, out.numpy(), dc.numpy()
        for k, g in gp.items():
            rec["g_%s__%s" % (tag, k)] = g.numpy()
        meta["ref_drift"][tag], meta["max_dcoeffs"][tag] = drift, big
    rec["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(GOLD, "g16_f_stacked.npz"), **rec)
    return meta


def main():
    torch.manual_seed(0)
    report = gen_solves() + [gen_stacked()]
    with open(os.path.join(GOLD, "MANIFEST_control.json"), "w") as f:
        json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
