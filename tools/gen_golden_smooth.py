"""Golden vectors for the smoothed-linear control paths (tests/golden/g14_*.npz + MANIFEST_smooth.json), produced by IMPORTING
the reference on the build machine -- the same way oracle/gen_golden.py does, whose import shims and helpers are reused.

    python tools/gen_golden_smooth.py

Layout of a solve case: g11's (coeffs = the LINEAR coefficients, t_out, z0, p_*, grad_out, z_out, dz0, d*, bp_dz0, bp_d*, meta).
Per case the manifest records the conditions the generator enforces, so that no test can hide behind them:
  vs_linear   relerr of z_out against the same solve on plain linear interpolation; must be >= 100 x the forward tolerance
  ref_drift   the reference in fp32 against itself in fp64 (z_out and every gradient); must be <= 1/4 of the tests' tolerances
  coeff_drift fp32 against fp64 matching coefficients, max abs
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
TIGHT_Z, E2E_G = 2e-5, 2e-4      # tests/test_gpu_parity.py:20-21, applied by tests/test_smooth_gpu.py


def solve(X, func, z0, t, gout, method, step, mode, adjoint, dtype):
    z0t = torch.from_numpy(z0).to(dtype).requires_grad_(True)
    for q in func.parameters():
        q.grad = None
    func.nfe = 0
    out = torchcde.cdeint(X, func, z0t, t.to(dtype), adjoint=adjoint, vector_field_type=mode, method=method, options={"step_size": step})
    (out * torch.from_numpy(gout).to(dtype)).sum().backward()
    return out.detach(), z0t.grad.detach(), [q.grad.detach().clone() for q in func.parameters()], func.nfe


def gen_solves():
    B, L = 10, 9
    ragged = np.array([0.0, 1.3, 4.0, 6.55, 8.0], np.float32)
    cases = [
        # name, quintic, eps, method, step, outputs, field kind, field input, (C, H, HH, nl), weight seed[, amplitude of the series]
        ("a_cubic_eps1_rk4", False, 1, "rk4", 1, "interval", "original", "matmul", (5, 16, 24, 3), 6),
        ("b_cubic_eps05_rk4", False, 0.5, "rk4", 1, "knots", "original", "matmul", (5, 16, 24, 3), 6),
        ("c_cubic_eps02_rk4_quarter", False, 0.2, "rk4", 0.25, ragged, "original", "matmul", (5, 16, 24, 3), 6),
        ("d_quintic_eps1_midpoint", True, 1, "midpoint", 1, "knots", "original", "matmul", (5, 16, 24, 3), 6),
        ("e_quintic_eps05_rk4", True, 0.5, "rk4", 1, "interval", "original", "matmul", (5, 16, 24, 3), 6),
        ("f_quintic_eps03_euler_tenth", True, 0.3, "euler", 0.1, ragged, "original", "matmul", (5, 16, 24, 3), 6),
        ("g_quintic_eps1_gru_evaluate", True, 1, "rk4", 1, "interval", "gru", "evaluate", (5, 16, 24, 3), 5, 4.0),      # (X(t) enters
        # the field's input, not a product with dX/dt: at unit amplitude the smoothed solve sits 1e-3 from the linear one, below the bar)
        ("h_quintic_eps05_rk4_half_c20", True, 0.5, "rk4", 0.5, "interval", "original", "matmul", (20, 32, 32, 3), 8),
    ]
    report = []
    for name, quintic, eps, method, step, outs, kind, mode, (C, H, HH, nl), seed, *amp in cases:
        name = "g14_" + name
        x = data.synthetic_series(B, L, C - 1, missing=0.0, seed=61 + C)
        if amp:
            x[:, :, 1:] *= np.float32(amp[0])      # (channel 0 is time)
        coeffs = torchcde.linear_interpolation_coeffs(torch.from_numpy(x))
        p = data.make_field_weights(H, HH, C, seed=seed) if kind == "original" else data.make_variant_weights(H, HH, C, seed=seed, kind=kind, mode=mode)
        rw = data.make_readin_weights(H, C, 1, seed=seed)
        z0 = gg.z0_from(x[:, 0], rw)
        names = [n for n in ("W0", "b0", "W1", "b1", "Wr", "br", "Wg", "bg", "Wo", "bo") if n in p]
        res = {}
        for dtype in (torch.float32, torch.float64):
            func = gg.ref_field_variant(p, C, H, HH, nl, kind, mode).to(dtype)
            assert [tuple(q.shape) for q in func.parameters()] == [tuple(p[n].shape) for n in names], "parameter order"
            X = RefSmooth(coeffs.to(dtype), gradient_matching_eps=eps, match_second_derivatives=quintic)
            t = X.grid_points if isinstance(outs, str) and outs == "knots" else (X.interval if isinstance(outs, str) else torch.from_numpy(outs))
            gout = gg.grad_out_like((B, len(t), H), seed=13)
            for adj in (True, False):
                res[dtype, adj] = solve(X, func, z0, t, gout, method, step, mode, adj, dtype)
            Xl = torchcde.LinearInterpolation(coeffs.to(dtype))
            res[dtype, "linear"] = solve(Xl, func, z0, t, gout, method, step, mode, True, dtype)
        z_ref, dz0_ref, gp_ref, nfe_ref = res[torch.float32, True]
        _, dz0_bp, gp_bp, _ = res[torch.float32, False]
        z64, dz0_64, gp64, _ = res[torch.float64, True]
        _, bdz0_64, bgp64, _ = res[torch.float64, False]
        vs_linear = gg.relerr(res[torch.float32, "linear"][0], z_ref)
        drift = {"z": gg.relerr(z_ref, z64), "dz0": gg.relerr(dz0_ref, dz0_64), "dtheta": max(gg.relerr(a, b) for a, b in zip(gp_ref, gp64)),
                 "bp_dz0": gg.relerr(dz0_bp, bdz0_64), "bp_dtheta": max(gg.relerr(a, b) for a, b in zip(gp_bp, bgp64))}
        m32 = RefSmooth(coeffs, gradient_matching_eps=eps, match_second_derivatives=quintic).gradient_matching_coeffs
        m64 = RefSmooth(coeffs.double(), gradient_matching_eps=eps, match_second_derivatives=quintic).gradient_matching_coeffs
        coeff_drift = float((m32.double() - m64).abs().max())
        print(f"{name:36s} vs_linear {vs_linear:.2e} coeff_drift {coeff_drift:.2e} ref_drift " + " ".join(f"{k} {v:.2e}" for k, v in drift.items()), "nfe", nfe_ref)
        assert vs_linear >= 100 * TIGHT_Z, "the smoothed solve is too close to the linear one to tell them apart"
        assert drift["z"] <= TIGHT_Z / 4 and max(v for k, v in drift.items() if k != "z") <= E2E_G / 4, "reference drifts: another seed / weight scale"
        rec = {"z_out": z_ref.numpy(), "dz0": dz0_ref.numpy(), "grad_out": gout, "bp_dz0": dz0_bp.numpy(), "coeffs": coeffs.numpy().copy(), "z0": z0,
               "t_out": t.numpy().astype(np.float32), "matching_coeffs": m32.numpy().copy()}
        for n, g, gb in zip(names, gp_ref, gp_bp):
            rec["d" + n], rec["bp_d" + n] = g.numpy(), gb.numpy()
        for k, v in p.items():
            rec["p_" + k] = v
        meta = {"name": name, "scheme": "quintic" if quintic else "cubic", "eps": eps, "method": method, "step_size": step,
                "outputs": outs if isinstance(outs, str) else "times", "field_kind": kind, "field_mode": mode, "nfe": nfe_ref,
                "dims": {"C": C, "H": H, "HH": HH, "nl": nl}, "param_names": names, "vs_linear": vs_linear, "ref_drift": drift,
                "coeff_drift": coeff_drift}
        rec["meta"] = np.array(json.dumps(meta))
        np.savez_compressed(os.path.join(GOLD, name + ".npz"), **rec)
        report.append(meta)
    return report


def gen_probe():
    """Case i: evaluate / derivative of the class at probe times incl. exact knots, k + eps and its fp32 neighbours; the matching
    coefficients themselves; fp32 and fp64."""
    B, L, C = 4, 7, 3
    x = data.synthetic_series(B, L, C - 1, missing=0.0, seed=71)
    coeffs = torchcde.linear_interpolation_coeffs(torch.from_numpy(x))
    rec = {"coeffs": coeffs.numpy().copy()}
    combos = []
    for quintic in (False, True):
        for eps in (0.5, 1):
            base = [0.0, 0.25, 0.999, 1.0, 1.1, 1.49, 2.0, 2.2, 2.75, 3.0, 3.3, 4.0, 4.05, 4.6, 5.0, 5.45, 5.9, 6.0]
            edge = []
            for k in (1, 2, 4, 5):
                e = np.float32(k + eps)
                edge += [float(e), float(np.nextafter(e, np.float32(-np.inf))), float(np.nextafter(e, np.float32(np.inf)))]
            times = np.array(sorted(set(base + edge + [1.0 + eps / 2, 3.0 + eps / 3, 5.0 + 0.9 * eps])), np.float64)
            times = times[times <= L - 1]
            tag = "%s_eps%s" % ("quintic" if quintic else "cubic", str(eps).replace(".", ""))
            rec["t_" + tag] = times
            for dtype, dn in ((torch.float32, "f32"), (torch.float64, "f64")):
                X = RefSmooth(coeffs.to(dtype), gradient_matching_eps=eps, match_second_derivatives=quintic)
                rec["m_%s_%s" % (tag, dn)] = X.gradient_matching_coeffs.numpy().copy()
                rec["ev_%s_%s" % (tag, dn)] = np.stack([X.evaluate(float(t)).numpy() for t in times])
                rec["dv_%s_%s" % (tag, dn)] = np.stack([X.derivative(float(t)).numpy() for t in times])
            combos.append({"tag": tag, "quintic": quintic, "eps": eps, "n_times": int(len(times))})
    meta = {"name": "g14_i_probe", "combos": combos}
    rec["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(GOLD, "g14_i_probe.npz"), **rec)
    return meta


class StepCounter:
    """Accepted / rejected attempts of the reference's adaptive solver: an attempt is accepted iff it moves the state's t1."""

    def __enter__(self):
        from torchdiffeq._impl import rk_common
        self.cls, self.orig = rk_common.RKAdaptiveStepsizeODESolver, rk_common.RKAdaptiveStepsizeODESolver._adaptive_step
        self.accepted = self.rejected = 0
        counter = self

        def counted(solver, state):
            new = counter.orig(solver, state)
            if bool(new.t1 != state.t1):
                counter.accepted += 1
            else:
                counter.rejected += 1
            return new
        self.cls._adaptive_step = counted
        return self

    def __exit__(self, *exc):
        self.cls._adaptive_step = self.orig


def gen_dopri5():
    """Cases j1 / j2: dopri5 on the cubic-smoothed path (eps 1), which the package runs on its unfused solver.
    j1: the reference's own configuration -- the NeuralCDE module, adjoint=False, the module's min_step 0.5 -- in fp64 (both sides then
        take the same free-running step sequence; the counts are recorded).
    j2: cdeint in fp32 with a pinned step (first_step = min_step = max_step = 0.75), adjoint=True and adjoint=False."""
    B, L, C, H, HH, nl, OUT = 10, 9, 5, 16, 24, 3, 2
    x = data.synthetic_series(B, L, C - 1, missing=0.0, seed=61 + C)
    coeffs = torchcde.linear_interpolation_coeffs(torch.from_numpy(x))
    # ---- j1
    torch.manual_seed(14)
    model = gg.RefNeuralCDE(C, H, OUT, hidden_hidden_dim=HH, num_layers=nl, interpolation="linear_cubic_smoothing", interpolation_eps=1,
                            solver="dopri5", adjoint=False).double()
    gout = gg.grad_out_like((B, 1, OUT), seed=13)[:, 0].astype(np.float64)
    with StepCounter() as sc:
        out = model(coeffs.double())
    (out * torch.from_numpy(gout)).sum().backward()
    lin = gg.RefNeuralCDE(C, H, OUT, hidden_hidden_dim=HH, num_layers=nl, interpolation="linear", solver="dopri5", adjoint=False).double()
    lin.load_state_dict(model.state_dict())
    vs_linear = gg.relerr(lin(coeffs.double()).detach(), out.detach())
    rec = {"coeffs": coeffs.double().numpy().copy(), "grad_out": gout, "out": out.detach().numpy()}
    for k, v in model.state_dict().items():
        rec["sd_" + k] = v.numpy().copy()
    for k, q in model.named_parameters():
        rec["g_" + k] = q.grad.numpy().copy()
    m1 = {"name": "g14_j1_module_dopri5_f64", "scheme": "cubic", "eps": 1, "method": "dopri5", "adjoint": False, "dtype": "float64",
          "dims": {"C": C, "H": H, "HH": HH, "nl": nl, "OUT": OUT}, "steps_fwd": [sc.accepted, sc.rejected], "vs_linear": vs_linear,
          "param_names": [k for k, _ in model.named_parameters()]}
    print(f"{m1['name']:36s} steps +{sc.accepted}/-{sc.rejected} vs_linear {vs_linear:.2e}")
    assert sc.rejected >= 1 and vs_linear >= 1e-3
    rec["meta"] = np.array(json.dumps(m1))
    np.savez_compressed(os.path.join(GOLD, m1["name"] + ".npz"), **rec)
    # ---- j2
    for wseed in (6, 7, 8, 9, 10):      # the first weight seed whose reference run meets the drift / vs_linear conditions (seed 6: z drift 2.55e-6 > 2.5e-6)
        p = data.make_field_weights(H, HH, C, seed=wseed)
        rw = data.make_readin_weights(H, C, 1, seed=wseed)
        z0 = gg.z0_from(x[:, 0], rw)
        opts = {"first_step": 0.75, "min_step": 0.75, "max_step": 0.75}
        res, steps = {}, {}
        for dtype in (torch.float32, torch.float64):
            func = gg.ref_field_original(p, C, H, HH, nl).to(dtype)
            X = RefSmooth(coeffs.to(dtype), gradient_matching_eps=1, match_second_derivatives=False)
            t = X.grid_points
            gout2 = gg.grad_out_like((B, len(t), H), seed=13)
            for kind, Xk in (("smooth", X), ("linear", torchcde.LinearInterpolation(coeffs.to(dtype)))):
                for adj in ((True, False) if kind == "smooth" else (True,)):
                    z0t = torch.from_numpy(z0).to(dtype).requires_grad_(True)
                    for q in func.parameters():
                        q.grad = None
                    with StepCounter() as sc:
                        o = torchcde.cdeint(Xk, func, z0t, t, adjoint=adj, method="dopri5", rtol=1e-3, atol=1e-5, options=dict(opts))
                        steps[dtype, kind, adj] = [sc.accepted, sc.rejected]      # (the forward's)
                        (o * torch.from_numpy(gout2).to(dtype)).sum().backward()
                    res[dtype, kind, adj] = (o.detach(), z0t.grad.detach(), [q.grad.detach().clone() for q in func.parameters()])
        names = ["W0", "b0", "W1", "b1", "Wo", "bo"]
        z_ref, dz0_ref, gp_ref = res[torch.float32, "smooth", True]
        _, dz0_bp, gp_bp = res[torch.float32, "smooth", False]
        a64, b64 = res[torch.float64, "smooth", True], res[torch.float64, "smooth", False]
        drift = {"z": gg.relerr(z_ref, a64[0]), "dz0": gg.relerr(dz0_ref, a64[1]), "dtheta": max(gg.relerr(a, b) for a, b in zip(gp_ref, a64[2])),
                 "bp_dz0": gg.relerr(dz0_bp, b64[1]), "bp_dtheta": max(gg.relerr(a, b) for a, b in zip(gp_bp, b64[2]))}
        vs_linear = gg.relerr(res[torch.float32, "linear", True][0], z_ref)
        print(f"{'g14_j2_cdeint_dopri5_pinned':36s} steps {steps[torch.float32, 'smooth', True]} vs_linear {vs_linear:.2e} ref_drift " +
              " ".join(f"{k} {v:.2e}" for k, v in drift.items()))
        assert steps[torch.float32, "smooth", True] == steps[torch.float64, "smooth", True] and steps[torch.float32, "smooth", True][1] == 0
        if vs_linear >= 100 * 1e-5 and drift["z"] <= 1e-5 / 4 and max(v for k, v in drift.items() if k != "z") <= 1e-4 / 4:
            break
    else:
        raise AssertionError("no weight seed meets the ref_drift / vs_linear conditions")
    rec = {"coeffs": coeffs.numpy().copy(), "z0": z0, "t_out": t.numpy().astype(np.float32), "grad_out": gout2, "z_out": z_ref.numpy(),
           "dz0": dz0_ref.numpy(), "bp_dz0": dz0_bp.numpy()}
    for n, g, gb in zip(names, gp_ref, gp_bp):
        rec["d" + n], rec["bp_d" + n] = g.numpy(), gb.numpy()
    for k, v in p.items():
        rec["p_" + k] = v
    m2 = {"name": "g14_j2_cdeint_dopri5_pinned", "scheme": "cubic", "eps": 1, "method": "dopri5", "options": opts, "rtol": 1e-3, "atol": 1e-5,
          "dims": {"C": C, "H": H, "HH": HH, "nl": nl}, "param_names": names, "steps_fwd": steps[torch.float32, "smooth", True],
          "vs_linear": vs_linear, "ref_drift": drift, "weight_seed": wseed}
    rec["meta"] = np.array(json.dumps(m2))
    np.savez_compressed(os.path.join(GOLD, m2["name"] + ".npz"), **rec)
    return [m1, m2]


def main():
    torch.manual_seed(0)
    if "--only-dopri5" in sys.argv:      # (the other fixtures stay as they are; their manifest entries are kept)
        with open(os.path.join(GOLD, "MANIFEST_smooth.json")) as f:
            report = [m for m in json.load(f) if not m["name"].startswith("g14_j")] + gen_dopri5()
    else:
        report = gen_solves() + [gen_probe()] + gen_dopri5()
    with open(os.path.join(GOLD, "MANIFEST_smooth.json"), "w") as f:
        json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
