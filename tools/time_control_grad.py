"""Price of the fused control-path gradients (run on the GPU box): adjoint=False training step at cfg2 dims, B 4096.

    python tools/time_control_grad.py [--rounds 4] [--out runs.json]

  (i)   coefficients without grad, exact discrete backward on the batch-tiled family (NCDE_FLAG_FORCE_TILED)
  (ii)  coefficients with grad on the fused route (ncde_backward_control: (i) on fp32 records + pass C)
  (iii) the same request on the unfused torch-op solver (what it ran on before the route existed), FEWER timed steps (2) -- stated in the output
  (iv)  a two-layer StackedNeuralCDE step, hidden sizes 32 and 32, adjoint=False: fused, and (v) with the control route switched off
  (vi)  coefficients with grad under interpolation="linear_cubic_smoothing", interpolation_eps 0.5, on the fused route (ncde_prepare_smooth,
        the time plan of the refined grid, ncde_backward_control + ncde_prepare_smooth_backward), and (vii) with the route switched off
The legs alternate: every round runs each leg once; the output holds every run, the median and the spread (max - min) / median."""
import json, os, sys, time, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
arg = lambda k, d=None: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d      # noqa: E731
import torch
sys.path.insert(0, ROOT)
import bench, ncde_amd
from ncde_amd import solver

c = dict(bench.CONFIGS["cfg2"])
B = int(os.environ.get("B", 4096))
coeffs = bench.make_inputs(c, B, 0, torch.device("cuda", 0))
y = (torch.rand(B, 1, device="cuda") > 0.5).float()
lf = torch.nn.BCEWithLogitsLoss()
route = solver._control_route_ok


def make(stacked, flags=0, smooth=False):
    torch.manual_seed(0)
    if smooth:
        m = ncde_amd.NeuralCDE(c["C"], c["H"], 1, hidden_hidden_dim=c["HH"], num_layers=c["nl"], interpolation="linear_cubic_smoothing",
                               interpolation_eps=0.5, adjoint=False, solver="rk4").cuda()
    elif stacked:
        m = ncde_amd.StackedNeuralCDE(c["C"], [32, 32], 1, adjoint=False).cuda()
    else:
        m = ncde_amd.NeuralCDE(c["C"], c["H"], 1, hidden_hidden_dim=c["HH"], num_layers=c["nl"], interpolation="linear", adjoint=False,
                               solver="rk4", kernel_flags=flags).cuda()
    return m, torch.optim.Adam(m.parameters(), lr=1e-3)


LEGS = [("i: no control grad, FORCE_TILED", make(False, 0x8000), False, True, 8),
        ("ii: control grad, fused", make(False), True, True, 8),
        ("iii: control grad, unfused (2 timed steps)", make(False), True, False, 2),
        ("iv: stacked [32, 32], fused", make(True), False, True, 8),
        ("v: stacked [32, 32], unfused (2 timed steps)", make(True), False, False, 2),
        ("vi: cubic-smoothed eps 0.5, control grad, fused", make(False, smooth=True), True, True, 8),
        ("vii: cubic-smoothed eps 0.5, control grad, unfused (2 timed steps)", make(False, smooth=True), True, False, 2)]
runs = {k[0]: [] for k in LEGS}
for rnd in range(int(arg("--rounds", 4))):
    for label, (m, opt), grad, fused, n in LEGS:
        solver._control_route_ok = route if fused else (lambda *a: False)
        x = coeffs.clone().requires_grad_(grad)

        def step():
            opt.zero_grad(set_to_none=True); x.grad = None; l = lf(m(x), y); l.backward(); opt.step(); return l
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            step(); torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(n): l = step()
            torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / n
        runs[label].append(round(dt * 1e3, 3))
        print("round %d %-46s %9.2f ms/step  loss %.4f" % (rnd, label, dt * 1e3, float(l.detach())), flush=True)
solver._control_route_ok = route
med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
k = [l[0] for l in LEGS]
out = {"what": "tools/time_control_grad.py: adjoint=False training step at cfg2 dims (B %d, %d knots), ms; legs alternate within one session" % (B, coeffs.shape[1]),
       "runs_ms": runs, "median_ms": med, "spread": {q: round((max(v) - min(v)) / med[q], 3) for q, v in runs.items()},
       "ii_over_i": round(med[k[1]] / med[k[0]], 3), "iii_over_ii": round(med[k[2]] / med[k[1]], 2), "v_over_iv": round(med[k[4]] / med[k[3]], 2),
       "vi_over_ii": round(med[k[5]] / med[k[1]], 3), "vii_over_vi": round(med[k[6]] / med[k[5]], 2)}
print(json.dumps(out, indent=1))
if arg("--out"):
    with open(arg("--out"), "w") as fh:
        json.dump(out, fh, indent=1)
