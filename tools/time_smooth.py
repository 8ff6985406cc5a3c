"""Training-step time of the smoothed-linear control paths at cfg2 dims (run on the GPU box): linear / cubic-smoothed eps 1 /
quintic eps 1 / quintic eps 0.5, and the yardstick for the quintic kind: a NaturalCubicSpline of the same shape on the batch-tiled
family (NCDE_FLAG_FORCE_TILED).  The smoothed paths build their refined coefficients (ncde_prepare_smooth) inside the step.

    python tools/time_smooth.py [--out runs.jsonl] [--label this]           all five legs
    NCDE_ROOT=<checkout of the parent commit, built> python tools/time_smooth.py --yardstick-only --out runs.jsonl --label parent
    python tools/time_smooth.py --summarise runs.jsonl > profiles/r07_time_smooth.json

Alternate the first two in one session; --summarise reports, per leg, every run and the median, and the quintic / parent-spline ratios."""
import json, os, sys, time
ROOT = os.environ.get("NCDE_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
arg = lambda k: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else None      # noqa: E731
if "--summarise" in sys.argv:
    runs = [json.loads(l) for l in open(arg("--summarise")) if l.strip()]
    legs = {}
    for r in runs:
        legs.setdefault("%s: %s" % (r["label"], r["leg"]), []).append(r["ms_per_step"])
    med = {k: sorted(v)[len(v) // 2] for k, v in legs.items()}
    out = {"what": "tools/time_smooth.py: training step at cfg2 dims, ms; runs alternate between the two checkouts in one session",
           "runs_ms": legs, "median_ms": med}
    y = med.get("parent: spline, batch-tiled")
    if y:
        out["ratio_to_parent_spline_batch_tiled"] = {k: round(v / y, 3) for k, v in med.items() if k != "parent: spline, batch-tiled"}
        out["parent_spline_spread"] = round((max(legs["parent: spline, batch-tiled"]) - min(legs["parent: spline, batch-tiled"])) / y, 3)
    print(json.dumps(out, indent=1))
    sys.exit(0)
import torch
sys.path.insert(0, ROOT)
import bench, ncde_amd
c = dict(bench.CONFIGS["cfg2"])
B = int(os.environ.get("B", 4096))
coeffs = bench.make_inputs(c, B, 0, torch.device("cuda", 0))
y = (torch.rand(B, 1, device="cuda") > 0.5).float()
T = coeffs.shape[1]
cubic = torch.zeros(B, T - 1, 4 * c["C"], device="cuda")      # the linear path as spline rows a | b | 0 | 0
cubic[..., :c["C"]], cubic[..., c["C"]:2 * c["C"]] = coeffs[:, :-1], coeffs[:, 1:] - coeffs[:, :-1]
RUNS = [("linear", "rectilinear", None, 0, coeffs), ("cubic-smoothed eps 1", "linear_cubic_smoothing", 1, 0, coeffs),
        ("quintic eps 1", "linear_quintic_smoothing", 1, 0, coeffs), ("quintic eps 0.5", "linear_quintic_smoothing", 0.5, 0, coeffs),
        ("spline, batch-tiled", "cubic", None, 0x8000, cubic)]
if "--yardstick-only" in sys.argv:
    RUNS = RUNS[-1:]
for label, interp, eps, flags, x in RUNS:
    torch.manual_seed(0)
    m = ncde_amd.NeuralCDE(c["C"], c["H"], 1, hidden_hidden_dim=c["HH"], num_layers=c["nl"], interpolation=interp, interpolation_eps=eps,
                           adjoint=True, solver="rk4", kernel_flags=flags).cuda()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    lf = torch.nn.BCEWithLogitsLoss()
    def step():
        opt.zero_grad(set_to_none=True); l = lf(m(x), y); l.backward(); opt.step(); return l
    step(); step(); torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(8): l = step()
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / 8
    print("%-22s %8.2f ms/step  loss %.4f" % (label, dt * 1e3, float(l.detach())), flush=True)
    if arg("--out"):
        with open(arg("--out"), "a") as fh:
            fh.write(json.dumps({"label": arg("--label") or "this", "leg": label, "ms_per_step": round(dt * 1e3, 3)}) + "\n")
