"""Training-step time of the low-rank vector field at cfg2 dims (B 4096, T 399, C 20, H = HH = 32, three layers, rk4; run on the GPU box)
beside the original field on the generic family (NCDE_FLAG_FORCE_GENERIC) and on its auto route.

    python tools/time_lowrank.py            # SPARSITY=0.9 ROUNDS=3 STEPS=5 B=4096

Step = forward + BCE loss + continuous-adjoint backward + Adam, as bench.py times it.  Every variant is warmed up (2 steps), then the
variants are timed ALTERNATING for ROUNDS rounds of STEPS steps each, a host clock around work that ends in a device synchronise; one
line per (variant, round) so that the spread is visible, then the median per variant."""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import ncde_amd  # noqa: E402
from ncde_amd import _lib  # noqa: E402

c = dict(bench.CONFIGS["cfg2"])
B, ROUNDS, STEPS = int(os.environ.get("B", 4096)), int(os.environ.get("ROUNDS", 3)), int(os.environ.get("STEPS", 5))
SPARSITY = float(os.environ.get("SPARSITY", 0.9))
coeffs = bench.make_inputs(c, B, 0, torch.device("cuda", 0))
T = coeffs.shape[1]
y = (torch.rand(B, 1, device="cuda") > 0.5).float()
VARIANTS = [("low-rank", dict(vector_field="low-rank", sparsity=SPARSITY)),
            ("original, generic family", dict(kernel_flags=_lib.FLAG_FORCE_GENERIC)),
            ("original, auto route", dict())]
steps = {}
for name, kw in VARIANTS:
    torch.manual_seed(0)
    m = ncde_amd.NeuralCDE(c["C"], c["H"], 1, hidden_hidden_dim=c["HH"], num_layers=c["nl"], interpolation="rectilinear", adjoint=True,
                           solver="rk4", **kw).cuda()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    lf = torch.nn.BCEWithLogitsLoss()

    def step(m=m, opt=opt, lf=lf):
        opt.zero_grad(set_to_none=True)
        loss = lf(m(coeffs), y)
        loss.backward()
        opt.step()
        return loss
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    steps[name] = step
    print("%-26s rank %s  head rows %d" % (name, getattr(m.func, "rank", "-"), sum(q.shape[0] for k, q in m.func.named_parameters()
                                                                                    if k.endswith("weight") and not k.startswith("net_to_hh"))), flush=True)
times = {name: [] for name, _ in VARIANTS}
for r in range(ROUNDS):
    for name, _ in VARIANTS:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            loss = steps[name]()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / STEPS
        times[name].append(dt)
        print("round %d  %-26s %8.2f ms/step  %.3e sample-steps/s  loss %.4f" % (r, name, dt * 1e3, B * (T - 1) / dt, float(loss)), flush=True)
for name, _ in VARIANTS:
    v = times[name]
    print("median   %-26s %8.2f ms/step  (min %.2f, max %.2f over %d rounds of %d steps; B %d, T %d, sparsity %g)"
          % (name, statistics.median(v) * 1e3, min(v) * 1e3, max(v) * 1e3, ROUNDS, STEPS, B, T, SPARSITY), flush=True)
