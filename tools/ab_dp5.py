"""A/B of dopri5 training-step time between library builds on ONE box: python tools/ab_dp5.py variants/a.so [variants/b.so ...]
(the shipped library first).  Same seeds, same data: the step sequences are identical wherever the builds compute the same numbers.

    python tools/ab_dp5.py --rounds 3 --out times.json variants/parent/libncde_hip.so

--rounds N: the FIRST library given is the yardstick (A), the shipped one is B; they run alternately, each round in child processes of
their own.  The rule of tools/family_bits.py --time: each B median must lie within max(A's own min-max spread over its rounds, 3 %) of
A's median; exit 1 otherwise.  --out: every run, the medians and the spreads as JSON."""
import json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import os, sys, time, torch
sys.path.insert(0, %r)
from ncde_amd import _lib
if sys.argv[1] != "-": _lib.LIB_PATH = os.path.join(%r, sys.argv[1])
import bench, ncde_amd
c = dict(bench.CONFIGS["cfg2"])
coeffs = bench.make_inputs(c, 4096, 0, torch.device("cuda", 0))
torch.manual_seed(1)
y = (torch.rand(4096, 1, device="cuda") > 0.5).float()
for adjoint in (True, False):
    torch.manual_seed(0)
    m = ncde_amd.NeuralCDE(c["C"], c["H"], 1, hidden_hidden_dim=c["HH"], num_layers=c["nl"], interpolation="rectilinear", solver="dopri5", adjoint=adjoint).cuda()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    lf = torch.nn.BCEWithLogitsLoss()
    def step():
        opt.zero_grad(set_to_none=True); l = lf(m(coeffs), y); l.backward(); opt.step(); return l
    step(); torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(4): step()
    torch.cuda.synchronize()
    print("%%-22s adjoint=%%-5s %%7.1f ms/step  nfe %%d" %% (sys.argv[1], adjoint, (time.perf_counter() - t0) / 4 * 1e3, m.func.nfe), flush=True)
''' % (ROOT, ROOT)


def child(lib):
    """-> {"adjoint=True": ms, "adjoint=False": ms} or None (a failed child: nothing more is started on the GPU)"""
    q = subprocess.run([sys.executable, "-c", CHILD, lib], capture_output=True, text=True, timeout=600)
    sys.stdout.write(q.stdout)
    sys.stdout.flush()
    if q.returncode != 0:
        sys.stderr.write(q.stderr[-4000:])
        return None
    return {ln.split()[1]: float(ln.split()[2]) for ln in q.stdout.splitlines() if " ms/step" in ln}


def rounds(lib_a, n, out_path):
    runs = {"A": [], "B": []}
    for _ in range(n):
        for side, lib in (("A", lib_a), ("B", "-")):
            r = child(lib)
            if r is None:
                return 1
            runs[side].append(r)
    report, bad = {"lib_A": lib_a, "lib_B": "the tree's own", "runs_ms_per_step": runs, "legs": {}}, 0
    for leg in runs["A"][0]:
        a, b = [r[leg] for r in runs["A"]], [r[leg] for r in runs["B"]]
        ma, mb = statistics.median(a), statistics.median(b)
        margin = max((max(a) - min(a)) / ma, 0.03)
        ok = abs(mb - ma) / ma <= margin
        bad += not ok
        report["legs"][leg] = {"A_median": ma, "B_median": mb, "A_spread": (max(a) - min(a)) / ma, "B_spread": (max(b) - min(b)) / mb,
                               "margin": margin, "B_over_A": mb / ma, "within_margin": bool(ok)}
        print("%-14s A %.1f ms  B %.1f ms  B/A %.4f  margin %.3f  %s" % (leg, ma, mb, mb / ma, margin, "ok" if ok else "OUTSIDE"))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    return 1 if bad else 0


if __name__ == "__main__":
    args, n, out = sys.argv[1:], 0, None
    while args and args[0] in ("--rounds", "--out"):
        if args[0] == "--rounds":
            n = int(args[1])
        else:
            out = args[1]
        args = args[2:]
    if n:
        sys.exit(rounds(args[0], n, out))
    for lib in ["-"] + args:
        if child(lib) is None:
            sys.exit(1)
