#!/usr/bin/env python3
"""Bits and kernel times of the three 16-sample-tile families (ncde_generic / ncde_variant / ncde_lowrank) through the C-ABI: the check
to run after moving their shared text (csrc/ncde_timeloop.h).  The library is built with -ffp-contract=off, so moved arithmetic must
give EQUAL bits, with no tolerance.  One library per process (one ctypes handle); run on the GPU box.

    python tools/family_bits.py --lib old/libncde_hip.so --out old.npz      # a fixed grid; every output tensor is stored
    python tools/family_bits.py --out new.npz
    python tools/family_bits.py --compare old.npz new.npz [--summary FILE]  # CPU; exit 1 at the first differing array, named

    python tools/family_bits.py --time --lib old/libncde_hip.so --other online-neural-cdes_amd/libncde_hip.so --out times.json

The grid: B 19 (two tiles, the second with 3 samples), T 7, C 3, H 10, widths [12, 12] (nothing a multiple of the tile); euler,
midpoint, rk4; a linear path on the default axis (interval and knots outputs), linear and cubic paths on a plan with step_size 0.5 and
output times on and off its grid; ncde_forward, ncde_forward_record (out + stage record), ncde_adjoint, ncde_backward (grad_z0 and every
parameter gradient); the original field on the generic kernels, the minimal- and GRU-gated fields and the original field with the
evaluate / derivative inputs on the variant kernels (all by NCDE_FLAG_FORCE_GENERIC), the low-rank field with R = 2.  A pass the host
refuses is printed and skipped.

--time: ncde_time_kernel of pass 0 and pass 1 at cfg2 dimensions (B 4096, T 399, C 20, H = HH = 32, three layers, rk4, rectilinear
path) for the generic family (by flag), the GRU-gated variant and the low-rank field (sparsity 0.9, R = 2); the two libraries run
ALTERNATELY, each round in a child process of its own, ROUNDS (default 3) rounds each.  Every other-library median must lie within
max(the first library's own min-max spread, 3 %) of the first library's median; exit 1 otherwise.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, T, C, H, WIDTHS, R = 19, 7, 3, 10, (12, 12), 2
METHODS = ("euler", "midpoint", "rk4")
AXES = (("linear", "interval"), ("linear", "knots"), ("linear", "times"), ("cubic", "times"))
T_OUT = (0.0, 0.5, 1.25, 1.3, 2.0, 3.3, 4.75, 6.0)       # plan step 0.5: rows on its grid, between grid points, two in one step
FIELDS = (  # name, kind, input mode, the family its kernels must belong to
    ("original", "original", "matmul", "generic"), ("minimal", "minimal", "matmul", "variant"), ("gru", "gru", "matmul", "variant"),
    ("evaluate", "original", "evaluate", "variant"), ("derivative", "original", "derivative", "variant"), ("lowrank", "lowrank", "matmul", "lowrank"))


def _uniform(gen, *shape):
    import torch
    fan_in = shape[-1] if len(shape) > 1 else shape[0]
    return ((torch.rand(*shape, generator=gen) * 2 - 1) / fan_in ** 0.5).float()


def make_field(kind, mode, Cc, Hh, widths, rank, seed, device, shared_inner=False):
    """-> (FieldSpec, {name: device tensor}) with seeded weights at torch's Linear scale"""
    import torch
    from ncde_amd import solver
    gen = torch.Generator().manual_seed(seed)
    d0 = Hh if mode == "matmul" else Hh + Cc
    p, layers, din = {}, [], d0
    for i, w in enumerate(widths):
        if shared_inner and i >= 2:
            layers.append(layers[1])
            continue
        p["W%d" % i], p["b%d" % i] = _uniform(gen, w, din), _uniform(gen, w)
        layers.append(("W%d" % i, "b%d" % i))
        din = w
    rows = Hh * Cc if mode == "matmul" else Hh
    rows_g = rows
    if kind == "lowrank":
        rows, rows_g = Hh * rank, rank * Cc
    p["Wo"], p["bo"] = _uniform(gen, rows, din), _uniform(gen, rows)
    if kind != "original":
        p["Wg"], p["bg"] = _uniform(gen, rows_g, din), _uniform(gen, rows_g)
    if kind == "gru":
        p["Wr"], p["br"] = _uniform(gen, d0, d0), _uniform(gen, d0)
    p = {k: v.to(device).contiguous() for k, v in p.items()}
    spec = solver.FieldSpec([(p[w], p[b]) for w, b in layers], p["Wo"], p["bo"], kind, mode, p.get("Wg"), p.get("bg"), p.get("Wr"), p.get("br"),
                            rank=rank if kind == "lowrank" else 0)
    return spec, p


def run_grid(out_path):
    import torch
    import ncde_amd
    from ncde_amd import _lib, solver
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    gen = torch.Generator().manual_seed(1234)
    coeffs = {"linear": torch.randn(B, T, C, generator=gen).to(dev), "cubic": (torch.randn(B, T - 1, 4 * C, generator=gen) * 0.5).to(dev)}
    z0 = (torch.randn(B, H, generator=gen) * 0.5).to(dev)
    store, names = {}, {}
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731
    for fi, (fname, kind, mode, family) in enumerate(FIELDS):
        spec, params = make_field(kind, mode, C, H, WIDTHS, R, 100 + fi, dev)
        flags = 0 if kind == "lowrank" else _lib.FLAG_FORCE_GENERIC
        for method in METHODS:
            for interp, axis in AXES:
                key = "%s/%s/%s-%s" % (fname, method, interp, axis)
                plan = None
                if axis == "times":
                    X = (ncde_amd.LinearInterpolation if interp == "linear" else ncde_amd.NaturalCubicSpline)(coeffs[interp])
                    plan = solver._time_plan(X, torch.tensor(T_OUT, dtype=torch.float32), method, 0.5, dev)
                output = _lib.OUT_KNOTS if axis == "knots" else _lib.OUT_INTERVAL
                p = solver.build_problem(coeffs[interp], interp, z0, spec, method, output, flags, plan)
                kn = [lib.ncde_kernel_name(ctypes.byref(p), k) for k in (0, 1, 2)]
                why = [None if n else lib.ncde_last_error_string().decode() for n in kn]
                kn = [n.decode() if n else None for n in kn]
                for k, n in enumerate(kn):
                    assert n is None or family in n, "%s pass %d runs on %s, not on the %s family" % (key, k, n, family)
                    if n is None:
                        print("REFUSED %s pass %d: %s" % (key, k, why[k]), flush=True)
                names[key] = kn
                n_out = solver._num_outputs(coeffs[interp], interp, output, plan)
                g = torch.Generator().manual_seed(77)
                gout = torch.randn(B, n_out, H, generator=g).to(dev)
                out = rec = None
                if kn[0]:
                    out = solver._alloc_out(z0, n_out).fill_(float("nan"))
                    solver._launch_forward(p, out, False, dev)
                    store[key + "/forward/out"] = out.cpu().numpy()
                    out2 = solver._alloc_out(z0, n_out).fill_(float("nan"))
                    rec = solver._launch_forward(p, out2, True, dev)
                    store[key + "/forward_record/out"] = out2.cpu().numpy()
                    store[key + "/forward_record/stages"] = rec.cpu().numpy()
                for k, call, src in ((1, "adjoint", out), (2, "backward", rec)):
                    if not kn[k] or src is None:
                        continue
                    bound = solver.bind_grads(spec, z0.shape, dev, fill=float("nan"))
                    ws = solver._workspace(p, k, dev)
                    fn = lib.ncde_adjoint if k == 1 else lib.ncde_backward
                    _lib.check(fn(ctypes.byref(p), src.data_ptr(), gout.data_ptr(), ctypes.byref(bound.g), ws.data_ptr(), ws.numel(), stream()),
                               "ncde_" + call)
                    torch.cuda.synchronize()
                    store["%s/%s/grad_z0" % (key, call)] = bound.grad_z0.cpu().numpy()
                    for name, q in params.items():
                        store["%s/%s/grad_%s" % (key, call, name)] = bound.of(q).cpu().numpy()
    store["kernel_names"] = np.array(json.dumps(names, sort_keys=True))
    np.savez(out_path, **store)
    print("%d arrays of %d cases -> %s" % (len(store) - 1, len(names), out_path))


def compare(a_path, b_path, summary):
    a, b = np.load(a_path), np.load(b_path)
    lines = []
    if sorted(a.files) != sorted(b.files):
        print("key sets differ: only in A %s, only in B %s" % (sorted(set(a.files) - set(b.files)), sorted(set(b.files) - set(a.files))))
        return 1
    na, nb = json.loads(str(a["kernel_names"])), json.loads(str(b["kernel_names"]))
    if na != nb:
        print("kernel names differ")
        return 1
    n = nan = 0
    for k in sorted(a.files):
        if k == "kernel_names":
            continue
        x, y = a[k], b[k]
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            bad = int((x.view(np.uint32) != y.view(np.uint32)).sum()) if x.shape == y.shape else -1
            print("DIFFERENT %s: %d of %d words" % (k, bad, x.size))
            return 1
        n += 1
        nan += int(np.isnan(x).any())
    lines.append("%d arrays compared (A = %s, B = %s): all equal bit for bit; %d of them hold a NaN (an element no kernel wrote)"
                 % (n, os.path.basename(a_path), os.path.basename(b_path), nan))
    lines.append("kernels per case (forward, adjoint, discrete backward), the same in A and B:")
    for k in sorted(na):
        lines.append("  %-36s %s" % (k, " | ".join(str(x) for x in na[k])))
    txt = "\n".join(lines) + "\n"
    sys.stdout.write(txt)
    if summary:
        with open(summary, "w") as f:
            f.write(txt)
    return 0


TIME_CASES = (("generic", "original", "matmul"), ("gru variant", "gru", "matmul"), ("low-rank", "lowrank", "matmul"))


def time_child(iters):
    """one round of one library: ms per launch of pass 0 and pass 1 of every TIME_CASES entry, as one JSON line"""
    import torch
    import bench
    from ncde_amd import _lib, solver
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    c = dict(bench.CONFIGS["cfg2"])
    coeffs = bench.make_inputs(c, 4096, 0, dev)
    Cc, Hh = coeffs.shape[2], c["H"]
    gen = torch.Generator().manual_seed(5)
    z0 = (torch.randn(coeffs.shape[0], Hh, generator=gen) * 0.5).to(dev)
    res = {}
    for name, kind, mode in TIME_CASES:
        spec, _ = make_field(kind, mode, Cc, Hh, (c["HH"],) * c["nl"], int(np.ceil(Cc * (1 - 0.9))), 9, dev, shared_inner=True)
        flags = 0 if kind == "lowrank" else _lib.FLAG_FORCE_GENERIC
        p = solver.build_problem(coeffs, "linear", z0, spec, "rk4", _lib.OUT_INTERVAL, flags)
        kn = [(lib.ncde_kernel_name(ctypes.byref(p), k) or b"?").decode() for k in (0, 1)]
        out = solver._alloc_out(z0, 2)
        solver._launch_forward(p, out, False, dev)          # z_out for pass 1, and the warm-up of pass 0
        gout = torch.randn(out.shape, generator=gen).to(dev) / out.shape[0]
        bound = solver.bind_grads(spec, z0.shape, dev)
        ms, t = ctypes.c_float(0), []
        for k in (0, 1):
            ws = solver._workspace(p, k, dev)
            args = (ctypes.byref(p), k, out.data_ptr(), gout.data_ptr() if k else None, ctypes.byref(bound.g) if k else None, ws.data_ptr(),
                    ws.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            if k:
                _lib.check(lib.ncde_time_kernel(*args, 1, ctypes.byref(ms)), "ncde_time_kernel")      # warm-up
            _lib.check(lib.ncde_time_kernel(*args, iters, ctypes.byref(ms)), "ncde_time_kernel")
            t.append(ms.value)
        res[name] = {"kernels": kn, "ms": t}
    print("TIMES " + json.dumps(res), flush=True)


def time_driver(lib_a, lib_b, rounds, iters, out_path):
    rows = {"A": [], "B": []}
    for r in range(rounds):
        for side, lib in (("A", lib_a), ("B", lib_b)):
            q = subprocess.run([sys.executable, os.path.abspath(__file__), "--time-child", "--lib", lib, "--iters", str(iters)],
                               capture_output=True, text=True, timeout=300)
            if q.returncode != 0:
                sys.stderr.write(q.stdout[-2000:] + q.stderr[-4000:])
                return 1          # (nothing more is started on the GPU after a failed child)
            rows[side].append(json.loads([ln for ln in q.stdout.splitlines() if ln.startswith("TIMES ")][0][6:]))
            print("round %d %s %s" % (r, side, json.dumps({k: v["ms"] for k, v in rows[side][-1].items()})), flush=True)
    report, bad = {"lib_A": os.path.relpath(lib_a, ROOT), "lib_B": os.path.relpath(lib_b, ROOT), "rounds": rows, "kernels": {}}, 0
    for name, _, _ in TIME_CASES:
        for k in (0, 1):
            a = [x[name]["ms"][k] for x in rows["A"]]
            b = [x[name]["ms"][k] for x in rows["B"]]
            ma, mb = statistics.median(a), statistics.median(b)
            margin = max((max(a) - min(a)) / ma, 0.03)
            ok = abs(mb - ma) / ma <= margin
            bad += not ok
            kern = rows["A"][0][name]["kernels"][k]
            report["kernels"]["%s pass %d" % (name, k)] = {"kernel": kern, "A_ms": a, "B_ms": b, "A_median": ma, "B_median": mb,
                                                           "A_spread": (max(a) - min(a)) / ma, "B_spread": (max(b) - min(b)) / mb,
                                                           "margin": margin, "B_over_A": mb / ma, "within_margin": bool(ok)}
            print("%-12s pass %d %-18s A %.3f ms  B %.3f ms  B/A %.4f  margin %.3f  %s" % (name, k, kern, ma, mb, mb / ma, margin, "ok" if ok else "OUTSIDE"))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", help="the library to load (default: the tree's own)")
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A.npz", "B.npz"))
    ap.add_argument("--summary", help="--compare: also write the summary here")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--other", help="--time: the second library")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--time-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.compare:
        return compare(a.compare[0], a.compare[1], a.summary)
    default = os.path.join(ROOT, "online-neural-cdes_amd", "libncde_hip.so")
    if a.time:
        return time_driver(os.path.abspath(a.lib or default), os.path.abspath(a.other or default), a.rounds, a.iters, a.out)
    from ncde_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    if a.time_child:
        return time_child(a.iters)
    assert a.out, "--out FILE.npz"
    return run_grid(a.out)


if __name__ == "__main__":
    sys.exit(main())
