#!/usr/bin/env python3
"""Bits of the fused dopri5 kernels (ncde_dpf_fwd / ncde_dpf_adj + ncde_dpf_reduce / ncde_dpf_tape) through cdeint: the check to run
after moving their shared text (csrc/ncde_dp_fused_stage.h).  The sibling of tools/family_bits.py: the library is built with
-ffp-contract=off, so moved arithmetic must give EQUAL bits, with no tolerance.  One library per process; run on the GPU box.

    python tools/dopri5_bits.py --lib old/libncde_hip.so --out old.npz
    python tools/dopri5_bits.py --out new.npz
    python tools/dopri5_bits.py --compare old.npz new.npz [--summary FILE]      # CPU; exit 1 at the first differing array, named

The grid (tests/dopri5_cases.py): the shapes h32, h32_nl2 and h32_pad_nl1 -- the NL = 3, 2, 1 instantiations of the adjoint and of the
taped sweep, full and zero-padded --, the axes A, B, Cl, Cc with the variant `end` plus Cl-inside, B = 21 and, for h32, B = 1 and 50.
Every case is driven by its replay lists, so the step sequence is the same whatever the build.  Stored per case: the forward z, the
adaptive adjoint's dz0 and parameter gradients, the taped backward's dz0 and parameter gradients.  NOT covered: NcdeGrads has no field for
the adjoint's time component (vt -> gvt -> the partial's last entry; it only enters the error norm, which a replayed sequence ignores)
nor for the sweep's Tpart / D1part (with `first_step` given, as here, they reach no output): that arithmetic is compared by the code
objects' resource records and by reading, not by these bits.

--shapes all: also h32_nl4, h64, h64_pad, h40 and h32_generic (`end` on the four axes, B = 21) -- the per-launch stage kernels and the
un-fused taped sweep, i.e. every route of the host code.  PARTIAL: on h32-Cl-end-B21 and h32_generic-Cl-end-B21 the adaptive adjoint once
more with adjoint_params = (Wo, bo): the layer tensors get no destination, so they leave the error norm's segments and the final
scatter's alike (stored: dz0, dWo, dbo)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

SHAPES = ("h32", "h32_nl2", "h32_pad_nl1")
MORE_SHAPES = ("h32_nl4", "h64", "h64_pad", "h40", "h32_generic")
PARTIAL = ("h32-Cl-end-B21", "h32_generic-Cl-end-B21")


def case_ids(shapes=SHAPES):
    import dopri5_cases as dc
    ids = []
    for sh in shapes:
        for ax in dc.AXES:
            ids.append("%s-%s-end-B%d" % (sh, ax, dc.BATCH))
            if sh in SHAPES:
                ids += ["%s-%s-end-B%d" % (sh, ax, b) for b in dc.BATCH_EXTRA.get(sh, ())]
        if sh in SHAPES:
            ids.append("%s-Cl-inside-B%d" % (sh, dc.BATCH))
    return ids


def run_grid(out_path, shapes=SHAPES):
    import ctypes
    import torch
    import dopri5_cases as dc
    import gpu_util
    import ncde_amd
    from ncde_amd import _lib, solver
    store, names = {}, {}
    for cid in case_ids(shapes):
        a = dc.arrays(cid)
        coeffs = torch.from_numpy(a["coeffs"]).cuda()
        kn = None if a["knots"] is None else torch.from_numpy(a["knots"]).cuda()
        X = (ncde_amd.LinearInterpolation if a["interp"] == "linear" else ncde_amd.NaturalCubicSpline)(coeffs, t=kn)
        func = gpu_util.CaseField(a["params"], a["layers"], "cuda")
        prob = solver.build_problem(coeffs, a["interp"], torch.from_numpy(a["z0"]).cuda(), func.fused_spec(), "rk4", _lib.OUT_INTERVAL, a["flags"])
        names[cid] = [(_lib.lib().ncde_dopri5_kernel_name(ctypes.byref(prob), k) or b"?").decode() for k in (0, 1, 2)]
        assert all(k.startswith(w) for k, w in zip(names[cid], a["route"])), (cid, names[cid])
        for mode, adjoint in (("adjoint", True), ("taped", False)) + ((("partial", True),) if cid in PARTIAL else ()):
            func = gpu_util.CaseField(a["params"], a["layers"], "cuda")
            z0 = torch.from_numpy(a["z0"]).cuda().requires_grad_(True)
            kept = ["Wo", "bo"] if mode == "partial" else a["names"]
            more = {"adjoint_params": tuple(func.p[n] for n in kept)} if mode == "partial" else {}
            out = ncde_amd.cdeint(X, func, z0, torch.from_numpy(a["t"]).cuda(), adjoint=adjoint, method="dopri5", rtol=dc.RTOL, atol=dc.ATOL,
                                  kernel_flags=a["flags"], options={"first_step": a["fwd"][0][0], "_replay": a["fwd"]},
                                  adjoint_options={"first_step": a["bwd"][0][0], "_replay": a["bwd"]}, **more)
            (out * torch.from_numpy(a["grad_out"]).cuda()).sum().backward()
            torch.cuda.synchronize()
            store["%s/%s/z" % (cid, mode)] = out.detach().cpu().numpy()
            store["%s/%s/dz0" % (cid, mode)] = z0.grad.cpu().numpy()
            for n in kept:
                store["%s/%s/d%s" % (cid, mode, n)] = func.p[n].grad.cpu().numpy()
            assert all(func.p[n].grad is None for n in a["names"] if n not in kept), (cid, mode)
        print(cid, names[cid], flush=True)
    store["kernel_names"] = np.array(json.dumps(names, sort_keys=True))
    np.savez(out_path, **store)
    print("%d arrays of %d cases -> %s" % (len(store) - 1, len(names), out_path))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", help="the library to load (default: the tree's own)")
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A.npz", "B.npz"))
    ap.add_argument("--summary", help="--compare: also write the summary here")
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), help="shapes of tests/dopri5_cases.py to run, or `all` (default: the three fused ones)")
    a = ap.parse_args()
    if a.compare:
        import family_bits
        return family_bits.compare(a.compare[0], a.compare[1], a.summary)
    from ncde_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    assert a.out, "--out FILE.npz"
    return run_grid(a.out, SHAPES + MORE_SHAPES if a.shapes == ["all"] else tuple(a.shapes))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.exit(main())
