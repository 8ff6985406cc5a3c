#!/usr/bin/env python3
"""Bits of the ten online step kernels (csrc/ncde_stream.hip) through the C-ABI: the check to run after moving their text.  The
library is built with -ffp-contract=off, so moved arithmetic must give EQUAL bits, with no tolerance.  One library per process (one
ctypes handle); --out runs on the GPU box, --compare on the CPU.

    python tools/stream_bits.py --lib old/libncde_hip.so --out old.npz      # a fixed grid; every output row and the final state is stored
    python tools/stream_bits.py --out new.npz
    python tools/stream_bits.py --compare old.npz new.npz [--summary FILE]  # exit 1 at the first differing array, named

The grid: B 19 (two tiles, the second with 3 streams), C 5, H 10, widths [12, 12] (nothing a multiple of 4 or 16); 7 rows with NaNs,
one of them in a first row; an `active` mask with one stream that never receives a row and one whose first row arrives in the middle
of a launch; rows 0 .. 3 fed as single-row calls, rows 4 .. 6 as one call of 3 rows; euler, midpoint, rk4.  The plain step on a linear
and on a rectilinear stream (time_index = the last channel), the Hermite step, the hybrid step (sparse channels {2, 4}; at row 3 no
stream takes piece B, at row 4 only the odd streams do); the field step for its five (field, input) pairs on linear, rectilinear and
Hermite and for the matmul / derivative inputs on hybrid; the low-rank step with R = 2 on all four paths; stacks of 2 and 3 layers,
H 10 -> 6 -> 12 (narrow after wide, wide after narrow).  Stored per case: `out` and `z_out` of every row, and z, last_row, prev_dx,
count after the last call.  The kernel names the queries answer are stored and compared as well.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

B, C, H, WIDTHS, R, ROWS, N_OUT = 19, 5, 10, (12, 12), 2, 7, 3
CALLS = ((0, 1), (1, 1), (2, 1), (3, 1), (4, 3))      # (first row, rows) of every launch
NEVER, LATE = 5, 7                                    # the stream without a row; the one whose first row is row 5, inside the last launch
SPARSE = (2, 4)
STACK_H = (10, 6, 12)
METHODS = ("euler", "midpoint", "rk4")
FIELD_PAIRS = (("minimal", "matmul"), ("original", "evaluate"), ("original", "derivative"), ("minimal", "evaluate"), ("minimal", "derivative"))
PATHS = {  # name: (interp, rectilinear, time_index, hybrid)
    "linear": ("linear", 0, 0, False), "rectilinear": ("linear", 1, C - 1, False), "hermite": ("cubic", 0, 0, False), "hybrid": ("linear", 0, 0, True)}
SUFFIX = {("step", "linear"): "", ("step", "rectilinear"): "", ("step", "hermite"): "_hermite", ("step", "hybrid"): "_hybrid",
          ("field", "linear"): "_field", ("field", "rectilinear"): "_field", ("field", "hermite"): "_field_hermite", ("field", "hybrid"): "_field_hybrid",
          ("lowrank", "linear"): "_lowrank", ("lowrank", "rectilinear"): "_lowrank", ("lowrank", "hermite"): "_lowrank",
          ("lowrank", "hybrid"): "_lowrank_hybrid"}


def cases():
    """-> [(name, family, kind, mode, path)]"""
    out = [("step/%s" % p, "step", "original", "matmul", p) for p in PATHS]
    for kind, mode in FIELD_PAIRS:
        out += [("field-%s-%s/%s" % (kind, mode, p), "field", kind, mode, p) for p in PATHS if not (p == "hybrid" and mode == "evaluate")]
    out += [("lowrank/%s" % p, "lowrank", "lowrank", "matmul", p) for p in PATHS]
    return out


def make_rows(gen):
    """x [ROWS, B, C] with time in channel 0 (strictly increasing per stream, never NaN) and the mask [ROWS, B] uint8"""
    import torch
    x = torch.randn(ROWS, B, C, generator=gen)
    x[:, :, 0] = torch.arange(ROWS, dtype=torch.float32)[:, None] + 0.25 * torch.rand(ROWS, B, generator=gen)
    nan = torch.rand(ROWS, B, C, generator=gen) < 0.25
    nan[0, 1, 2] = nan[5, LATE, 3] = True      # in a first row: of a launch-0 stream, and of the stream that starts mid-launch
    nan[3][:, list(SPARSE)] = True             # no sparse channel changes at row 3; at row 4 only those of the odd streams
    nan[4, 0::2, SPARSE[0]] = nan[4, 0::2, SPARSE[1]] = True
    nan[4, 1::2, SPARSE[0]] = False
    nan[:, :, 0] = False
    x[nan] = float("nan")
    act = (torch.rand(ROWS, B, generator=gen) < 0.85).to(torch.uint8)
    act[0], act[4] = 1, 1
    act[:, NEVER] = 0
    act[:5, LATE], act[5:, LATE] = 0, 1
    return x, act


def make_problem(_lib, spec, Cn, Hn, interp, method):
    p = _lib.NcdeProblem()
    p.abi_version = _lib.NCDE_ABI_VERSION
    p.batch, p.hidden, p.channels, p.n_knots = B, Hn, Cn, 2
    p.interp, p.method, p.output, p.flags = _lib.INTERP[interp], _lib.METHOD[method], _lib.OUT_KNOTS, 0
    p.n_layers = len(spec.layers)
    for i, (w, b) in enumerate(spec.layers):
        p.layer_out[i], p.layer_in[i] = w.shape
        p.layer_W[i], p.layer_b[i] = w.data_ptr(), b.data_ptr()
    p.Wo, p.bo = spec.Wo.data_ptr(), spec.bo.data_ptr()
    p.field_kind, p.field_input = _lib.FIELD_KIND[spec.kind], _lib.FIELD_INPUT[spec.mode]
    if spec.kind != "original":
        p.Wg, p.bg = spec.Wg.data_ptr(), spec.bg.data_ptr()
    if spec.kind == "lowrank":
        p.flags = _lib.FLAG_FIELD_RANK(spec.rank)
    return p


class Layer:
    """the state, the readout weights and the output buffers of one CDE"""

    def __init__(self, gen, Cn, Hn, dev, readout):
        import torch
        self.z = (torch.randn(B, Hn, generator=gen) * 0.5).to(dev)
        self.last, self.pdx = torch.zeros(B, Cn, device=dev), torch.zeros(B, Cn, device=dev)
        self.count = torch.zeros(B, dtype=torch.int32, device=dev)
        self.Wf = (torch.randn(N_OUT, Hn, generator=gen) / Hn ** 0.5).to(dev) if readout else None
        self.bf = torch.randn(N_OUT, generator=gen).to(dev) if readout else None
        self.out = torch.full((ROWS, B, N_OUT), float("nan"), device=dev) if readout else None
        self.z_out = torch.full((ROWS, B, Hn), float("nan"), device=dev)

    def stream(self, _lib, r0, m):
        s = _lib.NcdeStream()
        s.n_rows = m
        s.z, s.last_row, s.prev_dx, s.count = self.z.data_ptr(), self.last.data_ptr(), self.pdx.data_ptr(), self.count.data_ptr()
        s.z_out = self.z_out[r0:].data_ptr()
        if self.Wf is not None:
            s.n_out, s.Wf, s.bf, s.out = N_OUT, self.Wf.data_ptr(), self.bf.data_ptr(), self.out[r0:].data_ptr()
        return s

    def store(self, store, key):
        for name in ("out", "z_out", "z", "last", "pdx", "count"):
            if getattr(self, name) is not None:
                store["%s/%s" % (key, name)] = getattr(self, name).cpu().numpy()


def feed(s, x, act, r0, path):
    _, s.rectilinear, s.time_index, _ = PATHS[path]
    s.x, s.x_stride_m, s.x_stride_b = x[r0:].data_ptr(), x.stride(0), x.stride(1)
    s.active, s.initial_value_if_nan = act[r0:].data_ptr(), 0.5


def run_grid(out_path):
    import torch
    from family_bits import make_field
    from ncde_amd import _lib
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    gen = torch.Generator().manual_seed(4321)
    x, act = make_rows(gen)
    x_last = torch.roll(x, -1, dims=2).contiguous().to(dev)      # rectilinear: time in the last channel
    x, act = x.to(dev), act.to(dev)
    rmask = torch.zeros(C, dtype=torch.uint8)
    rmask[list(SPARSE)] = 1
    rmask = rmask.to(dev)
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731
    store, names = {}, {}
    for ci, (name, family, kind, mode, path) in enumerate(cases()):
        spec, _ = make_field(kind, mode, C, H, WIDTHS, R, 200 + ci, dev)
        suffix = SUFFIX[family, path]
        for method in METHODS:
            key = "%s/%s" % (name, method)
            p = make_problem(_lib, spec, C, H, PATHS[path][0], method)
            kn = getattr(lib, "ncde_stream%s_kernel_name" % suffix)(ctypes.byref(p))
            assert kn, "%s: %s" % (key, lib.ncde_last_error_string().decode())
            names[key] = kn.decode()
            layer = Layer(torch.Generator().manual_seed(300 + ci), C, H, dev, True)
            for r0, m in CALLS:
                s = layer.stream(_lib, r0, m)
                feed(s, x_last if path == "rectilinear" else x, act, r0, path)
                extra = (ctypes.c_void_p(rmask.data_ptr()),) if path == "hybrid" else ()
                _lib.check(getattr(lib, "ncde_stream_step%s" % suffix)(ctypes.byref(p), ctypes.byref(s), *extra, stream()), key)
            torch.cuda.synchronize()
            layer.store(store, key)
    P, S = ctypes.POINTER(_lib.NcdeProblem), ctypes.POINTER(_lib.NcdeStream)
    for n_stack in (2, 3):
        dims = [(C if i == 0 else STACK_H[i - 1], STACK_H[i]) for i in range(n_stack)]
        specs = [make_field("original", "matmul", c, h, WIDTHS, 0, 400 + 10 * n_stack + i, dev)[0] for i, (c, h) in enumerate(dims)]
        for method in METHODS:
            key = "stack%d/%s" % (n_stack, method)
            ps = [make_problem(_lib, specs[i], c, h, "linear", method) for i, (c, h) in enumerate(dims)]
            pp = (P * n_stack)(*[ctypes.pointer(q) for q in ps])
            kn = lib.ncde_stream_stack_kernel_name(pp, n_stack)
            assert kn, "%s: %s" % (key, lib.ncde_last_error_string().decode())
            names[key] = kn.decode()
            layers = [Layer(torch.Generator().manual_seed(500 + i), c, h, dev, i == n_stack - 1) for i, (c, h) in enumerate(dims)]
            for r0, m in CALLS:
                ss = [layer.stream(_lib, r0, m) for layer in layers]
                feed(ss[0], x, act, r0, "linear")
                sp = (S * n_stack)(*[ctypes.pointer(s) for s in ss])
                _lib.check(lib.ncde_stream_stack_step(pp, sp, n_stack, stream()), key)
            torch.cuda.synchronize()
            for i, layer in enumerate(layers):
                layer.store(store, "%s/layer%d" % (key, i))
    store["kernel_names"] = np.array(json.dumps(names, sort_keys=True))
    np.savez(out_path, **store)
    print("%d arrays of %d cases -> %s" % (len(store) - 1, len(names), out_path))


def compare(a_path, b_path, summary):
    a, b = np.load(a_path), np.load(b_path)
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
        nan += int(x.dtype.kind == "f" and np.isnan(x).any())
    lines = ["%d arrays compared (A = %s, B = %s): all equal bit for bit; %d of them hold a NaN (an element no kernel wrote)"
             % (n, os.path.basename(a_path), os.path.basename(b_path), nan),
             "cases per kernel (the same names in A and B):"]
    for kern in sorted(set(na.values())):
        lines.append("  %-40s %d" % (kern, sum(v == kern for v in na.values())))
    txt = "\n".join(lines) + "\n"
    sys.stdout.write(txt)
    if summary:
        with open(summary, "w") as f:
            f.write(txt)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", help="the library to load (default: the tree's own)")
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A.npz", "B.npz"))
    ap.add_argument("--summary", help="--compare: also write the summary here")
    a = ap.parse_args()
    if a.compare:
        return compare(a.compare[0], a.compare[1], a.summary)
    from ncde_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    assert a.out, "--out FILE.npz"
    return run_grid(a.out)


if __name__ == "__main__":
    sys.exit(main())
