#!/usr/bin/env python3
"""Dispatch table of the C-ABI's query functions over a fixed grid of problems (CPU only: nothing is launched).

One line per (problem, flags, pass): ncde_kernel_name, ncde_workspace_bytes, ncde_coop_status_offset, and the status code /
ncde_last_error_string() of each query that fails.  Two libraries dispatch identically iff their tables are byte-identical:

    python tools/dispatch_table.py --lib old/libncde_hip.so --out old.txt
    python tools/dispatch_table.py --out new.txt && cmp old.txt new.txt

`--fixture FILE` writes the reduced table tests/test_host_cpu.py replays (tests/golden/dispatch_table.json): for every distinct
(kernel name, error texts) of the full grid its first occurrences.  Generate it from the library the change is measured
AGAINST, never from the code under test.

`--dopri5` walks the adaptive solver's queries instead (DP_POINTS x interpolation x knot grid x n_t x batch): ncde_dopri5_kernel_name and
ncde_dopri5_workspace_bytes of the passes 0 / 1 / 2 and ncde_dopri5_record_bytes over DP_RECORD_OPTIONS, each with its status / error
text.  That grid is small: its fixture (tests/golden/dispatch_table_dopri5.json) is the whole table.
"""
import argparse
import ctypes
import hashlib
import importlib.util
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("_ncde_lib_binding", os.path.join(ROOT, "online-neural-cdes_amd", "_lib.py"))
_lib = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_lib)

FLAG_DEBUG_PROFILE, FLAG_CHAIN_DUMP = 0x100, 0x200      # (0x200: the internal chain-dump switch of the development adjoint kernels)
FLAGS = [
    ("none", 0), ("FORCE_GENERIC", _lib.FLAG_FORCE_GENERIC), ("FORCE_FAST", _lib.FLAG_FORCE_FAST), ("FORCE_TILED", _lib.FLAG_FORCE_TILED),
    ("FP32_MFMA", _lib.FLAG_FP32_MFMA), ("SPLIT_BF16", _lib.FLAG_SPLIT_BF16), ("ADJOINT_V1", _lib.FLAG_ADJOINT_V1),
    ("ADJOINT_V2", _lib.FLAG_ADJOINT_V2), ("ADJOINT_V4", _lib.FLAG_ADJOINT_V4), ("ADJOINT_SPLIT_FP16", _lib.FLAG_ADJOINT_SPLIT_FP16),
    ("DEBUG_PROFILE", FLAG_DEBUG_PROFILE), ("0x200", FLAG_CHAIN_DUMP), ("TILED_NS2", _lib.FLAG_TILED_NS2), ("NO_COOP", _lib.FLAG_NO_COOP),
    ("SPLIT_BF16|V4", _lib.FLAG_SPLIT_BF16 | _lib.FLAG_ADJOINT_V4), ("DEBUG_PROFILE|V2", FLAG_DEBUG_PROFILE | _lib.FLAG_ADJOINT_V2),
]
CHANNELS = [1, 4, 5, 8, 12, 13, 20, 21, 40, 41]
WIDTHS = [(32, 32), (32, 15), (16, 24), (64, 64), (48, 64), (33, 32), (128, 128)]
LAYERS = [(1, 1), (2, 1), (3, 1), (3, 0), (4, 1), (4, 0), (5, 1), (5, 0)]      # (n_layers, inner layers share one matrix): the same below 3
BATCHES = [16, 100, 8192]
KEYS = ("C", "H", "HH", "nl", "shared", "interp", "method", "output", "field", "B", "flags", "pass")
N_KNOTS = 49


def cases():
    """The grid, as dicts over KEYS.  A piecewise-quintic control (interp 2) never runs on a register-resident set, so it is walked
    with the flags that route around or onto those sets only."""
    quintic_flags = {"none", "FORCE_GENERIC", "FORCE_FAST", "FORCE_TILED"}
    for C, (H, HH), (nl, shared), interp, method, output, field, B in itertools.product(
            CHANNELS, WIDTHS, LAYERS, (0, 1, 2), (0, 1, 2), (0, 1, 2), (0, 1), BATCHES):
        for fname, flags in FLAGS:
            if interp == 2 and fname not in quintic_flags:
                continue
            for k in (0, 1, 2):
                yield dict(zip(KEYS, (C, H, HH, nl, shared, interp, method, output, field, B, flags, k)))


def build_problem(c):
    """A structurally valid problem with dummy (never dereferenced) device pointers."""
    p = _lib.NcdeProblem()
    p.abi_version = _lib.NCDE_ABI_VERSION
    p.batch, p.n_knots, p.channels, p.hidden = c["B"], N_KNOTS, c["C"], c["H"]
    p.interp, p.method, p.output, p.flags = c["interp"], c["method"], c["output"], c["flags"]
    p.n_layers = c["nl"]
    for l in range(c["nl"]):
        p.layer_in[l], p.layer_out[l] = (c["H"] if l == 0 else c["HH"]), c["HH"]
        slot = l if not c["shared"] else min(l, 1)
        p.layer_W[l], p.layer_b[l] = 0x10000 * (slot + 1), 0x10000 * (slot + 1) + 0x8000
    p.Wo, p.bo, p.coeffs, p.z0 = 0x300000, 0x310000, 0x400000, 0x500000
    p.coeffs_stride_b, p.coeffs_stride_t = N_KNOTS * 6 * c["C"], 6 * c["C"]
    if c["field"] == 1:      # minimal-gated field
        p.field_kind, p.Wg, p.bg = 1, 0x600000, 0x610000
    if c["output"] == _lib.OUT_TIMES:
        p.time_plan, p.n_t_out, p.n_steps_fwd, p.n_steps_adj = 0x900000, 5, 12, 14
    return p


# ---- the adaptive solver's queries ----------------------------------------------------------------------------------------------------
DP_KEYS = ("point", "C", "H", "HH", "nl", "tie", "field", "input", "flags", "interp", "user_knots", "n_t", "B")
DP_FIELDS = tuple("%s%d%s" % (q, k, e) for q in ("name", "workspace_bytes") for k in (0, 1, 2) for e in ("", "_error")) + \
    tuple("record_bytes_%d%s" % (i, e) for i in range(4) for e in ("", "_error"))
DP_RECORD_OPTIONS = [(0.0, 0), (0.125, 0), (0.0, 50), (0.125, 50)]      # (min_step, max_num_steps)
DP_KNOTS = 9
DP_USER_KNOTS = (0.25, 0.75, 2.0, 2.75, 4.75, 5.25, 6.0, 7.25, 9.25)
# tie: "inner" = one matrix for every layer but the first (the reference's stack), "none" = all distinct, "1=2" / "1=0" = only that pair
DP_POINTS = [      # (name, C, H, HH, nl, tie, field kind, field input, flags)
    ("h32_nl1", 20, 32, 32, 1, "inner", 0, 0, 0), ("h32_nl2", 20, 32, 32, 2, "inner", 0, 0, 0), ("h32_nl3", 20, 32, 32, 3, "inner", 0, 0, 0),
    ("h32_nl4", 20, 32, 32, 4, "inner", 0, 0, 0), ("h32_pad_nl1", 5, 16, 24, 1, "inner", 0, 0, 0), ("h32_pad_nl2", 6, 24, 32, 2, "inner", 0, 0, 0),
    ("h64", 4, 64, 64, 3, "inner", 0, 0, 0), ("h64_pad", 3, 48, 64, 2, "inner", 0, 0, 0), ("h40", 7, 40, 40, 2, "inner", 0, 0, 0),
    ("h32_generic", 20, 32, 32, 3, "inner", 0, 0, _lib.FLAG_FORCE_GENERIC),
    ("adjoint_lds", 80, 128, 512, 2, "inner", 0, 0, 0),       # beyond the adjoint's LDS
    ("hidden_144", 4, 144, 64, 2, "inner", 0, 0, 0),          # hidden > 128: refused by the taped sweep
    ("last_160", 4, 32, 160, 2, "inner", 0, 0, 0),            # last width > 128
    ("gated", 20, 32, 32, 3, "inner", 1, 0, 0), ("evaluate", 20, 32, 32, 3, "inner", 0, 1, 0),      # both refused
    ("tie_1=2", 20, 32, 32, 4, "1=2", 0, 0, 0), ("tie_1=0", 20, 32, 32, 3, "1=0", 0, 0, 0), ("tie_none", 20, 32, 32, 3, "none", 0, 0, 0),
]


def dp_cases():
    for pt, interp, user, n_t, B in itertools.product(DP_POINTS, (0, 1), (0, 1), (2, 5), (1, 21, 4096)):
        yield dict(zip(DP_KEYS, pt + (interp, user, n_t, B)))


def dp_problem(c):
    p = _lib.NcdeProblem()
    p.abi_version = _lib.NCDE_ABI_VERSION
    p.batch, p.n_knots, p.channels, p.hidden = c["B"], DP_KNOTS, c["C"], c["H"]
    p.interp, p.method, p.output, p.flags = c["interp"], 0, _lib.OUT_INTERVAL, c["flags"]
    p.n_layers = c["nl"]
    slots = {"inner": lambda l: min(l, 1), "none": lambda l: l, "1=2": lambda l: 1 if l == 2 else l, "1=0": lambda l: 0 if l == 1 else l}[c["tie"]]
    for l in range(c["nl"]):
        d_in = (c["H"] + c["C"] if c["input"] == 1 else c["H"]) if l == 0 else c["HH"]
        p.layer_in[l], p.layer_out[l] = d_in, c["HH"]
        p.layer_W[l], p.layer_b[l] = 0x10000 * (slots(l) + 1), 0x10000 * (slots(l) + 1) + 0x8000
    p.Wo, p.bo, p.coeffs, p.z0 = 0x300000, 0x310000, 0x400000, 0x500000
    parts = 1 if c["interp"] == 0 else 4
    p.coeffs_stride_b, p.coeffs_stride_t = DP_KNOTS * parts * c["C"], parts * c["C"]
    p.field_kind, p.field_input = c["field"], c["input"]
    if c["field"] == 1:
        p.Wg, p.bg = 0x600000, 0x610000
    return p


def dp_load(path):
    h = load(path)
    P, TS, AO = ctypes.POINTER(_lib.NcdeProblem), ctypes.POINTER(_lib.NcdeTimeSpec), ctypes.POINTER(_lib.NcdeAdaptiveOptions)
    h.ncde_dopri5_kernel_name.argtypes, h.ncde_dopri5_kernel_name.restype = [P, ctypes.c_int], ctypes.c_char_p
    h.ncde_dopri5_workspace_bytes.argtypes, h.ncde_dopri5_workspace_bytes.restype = [P, TS, ctypes.c_int], ctypes.c_int64
    h.ncde_dopri5_record_bytes.argtypes, h.ncde_dopri5_record_bytes.restype = [P, TS, AO], ctypes.c_int64
    return h


def dp_query(h, c):
    """The values of DP_FIELDS: per query its result (None / a negative status where it fails) and, where it fails, the error text."""
    p = ctypes.byref(dp_problem(c))
    kn = DP_USER_KNOTS if c["user_knots"] else tuple(float(k) for k in range(DP_KNOTS))
    n_t = c["n_t"]
    t = (ctypes.c_double * n_t)(*[kn[0] + (kn[-1] - kn[0]) * i / (n_t - 1) for i in range(n_t)])
    knots = (ctypes.c_double * DP_KNOTS)(*kn)
    ts = _lib.NcdeTimeSpec()
    ts.n_t, ts.time_is_f64, ts.t = n_t, 1, t
    if c["user_knots"]:
        ts.knots = knots
    calls = [lambda k=k: h.ncde_dopri5_kernel_name(p, k) for k in (0, 1, 2)]
    calls += [lambda k=k: h.ncde_dopri5_workspace_bytes(p, ctypes.byref(ts), k) for k in (0, 1, 2)]
    for min_step, max_num_steps in DP_RECORD_OPTIONS:
        o = _lib.NcdeAdaptiveOptions()
        o.rtol, o.atol, o.min_step, o.max_num_steps = 1e-3, 1e-5, min_step, max_num_steps
        calls.append(lambda o=o: h.ncde_dopri5_record_bytes(p, ctypes.byref(ts), ctypes.byref(o)))
    out = []
    for fn in calls:
        h.ncde_num_outputs(None)      # a known error text in front of every query (see query)
        r = fn()
        failed = r is None or (not isinstance(r, bytes) and r < 0)
        out += [r.decode() if isinstance(r, bytes) else r, h.ncde_last_error_string().decode() if failed else ""]
    return out


def dp_main(a):
    h = dp_load(a.lib)
    rows = [[c[k] for k in DP_KEYS] + dp_query(h, c) for c in dp_cases()]
    text = "".join(" ".join("%s=%s" % kv for kv in zip(DP_KEYS, r)) + " | " + " | ".join(str(x) for x in r[len(DP_KEYS):]) + "\n" for r in rows)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    if a.fixture:
        with open(a.fixture, "w") as f:
            f.write('{"keys": %s,\n "fields": %s,\n "rows": [\n' % (json.dumps(list(DP_KEYS)), json.dumps(list(DP_FIELDS))))
            f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in rows))
            f.write("\n]}\n")
    print(json.dumps({"lines": len(rows), "sha256": hashlib.sha256(text.encode()).hexdigest(), "fixture_rows": len(rows) if a.fixture else 0}))


def load(path):
    h = ctypes.CDLL(path)
    P = ctypes.POINTER(_lib.NcdeProblem)
    h.ncde_last_error_string.restype = ctypes.c_char_p
    h.ncde_num_outputs.argtypes, h.ncde_num_outputs.restype = [P], ctypes.c_int
    h.ncde_kernel_name.argtypes, h.ncde_kernel_name.restype = [P, ctypes.c_int], ctypes.c_char_p
    h.ncde_workspace_bytes.argtypes, h.ncde_workspace_bytes.restype = [P, ctypes.c_int], ctypes.c_int64
    h.ncde_coop_status_offset.argtypes, h.ncde_coop_status_offset.restype = [P, ctypes.c_int], ctypes.c_int64
    return h


def query(h, c):
    """[kernel name | None, its error text, workspace bytes | status, its error text, status offset | status, its error text]"""
    p, k = ctypes.byref(build_problem(c)), c["pass"]
    out = []
    for fn in (h.ncde_kernel_name, h.ncde_workspace_bytes, h.ncde_coop_status_offset):
        h.ncde_num_outputs(None)      # a known error text in front of every query: one that fails silently shows it, not an older one
        r = fn(p, k)
        failed = r is None or (not isinstance(r, bytes) and r < 0)
        out += [r.decode() if isinstance(r, bytes) else r, h.ncde_last_error_string().decode() if failed else ""]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", default=os.path.join(ROOT, "online-neural-cdes_amd", "libncde_hip.so"))
    ap.add_argument("--out", help="write the full table here (default: only its line count and SHA-256 are printed)")
    ap.add_argument("--fixture", help="write the reduced table (JSON) here")
    ap.add_argument("--per-key", type=int, default=2, help="occurrences kept per distinct (name, error texts) in the fixture")
    ap.add_argument("--dopri5", action="store_true", help="the adaptive solver's queries instead (see above)")
    a = ap.parse_args()
    if a.dopri5:
        return dp_main(a)
    h = load(a.lib)
    out = open(a.out, "w") if a.out else None
    sha, n, seen, rows = hashlib.sha256(), 0, {}, []
    for c in cases():
        r = query(h, c)
        line = " ".join("%s=%s" % (k, c[k]) for k in KEYS) + " | " + " | ".join(str(x) for x in r) + "\n"
        sha.update(line.encode())
        n += 1
        if out:
            out.write(line)
        key = (r[0], r[1], r[3], r[5])
        if a.fixture and seen.get(key, 0) < a.per_key:
            seen[key] = seen.get(key, 0) + 1
            rows.append([c[k] for k in KEYS] + r)
    if out:
        out.close()
    if a.fixture:
        with open(a.fixture, "w") as f:
            f.write('{"keys": %s,\n "fields": ["name", "name_error", "workspace_bytes", "workspace_error", "coop_status_offset", "coop_error"],\n "rows": [\n'
                    % json.dumps(list(KEYS)))
            f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in rows))
            f.write("\n]}\n")
    print(json.dumps({"lines": n, "sha256": sha.hexdigest(), "fixture_rows": len(rows), "distinct": len(seen)}))


if __name__ == "__main__":
    sys.exit(main())
