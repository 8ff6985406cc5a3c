#!/usr/bin/env python
"""Is the device code of two builds of csrc/ the same?  The check to run after a "pure move" of kernel text.

    python tools/compare_code_objects.py OLD_CSRC NEW_CSRC      # two directories that `make` has been run in
    python tools/compare_code_objects.py OLD_CSRC NEW_CSRC --may-differ ncde_generic.o ncde_variant.o

For every object file of OLD_CSRC: the kernel symbols of its gfx950 code object must be the same set as in NEW_CSRC; every kernel must
disassemble to the same sequence of (mnemonic, operands) -- branch operands are relative, so nothing is normalised; and its resource
record (VGPRs, AGPRs, SGPRs, scratch bytes, static LDS bytes: the code object's metadata note) must be equal.  Prints one line per
object and every difference; exit status 1 if there is one.  The units named after --may-differ (the ones a change rewrites on
purpose) are compared and printed like the others, but their differences do not count.
"""
import glob
import os
import re
import shutil
import subprocess
import sys

from isa_census import LLVM, code_object, disassemble

RESOURCES = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def resources(obj):
    """{kernel symbol: {resource: value}} from the AMDGPU metadata note of the object's device code."""
    co = code_object(obj)
    txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    shutil.rmtree(os.path.dirname(co), ignore_errors=True)
    out = {}
    for block in txt.split("\n  - ")[1:]:      # one list item of amdhsa.kernels each; a kernel's own keys sit at the item's indent
        keys = dict(re.findall(r"^(?:    )?\.(\w+):\s+(\S+)$", block, re.M))
        if "name" in keys:                     # (the note's version list is made of such items too)
            out[keys["name"]] = {k: int(keys[k]) for k in RESOURCES}
    return out


def kernels(obj):
    """disassemble(obj); {} for an object of host code alone (no gfx950 bundle in it)"""
    try:
        return disassemble(obj)
    except RuntimeError:
        return {}


def compare(old, new):
    """-> (kernels compared, [difference, ...]) of one pair of object files"""
    a, b = kernels(old), kernels(new)
    diffs = ["only in %s: %s" % (side, s) for side, syms in (("OLD", set(a) - set(b)), ("NEW", set(b) - set(a))) for s in sorted(syms)]
    ra, rb = resources(old) if a else {}, resources(new) if b else {}
    for s in sorted(set(a) & set(b)):
        ia, ib = [i[1:] for i in a[s]], [i[1:] for i in b[s]]
        if ia != ib:
            first = next((k for k, (x, y) in enumerate(zip(ia, ib)) if x != y), min(len(ia), len(ib)))
            diffs.append("%s: instructions differ (%d / %d, first at index %d)" % (s, len(ia), len(ib), first))
        if ra.get(s) != rb.get(s):
            diffs.append("%s: resources %s / %s" % (s, ra.get(s), rb.get(s)))
    return len(set(a) & set(b)), diffs


def main():
    old_dir, new_dir = sys.argv[1:3]
    may_differ = set(sys.argv[4:]) if sys.argv[3:4] == ["--may-differ"] else set()
    assert may_differ or len(sys.argv) == 3, __doc__
    total = bad = 0
    for old in sorted(glob.glob(os.path.join(old_dir, "*.o"))):
        name = os.path.basename(old)
        new = os.path.join(new_dir, name)
        n, diffs = compare(old, new) if os.path.exists(new) else (0, ["object missing in NEW"])
        print("%-24s %4d kernels compared, %d differences%s" % (name, n, len(diffs), " (may differ)" if name in may_differ else ""))
        for d in diffs:
            print("    " + d)
        total += n
        bad += 0 if name in may_differ else len(diffs)
    missing = sorted(set(map(os.path.basename, glob.glob(os.path.join(new_dir, "*.o")))) - set(map(os.path.basename, glob.glob(os.path.join(old_dir, "*.o")))))
    for name in missing:
        print("%-24s only in NEW" % name)
    print("total: %d kernels compared, %d differences outside %s" % (total, bad + len(missing), sorted(may_differ) or "nothing"))
    return 1 if bad or missing else 0


if __name__ == "__main__":
    sys.exit(main())
