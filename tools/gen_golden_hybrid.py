"""Golden vectors for the causal control-path builders (tests/golden/g18_*.npz + MANIFEST_hybrid.json), produced by IMPORTING the
reference on the build machine -- the way tools/gen_golden_lowrank.py does, through oracle/gen_golden.py's shims (``autots`` stub).

    python tools/gen_golden_hybrid.py

Three kinds of case, every reference function called on CLONES of the stored input (the reference writes into its argument):
  hybrid        src/ncde/interpolation.py:_prepare_linear_rectilinear_hybrid(x, rectilinear_indices)
                x, rect (int64 list), out, lengths (kept rows per sample, read off the padded table: hybrid_ref.lengths_of)
  fill          torchcde.linear_interpolation_coeffs(x, rectilinear=..., initial_value_if_nan=..., forward_fill=...): the four combinations
                of the two options, plain and with rectilinear=0;  x, out;  meta holds the arguments
  forward_fill  torchcde.misc.forward_fill(x);  x, out (leading NaNs stay)
meta["nan_linear"] of a hybrid case: whether a linear channel holds a NaN (if none does, the whole table only copies values).
The generator also checks tests/hybrid_ref.py against every case it writes.
"""
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import gen_golden as gg  # noqa: E402  (sets up the reference's import path and the autots stub)
import hybrid_ref as hr  # noqa: E402
from src.ncde import interpolation as ref_interpolation  # noqa: E402
from torchcde import misc as ref_misc  # noqa: E402

torchcde, GOLD = gg.torchcde, gg.GOLD
NAN = float("nan")


def series(rng, B, L, n_lin, n_rect, p_lin, p_rect, levels=4):
    """Integer times, smooth linear channels with a share p_lin missing, rectilinear channels that hold few distinct levels (so that
    a new observation often repeats the value before it) with a share p_rect missing."""
    t = np.broadcast_to(np.arange(L, dtype=np.float32).reshape(1, L, 1), (B, L, 1))
    lin = np.cumsum(rng.standard_normal((B, L, n_lin)).astype(np.float32), axis=1)
    lin[rng.random(lin.shape) < p_lin] = NAN
    rect = rng.integers(0, levels, (B, L, n_rect)).astype(np.float32) / 2
    rect[rng.random(rect.shape) < p_rect] = NAN
    return np.ascontiguousarray(np.concatenate([t, lin, rect], axis=2), dtype=np.float32)


def hybrid_cases():
    rng = np.random.default_rng(1801)
    out = []
    # the reference's own known answer (src/tests/test_interpolation.py)
    known = np.stack([np.array([0.0, 1.0, 2.0, 3.0, 4.0]), np.array([3.0, 1.4, NAN, 3.4, NAN]), np.array([NAN, 1.5, NAN, NAN, NAN]),
                      np.array([NAN, NAN, NAN, NAN, 1.2]), np.array([NAN] * 5)]).T[None].astype(np.float32)
    out.append(("known_answer", known, [2, 3, 4]))
    x = series(rng, 3, 9, 3, 2, 0.4, 0.0)[:, :, [0, 1, 4, 2, 5, 3]]      # 0 time; 1, 3, 5 linear; 2, 4 rectilinear
    for b, p in ((0, 1.0), (1, 0.7), (2, 0.2)):                  # nothing observed (only the time rows are kept), sparse, dense
        x[b][:, [2, 4]] = np.where(rng.random((9, 2)) < p, NAN, x[b][:, [2, 4]])
    out.append(("b3_l9_c6", x, [2, 4]))
    out.append(("l2", series(rng, 3, 2, 2, 2, 0.3, 0.3), [3, 4]))
    out.append(("no_rect", series(rng, 3, 7, 3, 0, 0.4, 0.0), []))
    x = series(rng, 2, 8, 2, 1, 0.0, 0.0)
    x[:, :, 3] = np.arange(8, dtype=np.float32)[None] * np.array([[1.0], [-2.0]], np.float32)      # changes at every step
    out.append(("every_row", x, [3]))
    x = series(rng, 3, 10, 2, 2, 0.3, 0.5)
    for b, n in ((0, 10), (1, 6), (2, 3)):                       # ragged: the final time repeated, nothing observed behind it
        x[b, n:, 0] = x[b, n - 1, 0]
        x[b, n:, 1:] = NAN
    out.append(("ragged", x, [3, 4]))
    out.append(("c2", series(rng, 3, 9, 0, 1, 0.0, 0.6), [1]))
    for L in (33, 65, 130, 257, 1025):                           # the wave (64 rows), the chunk (256 rows) and the carry between chunks
        x = series(rng, 2, L, 1, 1, 0.0, 0.6, levels=3)
        x[1, :, 1] = np.where(rng.random(L) < 0.5, NAN, x[1, :, 1])      # sample 1: a linear channel with gaps; sample 0: none
        out.append(("l%d" % L, x, [2]))
    out.append(("dense_linear", series(rng, 4, 12, 2, 2, 0.0, 0.6), [3, 4]))      # no NaN in a linear channel: the table only copies
    return out


def fill_input(rng):
    """[3, 9, 5]: channel 0 time; 1: leading gap; 2: interior gaps; 3: trailing gap (and more); 4: never observed."""
    x = series(rng, 3, 9, 4, 0, 0.0, 0.0)
    x[:, :3, 1] = NAN
    x[:, [2, 3, 6], 2] = NAN
    x[:, 5:, 3] = NAN
    x[1, 0, 3] = NAN
    x[2, 0, 2] = NAN
    x[2, 4, 1] = NAN
    x[:, :, 4] = NAN
    return x


def main():
    report = []

    def write(name, kind, meta, **arrays):
        meta = dict(meta, name=name, kind=kind)
        path = os.path.join(GOLD, name + ".npz")
        np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrays)
        assert os.path.getsize(path) < 1 << 20, (name, os.path.getsize(path))
        report.append(meta)

    for tag, x, rect in hybrid_cases():
        assert x.dtype == np.float32 and not np.isnan(x[..., 0]).any()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref = ref_interpolation._prepare_linear_rectilinear_hybrid(torch.from_numpy(x).clone(), list(rect)).numpy()
        lengths = hr.lengths_of(ref, rect)
        mine, mine_len = hr.hybrid(x, rect)
        assert mine.shape == ref.shape and np.array_equal(mine, ref) and np.array_equal(mine_len, lengths), tag
        lin = [c for c in range(x.shape[2]) if c != 0 and c not in rect]
        meta = {"dims": {"B": x.shape[0], "L": x.shape[1], "C": x.shape[2], "T": ref.shape[1]}, "rect": list(rect), "lengths": lengths.tolist(),
                "nan_linear": bool(np.isnan(x[..., lin]).any())}
        print("%-22s x %-14s out %-14s lengths %s" % (tag, x.shape, ref.shape, lengths.tolist()))
        write("g18_hybrid_" + tag, "hybrid", meta, x=x, rect=np.array(rect, np.int64), out=ref, lengths=lengths)

    x = fill_input(np.random.default_rng(1802))
    for rectilinear in (None, 0):
        for initial in (None, 0.0, -1.5):
            for ffill in (False, True):
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    ref = torchcde.linear_interpolation_coeffs(torch.from_numpy(x).clone(), rectilinear=rectilinear, initial_value_if_nan=initial,
                                                               forward_fill=ffill).numpy()
                mine = hr.linear_coeffs(x, rectilinear, initial, ffill)
                assert mine.shape == ref.shape and np.array_equal(mine, ref), (rectilinear, initial, ffill)
                tag = "%s_init%s_ff%d" % ("plain" if rectilinear is None else "rect0", "none" if initial is None else ("%g" % initial).replace("-", "m").replace(".", "p"),
                                          ffill)
                write("g18_fill_" + tag, "fill", {"rectilinear": rectilinear, "initial_value_if_nan": initial, "forward_fill": ffill}, x=x, out=ref)
    ref = ref_misc.forward_fill(torch.from_numpy(x).clone()).numpy()
    assert np.array_equal(hr.forward_fill(x), ref, equal_nan=True) and np.isnan(ref).any()
    write("g18_forward_fill", "forward_fill", {}, x=x, out=ref)
    with open(os.path.join(GOLD, hr.MANIFEST), "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
