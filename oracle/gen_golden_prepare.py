"""Golden g15: the reference's coefficient builders run in FLOAT64 (tests/golden/g15_coeffs_f64.npz + MANIFEST_prepare.json),
produced by IMPORTING the reference's vendored torchcde (this container only, like oracle/gen_golden.py).

    python oracle/gen_golden_prepare.py

``torchcde.linear_interpolation_coeffs`` / ``natural_cubic_coeffs`` on small series with every kind of gap (leading, trailing, no
observation, one observation, ends only, a long interior gap; L = 2, 3, 12), default and user time grid.  It pins two things:
  * tests/coeff_ref64.py (the float64 reference of the GPU tests): agreement at float64 round-off, the observed figure goes
    into the manifest and tests/test_prepare_cpu.py asserts 1e3 x that figure;
  * the fp32 host mirrors of oracle/coeff_oracle.py with ``t=``: compared here with the reference run in fp32 on the same inputs
    (asserted bit-exact) -- the committed counterpart is golden g8_coeffs_user_grid, re-checked by tests/test_prepare_cpu.py.
The file is written with fixed zip time stamps, so a second run reproduces it byte for byte.
"""
import io
import json
import os
import sys
import warnings
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
sys.path[:0] = [os.path.join(REF, "modules", "torchdiffeq"), os.path.join(REF, "modules", "torchcde")]

import torchcde  # noqa: E402  (the reference's vendored copy)

import coeff_oracle as data  # noqa: E402
import coeff_ref64 as ref64  # noqa: E402
import prepare_cases as pc  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SETS = (("L12", 6, 12, 4, 151), ("L3", 6, 3, 3, 152), ("L2", 6, 2, 3, 153))


def inputs(B, L, C, seed):
    x = data.synthetic_series(B, L, C - 1, missing=0.4, seed=seed)
    series = [(b, c) for b in range(B) for c in range(C)]
    stride = len(series) // len(pc.PATTERNS)
    for j, p in enumerate(pc.PATTERNS):
        b, c = series[j * stride]
        pc._apply(x[b, :, c], p)
    t = np.cumsum(0.3 + 1.4 * data.uniform01(seed, L, stream=3)).astype(np.float32)
    return x, t


def save_npz(path, arrays):
    """np.savez_compressed with fixed member time stamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    rec, worst = {}, {}
    for name, B, L, C, seed in SETS:
        x, t = inputs(B, L, C, seed)
        rec[name + "_x"], rec[name + "_t"] = x, t
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for grid, tt in (("", None), ("_t", t)):
                t64 = None if tt is None else torch.from_numpy(tt).double()
                t32 = None if tt is None else torch.from_numpy(tt)
                lin = torchcde.linear_interpolation_coeffs(torch.from_numpy(x.copy()).double(), t=t64).numpy()
                cub = torchcde.natural_cubic_coeffs(torch.from_numpy(x.copy()).double(), t=t64).numpy()
                assert lin.dtype == np.float64 and cub.dtype == np.float64
                rec[name + "_linear" + grid], rec[name + "_cubic" + grid] = lin, cub
                for what, got, want, ns in (("linear", ref64.linear(x, t=tt), lin, 1), ("cubic", ref64.natural_cubic(x, t=tt), cub, 4)):
                    e = float(pc.case_errors(got, want, ns, floor=1.0).max())
                    worst[name + "_" + what + grid] = e
                    print("%-20s coeff_ref64 vs reference (float64): %.3e" % (name + "_" + what + grid, e))
                # the fp32 host mirrors against the reference in fp32 on the same inputs
                lin32 = torchcde.linear_interpolation_coeffs(torch.from_numpy(x.copy()), t=t32).numpy()
                cub32 = torchcde.natural_cubic_coeffs(torch.from_numpy(x.copy()), t=t32).numpy()
                assert np.array_equal(data.linear_interpolation_coeffs(x, t=tt), lin32), (name, grid, "linear mirror")
                assert np.array_equal(data.natural_cubic_coeffs(x, t=tt), cub32), (name, grid, "cubic mirror")
        xc = data.synthetic_series(B, L, C - 1, missing=0.0, seed=seed + 10)
        cub32 = torchcde.natural_cubic_coeffs(torch.from_numpy(xc), t=torch.from_numpy(t)).numpy()
        assert np.array_equal(data.natural_cubic_coeffs(xc, t=t), cub32), (name, "complete cubic mirror on the user grid")
    print("fp32 host mirrors (default and user grid, with gaps and complete): bit-exact with the reference")
    save_npz(os.path.join(GOLD, "g15_coeffs_f64.npz"), rec)
    observed = max(worst.values())
    manifest = {"name": "g15_coeffs_f64", "sets": [{"name": n, "B": B, "L": L, "C": C, "seed": s} for n, B, L, C, s in SETS],
                "patterns": list(pc.PATTERNS), "dtype": "float64",
                "metric": "max over (sample, channel, section) of max_t |coeff_ref64 - reference| / max(max_t |reference|, max_t |section a of the series|)",
                "ref64_vs_reference": worst, "ref64_vs_reference_worst": observed, "bound_factor": 1e3}
    with open(os.path.join(GOLD, "MANIFEST_prepare.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print("worst %.3e -> tests assert %.3e" % (observed, 1e3 * observed))


if __name__ == "__main__":
    main()
