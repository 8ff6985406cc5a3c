"""Golden vectors for online inference (tests/golden/g19_*.npz + MANIFEST_stream.json), produced by IMPORTING the reference on the
build machine -- the way tools/gen_golden_control.py does, through oracle/gen_golden.py's shims.

    python tools/gen_golden_stream.py [NAME ...]

With names (``g19_e_rect_time2``), only those cases are written and their manifest entries replaced or appended; the other files stay
as committed (the zip bytes of an .npz are not reproducible).

The reference only ever solves in batch; its NeuralCDE(return_sequences=True, solver="rk4") output at knot k is what an online step
must reproduce after the k-th observation.  Every case is that model on coefficients from the reference's OWN builder
(torchcde.linear_interpolation_coeffs with rectilinear=<the case's time channel> / forward_fill=True and initial_value_if_nan), on the CPU, in fp32 and fp64.
A case holds
    x         raw observations [B, L, C] with NaNs (time in channel meta["time_index"], never NaN)       static    [B, static_dim] (case c)
    coeffs    what the builder made of them: [B, 2L-1, C] rectilinear, [B, L, C] linear (the filled rows: every 2nd / every row)
    sd_<key>  the model's state dict
    out       [B, L, n_out] outputs per observation         hidden    [B, T, H] the whole hidden sequence (T = 2L-1 / L)
    out64, hidden64  the same model in fp64
    meta      constructor arguments, dims, initial_value_if_nan, and
              causal_diff[_hidden]: max |output (hidden) row k  -  last output (hidden row) of the same model fed the sequence truncated
              at k|, k = 1 .. L-1: the target is causal.  ZERO for the hidden state in fp32 and fp64 and for the fp64 output; the fp32
              output may differ by the final Linear's BLAS rounding, which depends on how many rows the call gets (see main);  ref_drift: fp32 against fp64;  moved: how far the
              hidden state travels, relative to its size (a stream that stands still would test nothing).
"""
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import gen_golden as gg  # noqa: E402  (sets up the reference's import path and the autots stub)

torchcde, GOLD, RefNeuralCDE = gg.torchcde, gg.GOLD, gg.RefNeuralCDE
NAN = float("nan")
TIGHT_Z = 2e-5      # tests/test_control_grad_gpu.py:21

CASES = [
    # name, path, (C, H, HH, nl), B, L, n_out, static_dim, initial_value_if_nan, share of missing values, seed
    ("a_rect", "rectilinear", (3, 8, 8, 2), 5, 6, 2, None, 0.0, 0.35, 1),
    ("b_linear_ffill", "linear", (5, 12, 10, 3), 18, 5, 3, None, -0.5, 0.3, 2),
    ("c_rect_static", "rectilinear", (4, 16, 16, 1), 16, 4, 2, 2, 0.25, 0.3, 3),
    ("d_linear_single_step", "linear", (2, 8, 8, 2), 1, 2, 1, None, 0.0, 0.0, 4),
    ("e_rect_time2", "rectilinear", (5, 10, 12, 2), 7, 5, 2, None, -0.5, 0.3, 5),
]
TIME_INDEX = {"e_rect_time2": 2}      # the channel that holds time (default 0)


def observations(rng, B, L, C, missing):
    """Irregular increasing times in channel 0, random walks in the others with a share `missing` of NaNs (first row included)."""
    t = np.cumsum(rng.uniform(0.5, 1.5, (B, L, 1)), axis=1)
    v = np.cumsum(rng.standard_normal((B, L, C - 1)), axis=1)
    v[rng.random(v.shape) < missing] = NAN
    return np.ascontiguousarray(np.concatenate([t, v], axis=2), dtype=np.float32)


def build_coeffs(x, path, initial, time_index=0):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if path == "rectilinear":
            return torchcde.linear_interpolation_coeffs(x.clone(), rectilinear=time_index, initial_value_if_nan=initial)
        return torchcde.linear_interpolation_coeffs(x.clone(), initial_value_if_nan=initial, forward_fill=True)


def main(only=()):
    report = []
    for name, path, (C, H, HH, nl), B, L, n_out, static_dim, initial, missing, seed in CASES:
        time_index = TIME_INDEX.get(name, 0)
        name = "g19_" + name
        if only and name not in only:
            continue
        rng = np.random.default_rng(1900 + seed)
        x = observations(rng, B, L, C, missing)
        if missing:
            x[0, 0, 1] = NAN              # a first row with a missing value, and a value channel observed late
            x[B - 1, :2, C - 1] = NAN
            assert np.isnan(x[:, 1:]).any()
        if time_index:      # time moves into its channel; the value channels keep their order
            order = list(range(1, C))
            order.insert(time_index, 0)
            x = np.ascontiguousarray(x[:, :, order])
            assert not np.isnan(x[:, :, time_index]).any() and np.isnan(x[:, :, 0]).any()
        static = rng.standard_normal((B, static_dim)).astype(np.float32) if static_dim else None
        ctor = dict(input_dim=C, hidden_dim=H, output_dim=n_out, static_dim=static_dim, hidden_hidden_dim=HH, num_layers=nl,
                    interpolation=path, solver="rk4", return_sequences=True)
        torch.manual_seed(190 + seed)
        base = RefNeuralCDE(**ctor)
        sd = {k: v.clone() for k, v in base.state_dict().items()}
        res = {}
        for dtype in (torch.float32, torch.float64):
            xt = torch.from_numpy(x).to(dtype)
            st = None if static is None else torch.from_numpy(static).to(dtype)
            coeffs = build_coeffs(xt, path, initial, time_index)
            model = RefNeuralCDE(**ctor).to(dtype)
            model.load_state_dict({k: v.to(dtype) for k, v in sd.items()})
            hid = RefNeuralCDE(**dict(ctor, apply_final_linear=False, return_filtered_rectilinear=False)).to(dtype)
            hid.load_state_dict({k: v.to(dtype) for k, v in sd.items() if not k.startswith("final_linear")})
            with torch.no_grad():
                out = model(coeffs if st is None else (st, coeffs))
                hidden = hid(coeffs if st is None else (st, coeffs))
                causal, causal_h = 0.0, 0.0
                for k in range(1, L):      # the same model on the sequence truncated at k: its last output is output row k
                    ck = build_coeffs(xt[:, :k + 1], path, initial, time_index)
                    ok, hk = model(ck if st is None else (st, ck)), hid(ck if st is None else (st, ck))
                    causal = max(causal, float((ok[:, -1] - out[:, k]).abs().max()))
                    causal_h = max(causal_h, float((hk[:, -1] - hidden[:, 2 * k if path == "rectilinear" else k]).abs().max()))
            res[dtype] = (coeffs, out, hidden, causal, causal_h)
        coeffs, out, hidden, causal, causal_h = res[torch.float32]
        _, out64, hidden64, causal64, causal_h64 = res[torch.float64]
        T = 2 * L - 1 if path == "rectilinear" else L
        assert tuple(coeffs.shape) == (B, T, C) and tuple(out.shape) == (B, L, n_out) and tuple(hidden.shape) == (B, T, H)
        assert not torch.isnan(coeffs).any()
        # the hidden state is causal to the bit, and so is the fp64 output; the fp32 OUTPUT may differ in its last bits, because the
        # final Linear's BLAS call rounds a row differently when it is handed T rows instead of k + 1 (final_linear(hidden[:, k])
        # alone differs from row k of final_linear(hidden) by as much): allowed up to 4 ulp of the largest output, and recorded
        assert causal_h == 0.0 and causal_h64 == 0.0 and causal64 == 0.0, (name, "the reference at knot k depends on later observations",
                                                                             causal_h, causal_h64, causal64)
        assert causal <= 4 * float(np.spacing(np.float32(out.abs().max()))), (name, causal)
        drift = {"out": gg.relerr(out, out64), "hidden": gg.relerr(hidden, hidden64)}
        assert max(drift.values()) <= TIGHT_Z / 4, (name, "reference drifts: another seed", drift)
        moved = float((hidden - hidden[:, :1]).abs().max() / hidden.abs().max())
        assert moved >= 1e3 * TIGHT_Z, (name, "the hidden state hardly moves", moved)
        rec = {"x": x, "coeffs": coeffs.numpy(), "out": out.numpy(), "hidden": hidden.numpy(), "out64": out64.numpy(), "hidden64": hidden64.numpy()}
        if static is not None:
            rec["static"] = static
        for k, v in sd.items():
            rec["sd_" + k] = v.numpy().copy()
        meta = {"name": name, "path": path, "ctor": ctor, "dims": {"B": B, "L": L, "T": T, "C": C, "H": H, "HH": HH, "nl": nl, "n_out": n_out},
                "initial_value_if_nan": initial, "time_index": time_index, "state_dict_keys": list(sd.keys()), "causal_diff_hidden": causal_h, "causal_diff_hidden_fp64": causal_h64,
                "causal_diff": causal, "causal_diff_fp64": causal64, "ref_drift": drift, "moved": moved, "n_nan": int(np.isnan(x).sum()),
                "n_nan_first_row": int(np.isnan(x[:, 0]).sum())}
        print(f"{name:26s} nan {meta['n_nan']:3d} (first row {meta['n_nan_first_row']}) causal_diff {causal:g} moved {moved:.2e} ref_drift "
              + " ".join(f"{k} {v:.2e}" for k, v in drift.items()))
        path_npz = os.path.join(GOLD, name + ".npz")
        np.savez_compressed(path_npz, meta=np.array(json.dumps(meta)), **rec)
        assert os.path.getsize(path_npz) < 1 << 20
        report.append(meta)
    manifest = os.path.join(GOLD, "MANIFEST_stream.json")
    if only:      # keep the entries of the cases that were not regenerated, in their order
        with open(manifest) as f:
            old = json.load(f)
        new = {m["name"]: m for m in report}
        report = [new.pop(m["name"], m) for m in old] + list(new.values())
    with open(manifest, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(tuple(sys.argv[1:]))
