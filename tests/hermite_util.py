"""Shared by the Hermite online tests (tests/test_hermite_cpu.py, tests/test_online_hermite_gpu.py): seeded models and rows, and what
a step must return -- the same model's batch solve in fp64 on the CPU on tests/hermite_ref.py coefficients.  Helper only: no test
functions, and nothing here calls ``online.py``.  A reference is computed once per session and never modified."""
import functools
import warnings

import numpy as np
import torch

import hermite_ref
import stream_edges as se
import stream_ref as sr
from ncde_amd import unfused


def batch_reference(model, rows, static=None, initial_value_if_nan=0.0):
    """rows [L, B, C] (fp32 values, NaN = not observed), every stream receives every row -> (z [L, B, H], out [L, B, n_out]) in
    fp64: the hidden state and the answer of ``return_sequences=True`` at every knot of the Hermite path built with
    initial_value_if_nan and forward_fill=True.  (The path is causal -- tests/test_hermite_cpu.py checks it bit for bit -- so knot k
    of the whole path's solve is the solve of the prefix.)"""
    rows = np.asarray(rows)
    assert rows.dtype == np.float32 and rows.shape[0] >= 2
    c = hermite_ref.coeffs(np.swapaxes(rows, 0, 1), None, initial_value_if_nan, True)
    assert np.isfinite(c).all()
    coeffs = torch.from_numpy(np.ascontiguousarray(c))
    static = None if static is None else torch.from_numpy(np.asarray(static, np.float64))
    hid, full = sr._twin(model, False), sr._twin(model, model.apply_final_linear)
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        X, z0 = hid._control_and_start(coeffs if static is None else (static, coeffs))
        sol = unfused.cdeint_unfused(X, hid.func, z0, X.grid_points, False, hid.vector_field_type, hid.solver, 1.0)
        z, out = hid._readout(sol).numpy(), full._readout(sol).numpy()
    assert z.shape[1] == rows.shape[0]
    return np.ascontiguousarray(np.swapaxes(z, 0, 1)), np.ascontiguousarray(np.swapaxes(out, 0, 1))


# ---- the main case: C 5, H 12, HH 10, nl 2, B 19 (two tiles and a 3-stream tail), L 6, rk4 -------------------------------------------
MAIN = dict(C=5, H=12, HH=10, nl=2, B=19, L=6, n_out=3, init=0.5, model_seed=61, rows_seed=6101)


def main_model(path, device="cpu", dtype=torch.float32, **kw):
    s = MAIN
    return se.make_model(s["model_seed"], s["C"], s["H"], s["n_out"], s["HH"], s["nl"], path, device, dtype, **kw)


@functools.lru_cache(maxsize=None)
def main_rows():
    """30 % NaN in the non-time channels after row 0 and a NaN in row 0 (filled with MAIN['init'])."""
    s = MAIN
    x = se.make_rows(s["rows_seed"], s["L"], s["B"], s["C"])
    x[0] = np.where(np.isnan(x[0]), np.float32(0.25), x[0])
    x[0, 2, 3] = x[0, 17, 1] = np.nan
    assert not np.isnan(x[:, :, 0]).any() and np.isnan(x[1:, :, 1:]).mean() > 0.2 and np.isnan(x[0]).sum() == 2
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def main_reference():
    z, out = batch_reference(main_model("cubic_hermite"), main_rows(), None, MAIN["init"])
    z.setflags(write=False)
    out.setflags(write=False)
    return z, out
