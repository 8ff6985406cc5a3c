"""What an online step must return, computed without the online code: for every stream the batch ``NeuralCDE`` in fp64 on the CPU,
on the path built from exactly the rows that stream received.  Helper only: no test functions, and nothing here
imports or calls ``online.py``.

The path is ``linear_interpolation_coeffs(rows, rectilinear=time_index, initial_value_if_nan=v)`` on a rectilinear model and
``linear_interpolation_coeffs(rows, initial_value_if_nan=v, forward_fill=True)`` on a linear one.  The project's builder runs on the
GPU in fp32 only; with both causal options it does nothing but copy values (no NaN is left to interpolate), so the host restatement
that tests/test_hybrid_cpu.py pins to the reference's own outputs (hybrid_ref.linear_coeffs) gives the same rows, which are then
widened to fp64 without loss.  tests/test_online_edges_cpu.py validates this helper on every g19 golden: it reproduces the
reference's ``hidden64`` / ``out64`` to <= 1e-10 and the reference's coefficients bit for bit."""
import warnings

import numpy as np
import torch

import hybrid_ref
from ncde_amd import unfused

_CTOR = ("input_dim", "hidden_dim", "output_dim", "static_dim", "hidden_hidden_dim", "num_layers", "use_initial", "interpolation",
         "interpolation_eps", "sparsity", "vector_field", "vector_field_type", "solver")


def _twin(model, apply_final_linear):
    """A fresh fp64 CPU module of the same class and configuration holding the model's weights, answering at every observation."""
    kw = {k: getattr(model, k) for k in _CTOR}
    t = type(model)(return_sequences=True, return_filtered_rectilinear=True, apply_final_linear=apply_final_linear, adjoint=False, **kw).double()
    own = t.state_dict()
    t.load_state_dict({k: v.detach().cpu().double() for k, v in model.state_dict().items() if k in own})
    assert all(k in model.state_dict() for k in own)
    return t.eval()


def path64(xs, rect, initial_value_if_nan, time_index):
    """xs [1, k, C] (fp32 values, NaN = not observed) -> the control path's knots in fp64, [1, 2k-1 or k, C]."""
    c = hybrid_ref.linear_coeffs(xs, rectilinear=time_index if rect else None, initial_value_if_nan=initial_value_if_nan, forward_fill_=not rect)
    assert not np.isnan(c).any()
    return torch.from_numpy(c.astype(np.float64))


def _np(a, dtype=None):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a if dtype is None else a.astype(dtype)


def prefix_reference(model, rows, received=None, static=None, initial_value_if_nan=0.0, time_index=0):
    """rows [n, B, C]: the row offered to every stream at each of n calls; received [n, B] bool (None: every stream takes every row);
    static [B, static_dim] or None.
    -> (z [n, B, H], out [n, B, n_out]) in fp64: hidden state and answer of every stream after every call.  A stream that has received
    nothing answers the readout of z = 0; a stream that receives no row in a call repeats its previous answer."""
    rows = _np(rows)
    n, B, C = rows.shape
    x32 = rows.astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), rows.astype(np.float64), equal_nan=True), "rows must be fp32 values"
    received = np.ones((n, B), bool) if received is None else _np(received).astype(bool)
    assert received.shape == (n, B)
    static = None if static is None else torch.from_numpy(_np(static, np.float64))
    rect = model.interpolation == "rectilinear"
    hid, full = _twin(model, False), _twin(model, model.apply_final_linear)
    H = model.hidden_dim
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        zero_out = full.final_linear(torch.zeros(1, H, dtype=torch.float64)).numpy()[0]
        z = np.zeros((n, B, H))
        out = np.empty((n, B, zero_out.shape[0]))
        out[:] = zero_out
        for b in range(B):
            idx = np.nonzero(received[:, b])[0]
            if idx.size == 0:
                continue
            xs = x32[idx, b][None]
            if idx.size == 1:      # the builder wants two rows; the path is causal, so knot 0 does not see the row appended here
                pad = xs[:, -1:].copy()
                pad[..., time_index if rect else 0] += 1.0
                xs = np.concatenate([xs, np.where(np.isnan(pad), np.float32(0.0), pad)], axis=1)
            coeffs = path64(xs, rect, initial_value_if_nan, time_index)
            # (cdeint itself refuses CPU tensors: the module's own read-in, the package's torch-op solver, the modules' readouts)
            X, z0 = hid._control_and_start(coeffs if static is None else (static[b:b + 1], coeffs))
            sol = unfused.cdeint_unfused(X, hid.func, z0, X.grid_points, False, hid.vector_field_type, hid.solver, 1.0)
            zb, ob = hid._readout(sol).numpy()[0], full._readout(sol).numpy()[0]
            assert zb.shape[0] == xs.shape[1] and ob.shape[0] == xs.shape[1]
            seen = np.cumsum(received[:, b])
            for j in range(n):
                if seen[j]:
                    z[j, b], out[j, b] = zb[seen[j] - 1], ob[seen[j] - 1]
    return z, out
