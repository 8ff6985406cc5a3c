"""float64 numpy restatement of the Hermite cubic with backward differences (upstream torchcde's
``hermite_cubic_coefficients_with_backward_differences``), written from the stated definition: fill, knots, differences, coefficients.
Helper only: no test functions, no torch, nothing of the package.  The vendored torchcde does not hold the scheme, so there is no
golden; tests/test_hermite_cpu.py checks the properties that define it.

    fill(x, initial_value_if_nan, forward_fill)     the two causal options, values copied
    knots(x, t, initial_value_if_nan, forward_fill) the linear knots: interior gaps interpolated on the grid, ends held, no observation -> 0
    differences(knots, t) -> (h, d, dprev)           h[i] = t[i+1] - t[i],  d[i] = (knots[i+1] - knots[i]) / h[i],  dprev[0] = d[0], dprev[i] = d[i-1]
    coeffs(x, t, initial_value_if_nan, forward_fill) [..., L-1, 4C] = a | b | 2c | 3d
    evaluate(c, i, s) / derivative(c, i, s)          piece i at offset s from its left knot

With both causal options knot k holds observations up to k only, and piece i reads knots i-1, i, i+1.
"""
import numpy as np


def fill(x, initial_value_if_nan=None, forward_fill=False):
    x = np.array(x, dtype=np.float64, copy=True)
    if initial_value_if_nan is not None:
        first = x[..., 0, :]
        first[np.isnan(first)] = float(initial_value_if_nan)
    if forward_fill:
        L = x.shape[-2]
        idx = np.where(np.isnan(x), -1, np.arange(L).reshape(L, 1))
        idx = np.maximum.accumulate(idx, axis=-2)      # the last observation at or before i (-1: none yet, the NaN stays)
        x = np.where(idx < 0, np.nan, np.take_along_axis(x, np.maximum(idx, 0), axis=-2))
    return x


def grid(t, L):
    return np.arange(L, dtype=np.float64) if t is None else np.asarray(t, dtype=np.float64)


def knots(x, t=None, initial_value_if_nan=None, forward_fill=False):
    x = fill(x, initial_value_if_nan, forward_fill)
    L, C = x.shape[-2:]
    g = grid(t, L)
    flat = x.reshape(-1, L, C)
    for b, c in zip(*np.nonzero(np.isnan(flat).any(axis=1))):
        col = flat[b, :, c]
        obs = ~np.isnan(col)
        flat[b, :, c] = np.interp(g, g[obs], col[obs]) if obs.any() else 0.0      # np.interp holds the end values
    return flat.reshape(x.shape)


def differences(k, t=None):
    L = k.shape[-2]
    h = np.diff(grid(t, L)).reshape(L - 1, 1)
    d = (k[..., 1:, :] - k[..., :-1, :]) / h
    dprev = np.concatenate([d[..., :1, :], d[..., :-1, :]], axis=-2)
    return h, d, dprev


def coeffs_from_knots(k, t=None):
    h, d, dprev = differences(k, t)
    a = k[..., :-1, :]
    b = dprev
    two_c = 2 * (3 * ((k[..., 1:, :] - k[..., :-1, :]) / h - b) - d + dprev) / h
    three_d = (1 / h ** 2) * (d - b) - two_c / h
    return np.concatenate([a, b, two_c, three_d], axis=-1)


def coeffs(x, t=None, initial_value_if_nan=None, forward_fill=False):
    return coeffs_from_knots(knots(x, t, initial_value_if_nan, forward_fill), t)


def _parts(c, i):
    C = c.shape[-1] // 4
    row = c[..., i, :]
    return row[..., :C], row[..., C:2 * C], row[..., 2 * C:3 * C], row[..., 3 * C:]


def evaluate(c, i, s):
    a, b, two_c, three_d = _parts(c, i)
    return a + (b + (0.5 * two_c + three_d * s / 3) * s) * s


def derivative(c, i, s):
    _, b, two_c, three_d = _parts(c, i)
    return b + (two_c + three_d * s) * s
