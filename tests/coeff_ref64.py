"""float64 reference of the three control-path coefficient builders (test infrastructure; plain numpy, no torch).

NOT a restatement of the kernels' or the reference's operation order: the mathematical definition, evaluated in float64.
  * linear          forward fill + interleave (rectilinear), else end fill + ``np.interp`` on the time grid
  * natural_cubic   the natural spline through the observed knots from its SECOND-derivative (moment) system -- the
                    reference and the kernels solve for the knot FIRST derivatives --, re-expanded about the left end
                    of every grid interval
  * smooth          the matching polynomials of the smoothed-linear path in closed form (the polynomial of degree 3 / 5
                    that leaves knot k with the slope before it and meets the next linear piece at k + eps in value,
                    slope (and zero second derivative at both ends for degree 5))
tests/test_prepare_cpu.py pins it to the reference's own output (goldens g8, g14, and g15 in float64).
"""
import numpy as np


def _forward_fill(x):
    """NaNs along axis 1 of x[N, L, C] take the last observation before them; a leading gap stays."""
    mask = np.isnan(x)
    idx = np.where(~mask, np.arange(x.shape[1]).reshape(1, -1, 1), 0)
    idx = np.maximum.accumulate(idx, axis=1)
    return np.take_along_axis(x, idx, axis=1)


def _gappy(flat):
    """(sample, channel) index pairs of the series of flat[N, L, C] that hold a NaN."""
    return list(zip(*np.nonzero(np.isnan(flat).any(axis=1))))


def linear(x, t=None, rectilinear=None):
    """Knots of the (rectilinear) linear interpolation of x[..., L, C]; NaN = missing.  float64 out:
    [..., L, C], or [..., 2L-1, C] for ``rectilinear`` = index of the time channel."""
    x = np.array(x, dtype=np.float64)
    lead, (L, C) = x.shape[:-2], x.shape[-2:]
    flat = x.reshape(-1, L, C)
    if rectilinear is not None:
        rep = np.repeat(_forward_fill(flat), 2, axis=1)
        rep[:, :-1, rectilinear] = rep[:, 1:, rectilinear].copy()
        flat = np.ascontiguousarray(rep[:, :-1])
        grid = np.arange(2 * L - 1, dtype=np.float64)       # only leading gaps are left: the grid plays no part
    else:
        grid = np.arange(L, dtype=np.float64) if t is None else np.asarray(t, dtype=np.float64)
    for b, c in _gappy(flat):
        col = flat[b, :, c]
        obs = ~np.isnan(col)
        flat[b, :, c] = np.interp(grid, grid[obs], col[obs]) if obs.any() else 0.0      # np.interp holds the end values
    return flat.reshape(*lead, flat.shape[1], C)


def _moments(tk, xk):
    """Second derivatives M[m, ...] of the natural spline through (tk[m], xk[m, ...]), m >= 3: float64 Thomas sweep on
    h_{i-1} M_{i-1} + 2 (h_{i-1} + h_i) M_i + h_i M_{i+1} = 6 (s_i - s_{i-1}),  M_0 = M_{m-1} = 0."""
    h = np.diff(tk)
    s = np.diff(xk, axis=0) / h.reshape(-1, *([1] * (xk.ndim - 1)))
    n = tk.size - 2
    diag = 2.0 * (h[:-1] + h[1:])
    rhs = 6.0 * (s[1:] - s[:-1])
    cp = np.empty(n)
    dp = np.empty_like(rhs)
    cp[0] = h[1] / diag[0]
    dp[0] = rhs[0] / diag[0]
    for i in range(1, n):
        den = diag[i] - h[i] * cp[i - 1]
        cp[i] = h[i + 1] / den
        dp[i] = (rhs[i] - h[i] * dp[i - 1]) / den
    M = np.zeros_like(xk)
    M[n] = dp[n - 1]
    for i in range(n - 2, -1, -1):
        M[i + 1] = dp[i] - cp[i] * M[i + 2]
    return M


def _pieces(tk, xk):
    """(a, b, 2c, 3d)[m-1, ...] of the natural spline through the knots, each piece expanded about its left knot."""
    h = np.diff(tk).reshape(-1, *([1] * (xk.ndim - 1)))
    slope = np.diff(xk, axis=0) / h
    if tk.size == 2:      # two knots: the straight line
        z = np.zeros_like(slope)
        return xk[:-1], slope, z, z.copy()
    M = _moments(tk, xk)
    return xk[:-1], slope - h * (2.0 * M[:-1] + M[1:]) / 6.0, M[:-1].copy(), (M[1:] - M[:-1]) / (2.0 * h)


def natural_cubic(x, t=None):
    """a | b | 2c | 3d [..., L-1, 4C] (float64) of the natural cubic spline through x[..., L, C] on the grid t (default
    0..L-1).  NaN = missing: the ends are filled from the first / last observation, the spline runs through the observed
    knots, and interval [t_i, t_{i+1}) gets the piece that covers it, expanded about t_i.  No observation: zeros."""
    x = np.array(x, dtype=np.float64)
    lead, (L, C) = x.shape[:-2], x.shape[-2:]
    flat = x.reshape(-1, L, C)
    grid = np.arange(L, dtype=np.float64) if t is None else np.asarray(t, dtype=np.float64)
    out = np.empty((flat.shape[0], L - 1, 4, C))
    gappy = _gappy(flat)
    filled = flat.copy()
    for b, c in gappy:
        filled[b, :, c] = 0.0
    for q, part in enumerate(_pieces(grid, np.moveaxis(filled, 1, 0))):      # every complete series at once: [L-1, N, C]
        out[:, :, q, :] = np.moveaxis(part, 0, 1)
    for b, c in gappy:
        col = flat[b, :, c].copy()
        obs = np.nonzero(~np.isnan(col))[0]
        if obs.size == 0:
            out[b, :, :, c] = 0.0
            continue
        col[:obs[0]] = col[obs[0]]
        col[obs[-1] + 1:] = col[obs[-1]]
        kn = np.nonzero(~np.isnan(col))[0]
        a, bb, c2, d3 = _pieces(grid[kn], col[kn])
        k = np.clip(np.searchsorted(kn, np.arange(L - 1), side="right") - 1, 0, kn.size - 2)      # piece covering interval i
        s = grid[:-1] - grid[kn][k]
        out[b, :, 0, c] = a[k] + s * (bb[k] + s * (c2[k] / 2.0 + s * d3[k] / 3.0))
        out[b, :, 1, c] = bb[k] + s * (c2[k] + s * d3[k])
        out[b, :, 2, c] = c2[k] + 2.0 * s * d3[k]
        out[b, :, 3, c] = d3[k]
    return out.reshape(*lead, L - 1, 4 * C)


def smooth_pieces(T, eps):
    return 2 * T - 3 if eps < 1 else T - 1


def smooth(x, eps, order):
    """Rows a | b | 2c | 3d [| 4e | 5f] [..., P, (order+1) C] (float64) of the smoothed-linear path through the linear
    knots x[..., T, C] on its refined grid 0, 1, 1+eps, 2, 2+eps, ..., T-1 (eps == 1: the integer grid).  Piece 0 is
    linear; after every interior knot k the matching polynomial on [k, k+eps], then (eps < 1) the linear rest."""
    assert order in (3, 5) and 0 < eps <= 1
    x = np.array(x, dtype=np.float64)
    lead, (T, C) = x.shape[:-2], x.shape[-2:]
    flat = x.reshape(-1, T, C)
    W = order + 1
    P = smooth_pieces(T, eps)
    out = np.zeros((flat.shape[0], P, W, C))
    out[:, 0, 0], out[:, 0, 1] = flat[:, 0], flat[:, 1] - flat[:, 0]
    if T > 2:
        mid = flat[:, 1:-1]
        slope_in, slope_out = mid - flat[:, :-2], flat[:, 2:] - mid
        jump = slope_out - slope_in
        m = np.zeros((flat.shape[0], T - 2, W, C))
        m[:, :, 0], m[:, :, 1] = mid, slope_in
        if order == 3:      # p(s) = x + slope_in s + (2 jump / eps) s^2 - (jump / eps^2) s^3
            m[:, :, 2] = 4.0 * jump / eps
            m[:, :, 3] = -3.0 * jump / eps ** 2
        else:               # p(s) = x + slope_in s + (6 jump / eps^2) s^3 - (8 jump / eps^3) s^4 + (3 jump / eps^4) s^5
            m[:, :, 3] = 18.0 * jump / eps ** 2
            m[:, :, 4] = -32.0 * jump / eps ** 3
            m[:, :, 5] = 15.0 * jump / eps ** 4
        if eps < 1:
            out[:, 1::2] = m
            out[:, 2::2, 0] = mid + eps * slope_out
            out[:, 2::2, 1] = slope_out
        else:
            out[:, 1:] = m
    return out.reshape(*lead, P, W * C)
