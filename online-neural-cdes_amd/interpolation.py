"""Control paths: host-side mirrors of ``torchcde.LinearInterpolation`` / ``torchcde.NaturalCubicSpline``
(/root/reference/modules/torchcde/torchcde/interpolation_linear.py:183-234, interpolation_cubic.py:268-336) and of the
reference's own ``SmoothLinearInterpolation`` (src/ncde/interpolation.py:6-123 of the reference tree).

They keep the reference's constructor, ``grid_points``, ``interval``, ``evaluate`` and ``derivative``
(the last two in plain torch ops, used outside the solve, e.g. for ``h0 = Linear(X(0))``).  Inside
``cdeint`` the fused HIP kernels read the raw coefficient tensor and evaluate dX/dt on chip, so
the ``[B, T-1, C]`` derivative tensor the reference materialises in its constructor is never built.
"""
import weakref

import torch


class _Tagged(torch.Tensor):
    """A time tensor that remembers which grid of which control it is (avoids a device sync in cdeint)."""


def _tag(t, kind, owner):
    t = t.as_subclass(_Tagged)
    t._ncde_kind = kind
    t._ncde_owner = weakref.ref(owner)
    return t


_GRID_CACHE = {}   # (n_knots, dtype, device) -> (t, [t0, t_last]): the default integer grid is built once, not per forward


def _default_grid(n_knots, like):
    key = (n_knots, like.dtype, like.device)
    hit = _GRID_CACHE.get(key)
    if hit is None:
        t = torch.linspace(0, n_knots - 1, n_knots, dtype=like.dtype, device=like.device)
        hit = (t, torch.stack([t[0], t[-1]]))
        if len(_GRID_CACHE) > 64:
            _GRID_CACHE.clear()
        _GRID_CACHE[key] = hit
    return hit


class _ControlBase(torch.nn.Module):
    interp_name = None

    def _setup_t(self, t, n_knots, like):
        self._default_grid = t is None
        self._interval = None
        if t is None:
            t, self._interval = _default_grid(n_knots, like)
        self.register_buffer("_t", t)

    @property
    def grid_points(self):
        return _tag(self._t, "knots", self)

    @property
    def interval(self):
        iv = self._interval if self._interval is not None else torch.stack([self._t[0], self._t[-1]])
        return _tag(iv, "interval", self)

    def _plan_grid(self):
        """(knot grid the fused kernels walk -- None = the integer grid --, its number of knots): what the time plan is built on.
        For every control but the smoothed one this is the grid of ``grid_points``."""
        return (None if self._default_grid else self._t), self.n_knots

    def _at_first_knot(self, t):
        """X(t) at t = first knot of the default grid is the first coefficient row itself (fractional part 0): no
        bucketize / gather kernels for the ``h0 = Linear(X(0))`` of every forward (ncde.py:170-198)."""
        return self._default_grid and isinstance(t, (int, float)) and t == 0

    def _interpret_t(self, t, n_pieces):
        t = torch.as_tensor(t, dtype=self._t.dtype, device=self._t.device)
        index = torch.bucketize(t.detach(), self._t.detach()).sub(1).clamp(0, n_pieces - 1)
        return t - self._t[index], index

    def forward(self, t):  # convenience, not part of the reference interface
        return self.evaluate(t)


class LinearInterpolation(_ControlBase):
    """Piecewise linear path through ``coeffs[..., T, C]`` (output of linear_interpolation_coeffs;
    rectilinear data is simply a longer such tensor)."""

    interp_name = "linear"

    def __init__(self, coeffs, t=None, **kwargs):
        super().__init__(**kwargs)
        self._setup_t(t, coeffs.size(-2), coeffs)
        self.register_buffer("_coeffs", coeffs)

    @property
    def fused_coeffs(self):
        return self._coeffs

    @property
    def n_knots(self):
        return self._coeffs.size(-2)

    @property
    def channels(self):
        return self._coeffs.size(-1)

    def evaluate(self, t):
        if self._at_first_knot(t):
            return self._coeffs[..., 0, :]
        frac, index = self._interpret_t(t, self._coeffs.size(-2) - 1)
        prev_c = self._coeffs[..., index, :]
        next_c = self._coeffs[..., index + 1, :]
        dt = self._t[index + 1] - self._t[index]
        return prev_c + frac.unsqueeze(-1) * (next_c - prev_c) / dt.unsqueeze(-1)

    def derivative(self, t):
        _, index = self._interpret_t(t, self._coeffs.size(-2) - 1)
        dt = self._t[index + 1] - self._t[index]
        return (self._coeffs[..., index + 1, :] - self._coeffs[..., index, :]) / dt.unsqueeze(-1)


class NaturalCubicSpline(_ControlBase):
    """Natural cubic spline from ``coeffs[..., T-1, 4C] = a | b | 2c | 3d`` (natural_cubic_coeffs output)."""

    interp_name = "cubic"

    def __init__(self, coeffs, t=None, **kwargs):
        super().__init__(**kwargs)
        channels = coeffs.size(-1) // 4
        if channels * 4 != coeffs.size(-1):
            raise ValueError("Passed invalid coeffs.")
        self._setup_t(t, coeffs.size(-2) + 1, coeffs)
        self.register_buffer("_coeffs", coeffs)
        self._channels = channels

    @property
    def fused_coeffs(self):
        return self._coeffs

    @property
    def n_knots(self):
        return self._coeffs.size(-2) + 1

    @property
    def channels(self):
        return self._channels

    def _parts(self, index):
        c = self._channels
        row = self._coeffs[..., index, :]
        return row[..., :c], row[..., c:2 * c], row[..., 2 * c:3 * c], row[..., 3 * c:]

    def evaluate(self, t):
        if self._at_first_knot(t):
            return self._coeffs[..., 0, :self._channels]
        frac, index = self._interpret_t(t, self._coeffs.size(-2))
        frac = frac.unsqueeze(-1)
        a, b, two_c, three_d = self._parts(index)
        inner = 0.5 * two_c + three_d * frac / 3
        inner = b + inner * frac
        return a + inner * frac

    def derivative(self, t):
        frac, index = self._interpret_t(t, self._coeffs.size(-2))
        frac = frac.unsqueeze(-1)
        _, b, two_c, three_d = self._parts(index)
        return b + (two_c + three_d * frac) * frac


CubicSpline = NaturalCubicSpline      # upstream torchcde's name for the evaluator of any a | b | 2c | 3d tensor (natural or Hermite)


class SmoothLinearInterpolation(_ControlBase):
    """Piecewise linear path whose corners are rounded off: in ``(k, k + eps)`` after every interior knot ``k`` of the integer grid
    a cubic (``match_second_derivatives=False``) or quintic (``True``) polynomial takes the path from the slope of the piece before
    ``k`` to the slope of the piece after it (src/ncde/interpolation.py:6-123).  ``gradient_matching_eps=None`` is plain linear
    interpolation.

    Constructor, assertions, ``grid_points`` / ``interval`` (the integer grid: T entries), ``evaluate`` and ``derivative`` (scalar
    ``t``; region rule ``0 < index and frac < eps``, the left piece at an exact knot) are the reference's.  The torch-op
    ``evaluate`` / ``derivative`` keep its sequence of tensor operations -- coefficient tensor ``[B, T-2, C, order+1]`` with the
    polynomial index on the slowest memory axis, powers of ``frac`` highest first, product and ``sum`` over the last axis -- because
    they are compared bit for bit with recorded reference values; they serve ``h0 = Linear(X(0))`` and the unfused solver.

    Inside the fused ``cdeint`` the path is a piecewise polynomial on the REFINED knot grid ``0, 1, 1+eps, 2, 2+eps, ..., T-1``:
    ``fused_coeffs`` (built once per object by ``ncde_prepare_smooth``) is an ordinary ``a | b | 2c | 3d`` tensor for cubic matching
    -- every fused kernel family runs it -- and ``a | b | 2c | 3d | 4e | 5f`` (``NCDE_INTERP_QUINTIC``) for quintic matching.
    ``n_knots`` stays T (it describes ``grid_points``); the refined grid reaches the kernels through ``_plan_grid`` only.

    Coefficients that require grad (``adjoint=False``): with cubic matching the solve stays fused -- ``fused_coeffs`` is built from the
    detached coefficients and ``cdeint`` folds dL/d(rows) back onto them with ``ncde_prepare_smooth_backward`` (solver.py); quintic
    matching and ``gradient_matching_eps=None`` run on the unfused solver.
    """

    def __init__(self, coeffs, t=None, gradient_matching_eps=None, match_second_derivatives=False, **kwargs):
        super().__init__(**kwargs)
        eps = gradient_matching_eps
        if t is not None:
            assert eps is None, "times not implemented for gradient_matching_eps"
        if eps is not None:
            assert 0 < eps <= 1
        self.gradient_matching_eps = eps
        self.match_second_derivatives = match_second_derivatives
        self._setup_t(t, coeffs.size(-2), coeffs)
        self._integer_grid = self._default_grid
        # the default-axis kernels step from integer knot to integer knot: right for eps == 1 (and for no smoothing at all)
        self._default_grid = self._integer_grid and (eps is None or eps == 1)
        self.register_buffer("_coeffs", coeffs)
        # both derived tensors are built on first use and tied to the coefficient tensor they were built from (storage, version,
        # device, dtype): X.to(...), X.double() or an in-place edit of the coefficients rebuilds them.  A training step on the fused
        # path never builds the torch-op matching coefficients (h0 reads the first row; the kernels read fused_coeffs).
        self._matching = (None, None)
        self._fused = (None, None)
        self._host_grid = None

    def _coeffs_key(self):
        c = self._coeffs
        return (c.data_ptr(), c._version, c.device, c.dtype, tuple(c.shape))

    @property
    def gradient_matching_coeffs(self):
        """``[B, T-2, C, order+1]`` polynomial of every matching region, highest power first (the reference's attribute of this name);
        built by torch ops on the first ``evaluate`` / ``derivative`` that needs it -- never on the fused path."""
        if self.gradient_matching_eps is None:
            raise AttributeError("gradient_matching_coeffs: no smoothing (gradient_matching_eps is None)")
        key = self._coeffs_key()
        if self._matching[0] != key:
            self._matching = (key, _matching_coefficients(self._coeffs, self.gradient_matching_eps, 5 if self.match_second_derivatives else 3))
        return self._matching[1]

    def __len__(self):
        return self._t.numel()

    @property
    def interp_name(self):
        if self.gradient_matching_eps is None:
            return "linear"
        return "quintic" if self.match_second_derivatives else "cubic"

    @property
    def n_knots(self):
        return self._coeffs.size(-2)

    @property
    def channels(self):
        return self._coeffs.size(-1)

    @property
    def grid_points(self):
        t = _tag(self._t, "knots", self)
        if self._integer_grid:
            t._ncde_host = (t._version, torch.arange(self.n_knots, dtype=torch.double))
        return t

    @property
    def interval(self):
        t = _ControlBase.interval.fget(self)
        if self._integer_grid:
            t._ncde_host = (t._version, torch.tensor([0.0, float(self.n_knots - 1)], dtype=torch.double))
        return t

    def _at_first_knot(self, t):
        return self._integer_grid and isinstance(t, (int, float)) and t == 0

    def _plan_grid(self):
        eps = self.gradient_matching_eps
        if eps is None or eps == 1:
            return (None if self._integer_grid else self._t), self.n_knots
        if self._host_grid is None:
            k = torch.arange(1, self.n_knots - 1, dtype=torch.double)
            inner = torch.stack([k, k + eps], dim=1).reshape(-1)
            self._host_grid = torch.cat([torch.zeros(1, dtype=torch.double), inner, torch.full((1,), self.n_knots - 1.0, dtype=torch.double)])
        return self._host_grid, self._host_grid.numel()

    @property
    def fused_coeffs(self):
        """The tensor the fused kernels read: the linear coefficients themselves without smoothing, else the refined
        piecewise-polynomial rows (one ``ncde_prepare_smooth`` launch per coefficient tensor)."""
        eps = self.gradient_matching_eps
        if eps is None:
            return self._coeffs
        key = self._coeffs_key()
        if self._fused[0] != key:
            import ctypes
            from . import _lib
            x = self._coeffs.detach()
            if not (x.is_cuda and x.dtype == torch.float32):
                raise NotImplementedError("the fused smoothed path needs fp32 coefficients on the GPU; got %s on %s" % (x.dtype, x.device))
            T, C = x.shape[-2:]
            x = x.reshape(-1, T, C).contiguous()
            order = 5 if self.match_second_derivatives else 3
            lib = _lib.lib()
            P = _lib.check(lib.ncde_smooth_pieces(T, float(eps)), "ncde_smooth_pieces")
            out = torch.empty(x.shape[0], P, (order + 1) * C, dtype=torch.float32, device=x.device)
            with torch.cuda.device(x.device):
                _lib.check(lib.ncde_prepare_smooth(x.data_ptr(), x.shape[0], T, C, float(eps), order, out.data_ptr(),
                                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "ncde_prepare_smooth")
            self._fused = (key, out.reshape(*self._coeffs.shape[:-2], P, (order + 1) * C))
        return self._fused[1]

    def _locate(self, t):
        t = torch.as_tensor(t, dtype=self._coeffs.dtype, device=self._coeffs.device)
        index = torch.bucketize(t.detach(), self._t.detach()).sub(1).clamp(0, self._coeffs.size(-2) - 2)
        frac = t - self._t[index]
        eps = self.gradient_matching_eps
        matching = eps is not None and bool(0 < index) and bool(frac < eps)
        return frac, index, matching

    def evaluate(self, t):
        if self._at_first_knot(t):
            return self._coeffs[..., 0, :]
        frac, index, matching = self._locate(t)
        frac = frac.unsqueeze(-1)
        if matching:
            mc = self.gradient_matching_coeffs[:, index - 1]
            powers = torch.cat([frac ** i for i in range(mc.size(-1))]).flip(dims=[0]).to(mc.device)
            return (mc * powers).sum(dim=-1)
        prev_c, next_c = self._coeffs[..., index, :], self._coeffs[..., index + 1, :]
        dt = self._t[index + 1] - self._t[index]
        return prev_c + frac * (next_c - prev_c) / dt.unsqueeze(-1)

    def derivative(self, t):
        frac, index, matching = self._locate(t)
        if matching:
            mc = self.gradient_matching_coeffs[:, index - 1]
            powers = torch.tensor([i * frac ** (i - 1) for i in range(1, mc.size(-1))]).flip(dims=[0]).to(mc.device)
            return (mc[..., :-1] * powers).sum(dim=-1)
        dt = self._t[index + 1] - self._t[index]
        return (self._coeffs[..., index + 1, :] - self._coeffs[..., index, :]) / dt.unsqueeze(-1)


def _matching_coefficients(coeffs, eps, order):
    """Polynomial of the matching region after every interior knot, highest power first on the last axis: ``[B, T-2, C, order+1]``.
    It starts at the knot with the slope of the piece before it and meets the next linear piece at ``frac = eps`` in value and slope
    (order 3), and in second derivative -- zero at both ends -- as well (order 5).  Operation order of src/ncde/interpolation.py:151-191."""
    mid, nxt, prv = coeffs[..., 1:-1, :], coeffs[..., 2:, :], coeffs[..., :-2, :]
    at_eps = mid + eps * (nxt - mid)
    slope_in, slope_out = mid - prv, nxt - mid
    if order == 3:
        quad = (1 / eps ** 2) * (3 * (at_eps - slope_in * eps - mid) - eps * (slope_out - slope_in))
        cub = (1 / (3 * eps ** 2)) * (slope_out - slope_in - 2 * quad * eps)
        parts = [cub, quad, slope_in, mid]
    else:
        cub = (1 / eps ** 3) * (10 * (at_eps - slope_in * eps - mid) - 4 * eps * (slope_out - slope_in))
        quart = (1 / (2 * eps ** 3)) * (2 * (slope_out - slope_in) - 3 * cub * eps ** 2)
        quint = -(1 / (10 * eps ** 2)) * (6 * quart * eps + 3 * cub)
        parts = [quint, quart, cub, torch.zeros_like(mid), slope_in, mid]
    return torch.stack(parts).permute(1, 2, 3, 0)
