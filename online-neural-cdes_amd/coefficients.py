"""GPU construction of control-path coefficients: mirrors of ``torchcde.linear_interpolation_coeffs`` and
``torchcde.natural_cubic_coeffs`` (/root/reference/modules/torchcde/torchcde/interpolation_linear.py:131-180,
interpolation_cubic.py:170-190) for fp32 CUDA tensors, on the default integer time grid or a user grid ``t``, of the causal
builders of online prediction (the fill options, ``forward_fill``, the linear / rectilinear hybrid scheme) and of upstream
torchcde's ``hermite_cubic_coefficients_with_backward_differences``, backed by the HIP kernels in csrc/ncde_prepare.hip.  (Host/numpy mirrors used to build test inputs live in data.py.)"""
import ctypes

import torch

from . import _lib


def _check(x):
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32):
        raise NotImplementedError("coefficient construction runs on fp32 CUDA tensors (no CPU fallback)")
    if x.dim() < 2:
        raise ValueError("X must have at least two dimensions, corresponding to time and channels.")
    if x.size(-2) < 2:
        raise ValueError("Must have a time dimension of size at least 2.")
    return x.contiguous().reshape(-1, x.size(-2), x.size(-1))


def _grid(t, length, device):
    """misc.validate_input_path's checks on a user time grid (torchcde/misc.py:70-100) -> contiguous fp32 tensor on `device`."""
    if t is None:
        return None
    t = torch.as_tensor(t)
    if not t.is_floating_point():
        raise ValueError("t must both be floating point.")
    if t.dim() != 1:
        raise ValueError("t must be one dimensional. It instead has shape {}.".format(tuple(t.shape)))
    if t.numel() != length:
        raise ValueError("The time dimension of X must equal the length of t. X has time dimension {} and t has shape {}.".format(length, tuple(t.shape)))
    if not bool((t[1:] > t[:-1]).all()):
        raise ValueError("t must be monotonically increasing.")
    return t.to(device=device, dtype=torch.float32).contiguous()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _fill(x3, initial_value, fill_forward):
    """ncde_prepare_fill on a contiguous [B, L, C] tensor -> a new tensor (the input is never written)."""
    B, L, C = x3.shape
    out = torch.empty_like(x3)
    if out.numel() == 0:
        return out
    with torch.cuda.device(x3.device):
        rc = _lib.lib().ncde_prepare_fill(x3.data_ptr(), B, L, C, 0 if initial_value is None else 1, 0.0 if initial_value is None else float(initial_value),
                                          1 if fill_forward else 0, out.data_ptr(), _stream())
    _lib.check(rc, "ncde_prepare_fill")
    return out


def _fill_args(initial_value_if_nan, forward_fill):
    if initial_value_if_nan is not None and (isinstance(initial_value_if_nan, bool) or not isinstance(initial_value_if_nan, (int, float))):
        raise TypeError("initial_value_if_nan must be a float or None, not {!r}".format(initial_value_if_nan))
    if not isinstance(forward_fill, bool):
        raise TypeError("forward_fill must be a bool, not {!r}".format(forward_fill))


def forward_fill(x):
    """``torchcde.misc.forward_fill`` (misc.py:103-126) along dimension -2 of an fp32 CUDA tensor [..., L, C]: a NaN takes the last
    observation before it in its channel; NaNs in front of a channel's first observation stay NaN.  Returns a new tensor."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32):
        raise NotImplementedError("forward_fill runs on fp32 CUDA tensors (no CPU fallback)")
    if x.dim() < 2:
        raise ValueError("x must have at least two dimensions, corresponding to time and channels.")
    return _fill(x.contiguous().reshape(-1, x.size(-2), x.size(-1)), None, True).reshape(x.shape)


def linear_interpolation_coeffs(x, t=None, rectilinear=None, initial_value_if_nan=None, forward_fill=False):
    """Knots of the (rectilinear) linear interpolation; NaNs are missing values.

    The two causal options of the reference's fork (interpolation_linear.py:131-180), in its order of operations:
    ``initial_value_if_nan`` (a float) replaces the NaNs of the first time row; then the rectilinear preparation, if asked for; then,
    with ``forward_fill=True``, every channel is forward filled along time, so that a knot only holds observations made up to it; then
    the NaN handling that is left (interior gaps interpolated, leading / trailing gaps from the first / last observation).
    With both the result at knot k depends on x[..., :k+1, :] only.  Unlike the reference, which writes ``initial_value_if_nan`` into
    the caller's tensor, this function never modifies ``x``."""
    _fill_args(initial_value_if_nan, forward_fill)
    x3 = _check(x)
    B, L, C = x3.shape
    tg = _grid(t, 2 * L - 1 if rectilinear is not None else L, x.device)      # the reference validates t against the PREPARED path
    if initial_value_if_nan is not None or forward_fill:
        # the rectilinear preparation forward fills itself and a forward fill is idempotent: filling first gives what the reference's
        # fill after the preparation gives
        x3 = _fill(x3, initial_value_if_nan, forward_fill)
    if rectilinear is not None:
        assert isinstance(rectilinear, int) and 0 <= rectilinear < C, "Index of the time channel must be an integer in [0, {}]".format(C - 1)
        assert not torch.isnan(x3[..., rectilinear]).any(), "There exist nan values in the time column which is not allowed."
    T = 2 * L - 1 if rectilinear is not None else L
    out = torch.empty(B, T, C, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = _lib.lib().ncde_prepare_linear_grid(x3.data_ptr(), None if (tg is None or rectilinear is not None) else tg.data_ptr(), B, L, C,
                                                 -1 if rectilinear is None else rectilinear, out.data_ptr(), _stream())
    _lib.check(rc, "ncde_prepare_linear_grid")
    return out.reshape(*x.shape[:-2], T, C)


def _hybrid_args(x, rectilinear_indices, time_index):
    """The reference's asserts on the arguments of the hybrid scheme (src/ncde/interpolation.py:210-216), before anything runs."""
    if not isinstance(rectilinear_indices, list):
        raise TypeError("rectilinear_indices must be a list of channel indices, not {!r}".format(type(rectilinear_indices).__name__))
    if isinstance(time_index, bool) or not isinstance(time_index, int):
        raise TypeError("time_index must be an int, not {!r}".format(time_index))
    if time_index != 0:
        raise NotImplementedError("time_index must be 0: the reference's hybrid scheme lags channel 0 whatever time_index says "
                                  "(its rectilinear preparation is called with rectilinear=0), so any other value has no defined meaning")
    if not torch.is_tensor(x) or x.dim() < 2:
        raise ValueError("X must have at least two dimensions, corresponding to time and channels.")
    C = x.size(-1)
    for r in rectilinear_indices:
        if isinstance(r, bool) or not isinstance(r, int):
            raise TypeError("rectilinear_indices must hold ints, not {!r}".format(r))
        if not 0 <= r < C:
            raise ValueError("rectilinear index {} is outside [0, {}]".format(r, C - 1))
        if r == time_index:
            raise ValueError("rectilinear_indices must not hold the time index ({})".format(time_index))
    if len(set(rectilinear_indices)) != len(rectilinear_indices):
        raise ValueError("rectilinear_indices must be distinct: {}".format(rectilinear_indices))


def linear_rectilinear_hybrid_coeffs(x, rectilinear_indices, time_index=0, return_lengths=False):
    """The reference's linear / rectilinear hybrid scheme (``_prepare_linear_rectilinear_hybrid``, src/ncde/interpolation.py:191-253)
    for ICU-style data: densely sampled channels are interpolated linearly, the sparse ones in ``rectilinear_indices`` are
    rectilinear, and a knot is added only where one of them changes.

    x: [..., L, C] fp32 CUDA, NaN = missing, time in channel 0 without NaN (not checked: that would be a second synchronisation).
    Linear channels (all but time and the rectilinear ones): first-row NaNs become 0.0, then the linear NaN fill.  Rectilinear
    channels: first-row NaNs become 0.0, then a forward fill.  Of the 2L-1 rows  (t_i, lin_i, rect_i), (t_{i+1}, lin_{i+1}, rect_i)
    row 0 is kept and any other row iff its time or one of its rectilinear values differs from the row before; the kept rows of a
    sample are packed to the front, and samples shorter than the longest (T rows) repeat their last kept row.
    Returns [..., T, C], and with ``return_lengths=True`` also the int32 kept count per sample [...].

    T is data dependent: sizing the output reads ONE int32 back from the device, the only synchronisation of the call.
    Unlike the reference, which overwrites the linear channels and the first row of its argument, ``x`` is never modified.
    An empty ``rectilinear_indices`` gives ``linear_interpolation_coeffs(x, initial_value_if_nan=0.0)``."""
    _hybrid_args(x, rectilinear_indices, time_index)
    x3 = _check(x)
    B, L, C = x3.shape
    dev = x.device
    lin_idx = [c for c in range(C) if c != time_index and c not in rectilinear_indices]
    n_rect, lib = len(rectilinear_indices), _lib.lib()
    xf = _fill(x3, 0.0, True)                                                  # time and the rectilinear channels as the table holds them
    xl = None
    if lin_idx:
        xl = linear_interpolation_coeffs(x3[..., lin_idx].contiguous(), initial_value_if_nan=0.0)      # the existing NaN fill, gathered channels
    rect = torch.tensor(sorted(rectilinear_indices), dtype=torch.int32, device=dev) if n_rect else None
    need = _lib.check(lib.ncde_prepare_hybrid_workspace_bytes(B, L, C), "ncde_prepare_hybrid_workspace_bytes")
    ws = torch.empty(int(need), dtype=torch.uint8, device=dev)
    lengths = torch.empty(B + 1, dtype=torch.int32, device=dev)                 # [B] kept counts | their maximum
    with torch.cuda.device(dev):
        rc = lib.ncde_prepare_hybrid_count(xf.data_ptr(), B, L, C, None if rect is None else rect.data_ptr(), n_rect, ws.data_ptr(), ws.numel(),
                                           lengths.data_ptr(), lengths[B:].data_ptr(), _stream())
        _lib.check(rc, "ncde_prepare_hybrid_count")
        T = int(lengths[B].item())                                             # the one device-to-host read
        out = torch.empty(B, T, C, dtype=torch.float32, device=dev)
        rc = lib.ncde_prepare_hybrid_write(xf.data_ptr(), None if xl is None else xl.data_ptr(), B, L, C, n_rect, ws.data_ptr(), ws.numel(),
                                           lengths.data_ptr(), T, out.data_ptr(), _stream())
        _lib.check(rc, "ncde_prepare_hybrid_write")
    out = out.reshape(*x.shape[:-2], T, C)
    return (out, lengths[:B].reshape(x.shape[:-2])) if return_lengths else out


def natural_cubic_coeffs(x, t=None):
    """a | b | 2c | 3d of the natural cubic spline through x; NaNs are missing values."""
    x3 = _check(x)
    B, L, C = x3.shape
    tg = _grid(t, L, x.device)
    out = torch.empty(B, L - 1, 4 * C, dtype=torch.float32, device=x.device)
    need = _lib.check(_lib.lib().ncde_prepare_workspace_bytes(_lib.INTERP["cubic"], B, L, C), "ncde_prepare_workspace_bytes")
    ws = torch.empty(int(need), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        rc = _lib.lib().ncde_prepare_cubic_grid(x3.data_ptr(), None if tg is None else tg.data_ptr(), B, L, C, out.data_ptr(), ws.data_ptr(),
                                                ws.numel(), _stream())
    _lib.check(rc, "ncde_prepare_cubic_grid")
    return out.reshape(*x.shape[:-2], L - 1, 4 * C)


natural_cubic_spline_coeffs = natural_cubic_coeffs


def hermite_cubic_coefficients_with_backward_differences(x, t=None, initial_value_if_nan=None, forward_fill=False):
    """a | b | 2c | 3d of the Hermite cubic with backward differences (upstream torchcde's function of this name): the piece on
    [t_i, t_i+1] goes from knot i to knot i+1, starts with the slope of the linear piece before it (its own for i = 0, so the first
    piece is linear) and ends with its own.  The knots are ``linear_interpolation_coeffs(x, t, None, initial_value_if_nan,
    forward_fill)``; with both causal options piece i depends on x[..., :i+2, :] only -- the smooth path that can be stepped online
    (``NeuralCDE(interpolation="cubic_hermite").online``).  include/ncde_hip.h states the formulas (ncde_prepare_hermite).
    [..., L, C] fp32 CUDA -> [..., L-1, 4C], read by ``CubicSpline`` / ``NaturalCubicSpline``.  ``x`` is never modified."""
    knots = linear_interpolation_coeffs(x, t=t, initial_value_if_nan=initial_value_if_nan, forward_fill=forward_fill)      # (validates x and t)
    k3 = knots.reshape(-1, x.size(-2), x.size(-1))
    B, L, C = k3.shape
    tg = _grid(t, L, x.device)
    out = torch.empty(B, L - 1, 4 * C, dtype=torch.float32, device=x.device)
    if out.numel():
        with torch.cuda.device(x.device):
            rc = _lib.lib().ncde_prepare_hermite(k3.data_ptr(), None if tg is None else tg.data_ptr(), B, L, C, out.data_ptr(), _stream())
        _lib.check(rc, "ncde_prepare_hermite")
    return out.reshape(*x.shape[:-2], L - 1, 4 * C)
