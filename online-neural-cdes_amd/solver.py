"""``cdeint``: drop-in for ``torchcde.cdeint`` (/root/reference/modules/torchcde/torchcde/solver.py:140-238)
backed by the fused HIP kernels behind the C-ABI of include/ncde_hip.h.

What the reference does per call -- wrap (X, func) in a vector field, hand it to torchdiffeq's Python
time loop (solvers.py:94-119) and, for the backward pass, to OdeintAdjointMethod (adjoint.py:37-145)
-- happens here in ONE kernel launch per direction.  There is no CPU fallback.  What the fused kernels do
not cover but the reference accepts (an arbitrary ``func``, decreasing output times, gradients of the control
path under the continuous adjoint or of ``t``, non-fp32 tensors, shapes no fused kernel exists for -- hidden widths beyond 256 in training)
runs on the package's own UNFUSED torch-op solver on the GPU (unfused.py) behind a one-time UserWarning naming
the reason; what neither path covers raises NotImplementedError.
"""
import ctypes
import warnings

import numpy as np
import torch

from . import _lib
from .interpolation import LinearInterpolation, NaturalCubicSpline, SmoothLinearInterpolation

_FIXED_METHODS = ("euler", "midpoint", "rk4")
_ALL_METHODS = ("dopri8", "dopri5", "bosh3", "fehlberg2", "adaptive_heun", "euler", "midpoint", "rk4",
                "explicit_adams", "implicit_adams", "fixed_adams", "scipy_solver")


class FieldSpec:
    """What the fused kernels need to know about ``func``: the Linear+ReLU stack (entries may repeat
    the same Parameters = a shared layer) and the final Linear (+tanh, viewed [H, C])."""

    def __init__(self, layers, Wo, bo, kind="original", mode="matmul", Wg=None, bg=None, Wr=None, br=None, rank=0):
        self.layers = list(layers)
        self.Wo, self.bo = Wo, bo
        # variants (src/ncde/vector_fields/gating.py; vector_field_type of solver.py:112-137)
        self.kind, self.mode = kind, mode
        self.Wg, self.bg, self.Wr, self.br = Wg, bg, Wr, br
        # kind "lowrank" (src/ncde/vector_fields/sparsity.py:33-55): Wo, bo = M_h [H * rank, .], Wg, bg = M_o [rank * C, .]
        self.rank = int(rank)

    def extra_params(self):
        out = []
        if self.kind == "gru":
            out += [self.Wr, self.br]
        if self.kind in ("minimal", "gru", "lowrank"):
            out += [self.Wg, self.bg]
        return out

    def unique_params(self):
        seen, out = set(), []
        for p in [q for wb in self.layers for q in wb] + self.extra_params() + [self.Wo, self.bo]:
            if id(p) not in seen:
                seen.add(id(p))
                out.append(p)
        return out


def _field_spec(func):
    if hasattr(func, "fused_spec"):
        return func.fused_spec()
    raise NotImplementedError(      # (not reached from cdeint: a func without fused_spec() is routed to the unfused solver)
        "a fused kernel call needs `func` to expose fused_spec() (e.g. ncde_amd.OriginalVectorField or ncde_amd.MLPField)")


def _unfused_reason(X, func, z0, t, adjoint, adjoint_params, method=None):
    """Why this call cannot run on the fused kernels (None = it can).  Such calls run on the unfused torch-op solver
    (unfused.py) -- on the GPU: CPU tensors stay refused, there is no CPU fallback."""
    if not torch.is_tensor(z0):
        return None      # tuple-valued z0: refused further down, on either path
    if not hasattr(func, "fused_spec"):
        return "func does not expose fused_spec()"
    if method == "dopri5" and isinstance(X, SmoothLinearInterpolation) and X.gradient_matching_eps is not None:
        # (a free-running adaptive solve parts ways between the path's two round-off-equivalent forms -- the class's region rule and
        # the refined polynomial pieces -- as soon as one step is accepted on one side and rejected on the other: DESIGN.md)
        return "method='dopri5' on a smoothed-linear control path"
    if method == "dopri5":      # the adaptive kernels evaluate the original field with the matmul input only
        spec = func.fused_spec()
        if spec.kind != "original" or spec.mode != "matmul":
            return "method='dopri5' with a gated or low-rank vector field or the evaluate / derivative input"
    # decreasing output times?  X.interval / X.grid_points are tagged and known to increase: no device sync for them
    # (ADVICE round 4); any other tensor is copied to the host ONCE (_host_times, shared with _time_mode / _time_plan).
    if not _is_tagged_time(X, t):
        tv = _host_times(t)
        if tv.dim() == 1 and tv.numel() >= 2 and bool(tv[0] > tv[1]):
            return "decreasing output times"
    if torch.is_tensor(t) and t.requires_grad:
        return "the output times require gradients"
    ap = set(id(q) for q in adjoint_params) if adjoint_params is not None else set()
    for buffer in X.buffers():
        if buffer.requires_grad and (not adjoint or id(buffer) in ap):
            return "the control path requires gradients"
    if z0.is_cuda and (z0.dtype != torch.float32 or X._coeffs.dtype != torch.float32):
        return "tensors are not fp32"
    return None


def _is_tagged_time(X, t):
    """True for X's own interval / grid_points tensors (tagged by interpolation.py; a weakref, so a recycled id() of a dead
    control can never match): their values are known without looking at the device."""
    kind = getattr(t, "_ncde_kind", None)
    owner = getattr(t, "_ncde_owner", None)
    return kind is not None and owner is not None and owner() is X and t.numel() == (X.n_knots if kind == "knots" else 2)


def _host_times(t):
    """Host copy (fp64) of the output times: at most ONE device-to-host copy per tensor version, kept on the tensor object."""
    if not torch.is_tensor(t):
        return torch.as_tensor(t).detach().double()
    hit = getattr(t, "_ncde_host", None)
    if hit is not None and hit[0] == t._version:
        return hit[1]
    tv = t.detach().cpu().double()
    try:
        t._ncde_host = (t._version, tv)
    except Exception:      # (a tensor subclass that refuses attributes)
        pass
    return tv


def _time_mode(X, t):
    """-> _lib.OUT_INTERVAL / OUT_KNOTS.  Tagged tensors from X.interval / X.grid_points avoid a device sync."""
    if X._default_grid and _is_tagged_time(X, t):     # a control on a user knot grid always takes the time plan
        return _lib.OUT_KNOTS if t._ncde_kind == "knots" else _lib.OUT_INTERVAL
    tv = _host_times(t)
    assert tv.dim() == 1, "t must be one dimensional"
    assert (tv[1:] > tv[:-1]).all(), "t must be strictly increasing or decreasing"  # misc.py:336-343
    n = X.n_knots
    if X._default_grid:
        if tv.numel() == n and torch.equal(tv, torch.arange(n, dtype=torch.double)):
            return _lib.OUT_KNOTS
        if tv.numel() == 2 and tv[0] == 0 and tv[1] == n - 1:
            return _lib.OUT_INTERVAL
    return None     # any other increasing t: the general time axis (time plan)


_PLAN_CACHE = {}    # (method, step, t bytes, t dtype, knot bytes, n_knots, device) -> (device plan, info)


def _time_plan(X, t, method, step, device):
    """Build (once per distinct time axis) the table the plan-driven kernels walk: ncde_time_plan_build evaluates the
    reference's grid / stage-time / knot-index arithmetic on the host (solvers.py:78-87, 103-117; one device sync for t)."""
    tt = torch.as_tensor(t).detach()
    f64 = tt.dtype == torch.float64
    tv = np.ascontiguousarray(_host_times(t).numpy())
    # (the grid the kernels walk: X's own knots, except for a smoothed-linear path, whose polynomial pieces sit on a refined grid
    # while X.n_knots / X.grid_points keep describing the integer one)
    kn, n_knots = X._plan_grid()
    kn = None if kn is None else np.ascontiguousarray(kn.detach().cpu().double().numpy())
    key = (method, float(step), tv.tobytes(), f64, None if kn is None else kn.tobytes(), n_knots, str(device))
    hit = _PLAN_CACHE.get(key)
    if hit is not None:
        return hit
    p = _lib.NcdeProblem()
    p.abi_version, p.n_knots, p.method = _lib.NCDE_ABI_VERSION, n_knots, _lib.METHOD[method]
    dp = ctypes.POINTER(ctypes.c_double)
    ts = _lib.NcdeTimeSpec(n_t=len(tv), time_is_f64=int(f64), t=tv.ctypes.data_as(dp), step_size=float(step),
                           knots=None if kn is None else kn.ctypes.data_as(dp))
    info = _lib.NcdeTimePlanInfo()
    lib = _lib.lib()
    rc = lib.ncde_time_plan_build(ctypes.byref(p), ctypes.byref(ts), None, 0, ctypes.byref(info))
    if rc == -1:
        raise AssertionError(lib.ncde_last_error_string().decode())       # misc.py:336-343 asserts on a non-monotone t
    _lib.check(rc, "ncde_time_plan_build")
    buf = np.zeros(info.bytes // 4, dtype=np.int32)
    _lib.check(lib.ncde_time_plan_build(ctypes.byref(p), ctypes.byref(ts), buf.ctypes.data, buf.nbytes, ctypes.byref(info)),
               "ncde_time_plan_build")
    plan = torch.from_numpy(buf).to(device)
    hit = (plan, (info.n_t_out, info.n_steps_fwd, info.n_steps_adj))
    if len(_PLAN_CACHE) > 64:
        _PLAN_CACHE.clear()
    _PLAN_CACHE[key] = hit
    return hit


def build_problem(coeffs, interp, z0, spec, method, output, flags=0, plan=None):
    """Fill an NcdeProblem from torch tensors (all must stay alive while the call is in flight)."""
    p = _lib.NcdeProblem()
    p.abi_version = _lib.NCDE_ABI_VERSION
    B, H = z0.shape
    p.batch, p.hidden = B, H
    if interp == "linear":
        p.n_knots, p.channels = coeffs.shape[1], coeffs.shape[2]
    else:      # piecewise polynomial: one row of a | b | 2c | 3d [| 4e | 5f] per piece
        p.n_knots, p.channels = coeffs.shape[1] + 1, coeffs.shape[2] // _lib.INTERP_PARTS[interp]
    p.interp = _lib.INTERP[interp]
    p.method = _lib.METHOD[method]
    p.output = output
    p.flags = flags
    if len(spec.layers) > _lib.NCDE_MAX_LAYERS:
        raise NotImplementedError("at most %d hidden layers" % _lib.NCDE_MAX_LAYERS)
    p.n_layers = len(spec.layers)
    for i, (w, b) in enumerate(spec.layers):
        p.layer_out[i], p.layer_in[i] = w.shape
        p.layer_W[i], p.layer_b[i] = w.data_ptr(), b.data_ptr()
    p.Wo, p.bo = spec.Wo.data_ptr(), spec.bo.data_ptr()
    d_last = spec.layers[-1][0].shape[0] if spec.layers else H
    rows = H * p.channels if spec.mode == "matmul" else H
    rows_g = rows
    if spec.kind == "lowrank":      # M_h [H * R, .] and M_o [R * C, .]; the rank travels in the top byte of flags
        if not 1 <= spec.rank <= 255:
            raise ValueError("low-rank field: rank %d outside [1, 255]" % spec.rank)
        rows, rows_g = H * spec.rank, spec.rank * p.channels
        p.flags = flags | _lib.FLAG_FIELD_RANK(spec.rank)
    if tuple(spec.Wo.shape) != (rows, d_last):
        raise ValueError("final layer must be [%d, %d], got %s" % (rows, d_last, tuple(spec.Wo.shape)))
    p.field_kind, p.field_input = _lib.FIELD_KIND[spec.kind], _lib.FIELD_INPUT[spec.mode]
    if spec.kind != "original":
        if tuple(spec.Wg.shape) != (rows_g, d_last):
            raise ValueError("second head must be [%d, %d], got %s" % (rows_g, d_last, tuple(spec.Wg.shape)))
        p.Wg, p.bg = spec.Wg.data_ptr(), spec.bg.data_ptr()
    if spec.kind == "gru":
        d0 = H if spec.mode == "matmul" else H + p.channels
        if tuple(spec.Wr.shape) != (d0, d0):
            raise ValueError("reset net must be [%d, %d], got %s" % (d0, d0, tuple(spec.Wr.shape)))
        p.Wr, p.br = spec.Wr.data_ptr(), spec.br.data_ptr()
    p.coeffs = coeffs.data_ptr()
    p.coeffs_stride_b, p.coeffs_stride_t = coeffs.stride(0), coeffs.stride(1)
    p.z0 = z0.data_ptr()
    if plan is not None:          # general time axis: (device table, (n_t_out, n_steps_fwd, n_steps_adj))
        p.output = _lib.OUT_TIMES
        p.time_plan = plan[0].data_ptr()
        p.n_t_out, p.n_steps_fwd, p.n_steps_adj = plan[1]
    return p


def _stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_ARENA = {}      # (device index, stream, host thread) -> one byte tensor, grown on demand and reused by every solve issued there
_ARENA_MAX = 32


def clear_workspace_arena():
    """Drop every cached workspace (they are ordinary torch allocations: torch.cuda.empty_cache() can then return the memory)."""
    _ARENA.clear()


def _workspace_bytes(need, device):
    """Scratch for one C-ABI call: an arena per (device, stream, host thread) instead of an allocation per call.  The kernels are
    stream-ordered and a workspace is dead when its call's kernels are, so consecutive calls issued by ONE thread on ONE stream may
    share it.  Two host threads on the same stream could interleave their launches (ctypes drops the GIL) -- A's main kernel, B's
    main kernel, A's reduction reading B's partials -- so the thread is part of the key; entries of dead streams / threads are
    pruned once the table grows."""
    import threading
    need = max(int(need), 256)
    dev = torch.device(device)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(dev).cuda_stream,
           threading.get_ident())
    buf = _ARENA.get(key)
    if buf is None or buf.numel() < need:
        if len(_ARENA) >= _ARENA_MAX:
            _ARENA.clear()
        buf = torch.empty(need + need // 8, dtype=torch.uint8, device=dev)
        _ARENA[key] = buf
    return buf[:need]


def _workspace(p, pass_, device):
    return _workspace_bytes(_lib.check(_lib.lib().ncde_workspace_bytes(ctypes.byref(p), pass_), "ncde_workspace_bytes"), device)


# ---- the cooperative kernels' status word (include/ncde_hip.h: ncde_coop_status_offset) -------------------------------------------
# A cooperative launch that gives up (bounded spin: its workgroups never all became resident) is re-executed INSIDE the library by the
# per-workgroup kernels, so the tensors this module returns are correct either way.  What is left to the host is to notice -- the call
# took seconds longer -- and to stop asking for the cooperative path: after every call that could launch one, the status word is copied
# (stream-ordered, asynchronously) into a pinned host slot; the slots of finished calls are looked at -- without synchronising
# anything -- at the start of the next fused call, and a set word warns once and adds FLAG_NO_COOP to every later call on that device.
_COOP_SLOTS = {}         # device index -> (pinned int32 ring, next slot)
_COOP_PENDING = []       # (device index, pinned slot view, event)
_COOP_DISABLED = {}      # device index -> number of calls whose cooperative launches gave up


def _coop_track(p, pass_, ws, dev):
    off = _lib.lib().ncde_coop_status_offset(ctypes.byref(p), pass_)
    if off < 0:
        return
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    ring, nxt = _COOP_SLOTS.get(idx, (None, 0))
    if ring is None:
        ring = torch.zeros(256, dtype=torch.int32).pin_memory()
    if len(_COOP_PENDING) >= 192:      # (a caller that never comes back through cdeint: look now, blocking on the oldest)
        coop_status(wait=True)
    slot = ring[nxt:nxt + 1]
    slot.copy_(ws[int(off):int(off) + 4].view(torch.int32), non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    _COOP_PENDING.append((idx, slot, ev))
    _COOP_SLOTS[idx] = (ring, (nxt + 1) % 256)


def coop_status(wait=False):
    """Look at the status words of the fused calls issued so far (``wait=True``: of all of them, synchronising on their events;
    default: of those the GPU has finished).  Returns {device index: number of calls in which a cooperative launch gave up and the
    per-workgroup kernels re-executed the pass}; such a device no longer gets cooperative launches from this process."""
    keep = []
    for idx, slot, ev in _COOP_PENDING:
        if wait:
            ev.synchronize()
        if not ev.query():
            keep.append((idx, slot, ev))
            continue
        if int(slot[0]) != 0:
            if idx not in _COOP_DISABLED:
                warnings.warn("ncde_amd: a cooperative (XCD-wide) kernel launch on cuda:%d timed out -- its workgroups never all became "
                              "resident (another process's kernels on the GPU, a CU mask?).  The pass was re-executed on the per-workgroup "
                              "kernels, so the results are correct; this process now passes FLAG_NO_COOP on that device." % idx, RuntimeWarning)
            _COOP_DISABLED[idx] = _COOP_DISABLED.get(idx, 0) + 1
    _COOP_PENDING[:] = keep
    return dict(_COOP_DISABLED)


def _coop_flags(flags, device):
    """`flags` + FLAG_NO_COOP once a cooperative launch has given up on `device` (looked up without synchronising)."""
    if _COOP_PENDING:
        coop_status()
    idx = device.index if device.index is not None else torch.cuda.current_device()
    return flags | _lib.FLAG_NO_COOP if idx in _COOP_DISABLED else flags


def _check_tensor(x, name):
    if not (x.is_cuda and x.dtype == torch.float32):
        raise NotImplementedError("cdeint fused path needs fp32 tensors on the GPU; %s is %s on %s" % (name, x.dtype, x.device))


class BoundGrads:
    """What `bind_grads` returns: `g` (the NcdeGrads), `grad_z0` and `bufs` ({id(parameter): its gradient buffer}; `of(q)` looks one up)."""

    def __init__(self, g, grad_z0, bufs):
        self.g, self.grad_z0, self.bufs = g, grad_z0, bufs

    def of(self, q):
        return self.bufs[id(q)]


def bind_grads(spec, z0_shape, device, live=None, fill=None):
    """Allocate the destinations of one backward call and fill its NcdeGrads: one contiguous buffer per UNIQUE parameter (a shared
    layer is bound to the same buffer at every layer index), the sigmoid head for the gated fields, the reset net for the GRU one.
    live: ids of the parameters that get a destination -- the others keep NULL, which for the dopri5 adjoint means "not part of the
    augmented state", hence not of the mixed error norm (adjoint.py:176-189); None binds every parameter.
    fill: a value to initialise every buffer with (tests: NaN proves that a call wrote every element)."""
    new = (lambda x: x) if fill is None else (lambda x: x.fill_(fill))
    bufs = {id(q): new(torch.empty_like(q, memory_format=torch.contiguous_format)) for q in spec.unique_params()}
    grad_z0 = new(torch.empty(z0_shape, dtype=torch.float32, device=device))
    ptr = lambda q: bufs[id(q)].data_ptr() if live is None or id(q) in live else None      # noqa: E731
    g = _lib.NcdeGrads()
    g.grad_z0 = grad_z0.data_ptr()
    for i, (w, b) in enumerate(spec.layers):
        g.grad_layer_W[i], g.grad_layer_b[i] = ptr(w), ptr(b)
    g.grad_Wo, g.grad_bo = ptr(spec.Wo), ptr(spec.bo)
    if spec.kind != "original":
        g.grad_Wg, g.grad_bg = ptr(spec.Wg), ptr(spec.bg)
    if spec.kind == "gru":
        g.grad_Wr, g.grad_br = ptr(spec.Wr), ptr(spec.br)
    return BoundGrads(g, grad_z0, bufs)


def _num_outputs(coeffs, interp, output, plan):
    """Rows of the solution: the plan's output times, every knot of the control, or the two ends of the interval."""
    if plan is not None:
        return plan[1][0]
    return coeffs.shape[1] + (0 if interp == "linear" else 1) if output == _lib.OUT_KNOTS else 2


def _alloc_out(z0, n_out):
    return torch.empty(z0.shape[0], n_out, z0.shape[1], dtype=torch.float32, device=z0.device)


def _launch_forward(p, out, record, dev):
    """ncde_forward, or with `record` ncde_forward_record (-> the stage record, else None), of `p` into `out`; the cooperative
    status word is tracked and rc checked under the name of the entry point that was called."""
    lib = _lib.lib()
    stages = None
    with torch.cuda.device(dev):   # the C-ABI launches on the calling thread's current device / stream
        ws = _workspace(p, 0, dev)
        if record:
            nbytes = _lib.check(lib.ncde_stage_record_bytes(ctypes.byref(p)), "ncde_stage_record_bytes")
            stages = torch.empty(max(int(nbytes) // 4, 1), dtype=torch.float32, device=dev)
            rc = lib.ncde_forward_record(ctypes.byref(p), out.data_ptr(), stages.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr())
        else:
            rc = lib.ncde_forward(ctypes.byref(p), out.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr())
        if rc >= 0:
            _coop_track(p, 0, ws, dev)
    _lib.check(rc, "ncde_forward_record" if record else "ncde_forward")
    return stages


class _FusedCdeint(torch.autograd.Function):
    """adjoint=True : forward = ncde_forward, backward = ncde_adjoint (continuous adjoint, adjoint.py:37-145).
    adjoint=False: forward = ncde_forward_record (solution + every stage input), backward = ncde_backward, the exact
    transpose of the discretised solve -- the gradients autograd produces in the reference when ``odeint`` is
    taped (solver.py:224), without a tape.
    cfg["control"] (adjoint=False with a coefficient tensor that requires grad; a stacked CDE: layer i's hidden sequence is layer
    i+1's linear coefficients): `coeffs` is a differentiable input, the forward keeps its usual route and the backward is
    ncde_backward_control -- ncde_backward on the batch-tiled family plus dL/dcoeffs (pass C: ncde_dctl_tiled + ncde_dctl_fold).
    cfg["smooth"] = (rows, eps) on that route (a cubic-smoothed control): `coeffs` is still the differentiable input, the LINEAR
    coefficients [B, T, C]; the kernels read `rows`, the a | b | 2c | 3d tensor ncde_prepare_smooth built from them, and the backward
    folds ncde_backward_control's dL/d(rows) back onto the linear coefficients with ncde_prepare_smooth_backward."""

    @staticmethod
    def forward(ctx, z0, coeffs, cfg, *params):
        control = bool(cfg.get("control"))
        if control:
            ctx.x_shape = coeffs.shape
            coeffs = cfg["smooth"][0] if cfg.get("smooth") else coeffs.detach()
        z0c = z0.detach().contiguous()
        p = build_problem(coeffs, cfg["interp"], z0c, cfg["spec"], cfg["method"], cfg["output"], cfg["flags"], cfg["plan"])
        out = _alloc_out(z0, _num_outputs(coeffs, cfg["interp"], cfg["output"], cfg["plan"]))
        record = (not cfg["adjoint"]) and cfg.get("needs_grad", True) and any(ctx.needs_input_grad)
        stages = _launch_forward(p, out, record, z0.device)
        ctx.cfg, ctx.z0_shape, ctx.recorded = cfg, z0.shape, record
        ctx.coeffs = None if control else coeffs
        ctx.save_for_backward(out, *([stages] if record else []), *([coeffs] if control else []), *params)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable     # the kernels are not themselves differentiable: no create_graph
    def backward(ctx, grad_out):
        cfg = ctx.cfg
        control = bool(cfg.get("control"))
        params = list(ctx.saved_tensors)
        out = params.pop(0)
        stages = params.pop(0) if ctx.recorded else None
        coeffs = params.pop(0) if control else ctx.coeffs
        spec, dev = cfg["spec"], out.device
        grad_out = grad_out.contiguous().float()
        z0 = out[:, 0]     # only its shape matters here: the backward kernels never read z0 (row 0 of `out` is a valid pointer)
        p = build_problem(coeffs, cfg["interp"], z0, spec, cfg["method"], cfg["output"], cfg["flags"], cfg["plan"])
        bound = bind_grads(spec, ctx.z0_shape, dev)
        grad_coeffs = torch.empty(coeffs.shape, dtype=torch.float32, device=dev) if control else None
        lib = _lib.lib()
        with torch.cuda.device(dev):
            if control:
                name = "ncde_backward_control"
                ws = _workspace_bytes(_lib.check(lib.ncde_control_workspace_bytes(ctypes.byref(p)), "ncde_control_workspace_bytes"), dev)
                rc = lib.ncde_backward_control(ctypes.byref(p), stages.data_ptr(), grad_out.data_ptr(), ctypes.byref(bound.g),
                                               grad_coeffs.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr())
                if rc >= 0 and cfg.get("smooth"):      # dL/d(rows) -> dL/d(linear coefficients), same stream
                    name = "ncde_prepare_smooth_backward"
                    B, T, C = ctx.x_shape
                    grad_rows, grad_coeffs = grad_coeffs, torch.empty(ctx.x_shape, dtype=torch.float32, device=dev)
                    rc = lib.ncde_prepare_smooth_backward(grad_rows.data_ptr(), B, T, C, float(cfg["smooth"][1]), 3, grad_coeffs.data_ptr(),
                                                          _stream_ptr())
            elif ctx.recorded:
                name = "ncde_backward"
                ws = _workspace(p, 2, dev)
                rc = lib.ncde_backward(ctypes.byref(p), stages.data_ptr(), grad_out.data_ptr(), ctypes.byref(bound.g),
                                       ws.data_ptr(), ws.numel(), _stream_ptr())
            else:
                name = "ncde_adjoint"
                ws = _workspace(p, 1, dev)
                rc = lib.ncde_adjoint(ctypes.byref(p), out.data_ptr(), grad_out.data_ptr(), ctypes.byref(bound.g),
                                      ws.data_ptr(), ws.numel(), _stream_ptr())
            if rc >= 0 and not control:      # (the control route pins NCDE_FLAG_NO_COOP: nothing cooperative to track)
                _coop_track(p, 2 if ctx.recorded else 1, ws, dev)
        _lib.check(rc, name)
        if not ctx.recorded and cfg["func"] is not None and hasattr(cfg["func"], "nfe"):
            cfg["func"].nfe += cfg["nfe_adjoint"]   # the adjoint sweep re-evaluates f (base.py:90); autograd does not
        keep = cfg.get("adjoint_param_ids")     # adjoint_params of odeint_adjoint (adjoint.py:176-183): others get no gradient
        grads = [bound.of(q) if needs and (keep is None or id(q) in keep) else None for q, needs in zip(params, ctx.needs_input_grad[3:])]
        return (bound.grad_z0 if ctx.needs_input_grad[0] else None, grad_coeffs if ctx.needs_input_grad[1] else None, None, *grads)


_CONTROL_REASON = "the control path requires gradients"


def _control_route(reason, adjoint, method, plain_control, cuda_fp32, coeffs_grad, other_grad, t_grad):
    """The routing decision on plain values: a call that `_unfused_reason` sends away for `reason` may take the fused
    control-gradient route iff adjoint=False, a fixed-step method, a plain LinearInterpolation / NaturalCubicSpline or a cubic-smoothed
    SmoothLinearInterpolation (`plain_control`), z0 and the coefficients CUDA fp32 (`cuda_fp32`), the coefficient tensor requires grad
    and is the control's only buffer that does (knots that require grad stay unfused), and `t` does not."""
    return bool(reason == _CONTROL_REASON and not adjoint and method in _FIXED_METHODS and plain_control and cuda_fp32 and
                coeffs_grad and not other_grad and not t_grad)


def _cubic_smoothed(X):
    """A SmoothLinearInterpolation whose fused form is an a | b | 2c | 3d tensor with a transpose kernel (ncde_prepare_smooth_backward):
    cubic matching on the integer grid.  Quintic matching, no smoothing at all and a user `t` are not."""
    return (type(X) is SmoothLinearInterpolation and X.gradient_matching_eps is not None and not X.match_second_derivatives
            and X._integer_grid)


def _control_route_ok(reason, X, z0, t, adjoint, method):
    """`_control_route` of a call's arguments (looks at the arguments only: type, device, dtype, requires_grad)."""
    if not (type(X) in (LinearInterpolation, NaturalCubicSpline) or _cubic_smoothed(X)) or not torch.is_tensor(z0):
        return False
    coeffs = X._coeffs
    cuda_fp32 = z0.is_cuda and coeffs.is_cuda and z0.dtype == torch.float32 and coeffs.dtype == torch.float32
    other_grad = any(b.requires_grad for b in X.buffers() if b is not coeffs)
    return _control_route(reason, adjoint, method, True, cuda_fp32, coeffs.requires_grad, other_grad, torch.is_tensor(t) and t.requires_grad)


_STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}


def _fixed_axis(X, t, method, step, device):
    """-> (output, plan, nfe, nfe_adjoint) of a fixed-step solve: the default axis when `_time_mode` recognises X's own interval /
    knots under step 1, else the time plan.  None for a `t` the plan cannot take (not one-dimensional): the caller reports it."""
    output = _time_mode(X, t) if float(step) == 1.0 else None
    if output is not None:
        nfe = _STAGES[method] * (X.n_knots - 1)
        return output, None, nfe, nfe
    tq = torch.as_tensor(t)
    if tq.dim() != 1:
        return None
    plan = _time_plan(X, tq, method, step, device)
    return _lib.OUT_TIMES, plan, _STAGES[method] * plan[1][1], _STAGES[method] * plan[1][2]


def _flatten_batch(z0, coeffs):
    """Any number of batch dimensions, as the reference allows, flattened for the kernels: z0 [B, H], coeffs [B, T, K] with unit
    stride in K and rows that do not overlap.  `_restore_batch` undoes it on the solution.  The batch and time strides are handed to
    the kernels as they are (include/ncde_hip.h: any batch stride >= 0, a time stride of at least one row); a time stride smaller than
    the row -- a constant path expanded over time has 0 -- is copied, as a non-unit channel stride is."""
    if z0.dim() != 2:
        z0 = z0.reshape(-1, z0.shape[-1])
        coeffs = coeffs.reshape(-1, coeffs.shape[-2], coeffs.shape[-1])
    if coeffs.stride(2) != 1 or coeffs.stride(1) < coeffs.shape[2]:
        coeffs = coeffs.contiguous()
    return z0, coeffs


def _restore_batch(out, batch_shape):
    return out if len(batch_shape) == 1 else out.reshape(*batch_shape, out.shape[-2], out.shape[-1])


def _fused_control(X, func, z0, t, vector_field_type, method, options, flags):
    """The fused control-gradient route of a call `_control_route_ok` accepted, or None when anything about it is outside what
    ncde_backward_control covers (options beyond a positive step_size, a gated field or direct input, parameters that are not
    contiguous CUDA fp32, a shape beyond the batch-tiled backward): the caller then runs the unfused solver as before."""
    if set(options) - {"step_size", "perturb"} or options.get("perturb") or options.get("step_size") is None:
        return None
    step = options["step_size"]
    step = step.item() if torch.is_tensor(step) else step
    if not float(step) > 0.0 or z0.dim() < 1:
        return None
    coeffs = X._coeffs
    batch_shape = z0.shape[:-1]
    if coeffs.dim() < 2 or tuple(coeffs.shape[:-2]) != tuple(batch_shape):
        return None
    spec = func.fused_spec()
    uniq = spec.unique_params()
    if spec.kind != "original" or spec.mode != "matmul" or vector_field_type != "matmul" or not spec.layers:
        return None
    if not all(q.is_cuda and q.dtype == torch.float32 and q.is_contiguous() for q in uniq):
        return None
    z0, coeffs = _flatten_batch(z0, coeffs)
    smooth = None
    if _cubic_smoothed(X):      # the kernels read the refined rows (built from the detached coefficients, cached per tensor version)
        rows = X.fused_coeffs
        smooth = (rows.reshape(-1, rows.shape[-2], rows.shape[-1]), X.gradient_matching_eps)
    flags = _coop_flags(flags, z0.device)
    axis = _fixed_axis(X, t, method, step, z0.device)
    if axis is None:
        return None
    output, plan, nfe, _ = axis
    p = build_problem(smooth[0] if smooth else coeffs.detach(), X.interp_name, z0.detach(), spec, method, output, flags, plan)
    lib = _lib.lib()
    if lib.ncde_control_workspace_bytes(ctypes.byref(p)) < 0 or lib.ncde_workspace_bytes(ctypes.byref(p), 0) < 0:
        return None
    cfg = {"spec": spec, "interp": X.interp_name, "method": method, "output": output, "flags": flags, "plan": plan,
           "needs_grad": torch.is_grad_enabled(), "adjoint": False, "control": True, "smooth": smooth}
    out = _FusedCdeint.apply(z0, coeffs, cfg, *uniq)
    if hasattr(func, "nfe"):
        func.nfe += nfe
    return _restore_batch(out, batch_shape)


class _AdaptiveSpec:
    """Host description of one dopri5 call: output times / knots as host doubles + NcdeAdaptiveOptions."""

    def __init__(self, X, t, rtol, atol, options):
        tt = torch.as_tensor(t).detach()
        self.tv = np.ascontiguousarray(tt.cpu().double().numpy())
        assert self.tv.ndim == 1, "t must be one dimensional"
        assert (self.tv[1:] > self.tv[:-1]).all() or (self.tv[1:] < self.tv[:-1]).all(), "t must be strictly increasing or decreasing"
        if self.tv[1] < self.tv[0]:
            raise NotImplementedError("decreasing output times are outside the fused path")
        self.kn = None if X._default_grid else np.ascontiguousarray(X._t.detach().cpu().double().numpy())
        dp = ctypes.POINTER(ctypes.c_double)
        self.ts = _lib.NcdeTimeSpec(n_t=len(self.tv), time_is_f64=1, t=self.tv.ctypes.data_as(dp), step_size=1.0,
                                    knots=None if self.kn is None else self.kn.ctypes.data_as(dp))
        o = _lib.NcdeAdaptiveOptions()
        o.rtol, o.atol = float(rtol), float(atol)
        for k in ("min_step", "max_step", "first_step", "safety", "ifactor", "dfactor"):
            if options.get(k) is not None:
                setattr(o, k, float(options[k]))
        if options.get("max_num_steps") is not None:
            o.max_num_steps = int(options["max_num_steps"])
        self.trace = None
        if options.get("_trace"):           # diagnostics (tests): keep the step sequence (t0, dt, accepted, error ratio)
            self.trace = np.zeros((int(options["_trace"]), 4), dtype=np.float64)
            o.trace_capacity = self.trace.shape[0]
            o.trace = self.trace.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        self.replay = None
        if options.get("_replay") is not None:      # verification (tests): force a recorded step sequence, rows of (dt, accepted)
            self.replay = np.ascontiguousarray(np.asarray(options["_replay"], dtype=np.float64).reshape(-1, 2))
            o.replay_count = self.replay.shape[0]
            o.replay = self.replay.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        self.opt = o


def _dopri5_call(name, cfg, ad, coeffs, z0, pass_, launch, book=None):
    """One adaptive C-ABI call `name` of pass `pass_` (0 forward, 1 adjoint, 2 taped backward) under the time / option structs `ad`:
    builds the problem ("rk4" and OUT_INTERVAL only fill the fields; `ad.ts` carries the output times), sizes the workspace and
    runs `launch(entry point, leading arguments (problem, times, options), trailing arguments (workspace, its size, stream[,
    stats])) -> rc` on z0's device.  book = "forward" / "backward" for the solves that step adaptively: an rc of -1 is the
    reference's assertion (rk_common.py:232-233, 195), and their statistics go to cfg["stats_<book>"], `func.nfe` and, when a trace was
    asked for (diagnostics, tests), `func.dopri5_trace[_backward]`."""
    lib = _lib.lib()
    p = build_problem(coeffs, cfg["interp"], z0, cfg["spec"], "rk4", _lib.OUT_INTERVAL, cfg["flags"])
    stats = _lib.NcdeAdaptiveStats()
    with torch.cuda.device(z0.device):
        need = _lib.check(lib.ncde_dopri5_workspace_bytes(ctypes.byref(p), ctypes.byref(ad.ts), pass_), "ncde_dopri5_workspace_bytes")
        ws = _workspace_bytes(int(need), z0.device)
        tail = (ws.data_ptr(), ws.numel(), _stream_ptr()) + ((ctypes.byref(stats),) if book else ())
        rc = launch(getattr(lib, name), (ctypes.byref(p), ctypes.byref(ad.ts), ctypes.byref(ad.opt)), tail)
    if book and rc == -1:
        raise AssertionError(lib.ncde_last_error_string().decode())
    _lib.check(rc, name)
    if not book:
        return
    cfg["stats_" + book] = (stats.nfe, stats.n_accepted, stats.n_rejected)
    func = cfg["func"]
    if func is not None and ad.trace is not None:
        setattr(func, "dopri5_trace" if book == "forward" else "dopri5_trace_backward", ad.trace[:stats.n_accepted + stats.n_rejected].copy())
    if func is not None and hasattr(func, "nfe"):
        func.nfe += stats.nfe


def _dopri5_forward(z0, coeffs, cfg, taped=False):
    """The adaptive forward solve -> (solution, the contiguous z0 it started from, step record or None).  taped: ncde_dopri5_forward_record
    keeps a record of the accepted steps for ncde_dopri5_backward."""
    ad = cfg["adaptive"]
    z0c = z0.detach().contiguous()
    out = _alloc_out(z0, len(ad.tv))
    rec = None

    def launch_record(fn, head, tail):
        # The record holds one start state per ACCEPTED step; its default size is a guess when the options give no min_step
        # (ncde_dopri5_record_bytes).  A solve that outgrows it reports NCDE_ERR_WORKSPACE: repeat it with twice the record
        # -- the forward is deterministic -- where the reference's autograd tape would simply have grown.
        nonlocal rec
        lib = _lib.lib()
        rbytes = int(_lib.check(lib.ncde_dopri5_record_bytes(*head), "ncde_dopri5_record_bytes"))
        rbytes = int(cfg.get("record_bytes") or rbytes)
        for _ in range(8):
            rec = torch.empty(rbytes, dtype=torch.uint8, device=z0.device)
            rc = fn(*head, out.data_ptr(), rec.data_ptr(), rec.numel(), *tail)
            if rc != -3 or b"record" not in (lib.ncde_last_error_string() or b""):
                break
            rec = None
            rbytes *= 2
        return rc

    if taped:
        _dopri5_call("ncde_dopri5_forward_record", cfg, ad, coeffs, z0c, 0, launch_record, "forward")
    else:
        _dopri5_call("ncde_dopri5_forward", cfg, ad, coeffs, z0c, 0, lambda fn, head, tail: fn(*head, out.data_ptr(), *tail), "forward")
    return out, z0c, rec


class _FusedDopri5(torch.autograd.Function):
    """method='dopri5': forward = ncde_dopri5_forward; backward = ncde_dopri5_adjoint (one adaptive reverse solve per output
    interval, adjoint.py:37-145).  Both calls synchronise: the number of attempts depends on the data."""

    @staticmethod
    def forward(ctx, z0, coeffs, cfg, *params):
        out = _dopri5_forward(z0, coeffs, cfg)[0]
        ctx.cfg, ctx.coeffs, ctx.z0_shape = cfg, coeffs, z0.shape
        ctx.save_for_backward(out, *params)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        cfg = ctx.cfg
        out, *params = ctx.saved_tensors
        grad_out = grad_out.contiguous().float()
        # the adjoint's parameters (adjoint.py:176-189): those that require a gradient and, if given, are listed in adjoint_params; the
        # others get a NULL destination = they are not part of the augmented state, hence not of the mixed error norm
        keep = cfg["adjoint_param_ids"]
        live = {id(q) for q, needs in zip(params, ctx.needs_input_grad[3:]) if needs and (keep is None or id(q) in keep)}
        bound = bind_grads(cfg["spec"], ctx.z0_shape, out.device, live)
        _dopri5_call("ncde_dopri5_adjoint", cfg, cfg["adaptive_backward"], ctx.coeffs, out[:, 0], 1,
                     lambda fn, head, tail: fn(*head, out.data_ptr(), grad_out.data_ptr(), ctypes.byref(bound.g), *tail), "backward")
        grads = [bound.of(q) if id(q) in live else None for q in params]
        return (bound.grad_z0 if ctx.needs_input_grad[0] else None, None, None, *grads)


class _FusedDopri5Taped(torch.autograd.Function):
    """method='dopri5' with adjoint=False (torchdiffeq.odeint under autograd, torchcde/solver.py:224-225): forward =
    ncde_dopri5_forward_record (the adaptive solve keeping a record of its accepted steps), backward = ncde_dopri5_backward
    (reverse-mode sweep over that record incl. the gradient of the first step size).  The backward evaluates no vector field
    the reference would count: func.nfe grows by the forward's evaluations only, as under autograd."""

    @staticmethod
    def forward(ctx, z0, coeffs, cfg, *params):
        # nothing to differentiate (torch.no_grad(), frozen inputs): the plain solve, no step record at all
        taped = cfg.get("needs_grad", True) and any(ctx.needs_input_grad)
        out, z0c, rec = _dopri5_forward(z0, coeffs, cfg, taped)
        ctx.cfg, ctx.coeffs, ctx.z0_shape = cfg, coeffs, z0.shape
        if taped:
            ctx.save_for_backward(z0c, rec, *params)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        cfg = ctx.cfg
        z0c, rec, *params = ctx.saved_tensors
        grad_out = grad_out.contiguous().float()
        bound = bind_grads(cfg["spec"], ctx.z0_shape, z0c.device)
        _dopri5_call("ncde_dopri5_backward", cfg, cfg["adaptive"], ctx.coeffs, z0c, 2,
                     lambda fn, head, tail: fn(*head, rec.data_ptr(), rec.numel(), grad_out.data_ptr(), ctypes.byref(bound.g), *tail))
        grads = [bound.of(q) if needs else None for q, needs in zip(params, ctx.needs_input_grad[3:])]
        return (bound.grad_z0 if ctx.needs_input_grad[0] else None, None, None, *grads)


_DOPRI5_OPTIONS = ("min_step", "max_step", "first_step", "safety", "ifactor", "dfactor", "max_num_steps", "_trace", "_replay",
                   "_record_bytes")      # _record_bytes: initial size of the step record of adjoint=False (default: the library's estimate)


def _run_unfused(reason, X, func, z0, t, adjoint, vector_field_type, method, options, adjoint_params, rtol, atol, adjoint_rtol,
                 adjoint_atol, adjoint_options, warned=False):
    """Outside the fused kernels: the own unfused torch-op solver, same algorithms (unfused.py), on the tensors' device.
    warned: the caller has already been through the fused path's argument checks (a shape without a fused kernel is discovered after
    them), so the reference's warnings -- unexpected arguments, control buffers requiring gradients -- are not repeated."""
    from . import unfused
    options = dict(options)
    if not z0.is_cuda:
        raise NotImplementedError("cdeint needs tensors on the GPU (there is no CPU fallback); z0 is on %s" % z0.device)
    adaptive_cfg = None
    if method == "dopri5":      # adaptive dopri5 on the unfused path too (same options as the fused one)
        if options.pop("norm", None) is not None:
            raise NotImplementedError("a custom error norm is not supported (the reference's rms / mixed norms are built in)")
        aopt = {k: options.pop(k) for k in list(options) if k in _DOPRI5_OPTIONS and not k.startswith("_")}
        for k in [k for k in options if k.startswith("_")]:
            options.pop(k)
        bopt = dict(aopt) if adjoint_options is None else {k: v for k, v in adjoint_options.items() if k in _DOPRI5_OPTIONS and not k.startswith("_")}
        adaptive_cfg = {"rtol": rtol, "atol": atol, "options": aopt, "adjoint_rtol": rtol if adjoint_rtol is None else adjoint_rtol,
                        "adjoint_atol": atol if adjoint_atol is None else adjoint_atol, "adjoint_options": bopt}
    step = options.pop("step_size", None)
    if "grid_constructor" in options:
        raise NotImplementedError("options['grid_constructor'] is not supported; give options={'step_size': h}")
    options.pop("perturb", None)
    for k in options:
        if not warned:
            warnings.warn("cdeint: Unexpected arguments {}".format({k: options[k]}))
    if adjoint and not warned:
        ids = set(id(q) for q in adjoint_params) if adjoint_params is not None else set()
        for buffer in X.buffers():
            if buffer.requires_grad and id(buffer) not in ids:      # the reference's warning (solver.py:207-221)
                warnings.warn("One of the inputs to the control path X requires gradients but is not listed in "
                              "`options['adjoint_params']`. It will not receive a gradient when using the adjoint method.")
    unfused.warn_once(reason)
    if torch.is_tensor(step):
        step = step.item()
    return unfused.cdeint_unfused(X, func, z0, t, adjoint, vector_field_type, method, step, adjoint_params, adaptive_cfg)


def _no_kernel_reason(p, passes, dopri5_ts=None):
    """None if the library has a fused kernel for every pass in `passes` (0 forward, 1 continuous adjoint, 2 exact discrete
    backward) of problem `p`, else a sentence naming the shape.  Asked BEFORE the forward runs: a model
    the reference trains -- hidden_dim up to 256, hidden_hidden_dim up to 196, configurations.json5:34-35 -- must not pass its
    forward and then fail inside loss.backward()."""
    lib = _lib.lib()
    for ps in passes:
        if dopri5_ts is not None:
            rc = lib.ncde_dopri5_workspace_bytes(ctypes.byref(p), ctypes.byref(dopri5_ts), ps)
        else:
            rc = lib.ncde_workspace_bytes(ctypes.byref(p), ps)
        if rc == -2:      # NCDE_ERR_UNSUPPORTED (anything else is reported by the call itself)
            what = ("forward", "continuous adjoint", "exact discrete backward")[ps]
            widths = [int(p.layer_out[l]) for l in range(p.n_layers)]
            return "no fused %s kernel for hidden=%d, layer widths %s, channels=%d: %s" % (
                what, p.hidden, widths, p.channels, (lib.ncde_last_error_string() or b"").decode())
    return None


def cdeint(X, func, z0, t, adjoint=True, vector_field_type="matmul", **kwargs):
    r"""Solve ``z_t = z_{t_0} + \int f(z_s) dX_s``; returns ``[batch, len(t), hidden]`` like the reference.

    Same arguments as ``torchcde.cdeint`` (solver.py:140): X a LinearInterpolation / NaturalCubicSpline (default integer grid
    or a user knot grid) or a SmoothLinearInterpolation (fixed-step methods fused; dopri5 on the unfused solver), ``func`` any ``nn.Module (t, z) -> [..., H, C]``, ``method`` in {euler, midpoint, rk4} (with
    ``options={'step_size': h}``) or dopri5, CUDA tensors, ``t`` any monotone times.
    The FUSED kernels run when ``func`` exposes ``fused_spec()`` (the package's vector fields), tensors are fp32, ``t``
    increases and nothing upstream of the control path needs a gradient: the reference's NeuralCDE setting -- default grid,
    step 1, t = X.interval or X.grid_points -- on the shape-specialised / batch-tiled kernels, any other time axis on their
    plan-driven forms.  Every other request the reference accepts -- and shapes no fused kernel covers (training with hidden
    widths > 256, checked here before the forward) -- runs on the unfused torch-op solver on the GPU (unfused.py), with one
    UserWarning per reason.
    """
    if vector_field_type not in ("matmul", "evaluate", "derivative"):
        raise ValueError("vector_field_type string not recognised")
    kwargs.setdefault("atol", 1e-6)
    kwargs.setdefault("rtol", 1e-4)
    method = kwargs.pop("method", None)
    options = dict(kwargs.pop("options", None) or {})
    options_in = dict(options)      # (as given: what the unfused solver is handed if the call ends up there)
    flags = kwargs.pop("kernel_flags", 0)
    adjoint_params = kwargs.pop("adjoint_params", None)
    atol, rtol = kwargs.pop("atol"), kwargs.pop("rtol")
    adjoint_rtol, adjoint_atol = kwargs.pop("adjoint_rtol", None), kwargs.pop("adjoint_atol", None)
    adjoint_options = kwargs.pop("adjoint_options", None)
    adjoint_method = kwargs.pop("adjoint_method", None)
    for k in kwargs:
        warnings.warn("cdeint: Unexpected arguments {}".format({k: kwargs[k]}))  # misc.py:9-11
    if method is None:
        method = "dopri5"
    if method not in _ALL_METHODS:
        raise ValueError('Invalid method "{}". Must be one of {}'.format(method, '{"' + '", "'.join(_ALL_METHODS) + '"}.'))
    if method not in _FIXED_METHODS and method != "dopri5":
        raise NotImplementedError("method '%s': the fixed-step solvers %s and adaptive dopri5 are implemented" % (method, _FIXED_METHODS))
    if adjoint_method is not None and adjoint_method != method:
        raise NotImplementedError("adjoint_method != method is not implemented")
    if not isinstance(X, (LinearInterpolation, NaturalCubicSpline, SmoothLinearInterpolation)):
        raise NotImplementedError("X must be ncde_amd.LinearInterpolation, ncde_amd.NaturalCubicSpline or ncde_amd.SmoothLinearInterpolation")

    z0_in = z0      # (z0 is flattened further down; the unfused solver takes it as given)

    def unfused_(reason, warned=False):
        return _run_unfused(reason, X, func, z0_in, t, adjoint, vector_field_type, method, options_in, adjoint_params, rtol, atol,
                            adjoint_rtol, adjoint_atol, adjoint_options, warned)

    reason = _unfused_reason(X, func, z0, t, adjoint, adjoint_params, method)
    if reason is not None:
        if _control_route_ok(reason, X, z0, t, adjoint, method):      # adjoint=False, coefficients that require grad: ncde_backward_control
            out = _fused_control(X, func, z0, t, vector_field_type, method, options_in, flags)
            if out is not None:
                return out
        return unfused_(reason)
    adaptive = method == "dopri5"
    if adaptive:
        for k in list(options):
            if k not in _DOPRI5_OPTIONS and k != "norm":
                warnings.warn("cdeint: Unexpected arguments {}".format({k: options.pop(k)}))
        if options.pop("norm", None) is not None:
            raise NotImplementedError("a custom error norm is outside the fused path (the reference's rms / mixed norms are built in)")
        options.setdefault("step_size", 1.0)      # unused by the adaptive solver; keeps the common argument checks below uniform
    step = options.pop("step_size", None)
    if "grid_constructor" in options:
        raise NotImplementedError("options['grid_constructor'] is outside the fused path; give options={'step_size': h}")
    if step is None:
        raise NotImplementedError("options={'step_size': h} is required on the fused path (without it torchdiffeq steps "
                                  "from output time to output time, solvers.py:69-71)")
    if torch.is_tensor(step):
        step = step.item()
    if not float(step) > 0.0:
        raise ValueError("step_size must be positive")
    if options.pop("perturb", False):
        warnings.warn("cdeint: options['perturb'] is ignored by the fused fixed-step kernels (stage times are exact knots/fractions)")
    ad_options = {k: options.pop(k) for k in list(options) if adaptive and k in _DOPRI5_OPTIONS}
    for k in options:
        warnings.warn("cdeint: Unexpected arguments {}".format({k: options[k]}))
    if not torch.is_tensor(z0):
        raise NotImplementedError("tuple-valued z0 is outside the fused path")
    batch_shape = z0.shape[:-1]          # any number of batch dimensions, as the reference allows (flattened for the kernels)
    if z0.dim() < 1:
        raise ValueError("z0 must have a hidden dimension")
    ap = set(id(q) for q in adjoint_params) if adjoint_params is not None else None
    for buffer in X.buffers():
        if not buffer.requires_grad:
            continue
        if adjoint and (ap is None or id(buffer) not in ap):       # the reference's warning (solver.py:207-221)
            warnings.warn("One of the inputs to the control path X requires gradients but is not listed in "
                          "`options['adjoint_params']`. It will not receive a gradient when using the adjoint method.")
        else:
            # adjoint=False tapes the solve in the reference, so the path's coefficients (and whatever produced them)
            # would receive gradients; the fused backward has no dL/dcoeffs -- refuse rather than drop it silently
            raise NotImplementedError("cdeint: gradients with respect to the control path's coefficients are not "
                                      "implemented on the fused path; detach() the coefficients")
    coeffs = X.fused_coeffs
    if coeffs.dim() < 2 or tuple(coeffs.shape[:-2]) != tuple(batch_shape):
        raise ValueError("batch dimensions of X %s != batch dimensions of z0 %s" % (tuple(coeffs.shape[:-2]), tuple(batch_shape)))
    _check_tensor(z0, "z0")
    _check_tensor(coeffs, "coeffs")
    z0, coeffs = _flatten_batch(z0, coeffs)
    if coeffs.shape[0] != z0.shape[0]:
        raise ValueError("batch of X (%d) != batch of z0 (%d)" % (coeffs.shape[0], z0.shape[0]))
    spec = _field_spec(func)
    if spec.mode != vector_field_type:
        raise ValueError("vector_field_type='%s' but func was built for '%s'" % (vector_field_type, spec.mode))
    uniq = spec.unique_params()
    for q in uniq:
        _check_tensor(q, "a vector-field parameter")
        if not q.is_contiguous():
            raise NotImplementedError("vector-field parameters must be contiguous")
    if adjoint and ap is not None:
        ap = ap & set(id(q) for q in uniq)
    else:
        ap = None
    # does anything need a gradient?  (torch.no_grad() evaluation with trainable parameters does not: needs_input_grad inside an
    # autograd.Function mirrors requires_grad whatever the grad mode, so the decision is taken here -- ADVICE round 4)
    needs_grad = torch.is_grad_enabled() and (z0.requires_grad or any(q.requires_grad for q in uniq))
    # (a family pinned by a development flag keeps the old contract -- the forward runs, a missing backward kernel is reported when a
    # backward is actually asked for: the caller named the kernels, rerouting to the unfused solver would not be what was asked)
    pinned = flags & (_lib.FLAG_FORCE_GENERIC | _lib.FLAG_FORCE_FAST | _lib.FLAG_FORCE_TILED)
    passes = (0,) + (((1,) if adjoint else (2,)) if (needs_grad and not pinned) else ())
    if adaptive:
        if spec.kind != "original" or spec.mode != "matmul":
            raise NotImplementedError("method='dopri5' runs the original vector field with the matmul input only")
        bopt = dict(ad_options) if adjoint_options is None else {k: v for k, v in adjoint_options.items() if k in _DOPRI5_OPTIONS}
        cfg = {"spec": spec, "interp": X.interp_name, "flags": flags, "func": func, "adjoint_param_ids": ap, "needs_grad": needs_grad,
               "adaptive": _AdaptiveSpec(X, t, rtol, atol, ad_options), "record_bytes": ad_options.get("_record_bytes"),
               "adaptive_backward": _AdaptiveSpec(X, t, rtol if adjoint_rtol is None else adjoint_rtol,
                                                  atol if adjoint_atol is None else adjoint_atol, bopt)}
        why = _no_kernel_reason(build_problem(coeffs, X.interp_name, z0.detach(), spec, "rk4", _lib.OUT_INTERVAL, flags), passes, cfg["adaptive"].ts)
        if why is not None:
            return unfused_(why, warned=True)
        return _restore_batch((_FusedDopri5 if adjoint else _FusedDopri5Taped).apply(z0, coeffs.detach(), cfg, *uniq), batch_shape)
    flags = _coop_flags(flags, z0.device)
    axis = _fixed_axis(X, t, method, step, z0.device)
    assert axis is not None, "t must be one dimensional"
    output, plan, nfe, nfe_adj = axis
    why = _no_kernel_reason(build_problem(coeffs, X.interp_name, z0.detach(), spec, method, output, flags, plan), passes)
    if why is not None:
        return unfused_(why, warned=True)
    cfg = {"spec": spec, "interp": X.interp_name, "method": method, "output": output, "flags": flags, "plan": plan, "needs_grad": needs_grad,
           "adjoint": bool(adjoint), "func": func, "nfe_per_solve": nfe, "nfe_adjoint": nfe_adj, "adjoint_param_ids": ap}
    out = _FusedCdeint.apply(z0, coeffs.detach(), cfg, *uniq)
    if hasattr(func, "nfe"):
        func.nfe += nfe
    return _restore_batch(out, batch_shape)
