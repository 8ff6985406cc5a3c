"""Online inference: carry the CDE state of a batch of streams from one observation to the next.

``NeuralCDE.online(batch_size)`` returns an ``OnlineNeuralCDE`` over the module's own parameters.  ``step(x_new)`` fills the new
observation row(s) causally, appends the one (linear, Hermite cubic) or two (rectilinear) pieces they add to the control path, takes
one solver step per piece and returns the readout -- what ``NeuralCDE(return_sequences=True)`` on the whole prefix gives at the same
knot, at the cost of the new pieces only.  On the GPU (fp32) a call is ONE launch (csrc/ncde_stream.hip): ``ncde_stream_step`` /
``ncde_stream_step_hermite`` for the original field with the matmul input, ``ncde_stream_step_field`` /
``ncde_stream_step_field_hermite`` for the minimal-gated field and for the evaluate / derivative inputs of those two fields, and
``ncde_stream_step_lowrank`` for the low-rank field, each on a linear, rectilinear or Hermite path.  Anything else -- the GRU-gated
field, a shape whose LDS plan the kernel's query refuses -- takes the torch-op step below behind the once-only "unfused" warning.

``interpolation="cubic_hermite"`` is the smooth path that is causal: the Hermite cubic with backward differences
(``hermite_cubic_coefficients_with_backward_differences(x, initial_value_if_nan=v, forward_fill=True)``), whose piece reads the new
row, the last row and the previous piece's slope -- the state below, unchanged.

``rectilinear_indices=[...]`` on a linear model selects the linear / rectilinear HYBRID path, the online half of
``linear_rectilinear_hybrid_coeffs(x, rectilinear_indices)`` (DESIGN.md 5.7a, 5.14 "Hybrid step"): time is channel 0, the listed
(sparse) channels step rectilinearly, every other channel is interpolated linearly.  A new row adds piece A (time and the linear
channels move) and then, only for a stream whose filled sparse values differ from its last row's, piece B (the sparse channels
move); a re-observed unchanged value adds nothing.  ``step`` answers ``NeuralCDE(interpolation="linear", return_sequences=True)`` on
the hybrid coefficients of the stream's causally filled rows so far, read at the stream's last kept knot.  One launch of
``ncde_stream_step_hybrid`` / ``ncde_stream_step_field_hybrid`` (matmul and derivative inputs) / ``ncde_stream_step_lowrank_hybrid``;
the evaluate input takes the torch-op step (its stage offset is the stream's knot index, which the state does not carry).
Precondition, not checked: a stream's time strictly increases from row to row (a repeated time is outside the contract).
Causality: the batch builder closes interior NaN gaps of the LINEAR channels by interpolation, which looks ahead; this handle
forward-fills them.  The two agree exactly when the linear channels are forward-filled first or hold no NaN -- the scheme's premise.

State per stream: ``z`` [B, H], ``last_row`` [B, C] (the last filled row), ``prev_dx`` [B, C] (dX/dt of the last piece: stage 1 of
the next step reads it, the reference's left-piece rule, interpolation_linear.py:212-219) and ``count`` [B] (observations received).
"""
import ctypes

import torch

from . import _lib, unfused

_THIRD = 1.0 / 3.0
_STAGE_TIMES = {"euler": (0.0,), "midpoint": (0.0, 0.5), "rk4": (0.0, _THIRD, 2.0 * _THIRD, 1.0)}
STATE_KEYS = ("z", "last_row", "prev_dx", "count")


def _rk_increment(f, method, y):
    """Increment of one step with dt = 1, in the operation order of unfused._step (fixed_grid.py:6-29, rk_common.py:106-114);
    f(j, y) evaluates stage j."""
    if method == "euler":
        return f(0, y)
    if method == "midpoint":
        return f(1, y + 0.5 * f(0, y))
    k1 = f(0, y)
    k2 = f(1, y + k1 * _THIRD)
    k3 = f(2, y + (k2 - k1 * _THIRD))
    k4 = f(3, y + (k1 - k2 + k3))
    return (k1 + 3.0 * (k2 + k3) + k4) * 0.125


class OnlineNeuralCDE:
    def __init__(self, model, batch_size, initial_value_if_nan=0.0, time_index=0, rectilinear_indices=None):
        if rectilinear_indices is not None:      # the hybrid path: what the batch builder demands of the same arguments
            if model.interpolation != "linear":
                raise ValueError("rectilinear_indices selects the linear / rectilinear hybrid path: the model's interpolation must be "
                                 "'linear' (the hybrid coefficients are linear coefficients), not '%s'" % model.interpolation)
            if int(time_index) != 0:
                raise NotImplementedError("the hybrid path takes time in channel 0 only (time_index %d)" % int(time_index))
            idx = list(rectilinear_indices)
            if any(isinstance(i, bool) or not isinstance(i, int) for i in idx):
                raise ValueError("rectilinear_indices must be ints, got %r" % (idx,))
            if len(set(idx)) != len(idx):
                raise ValueError("rectilinear_indices must be unique, got %r" % (idx,))
            if any(not 1 <= i < model.input_dim for i in idx):
                raise ValueError("rectilinear_indices must lie in [1, %d] (channel 0 is time), got %r" % (model.input_dim - 1, idx))
        if model.interpolation not in ("linear", "rectilinear", "cubic_hermite"):
            raise ValueError("online inference needs a causal control path: interpolation 'linear' or 'rectilinear', not '%s' (a natural "
                             "cubic or smoothed path at knot k depends on later observations)" % model.interpolation)
        if model.solver not in _STAGE_TIMES:
            raise ValueError("online inference takes fixed steps (solver 'rk4', 'midpoint' or 'euler'), not '%s'" % model.solver)
        if isinstance(initial_value_if_nan, bool) or not isinstance(initial_value_if_nan, (int, float)):
            raise ValueError("initial_value_if_nan must be a float (a stream whose first row holds a NaN needs a value to be causal)")
        if int(batch_size) < 1:
            raise ValueError("batch_size must be >= 1")
        self.model = model
        self.batch_size = int(batch_size)
        self.rectilinear = model.interpolation == "rectilinear"
        self.hermite = model.interpolation == "cubic_hermite"
        self.initial_value_if_nan = float(initial_value_if_nan)
        self.time_index = int(time_index)
        if self.rectilinear and not 0 <= self.time_index < model.input_dim:
            raise ValueError("Time index must be in [0, %d], was given %d." % (model.input_dim - 1, self.time_index))
        ref = next(model.func.parameters())
        B, C, H = self.batch_size, model.input_dim, model.hidden_dim
        self.z = torch.zeros(B, H, dtype=ref.dtype, device=ref.device)
        self.last_row = torch.zeros(B, C, dtype=ref.dtype, device=ref.device)
        self.prev_dx = torch.zeros(B, C, dtype=ref.dtype, device=ref.device)
        self.count = torch.zeros(B, dtype=torch.int32, device=ref.device)
        self.hybrid = rectilinear_indices is not None
        self.rect_mask = None      # hybrid: uint8 [C] on the state's device, 1 = the channel steps rectilinearly
        if self.hybrid:
            self.rect_mask = torch.zeros(C, dtype=torch.uint8, device=ref.device)
            if idx:
                self.rect_mask[idx] = 1
        self._route = {}
        self._may_init = True      # a stream may still be waiting for its first row (known on the host without a synchronisation)

    # ---- state ---------------------------------------------------------------------------------------------------------------
    def reset(self, mask=None):
        """Forget every stream, or the streams of ``mask`` [B] (bool): their next row is a first row again."""
        with torch.no_grad():
            if mask is None:
                for k in STATE_KEYS:
                    getattr(self, k).zero_()
            else:
                mask = torch.as_tensor(mask, device=self.z.device).bool()
                if tuple(mask.shape) != (self.batch_size,):
                    raise ValueError("mask must be [%d], got %s" % (self.batch_size, tuple(mask.shape)))
                for k in STATE_KEYS:
                    t = getattr(self, k)
                    t.masked_fill_(mask if t.dim() == 1 else mask[:, None], 0)
        self._may_init = True

    def state_dict(self):
        return {k: getattr(self, k).detach().clone() for k in STATE_KEYS}

    def load_state_dict(self, state):
        for k in STATE_KEYS:
            if k not in state:
                raise ValueError("state_dict lacks '%s'" % k)
            if tuple(state[k].shape) != tuple(getattr(self, k).shape):
                raise ValueError("state '%s' must be %s, got %s" % (k, tuple(getattr(self, k).shape), tuple(state[k].shape)))
        with torch.no_grad():
            for k in STATE_KEYS:
                getattr(self, k).copy_(state[k])
        self._may_init = True

    def _check_step(self, x_new, static, active):
        """The arguments of step() as the advance routines take them: (x [m, B, C], act [m, B] uint8 or None, whether x_new was one row)."""
        m_ = self.model
        B, C = self.batch_size, m_.input_dim
        if not torch.is_tensor(x_new) or x_new.dim() not in (2, 3) or tuple(x_new.shape[-2:]) != (B, C):
            raise ValueError("x_new must be [%d, %d] or [m, %d, %d], got %s" % (B, C, B, C, tuple(getattr(x_new, "shape", ()))))
        single = x_new.dim() == 2
        x = x_new.unsqueeze(0) if single else x_new
        m = x.size(0)
        if m < 1:
            raise ValueError("x_new holds no row")
        if x.dtype != self.z.dtype or x.device != self.z.device:
            raise ValueError("x_new is %s on %s, the model's state %s on %s" % (x.dtype, x.device, self.z.dtype, self.z.device))
        if x.requires_grad or any(getattr(self, k).requires_grad for k in STATE_KEYS):
            raise ValueError("online inference runs under no_grad: the state and the observations must not require grad")
        act = None
        if active is not None:
            act = torch.as_tensor(active, device=x.device)
            if act.dim() == 1 and single:
                act = act.unsqueeze(0)
            if tuple(act.shape) != (m, B):
                raise ValueError("active must be [%d] or [%d, %d], got %s" % (B, m, B, tuple(act.shape)))
            act = (act != 0).to(torch.uint8).contiguous()
        if m_.static_dim and self._may_init:
            if static is None or tuple(static.shape) != (B, m_.static_dim):
                raise ValueError("static must be [%d, %d] while a stream may still receive its first row" % (B, m_.static_dim))
        return x, act, single

    # ---- one call ------------------------------------------------------------------------------------------------------------
    def step(self, x_new, static=None, active=None):
        """x_new [B, C] or [m, B, C] (NaN = not observed; the time channel is never NaN) -> [B, out] or [m, B, out] (the hidden
        state with apply_final_linear=False).  static [B, static_dim]: read while a stream may still receive its first row.
        active [B] or [m, B] (bool / uint8): which streams received the row; the others keep their state untouched and answer
        the readout of their unchanged z."""
        x, act, single = self._check_step(x_new, static, active)
        m = x.size(0)
        with torch.no_grad():
            advance = self._advance_kernel if self._use_kernel(x) else self._advance_torch
            outs, r = [], 0
            while self._may_init and r < m:      # rows that may be a stream's first: z(t0) from the read-in layer, row by row
                ar = None if act is None else act[r]
                self._start(x[r], static, ar)
                outs.append(advance(x[r:r + 1], None if act is None else act[r:r + 1]))
                if act is None:
                    self._may_init = False
                r += 1
            if r < m:
                outs.append(advance(x[r:], None if act is None else act[r:]))
            out = outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)
        return out[0] if single else out

    def _start(self, xr, static, act_r):
        """z(t0) of the streams for which this row is the first (the model's read-in layer on [static,] [filled row])."""
        m_ = self.model
        first = self.count == 0
        if act_r is not None:
            first = first & (act_r != 0)
        x0 = torch.where(torch.isnan(xr), torch.full_like(xr, self.initial_value_if_nan), xr)
        feats = ([static] if m_.static_dim else []) + ([x0] if m_.use_initial else [])
        if feats:
            h0 = m_.initial_linear(feats[0] if len(feats) == 1 else torch.cat(feats, dim=-1))
        else:
            h0 = torch.zeros_like(self.z)
        self.z.copy_(torch.where(first[:, None], h0, self.z))

    def _readout(self, z):
        return self.model.final_linear(z) if self.model.apply_final_linear else z

    # ---- the torch-op step (any device, any dtype, every field) ----------------------------------------------------------------
    def _advance_torch(self, x, act):
        m_ = self.model
        func, mode, method = m_.func, m_.vector_field_type, m_.solver
        t0 = x.new_zeros(())
        outs = []
        for r in range(x.size(0)):
            a = torch.ones_like(self.count, dtype=torch.bool) if act is None else act[r] != 0
            xr = x[r]
            fresh = (self.count == 0)[:, None]
            fill = torch.where(torch.isnan(xr), torch.where(fresh, torch.full_like(xr, self.initial_value_if_nan), self.last_row), xr)
            steps = (a & (self.count > 0))[:, None]
            if self.rectilinear:      # the lagged row: new time, old values
                mid = self.last_row.clone()
                mid[:, self.time_index] = fill[:, self.time_index]
            elif self.hybrid:         # the lagged row: old values in the sparse channels only
                mid = torch.where(self.rect_mask.bool(), self.last_row, fill)
            else:
                mid = fill
            da, db = mid - self.last_row, fill - mid
            has_b = (db != 0).any(dim=1, keepdim=True) if self.hybrid else None      # hybrid: piece B per stream, where a sparse value changed
            dl = torch.where((self.count == 1)[:, None], da, self.prev_dx)
            if self.hermite:      # the piece's b is dl; a stage's offset in the piece as the batch solve forms it, (n + offset) - n
                two_c = 2 * (3 * (da - dl) - da + dl)
                three_d = (da - dl) - two_c
                n = (self.count - 1).to(xr.dtype)[:, None]
                frac = [(n + s) - n for s in _STAGE_TIMES[method]]
            z = self.z
            for start, left, own, take in [(self.last_row, dl, da, None)] + ([(mid, da, db, has_b)] if self.rectilinear or self.hybrid else []):
                def f(j, y, start=start, left=left, own=own):
                    if self.hermite and j > 0:      # stage 1 sits on the knot: the left piece at frac = 1, which is b (and X = the knot)
                        s = frac[j]
                        if mode == "evaluate":
                            return func(t0, torch.cat([y, start + (left + (0.5 * two_c + three_d * s / 3) * s) * s], dim=-1))
                        dx = left + (two_c + three_d * s) * s
                    else:
                        dx = left if j == 0 else own
                    if mode == "matmul":
                        return (func(t0, y) @ dx.unsqueeze(-1)).squeeze(-1)
                    if mode == "derivative":
                        return func(t0, torch.cat([y, dx], dim=-1))
                    # evaluate: X at the stage time; at the knot it is the knot's row itself (the batch solve forms it as
                    # prev + 1 * (next - prev) on the left piece: equal up to one rounding)
                    return func(t0, torch.cat([y, start if j == 0 else start + _STAGE_TIMES[method][j] * own], dim=-1))
                z_next = z + _rk_increment(f, method, z)
                z = z_next if take is None else torch.where(take, z_next, z)
            self.z.copy_(torch.where(steps, z, self.z))
            taken = torch.where(has_b, db, da) if self.hybrid else (db if self.rectilinear else da)
            self.prev_dx.copy_(torch.where(steps, taken, self.prev_dx))
            self.last_row.copy_(torch.where(a[:, None], fill, self.last_row))
            self.count.add_(a.to(torch.int32))
            outs.append(self._readout(self.z).clone())
        return torch.stack(outs, dim=0)

    # ---- the fused step --------------------------------------------------------------------------------------------------------
    def _problem(self):
        m_ = self.model
        spec = m_.func.fused_spec()
        p = _lib.NcdeProblem()
        p.abi_version = _lib.NCDE_ABI_VERSION
        p.batch, p.hidden, p.channels, p.n_knots = self.batch_size, m_.hidden_dim, m_.input_dim, 2
        p.interp, p.method, p.output, p.flags = _lib.INTERP["cubic" if self.hermite else "linear"], _lib.METHOD[m_.solver], _lib.OUT_KNOTS, 0
        if len(spec.layers) > _lib.NCDE_MAX_LAYERS:
            raise NotImplementedError("at most %d hidden layers" % _lib.NCDE_MAX_LAYERS)
        p.n_layers = len(spec.layers)
        for i, (w, b) in enumerate(spec.layers):
            p.layer_out[i], p.layer_in[i] = w.shape
            p.layer_W[i], p.layer_b[i] = w.data_ptr(), b.data_ptr()
        p.Wo, p.bo = spec.Wo.data_ptr(), spec.bo.data_ptr()
        p.field_kind, p.field_input = _lib.FIELD_KIND[spec.kind], _lib.FIELD_INPUT[spec.mode]
        if spec.kind != "original":      # the second head, as solver.build_problem fills it
            p.Wg, p.bg = spec.Wg.data_ptr(), spec.bg.data_ptr()
        if spec.kind == "lowrank":      # the rank travels in the top byte of flags
            if not 1 <= spec.rank <= 255:
                raise ValueError("low-rank field: rank %d outside [1, 255]" % spec.rank)
            p.flags = _lib.FLAG_FIELD_RANK(spec.rank)
        return p

    def _kernel_entry(self, spec):
        """(query, entry) of the step kernel that covers this field on this path, or None (the GRU-gated field): the original field
        with the matmul input has ncde_stream_step / ncde_stream_step_hermite; the minimal-gated field and the evaluate / derivative
        inputs of the two have ncde_stream_step_field / ncde_stream_step_field_hermite; the low-rank field has
        ncde_stream_step_lowrank on all three paths (the problem's interp says which).  The hybrid path has an entry of its own per
        family (the query of the field one refuses the evaluate input)."""
        family = "step" if (spec.kind, spec.mode) == ("original", "matmul") else self._FAMILY.get(spec.kind)
        return self._ENTRY.get((family, "hybrid" if self.hybrid else ("hermite" if self.hermite else "linear")))

    # (family, path) -> (query, entry); a field kind without a family (the GRU-gated field) has none.  Read at every step: the names
    # are formed here, once.
    _FAMILY = {"original": "field", "minimal": "field", "lowrank": "lowrank"}
    _ENTRY = {key: ("ncde_stream%s_workspace_bytes" % suffix, "ncde_stream_step%s" % suffix) for key, suffix in (
        (("step", "linear"), ""), (("step", "hermite"), "_hermite"), (("step", "hybrid"), "_hybrid"),
        (("field", "linear"), "_field"), (("field", "hermite"), "_field_hermite"), (("field", "hybrid"), "_field_hybrid"),
        (("lowrank", "linear"), "_lowrank"), (("lowrank", "hermite"), "_lowrank"), (("lowrank", "hybrid"), "_lowrank_hybrid"))}

    def _use_kernel(self, x):
        """The route, in the house style: CUDA fp32, a field one of the step kernels covers (_kernel_entry) and a shape its query
        accepts take that kernel; anything else the torch-op step, behind the once-only warning.  Nothing here reads the device."""
        key = (x.device.type, x.dtype)
        if key in self._route:      # (the shapes of a module do not change: one query per device / dtype)
            return self._route[key]
        reason = None
        if not hasattr(self.model.func, "fused_spec"):
            reason = "online step: func does not expose fused_spec()"
        elif not x.is_cuda or x.dtype != torch.float32:
            reason = "online step: tensors are not fp32 on the GPU"
        else:
            pick = self._kernel_entry(self.model.func.fused_spec())
            if pick is None:
                reason = "online step: a gated or low-rank vector field or the evaluate / derivative input"
            else:
                query = pick[0]
                rc = getattr(_lib.lib(), query)(ctypes.byref(self._problem()))
                if rc == -2:
                    reason = "online step: " + (_lib.lib().ncde_last_error_string() or b"").decode()
                else:
                    _lib.check(rc, query)
        if reason is not None:
            unfused.warn_once(reason)
        self._route[key] = reason is None
        return reason is None

    def _stream_args(self, x, act, m, readout=True):
        """NcdeStream of this handle's state, the rows x [m, B, C] (act [m, B] uint8 or None) and the readout -> (struct, the output
        tensor it writes, the tensors its pointers must outlive).  An inner layer of a stack: x None, and readout=False (the state only)."""
        m_ = self.model
        B, H = self.batch_size, m_.hidden_dim
        s = _lib.NcdeStream()
        s.n_rows, s.rectilinear, s.time_index = m, int(self.rectilinear), self.time_index
        if x is not None:
            if x.stride(2) != 1 or x.stride(1) < m_.input_dim or x.stride(0) < 0:      # what the ABI takes: unit channels, rows that do not overlap
                x = x.contiguous()                                                       # (an expand()ed batch has stride 0: copied)
            s.x, s.x_stride_m, s.x_stride_b = x.data_ptr(), x.stride(0), x.stride(1)
        s.active = None if act is None else act.data_ptr()
        s.initial_value_if_nan = self.initial_value_if_nan
        s.z, s.last_row, s.prev_dx, s.count = self.z.data_ptr(), self.last_row.data_ptr(), self.prev_dx.data_ptr(), self.count.data_ptr()
        out = None
        if readout and m_.apply_final_linear:
            fl = m_.final_linear
            out = torch.empty(m, B, fl.out_features, dtype=torch.float32, device=self.z.device)
            s.n_out, s.Wf, s.bf, s.out = fl.out_features, fl.weight.data_ptr(), (None if fl.bias is None else fl.bias.data_ptr()), out.data_ptr()
        elif readout:
            out = torch.empty(m, B, H, dtype=torch.float32, device=self.z.device)
            s.z_out = out.data_ptr()
        return s, out, (x, act)

    def _advance_kernel(self, x, act):
        p = self._problem()
        s, out, keep = self._stream_args(x, act, x.size(0))
        with torch.cuda.device(x.device):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            entry = self._kernel_entry(self.model.func.fused_spec())[1]
            extra = (ctypes.c_void_p(self.rect_mask.data_ptr()),) if self.hybrid else ()
            _lib.check(getattr(_lib.lib(), entry)(ctypes.byref(p), ctypes.byref(s), *extra, stream), entry)
        return out


class OnlineStackedNeuralCDE:
    """``StackedNeuralCDE.online(batch_size)``: what ``StackedNeuralCDE(return_sequences=True)`` on the whole prefix gives at the newest
    knot, carried forward.  ``layers[i]`` is the ``OnlineNeuralCDE`` of ``ncdes[i]`` and owns that layer's state; layer i + 1 reads
    layer i's hidden state as its observation.  By default the layer handles' own ``step`` are chained, each on its own route (one
    launch of ``ncde_stream_step`` per layer on the GPU): measured, that is the faster form, because the host prepares layer i + 1's
    launch while layer i's kernel runs ("Stacked step").  ``one_launch=True`` asks for ONE launch of
    ``ncde_stream_stack_step`` for all layers where it applies (CUDA fp32, every layer's field fused, a stack the query accepts), bit
    for bit the chain's results.  ``fused`` says which route the last step took (None before the first)."""

    def __init__(self, model, batch_size, initial_value_if_nan=0.0, one_launch=False):
        self.model = model
        self.one_launch = bool(one_launch)
        self.layers = [OnlineNeuralCDE(ncde, batch_size, initial_value_if_nan=initial_value_if_nan) for ncde in model.ncdes]
        self.batch_size = self.layers[0].batch_size
        self.fused = None
        self._route = {}

    @property
    def _may_init(self):
        return any(lay._may_init for lay in self.layers)

    # ---- state ---------------------------------------------------------------------------------------------------------------
    def reset(self, mask=None):
        for lay in self.layers:
            lay.reset(mask)

    def state_dict(self):
        return {"layers.%d.%s" % (i, k): v for i, lay in enumerate(self.layers) for k, v in lay.state_dict().items()}

    def load_state_dict(self, state):
        per_layer = []
        for i, lay in enumerate(self.layers):
            for k in STATE_KEYS:
                if "layers.%d.%s" % (i, k) not in state:
                    raise ValueError("state_dict lacks 'layers.%d.%s'" % (i, k))
            per_layer.append({k: state["layers.%d.%s" % (i, k)] for k in STATE_KEYS})
            for k in STATE_KEYS:      # every shape before any layer is written
                if tuple(per_layer[i][k].shape) != tuple(getattr(lay, k).shape):
                    raise ValueError("state 'layers.%d.%s' must be %s, got %s" % (i, k, tuple(getattr(lay, k).shape), tuple(per_layer[i][k].shape)))
        for lay, st in zip(self.layers, per_layer):
            lay.load_state_dict(st)

    # ---- one call ------------------------------------------------------------------------------------------------------------
    def _static_of(self, i, static):
        return static if self.layers[i].model.static_dim else None

    def step(self, x_new, static=None, active=None):
        """The contract of OnlineNeuralCDE.step: x_new [B, C] or [m, B, C] -> [B, output_dim] or [m, B, output_dim], the last
        layer's final_linear as StackedNeuralCDE.forward returns it.  static goes to layer 0, and to the inner layers with
        static_in_all_layers; active governs every layer."""
        x, act, single = self.layers[0]._check_step(x_new, static, active)
        if self.model.static_in_all_layers and self.model.static_dim and self._may_init and static is None:
            raise ValueError("static must be [%d, %d] while a stream may still receive its first row" % (self.batch_size, self.model.static_dim))
        self.fused = self._use_kernel(x)
        if not self.fused:      # the chain: every layer steps on its own route
            h = x
            for i, lay in enumerate(self.layers):
                h = lay.step(h, static=self._static_of(i, static), active=act)
            return h[0] if single else h
        m = x.size(0)
        with torch.no_grad():
            outs, r = [], 0
            while self._may_init and r < m:      # rows that may be a stream's first: z(t0) of every layer, layer i from layer i - 1's
                ar = None if act is None else act[r]
                h = x[r]
                for i, lay in enumerate(self.layers):
                    lay._start(h, self._static_of(i, static), ar)
                    h = lay.z
                outs.append(self._advance_kernel(x[r:r + 1], None if act is None else act[r:r + 1]))
                if act is None:
                    for lay in self.layers:
                        lay._may_init = False
                r += 1
            if r < m:
                outs.append(self._advance_kernel(x[r:], None if act is None else act[r:]))
            out = outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)
        return out[0] if single else out

    def _problems(self):
        ps = [lay._problem() for lay in self.layers]
        return ps, (ctypes.POINTER(_lib.NcdeProblem) * len(ps))(*[ctypes.pointer(p) for p in ps])

    def _use_kernel(self, x):
        """one_launch, CUDA fp32 and a stack ncde_stream_stack_workspace_bytes accepts take the one launch.  Anything else takes the
        chain without a warning of its own: each layer handle then picks, and announces, its own route."""
        if not self.one_launch:
            return False
        key = (x.device.type, x.dtype)
        if key not in self._route:
            ok = x.is_cuda and x.dtype == torch.float32 and all(hasattr(lay.model.func, "fused_spec") for lay in self.layers)
            if ok:
                ps, arr = self._problems()
                rc = _lib.lib().ncde_stream_stack_workspace_bytes(arr, len(ps))
                if rc == -2:
                    ok = False
                else:
                    _lib.check(rc, "ncde_stream_stack_workspace_bytes")
            self._route[key] = ok
        return self._route[key]

    def _advance_kernel(self, x, act):
        ps, parr = self._problems()
        n = len(self.layers)
        args = [lay._stream_args(x if i == 0 else None, act, x.size(0), readout=i == n - 1) for i, lay in enumerate(self.layers)]
        sarr = (ctypes.POINTER(_lib.NcdeStream) * n)(*[ctypes.pointer(a[0]) for a in args])
        with torch.cuda.device(x.device):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.check(_lib.lib().ncde_stream_stack_step(parr, sarr, n, stream), "ncde_stream_stack_step")
        return args[-1][1]
