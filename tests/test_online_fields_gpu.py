"""The field step on the GPU (ncde_stream_step_field, csrc/ncde_stream.hip): ``NeuralCDE.online`` for the minimal-gated field and
for the evaluate / derivative inputs of the original and the minimal-gated field, on linear and rectilinear paths.

Reference: tests/stream_ref.prefix_reference (per stream, this package's batch model in fp64 on the CPU on the rows the stream
received) within the project's forward bound su.TIGHT_Z = 2e-5 of max |ref|, for z and the readout at every step.  Bit for bit:
rows per call, streams run alone or in halves, masks, the state dict, a refused call.  Within the same bound: the torch-op step on
the same GPU tensors and this package's fp32 batch forward (not bit for bit: the step streams every weight, a batch solve that
keeps weights resident in LDS sums in two accumulators).

Observed on the MI355X (max over steps of |delta| / max |ref|, z or readout, whichever is larger):
  parity, 10 cases                       1.1e-7 .. 2.6e-7 (evaluate against derivative on the same weights: 0.20 .. 0.62)
  euler / midpoint                       1.6e-7 / 1.8e-7
  shape edges, 11 cases, and nl 0        1.1e-7 .. 4.5e-7 (the largest: C 1, rectilinear, minimal/matmul)
  staggered schedule, 3 pairs            <= 2.5e-7
  vs the torch-op step / the fp32 batch  7.6e-8 .. 1.4e-7 / 9.2e-8 .. 1.5e-7 (not 0, as expected)
  LDS boundary H 352 fused / H 353 torch 1.1e-7 / 9.7e-8"""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import stream_edges as se
import stream_ref as sr
import stream_util as su

pytestmark = pytest.mark.gpu
F32 = torch.float32
INVALID, UNSUPPORTED = -1, -2      # NcdeStatus (include/ncde_hip.h)
PAIRS = [("original", "evaluate"), ("original", "derivative"), ("minimal", "matmul"), ("minimal", "evaluate"), ("minimal", "derivative")]
PATHS = ["linear", "rectilinear"]
BASE = dict(C=5, H=12, HH=10, nl=2, n_out=3, B=19, rows=6, init=-0.5)


# ---- helpers -------------------------------------------------------------------------------------------------------------------------
def _model(kind, mode, path, device, seed=81, C=5, H=12, HH=10, nl=2, n_out=3, **kw):
    """Built on the CPU under the seed, then moved: the evaluate and the derivative model of a seed hold the same weights."""
    return se.make_model(seed, C, H, n_out, HH, nl, path, device, F32, vector_field=kind, vector_field_type=mode, **kw)


def _reference(key, build_model, rows, init, ti=0, received=None):
    """(z, out) of prefix_reference in fp64: computed once per key, shared, never modified."""
    return se.reference(("fields",) + key, lambda: sr.prefix_reference(build_model(), rows, received, None, init, ti))


def _kernel_name(lib, h):
    return lib.ncde_stream_field_kernel_name(ctypes.byref(h._problem()))


def _steps(model, x, init, ti=0):
    """One call per row on the fused route (any warning is an error) -> (outs, zs) as numpy, the handle."""
    with se.stepping("cuda"):
        h = model.online(x.size(1), initial_value_if_nan=init, time_index=ti)
        outs, zs, _ = su.step_through(h, x, None, quiet=False)
    return outs, zs, h


def _worst(outs, zs, z_ref, o_ref, what):
    worst = 0.0
    for k in range(outs.shape[0]):
        e_out, e_z = se.err(outs[k], o_ref[k]), se.err(zs[k], z_ref[k])
        print("%s step %d: out %.3e z %.3e" % (what, k, e_out, e_z))
        assert e_out <= su.TIGHT_Z and e_z <= su.TIGHT_Z, (what, k, e_out, e_z)
        worst = max(worst, e_out, e_z)
    assert np.abs(z_ref[-1] - z_ref[0]).max() > 1e-3      # the state moved: not a vacuous pass
    print("%s: worst %.3e" % (what, worst))
    return worst


def _check(lib, what, key, build, rows, init, ti=0, B=None):
    """A model (build(device)) on `rows` through the handle against the fp64 reference of `key`."""
    z_ref, o_ref = _reference(key, lambda: build("cpu"), rows, init, ti)
    outs, zs, h = _steps(build("cuda"), se.dev(rows, "cuda"), init, ti)
    assert _kernel_name(lib, h) == b"ncde_stream_step_field"
    assert h.count.cpu().tolist() == [rows.shape[0]] * rows.shape[1]
    return _worst(outs, zs, z_ref, o_ref, what), zs, z_ref


def _state_equal(a, b, where):
    for k in a.state_dict():
        assert torch.equal(a.state_dict()[k], b.state_dict()[k]), (where, k)


# ---- 1. parity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("kind,mode", PAIRS)
def test_parity_with_the_fp64_prefix_reference(gpu_lib, kind, mode, path):
    s = BASE
    rows = se.make_rows(8101, s["rows"], s["B"], s["C"])
    assert np.isnan(rows).any()
    _, zs, z_ref = _check(gpu_lib, "%s/%s %s" % (kind, mode, path), (kind, mode, path), lambda d: _model(kind, mode, path, d), rows, s["init"])
    if mode == "evaluate":      # the value image and the derivative image are different inputs: the same weights on dX/dt answer otherwise
        _, z_der, _ = _steps(_model(kind, "derivative", path, "cuda"), se.dev(rows, "cuda"), s["init"])
        gap = np.abs(zs - z_der).max() / np.abs(z_ref).max()
        print("%s evaluate vs derivative on the same weights: %.3e" % (kind, gap))
        assert gap > 1e-3, gap


# ---- 2. the other methods ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["euler", "midpoint"])
def test_euler_and_midpoint(gpu_lib, method):
    s = BASE
    rows = se.make_rows(8102, s["rows"], s["B"], s["C"])
    _check(gpu_lib, "minimal/derivative linear %s" % method, ("method", method),
           lambda d: _model("minimal", "derivative", "linear", d, solver=method), rows, s["init"])


# ---- 3. shape edges ------------------------------------------------------------------------------------------------------------------
class HeadOnlyField(torch.nn.Module):
    """A field without inner layers: the heads read the field input u = [z, control] directly."""

    def __init__(self, C, H, kind, mode):
        super().__init__()
        self.C, self.H, self.kind, self.mode = C, H, kind, mode
        d0, rows = (H, H * C) if mode == "matmul" else (H + C, H)
        self.tanh_head = torch.nn.Linear(d0, rows)
        if kind == "minimal":
            self.gate_head = torch.nn.Linear(d0, rows)

    def fused_spec(self):
        import ncde_amd
        g = getattr(self, "gate_head", None)
        return ncde_amd.FieldSpec([], self.tanh_head.weight, self.tanh_head.bias, self.kind, self.mode, *(() if g is None else (g.weight, g.bias)))

    def forward(self, t, u):
        m = torch.tanh(self.tanh_head(u))
        if self.kind == "minimal":
            m = torch.sigmoid(self.gate_head(u)) * m
        return m.view(-1, self.H, self.C) if self.mode == "matmul" else m


def _head_only_class():
    import ncde_amd

    class HeadOnlyCDE(ncde_amd.NeuralCDE):      # (the reference twin is type(model)(**the model's own constructor arguments))
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.func = HeadOnlyField(self.input_dim, self.hidden_dim, self.vector_field, self.vector_field_type)
    return HeadOnlyCDE


def _head_only(kind, mode, path, device, C=5, H=12, n_out=3):
    torch.manual_seed(83)
    m = _head_only_class()(C, H, n_out, hidden_hidden_dim=4, num_layers=1, interpolation=path, return_sequences=True, solver="rk4",
                           vector_field=kind, vector_field_type=mode)
    return m.to(device=device, dtype=F32)


EDGES = [      # (id, kind, mode, path, model dims, B, time_index)
    ("B1", "minimal", "evaluate", "rectilinear", {}, 1, 0),
    ("B16", "minimal", "evaluate", "rectilinear", {}, 16, 0),
    ("B17", "minimal", "evaluate", "rectilinear", {}, 17, 0),
    ("C1_rect_evaluate", "original", "evaluate", "rectilinear", dict(C=1), 5, 0),      # the time channel alone
    ("C1_rect_matmul", "minimal", "matmul", "rectilinear", dict(C=1), 5, 0),
    ("C9_derivative", "minimal", "derivative", "linear", dict(C=9), 5, 0),
    ("C9_rect_matmul", "minimal", "matmul", "rectilinear", dict(C=9), 5, 0),
    ("H7_HH24_evaluate", "original", "evaluate", "linear", dict(C=6, H=7, HH=24), 5, 0),      # d0 = 13: no multiple of 4 or 16
    ("H7_HH24_derivative", "minimal", "derivative", "rectilinear", dict(C=6, H=7, HH=24), 5, 0),
    ("time_last_evaluate", "minimal", "evaluate", "rectilinear", {}, 5, 4),
    ("time_last_original", "original", "evaluate", "rectilinear", {}, 17, 4),
]


@pytest.mark.parametrize("case", EDGES, ids=[c[0] for c in EDGES])
def test_shape_edges(gpu_lib, case):
    name, kind, mode, path, dims, B, ti = case
    C = dims.get("C", 5)
    rows = se.make_rows(8103, 5, B, C, time_index=ti)
    _check(gpu_lib, name, ("edge", name), lambda d: _model(kind, mode, path, d, **dims), rows, 0.25, ti)


@pytest.mark.parametrize("kind,mode", [("original", "derivative"), ("minimal", "evaluate")])
def test_no_inner_layer_the_heads_read_the_field_input(gpu_lib, kind, mode):
    rows = se.make_rows(8104, 5, 17, 5)
    model = _head_only(kind, mode, "rectilinear", "cuda")
    assert model.online(17)._problem().n_layers == 0
    _check(gpu_lib, "nl 0 %s/%s" % (kind, mode), ("nl0", kind, mode), lambda d: _head_only(kind, mode, "rectilinear", d), rows, 0.25)


# ---- 4. bit-identities ---------------------------------------------------------------------------------------------------------------
BITS = [("minimal", "evaluate", "rectilinear"), ("original", "derivative", "linear"), ("minimal", "matmul", "rectilinear")]


@pytest.mark.parametrize("kind,mode,path", BITS)
def test_rows_in_one_call_and_interleaved_halves(gpu_lib, kind, mode, path):
    s = BASE
    model = _model(kind, mode, path, "cuda")
    x = se.dev(se.make_rows(8105, s["rows"], s["B"], s["C"]), "cuda")
    with se.stepping("cuda"):
        h1, h2 = model.online(s["B"], initial_value_if_nan=s["init"]), model.online(s["B"], initial_value_if_nan=s["init"])
        many = torch.cat([h1.step(x[0])[None], h1.step(x[1:])])      # m = 5 rows in one launch
        singles = torch.stack([h2.step(x[k]) for k in range(s["rows"])])
        assert torch.equal(many, singles)
        _state_equal(h1, h2, "m rows in one call")
        for half in (slice(0, None, 2), slice(1, None, 2)):      # streams of one tile spread over two tiles and the reverse
            xh = x[:, half].contiguous()
            hh = model.online(xh.size(1), initial_value_if_nan=s["init"])
            assert torch.equal(torch.stack([hh.step(xh[k]) for k in range(s["rows"])]), singles[:, half])
            for k in hh.state_dict():
                assert torch.equal(hh.state_dict()[k], h2.state_dict()[k][half]), k
    assert (singles[-1] - singles[0]).abs().max() > 1e-3


@pytest.mark.parametrize("kind,mode,path", BITS)
def test_masks_and_a_tile_of_mixed_counts(gpu_lib, kind, mode, path):
    """The staggered schedule of tests/stream_edges.py: at call 3 one tile holds streams with 0, 1 and >= 2 rows behind them next to
    streams that receive nothing.  Every stream answers what it answers alone in a handle of batch 1, non-receivers keep their state,
    and -- after an unmasked first call -- the [m, B] mask in ONE launch equals the masked single calls."""
    s = se.STAG
    x_np, A = se.staggered_rows()
    se.assert_schedule(A)
    z_ref, o_ref = _reference(("staggered", kind, mode, path), lambda: _model(kind, mode, path, "cpu"), x_np, s["init"], 0, A)
    model = _model(kind, mode, path, "cuda")
    x, act = se.dev(x_np, "cuda"), se.dev(A, "cuda")
    with se.stepping("cuda"):
        h = model.online(s["B"], initial_value_if_nan=s["init"])
        alone = [model.online(1, initial_value_if_nan=s["init"]) for _ in range(s["B"])]
        for j in range(s["calls"]):
            before = h.state_dict()
            out = h.step(x[j], active=act[j])
            after = h.state_dict()
            for key in before:
                assert torch.equal(before[key][~act[j]], after[key][~act[j]]), (j, key)
            e_out, e_z = se.err(out, o_ref[j]), se.err(h.z, z_ref[j])
            print("staggered %s/%s %s call %d: out %.3e z %.3e" % (kind, mode, path, j, e_out, e_z))
            assert e_out <= su.TIGHT_Z and e_z <= su.TIGHT_Z, (j, e_out, e_z)
            for b in np.nonzero(A[j])[0]:
                ob = alone[b].step(x[j, b:b + 1])
                assert torch.equal(ob[0], out[b]) and all(torch.equal(alone[b].state_dict()[k][0], after[k][b]) for k in after), (j, b)
        assert h.count.cpu().tolist() == A.sum(axis=0).tolist()
        # the [m, B] mask in one launch
        x_np, A = se.staggered_rows(first_all=True)
        x, act = se.dev(x_np, "cuda"), se.dev(A, "cuda")
        h1, h2 = model.online(s["B"], initial_value_if_nan=s["init"]), model.online(s["B"], initial_value_if_nan=s["init"])
        first = h1.step(x[0])
        assert h1._may_init is False
        many = h1.step(x[1:], active=act[1:])
        singles = [h2.step(x[0])] + [h2.step(x[j], active=act[j]) for j in range(1, s["calls"])]
        assert torch.equal(torch.cat([first[None], many]), torch.stack(singles))
        _state_equal(h1, h2, "row mask in one launch")


@pytest.mark.parametrize("kind,mode,path", BITS)
def test_state_dict_round_trip_and_a_refused_call(gpu_lib, kind, mode, path):
    from ncde_amd import _lib
    s = BASE
    model = _model(kind, mode, path, "cuda")
    x = se.dev(se.make_rows(8106, s["rows"], s["B"], s["C"]), "cuda")
    with se.stepping("cuda"):
        ha, hb = model.online(s["B"], initial_value_if_nan=s["init"]), model.online(s["B"], initial_value_if_nan=s["init"])
        ha.step(x[:3])
        saved = ha.state_dict()
        hb.load_state_dict(saved)
        assert torch.equal(ha.step(x[3:]), hb.step(x[3:]))
        _state_equal(ha, hb, "round trip")
        # a refusal through the ABI: nothing is launched, the state keeps its bits
        before = ha.state_dict()
        p = ha._problem()
        st, out, keep = ha._stream_args(x[:1], None, 1)
        st.n_rows = 0
        rc = gpu_lib.ncde_stream_step_field(ctypes.byref(p), ctypes.byref(st), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == INVALID and b"n_rows" in gpu_lib.ncde_last_error_string()
        p.field_kind = _lib.FIELD_KIND["gru"]
        st.n_rows = 1
        assert gpu_lib.ncde_stream_step_field(ctypes.byref(p), ctypes.byref(st), None) == UNSUPPORTED
        torch.cuda.synchronize()
        for k in before:
            assert torch.equal(before[k], ha.state_dict()[k]), k


# ---- 5. against the two routes that exist without the kernel ---------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("kind,mode", [("minimal", "matmul"), ("original", "evaluate")])
def test_against_the_torch_step_and_the_batch_forward(gpu_lib, kind, mode, path):
    import ncde_amd
    s = BASE
    rect = path == "rectilinear"
    model = _model(kind, mode, path, "cuda", apply_final_linear=False)
    x = se.dev(se.make_rows(8107, s["rows"], s["B"], s["C"]), "cuda")
    _, zs, h = _steps(model, x, s["init"])
    assert _kernel_name(gpu_lib, h) == b"ncde_stream_step_field"
    # the torch-op step on the same tensors (the route this handle took before the kernel existed)
    ht = model.online(s["B"], initial_value_if_nan=s["init"])
    ht._route[("cuda", F32)] = False
    _, z_torch, _ = su.step_through(ht, x, None)
    # this package's fp32 batch forward on the coefficients built from the same rows
    coeffs = ncde_amd.linear_interpolation_coeffs(x.transpose(0, 1).contiguous(), rectilinear=0 if rect else None,
                                                  initial_value_if_nan=s["init"], forward_fill=not rect)
    with torch.no_grad():
        z_batch = model(coeffs).transpose(0, 1).cpu().numpy()
    assert z_batch.shape == zs.shape
    e_torch = max(se.err(zs[k], z_torch[k]) for k in range(s["rows"]))
    e_batch = max(se.err(zs[k], z_batch[k]) for k in range(s["rows"]))
    print("%s/%s %s: vs the torch-op step %.3e, vs the fp32 batch forward %.3e" % (kind, mode, path, e_torch, e_batch))
    assert e_torch <= su.TIGHT_Z and e_batch <= su.TIGHT_Z, (e_torch, e_batch)
    assert np.abs(z_batch[-1] - z_batch[0]).max() > 1e-3


# ---- 6. the LDS boundary ---------------------------------------------------------------------------------------------------------------
def _wide(H, device):
    return se.make_model(85, 4, H, 2, H, 2, "linear", device, F32, apply_final_linear=False, vector_field_type="evaluate")


def test_last_width_the_lds_plan_holds_steps_fused(gpu_lib):
    """C 4, HH = H, nl 2, evaluate: H 352 is the last width the query accepts (tests/test_online_fields_cpu.py finds it)."""
    rows = se.make_rows(8108, 3, 3, 4)
    assert gpu_lib.ncde_stream_field_workspace_bytes(ctypes.byref(_wide(352, "cuda").online(3)._problem())) == 0
    _check(gpu_lib, "H352 evaluate", ("wide", 352), lambda d: _wide(352, d), rows, 0.0)


def test_first_width_the_lds_plan_refuses_takes_the_torch_step(gpu_lib):
    from ncde_amd import unfused
    rows = se.make_rows(8108, 3, 3, 4)
    model = _wide(353, "cuda")
    assert gpu_lib.ncde_stream_field_workspace_bytes(ctypes.byref(model.online(3)._problem())) == UNSUPPORTED
    assert gpu_lib.ncde_stream_field_kernel_name(ctypes.byref(model.online(3)._problem())) is None
    z_ref, o_ref = _reference(("wide", 353), lambda: _wide(353, "cpu"), rows, 0.0)
    unfused._WARNED.clear()
    h = model.online(3)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        outs, zs, _ = su.step_through(h, se.dev(rows, "cuda"), None, quiet=False)
    msgs = [str(w.message) for w in rec]
    assert len(msgs) == 1 and "unfused" in msgs[0] and "online step" in msgs[0] and "LDS" in msgs[0], msgs
    _worst(outs, zs, z_ref, o_ref, "H353 evaluate on the torch-op step")
