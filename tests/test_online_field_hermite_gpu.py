"""The field step on the Hermite path on the GPU (ncde_stream_step_field_hermite, csrc/ncde_stream.hip): ``NeuralCDE.online`` with
``interpolation="cubic_hermite"`` for the minimal-gated field and for the evaluate / derivative inputs of the original and the
minimal-gated field.

Reference: tests/hermite_util.batch_reference (this package's batch model in fp64 on the CPU on the Hermite coefficients of the
rows) within the project's forward bound su.TIGHT_Z = 2e-5 of max |ref|, for z and the readout at every step.  Bit for bit: rows
per call, streams run alone or in halves, masks, the state dict, a refused call.  Within the same bound: the torch-op step on the
same GPU tensors.

Observed on the MI355X (max over steps of |delta| / max |ref|, z or readout, whichever is larger; not bounds):
  parity, 5 pairs                        1.3e-7 .. 2.2e-7 (evaluate against derivative on the same weights: 0.40)
  euler / midpoint                       1.2e-7 / 1.2e-7
  shape edges, 8 cases, and nl 0         1.2e-7 .. 2.5e-7 (the largest: C 1, minimal/matmul)
  vs the torch-op step                   1.1e-7 .. 1.4e-7
  LDS boundary H 352 fused / H 353 torch 9.4e-8 / 9.9e-8"""
import ctypes

import numpy as np
import pytest
import torch

import hermite_util as hu
import online_step_checks as oc
import stream_edges as se

pytestmark = pytest.mark.gpu
F32 = torch.float32
PAIRS = [("original", "evaluate"), ("original", "derivative"), ("minimal", "matmul"), ("minimal", "evaluate"), ("minimal", "derivative")]
NAME = b"ncde_stream_step_field_hermite"
PATH = "cubic_hermite"


def _model(kind, mode, device, seed=None, C=None, H=None, HH=None, nl=None, n_out=None, dtype=F32, **kw):
    """hermite_util.MAIN's dimensions unless given.  Built on the CPU under the seed, then moved: the evaluate and the derivative
    model of a seed hold the same weights."""
    s = hu.MAIN
    pick = lambda v, k: s[k] if v is None else v      # noqa: E731
    return se.make_model(pick(seed, "model_seed"), pick(C, "C"), pick(H, "H"), pick(n_out, "n_out"), pick(HH, "HH"), pick(nl, "nl"), PATH, device, dtype,
                         vector_field=kind, vector_field_type=mode, **kw)


def _check(lib, what, key, build, rows, init):
    return oc.check(lib.ncde_stream_field_hermite_kernel_name, NAME, what, ("field_hermite",) + key, build, rows, init)


# ---- 1. parity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mode", PAIRS)
def test_parity_with_the_fp64_batch_reference(gpu_lib, kind, mode):
    s = hu.MAIN
    rows = hu.main_rows()
    _, zs, z_ref = _check(gpu_lib, "%s/%s" % (kind, mode), (kind, mode), lambda d: _model(kind, mode, d), rows, s["init"])
    if mode == "evaluate":      # the value image is not the slope image: the same weights on dX/dt answer otherwise
        _, z_der, _ = oc.steps(_model(kind, "derivative", "cuda"), se.dev(rows, "cuda"), s["init"])
        gap = np.abs(zs - z_der).max() / np.abs(z_ref).max()
        print("%s evaluate vs derivative on the same weights: %.3e" % (kind, gap))
        assert gap > 1e-3, gap


@pytest.mark.parametrize("method", ["euler", "midpoint"])
def test_euler_and_midpoint(gpu_lib, method):
    s = hu.MAIN
    rows = se.make_rows(7102, s["L"], s["B"], s["C"])
    _check(gpu_lib, "minimal/evaluate %s" % method, ("method", method), lambda d: _model("minimal", "evaluate", d, solver=method), rows, s["init"])


# ---- 2. shape edges ------------------------------------------------------------------------------------------------------------------
EDGES = [      # (id, kind, mode, model dims, B)
    ("B1", "minimal", "evaluate", {}, 1),
    ("B17", "original", "derivative", {}, 17),
    ("C1_evaluate", "original", "evaluate", dict(C=1), 5),      # the time channel alone
    ("C1_matmul", "minimal", "matmul", dict(C=1), 5),
    ("C9_derivative", "minimal", "derivative", dict(C=9), 5),
    ("C9_matmul", "minimal", "matmul", dict(C=9), 5),
    ("H7_HH24_evaluate", "original", "evaluate", dict(C=6, H=7, HH=24), 5),      # d0 = 13: no multiple of 4 or 16
    ("H7_HH24_derivative", "minimal", "derivative", dict(C=6, H=7, HH=24), 5),
]


@pytest.mark.parametrize("case", EDGES, ids=[c[0] for c in EDGES])
def test_shape_edges(gpu_lib, case):
    name, kind, mode, dims, B = case
    rows = se.make_rows(7103, 5, B, dims.get("C", hu.MAIN["C"]))
    _check(gpu_lib, name, ("edge", name), lambda d: _model(kind, mode, d, **dims), rows, 0.25)


class HeadOnlyField(torch.nn.Module):
    """A field without inner layers: the heads read the field input u = [z, control] directly (as in tests/test_online_fields_gpu.py)."""

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


def _head_only(kind, mode, device, dtype=F32, C=5, H=12, n_out=3):
    torch.manual_seed(73)
    m = _head_only_class()(C, H, n_out, hidden_hidden_dim=4, num_layers=1, interpolation=PATH, return_sequences=True, solver="rk4",
                           vector_field=kind, vector_field_type=mode)
    return m.to(device=device, dtype=dtype)


@pytest.mark.parametrize("kind,mode", [("original", "derivative"), ("minimal", "evaluate")])
def test_no_inner_layer_the_heads_read_the_field_input(gpu_lib, kind, mode):
    rows = se.make_rows(7104, 5, 17, 5)
    assert _head_only(kind, mode, "cuda").online(17)._problem().n_layers == 0
    _check(gpu_lib, "nl 0 %s/%s" % (kind, mode), ("nl0", kind, mode), lambda d: _head_only(kind, mode, d), rows, 0.25)


# ---- 3. bit-identities ---------------------------------------------------------------------------------------------------------------
BITS = [("minimal", "evaluate"), ("original", "derivative"), ("minimal", "matmul")]


@pytest.mark.parametrize("kind,mode", BITS)
def test_rows_in_one_call_and_interleaved_halves(gpu_lib, kind, mode):
    s = hu.MAIN
    oc.rows_in_one_call_and_interleaved_halves(_model(kind, mode, "cuda"), se.dev(se.make_rows(7105, s["L"], s["B"], s["C"]), "cuda"), s["init"])


@pytest.mark.parametrize("kind,mode", BITS)
def test_masks_and_a_tile_of_mixed_counts(gpu_lib, kind, mode):
    s = se.STAG
    oc.masks_and_a_tile_of_mixed_counts(lambda d: _model(kind, mode, d, seed=41, C=s["C"], H=s["H"], HH=s["HH"], nl=s["nl"], n_out=s["n_out"]),
                                        ("field_hermite", "staggered", kind, mode), "%s/%s" % (kind, mode))


@pytest.mark.parametrize("kind,mode", BITS)
def test_state_dict_round_trip_and_a_refused_call(gpu_lib, kind, mode):
    s = hu.MAIN
    x = se.dev(se.make_rows(7106, s["L"], s["B"], s["C"]), "cuda")
    oc.state_dict_round_trip_and_a_refused_call(gpu_lib, "ncde_stream_step_field_hermite", _model(kind, mode, "cuda"), x, s["init"])


# ---- 4. against the torch-op step ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mode", [("minimal", "matmul"), ("original", "evaluate")])
def test_against_the_torch_step(gpu_lib, kind, mode):
    s = hu.MAIN
    x = se.dev(se.make_rows(7107, s["L"], s["B"], s["C"]), "cuda")
    _, h = oc.against_the_torch_step(_model(kind, mode, "cuda", apply_final_linear=False), x, s["init"], "%s/%s" % (kind, mode))
    assert gpu_lib.ncde_stream_field_hermite_kernel_name(ctypes.byref(h._problem())) == NAME


# ---- 5. the LDS boundary ---------------------------------------------------------------------------------------------------------------
def _wide(H, device):
    return se.make_model(75, 4, H, 2, H, 2, PATH, device, F32, apply_final_linear=False, vector_field_type="evaluate")


def test_last_width_the_lds_plan_holds_steps_fused(gpu_lib):
    """C 4, HH = H, nl 2, evaluate: H 352 is the last width the query accepts (tests/test_online_field_hermite_cpu.py)."""
    rows = se.make_rows(7108, 3, 3, 4)
    assert gpu_lib.ncde_stream_field_hermite_workspace_bytes(ctypes.byref(_wide(352, "cuda").online(3)._problem())) == 0
    _check(gpu_lib, "H352 evaluate", ("wide", 352), lambda d: _wide(352, d), rows, 0.0)


def test_first_width_the_lds_plan_refuses_takes_the_torch_step(gpu_lib):
    rows = se.make_rows(7108, 3, 3, 4)
    model = _wide(353, "cuda")
    assert gpu_lib.ncde_stream_field_hermite_workspace_bytes(ctypes.byref(model.online(3)._problem())) == oc.UNSUPPORTED
    assert gpu_lib.ncde_stream_field_hermite_kernel_name(ctypes.byref(model.online(3)._problem())) is None
    z_ref, o_ref = oc.reference(("field_hermite", "wide", 353), lambda d: _wide(353, d), rows, 0.0)
    oc.torch_step_behind_one_lds_warning(model, rows, 0.0, z_ref, o_ref, "H353 evaluate on the torch-op step")
