"""The low-rank step on the GPU (ncde_stream_step_lowrank / ncde_stream_step_lowrank_hermite, csrc/ncde_stream.hip):
``NeuralCDE.online`` for ``vector_field="low-rank"`` on linear, rectilinear and Hermite paths.

Reference: the batch model in fp64 on the CPU (tests/online_step_checks.reference: stream_ref.prefix_reference on linear and
rectilinear paths, hermite_util.batch_reference on the Hermite path) within the project's forward bound su.TIGHT_Z = 2e-5 of
max |ref|, for z and the readout at every step.  Bit for bit: rows per call, streams run alone or in halves, masks, the state dict,
a refused call.  Within the same bound: the torch-op step on the same GPU tensors and this package's fp32 batch forward (the step
streams the heads and ncde_fwd_lowrank keeps them resident in LDS at these sizes: the same sums in the same order, so the two can
agree bit for bit, which is observed below and not asserted -- the batch loaders form dX/dt from coefficients).

Observed on the MI355X (max over steps of |delta| / max |ref|, z or readout, whichever is larger; not bounds):
  parity linear / rectilinear / Hermite  3.5e-7 / 2.9e-7 / 3.0e-7
  euler / midpoint (Hermite)             5.5e-7 / 6.7e-7
  shape edges, 9 cases                   1.5e-7 .. 3.6e-7 (the largest: time in the last channel, rectilinear)
  staggered schedule, rectilinear        <= 2.1e-7
  vs the torch-op step                   2.2e-7 .. 3.0e-7
  vs the fp32 batch forward              0 (linear, rectilinear), 1.0e-7 (Hermite)
  LDS boundary H 304 fused / H 305 torch 1.3e-7 / 1.2e-7"""
import ctypes

import numpy as np
import pytest
import torch

import online_step_checks as oc
import stream_edges as se
import stream_util as su

pytestmark = pytest.mark.gpu
F32 = torch.float32
PATHS = ["linear", "rectilinear", "cubic_hermite"]
BASE = dict(C=5, H=12, HH=10, nl=2, n_out=3, B=19, rows=6, init=-0.5, sparsity=0.5)      # R = ceil(5 * 0.5) = 3
NAMES = {"linear": b"ncde_stream_step_lowrank", "rectilinear": b"ncde_stream_step_lowrank", "cubic_hermite": b"ncde_stream_step_lowrank_hermite"}


def _model(path, device, seed=91, C=5, H=12, HH=10, nl=2, n_out=3, sparsity=0.5, dtype=F32, **kw):
    return se.make_model(seed, C, H, n_out, HH, nl, path, device, dtype, vector_field="low-rank", sparsity=sparsity, **kw)


def _rank(model):
    return model.func.fused_spec().rank


def _check(lib, what, key, build, rows, init, ti=0):
    path = build("cpu").interpolation
    return oc.check(lib.ncde_stream_lowrank_kernel_name, NAMES[path], what, ("lowrank",) + key, build, rows, init, ti)


# ---- 1. parity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_parity_with_the_fp64_reference(gpu_lib, path):
    s = BASE
    rows = se.make_rows(9101, s["rows"], s["B"], s["C"])
    assert np.isnan(rows).any() and _rank(_model(path, "cpu")) == 3
    _check(gpu_lib, "low-rank %s" % path, ("parity", path), lambda d: _model(path, d), rows, s["init"])


@pytest.mark.parametrize("method", ["euler", "midpoint"])
def test_euler_and_midpoint(gpu_lib, method):
    s = BASE
    rows = se.make_rows(9102, s["rows"], s["B"], s["C"])
    _check(gpu_lib, "low-rank cubic_hermite %s" % method, ("method", method), lambda d: _model("cubic_hermite", d, solver=method), rows, s["init"])


# ---- 2. shape edges ------------------------------------------------------------------------------------------------------------------
EDGES = [      # (id, path, model dims, rank, B, time_index)
    ("B1", "rectilinear", {}, 3, 1, 0),
    ("B16", "cubic_hermite", {}, 3, 16, 0),
    ("B17", "linear", {}, 3, 17, 0),
    ("C1_rect", "rectilinear", dict(C=1), 1, 5, 0),                                  # the time channel alone, R 1
    ("R5_above_the_register_ranks", "linear", dict(C=6, sparsity=0.2), 5, 5, 0),     # R 5 > LR_RREG = 4: the LDS tail of lr_rank_sum
    ("stacked_rows_64", "cubic_hermite", dict(C=4, H=12, sparsity=0.0), 4, 5, 0),    # (H + C) R = 64: PQ has no pad row
    ("stacked_rows_68", "rectilinear", dict(C=4, H=13, sparsity=0.0), 4, 5, 0),      # (H + C) R = 68: twelve pad rows
    ("last_width_15", "linear", dict(HH=15), 3, 5, 0),                               # no multiple of 4 or 16
    ("time_last_rect", "rectilinear", {}, 3, 17, 4),
]


@pytest.mark.parametrize("case", EDGES, ids=[c[0] for c in EDGES])
def test_shape_edges(gpu_lib, case):
    name, path, dims, rank, B, ti = case
    C = dims.get("C", 5)
    assert _rank(_model(path, "cpu", **dims)) == rank
    rows = se.make_rows(9103, 5, B, C, time_index=ti)
    _check(gpu_lib, name, ("edge", name), lambda d: _model(path, d, **dims), rows, 0.25, ti)


# ---- 3. bit-identities ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_rows_in_one_call_and_interleaved_halves(gpu_lib, path):
    s = BASE
    oc.rows_in_one_call_and_interleaved_halves(_model(path, "cuda"), se.dev(se.make_rows(9105, s["rows"], s["B"], s["C"]), "cuda"), s["init"])


@pytest.mark.parametrize("path", ["rectilinear", "cubic_hermite"])
def test_masks_and_a_tile_of_mixed_counts(gpu_lib, path):
    oc.masks_and_a_tile_of_mixed_counts(lambda d: _model(path, d, seed=41), ("lowrank", "staggered", path), "low-rank %s" % path)


@pytest.mark.parametrize("path", ["linear", "cubic_hermite"])
def test_state_dict_round_trip_and_a_refused_call(gpu_lib, path):
    s = BASE
    x = se.dev(se.make_rows(9106, s["rows"], s["B"], s["C"]), "cuda")
    oc.state_dict_round_trip_and_a_refused_call(gpu_lib, "ncde_stream_step_lowrank", _model(path, "cuda"), x, s["init"])


# ---- 4. against the two routes that exist without the kernel ---------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_against_the_torch_step_and_the_batch_forward(gpu_lib, path):
    import ncde_amd
    s = BASE
    model = _model(path, "cuda", apply_final_linear=False)
    x = se.dev(se.make_rows(9107, s["rows"], s["B"], s["C"]), "cuda")
    zs, h = oc.against_the_torch_step(model, x, s["init"], "low-rank %s" % path)
    assert gpu_lib.ncde_stream_lowrank_kernel_name(ctypes.byref(h._problem())) == NAMES[path]
    xb = x.transpose(0, 1).contiguous()
    if path == "cubic_hermite":
        coeffs = ncde_amd.hermite_cubic_coefficients_with_backward_differences(xb, initial_value_if_nan=s["init"], forward_fill=True)
    else:
        rect = path == "rectilinear"
        coeffs = ncde_amd.linear_interpolation_coeffs(xb, rectilinear=0 if rect else None, initial_value_if_nan=s["init"], forward_fill=not rect)
    with torch.no_grad():
        z_batch = model(coeffs).transpose(0, 1).cpu().numpy()
    assert z_batch.shape == zs.shape
    e_batch = max(se.err(zs[k], z_batch[k]) for k in range(s["rows"]))
    print("low-rank %s: vs the fp32 batch forward %.3e" % (path, e_batch))
    assert e_batch <= su.TIGHT_Z, e_batch
    assert np.abs(z_batch[-1] - z_batch[0]).max() > 1e-3


# ---- 5. the LDS boundary ---------------------------------------------------------------------------------------------------------------
WIDE = dict(C=4, sparsity=0.75, last=304, first=305)      # R 1, HH = H, nl 2: tests/test_online_lowrank_cpu.py finds the two widths


def _wide(H, device):
    return _model("linear", device, seed=95, C=WIDE["C"], H=H, HH=H, n_out=2, sparsity=WIDE["sparsity"], apply_final_linear=False)


def test_last_width_the_lds_plan_holds_steps_fused(gpu_lib):
    rows = se.make_rows(9108, 3, 3, WIDE["C"])
    assert gpu_lib.ncde_stream_lowrank_workspace_bytes(ctypes.byref(_wide(WIDE["last"], "cuda").online(3)._problem())) == 0
    _check(gpu_lib, "H%d low-rank" % WIDE["last"], ("wide", WIDE["last"]), lambda d: _wide(WIDE["last"], d), rows, 0.0)


def test_first_width_the_lds_plan_refuses_takes_the_torch_step(gpu_lib):
    rows = se.make_rows(9108, 3, 3, WIDE["C"])
    model = _wide(WIDE["first"], "cuda")
    assert gpu_lib.ncde_stream_lowrank_workspace_bytes(ctypes.byref(model.online(3)._problem())) == oc.UNSUPPORTED
    assert gpu_lib.ncde_stream_lowrank_kernel_name(ctypes.byref(model.online(3)._problem())) is None
    z_ref, o_ref = oc.reference(("lowrank", "wide", WIDE["first"]), lambda d: _wide(WIDE["first"], d), rows, 0.0)
    oc.torch_step_behind_one_lds_warning(model, rows, 0.0, z_ref, o_ref, "H%d low-rank on the torch-op step" % WIDE["first"])
