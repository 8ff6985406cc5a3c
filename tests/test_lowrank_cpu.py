"""The low-rank vector field without a GPU: the module (rank, state_dict, forward), the model class, and the library's validation
and routing of NCDE_FIELD_LOWRANK through dummy-pointer problems (in the style of tests/test_host_cpu.py)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import golden_util as gu
import lowrank_util as lu
import ncde_amd
from ncde_amd import _lib

INVALID, UNSUPPORTED = -1, -2
LOWRANK, GRU = 3, 2


def _problem(B=20, T=9, C=5, H=8, HH=12, nl=2, rank=2, kind=LOWRANK, field_input=0, interp=0, method=2, output=0, flags=0):
    """A structurally valid low-rank problem with dummy (never dereferenced) device pointers."""
    p = _lib.NcdeProblem()
    p.abi_version = _lib.NCDE_ABI_VERSION
    p.batch, p.n_knots, p.channels, p.hidden = B, T, C, H
    p.interp, p.method, p.output = interp, method, output
    p.flags = flags | _lib.FLAG_FIELD_RANK(rank)
    p.n_layers = nl
    d0 = H if field_input == 0 else H + C
    for l in range(nl):
        p.layer_in[l], p.layer_out[l] = (d0 if l == 0 else HH), HH
        p.layer_W[l] = 0x1000 if l == 0 else 0x2000
        p.layer_b[l] = 0x1100 if l == 0 else 0x2100
    p.Wo, p.bo, p.coeffs, p.z0 = 0x3000, 0x3100, 0x4000, 0x5000
    p.Wg, p.bg, p.Wr, p.br = 0x6000, 0x6100, 0x7000, 0x7100
    p.field_kind, p.field_input = kind, field_input
    p.coeffs_stride_b, p.coeffs_stride_t = T * C, (4 * C if interp == 1 else C)
    return p


@pytest.mark.parametrize("C,sparsity,rank", [(5, 0.6, 2), (10, 0.7, 4), (20, 0.95, 2), (5, 0.0, 5)])
def test_rank_is_the_references_expression(C, sparsity, rank):
    """int(np.ceil(C * (1 - sparsity))) in floating point: (10, 0.7) gives 4, not 3, and (20, 0.95) gives 2, not 1."""
    f = ncde_amd.LowRankVectorField(C, 8, 12, 2, sparsity=sparsity)
    assert f.rank == rank == lu.rank_of(C, sparsity)
    spec = f.fused_spec()
    assert (spec.kind, spec.mode, spec.rank) == ("lowrank", "matmul", rank)
    assert spec.extra_params() == [spec.Wg, spec.bg] and spec.Wo is f.M_h.weight and spec.Wg is f.M_o.weight


def test_state_dict_keys_and_shapes():
    C, H, HH, nl, R = 5, 8, 12, 3, 2
    f = ncde_amd.LowRankVectorField(C, H, HH, nl, sparsity=0.6)
    shapes = {k: tuple(v.shape) for k, v in f.state_dict().items()}
    assert shapes == {"net_to_hh.0.weight": (HH, H), "net_to_hh.0.bias": (HH,), "net_to_hh.2.weight": (HH, HH), "net_to_hh.2.bias": (HH,),
                      "net_to_hh.4.weight": (HH, HH), "net_to_hh.4.bias": (HH,), "M_h.weight": (H * R, HH), "M_h.bias": (H * R,),
                      "M_o.weight": (R * C, HH), "M_o.bias": (R * C,)}
    assert f.net_to_hh[2] is f.net_to_hh[4]
    assert len(f.fused_spec().unique_params()) == 8
    with pytest.raises(AssertionError):
        ncde_amd.LowRankVectorField(C, H, HH, nl)                                               # no sparsity
    with pytest.raises(AssertionError):
        ncde_amd.LowRankVectorField(C, H, HH, nl, sparsity=0.6, vector_field_type="evaluate")   # matmul only


@pytest.mark.parametrize("C,H,HH,nl,sparsity", [(5, 8, 12, 2, 0.6), (4, 16, 16, 3, 0.0), (24, 32, 32, 1, 0.875)])
def test_forward_matches_the_restated_formula(C, H, HH, nl, sparsity):
    R = lu.rank_of(C, sparsity)
    p = lu.make_weights(gu.data, H, HH, C, R, nl, seed=11)
    z = (gu.data.normal(5, 7 * H, stream=2).reshape(7, H) * 0.7).astype(np.float32)
    ref = lu.restated_forward(p, z, H, C, R, nl)
    f64, _ = lu.make_field(ncde_amd, p, C, H, HH, nl, sparsity, dtype=torch.float64)
    out = f64(0.0, torch.from_numpy(z).double())
    assert out.shape == (7, H, C) and f64.nfe == 1
    assert gu.relerr(out.detach().numpy(), ref.numpy()) <= 1e-13
    f32, _ = lu.make_field(ncde_amd, p, C, H, HH, nl, sparsity)
    assert gu.relerr(f32(0.0, torch.from_numpy(z)).detach().numpy(), ref.numpy()) <= 2e-6


def test_model_constructs_the_field_and_sparse_stays_refused():
    m = ncde_amd.NeuralCDE(5, 8, 2, hidden_hidden_dim=12, num_layers=2, vector_field="low-rank", sparsity=0.6)
    assert type(m.func) is ncde_amd.LowRankVectorField and m.func.rank == 2
    assert {"func.M_h.weight", "func.M_o.bias", "func.net_to_hh.0.weight"} <= set(m.state_dict())
    with pytest.raises(NotImplementedError, match="sparselinear"):
        ncde_amd.NeuralCDE(5, 8, 2, vector_field="sparse", sparsity=0.6)
    for cls in (ncde_amd.OriginalVectorField, ncde_amd.MinimalGatedVectorField, ncde_amd.GRUGatedVectorField):
        with pytest.raises(NotImplementedError):
            cls(5, 8, 12, 2, sparsity=0.5)
        assert cls(5, 8, 12, 2).sparsity is None


def test_library_names_the_lowrank_kernels():
    lib = ncde_amd.lib()
    for kw in ({}, {"output": 1}, {"interp": 1, "method": 1}, {"C": 24, "H": 32, "HH": 32, "nl": 3, "rank": 3, "B": 81}, {"rank": 5}):
        p = _problem(**kw)
        names = [(lib.ncde_kernel_name(ctypes.byref(p), ps) or b"").decode() for ps in (0, 1, 2)]
        assert names == ["ncde_fwd_lowrank", "ncde_adj_lowrank", "ncde_adj_lowrank<discrete>"], (kw, lib.ncde_last_error_string())
        assert lib.ncde_workspace_bytes(ctypes.byref(p), 0) > 0
        n_wg = (p.batch + 15) // 16
        theta = sum(p.layer_out[l] * (p.layer_in[l] + 1) for l in range(2 if p.n_layers > 1 else 1))
        theta += (p.hidden + p.channels) * (p.flags >> 24) * (p.layer_out[0] + 1)
        for ps in (1, 2):
            assert lib.ncde_workspace_bytes(ctypes.byref(p), ps) == 4 * n_wg * theta + 256
    assert lib.ncde_coop_status_offset(ctypes.byref(_problem()), 1) == UNSUPPORTED


def test_library_validates_the_lowrank_problem():
    lib = ncde_amd.lib()

    def rc(p):
        return lib.ncde_workspace_bytes(ctypes.byref(p), 0)
    assert rc(_problem()) > 0
    for mode in (1, 2):
        assert rc(_problem(field_input=mode)) == INVALID, mode
    assert rc(_problem(rank=0)) == INVALID
    assert b"rank" in lib.ncde_last_error_string()
    assert rc(_problem(rank=6)) == INVALID                # above channels = 5
    assert rc(_problem(rank=5)) > 0                       # R = C is allowed
    p = _problem()
    p.Wg = None
    assert rc(p) == INVALID
    p = _problem()
    p.bg = None
    assert rc(p) == INVALID
    p = _problem()
    p.Wr, p.br = None, None                               # unused by this field
    assert rc(p) > 0
    assert lib.ncde_num_outputs(ctypes.byref(_problem(output=1))) == 9


def test_library_refuses_what_the_field_has_no_kernel_for():
    lib = ncde_amd.lib()
    for flag in (_lib.FLAG_FORCE_FAST, _lib.FLAG_FORCE_TILED):
        for ps in (0, 1, 2):
            assert lib.ncde_workspace_bytes(ctypes.byref(_problem(flags=flag)), ps) == UNSUPPORTED
            assert lib.ncde_kernel_name(ctypes.byref(_problem(flags=flag)), ps) is None
    for ps in (0, 1, 2):
        assert lib.ncde_dopri5_kernel_name(ctypes.byref(_problem()), ps) is None
    assert lib.ncde_control_kernel_name(ctypes.byref(_problem())) is None
    assert lib.ncde_control_workspace_bytes(ctypes.byref(_problem())) == UNSUPPORTED
    # beyond the family's limits: refused by the queries, before anything is launched
    for kw in ({"HH": 144}, {"H": 144}, {"C": 130, "rank": 3}, {"nl": 0}, {"H": 128, "C": 128, "rank": 128, "HH": 128}):
        for ps in (0, 1, 2):
            assert lib.ncde_workspace_bytes(ctypes.byref(_problem(**kw)), ps) == UNSUPPORTED, (kw, ps)
            assert lib.ncde_kernel_name(ctypes.byref(_problem(**kw)), ps) is None


def test_rank_byte_is_ignored_by_the_other_fields():
    """A GRU problem (and the original field) with a non-zero top byte in flags validates and routes as with 0."""
    lib = ncde_amd.lib()
    for kind in (0, 1, GRU):
        for ps in (0, 1, 2):
            a, b = _problem(kind=kind, rank=0), _problem(kind=kind, rank=7)
            assert lib.ncde_kernel_name(ctypes.byref(a), ps) == lib.ncde_kernel_name(ctypes.byref(b), ps) is not None
            assert lib.ncde_workspace_bytes(ctypes.byref(a), ps) == lib.ncde_workspace_bytes(ctypes.byref(b), ps) > 0
    big = dict(B=32, T=49, C=20, H=32, HH=32, nl=3, kind=0)
    assert lib.ncde_kernel_name(ctypes.byref(_problem(rank=0, **big)), 1) == lib.ncde_kernel_name(ctypes.byref(_problem(rank=200, **big)), 1)
    assert _lib.FIELD_KIND["lowrank"] == LOWRANK and _lib.FLAG_FIELD_RANK(3) == 3 << 24 and _lib.NCDE_ABI_VERSION == 4


def test_build_problem_carries_the_rank_in_flags():
    from ncde_amd import solver
    f = ncde_amd.LowRankVectorField(5, 8, 12, 2, sparsity=0.6)
    coeffs, z0 = torch.zeros(3, 9, 5), torch.zeros(3, 8)
    p = solver.build_problem(coeffs, "linear", z0, f.fused_spec(), "rk4", _lib.OUT_KNOTS, flags=_lib.FLAG_FORCE_GENERIC)
    assert p.field_kind == LOWRANK and p.flags == (2 << 24) | _lib.FLAG_FORCE_GENERIC
    assert p.Wo == f.M_h.weight.data_ptr() and p.Wg == f.M_o.weight.data_ptr() and not p.Wr
    assert (ncde_amd.lib().ncde_kernel_name(ctypes.byref(p), 0) or b"").decode() == "ncde_fwd_lowrank"
    spec = f.fused_spec()
    spec.rank = 3
    with pytest.raises(ValueError):
        solver.build_problem(coeffs, "linear", z0, spec, "rk4", _lib.OUT_KNOTS)


def test_golden_manifest_lists_every_file_present():
    with open(os.path.join(gu.GOLD, "MANIFEST_lowrank.json")) as fh:
        manifest = {e["name"]: e for e in json.load(fh)}
    with open(os.path.join(gu.GOLD, "MANIFEST_smooth_control.json")) as fh:      # the other owner of the g17_ prefix
        other = {e["name"] for e in json.load(fh)}
    present = {n[:-4] for n in os.listdir(gu.GOLD) if n.startswith("g17_") and n.endswith(".npz")} - other
    assert present == set(manifest) and len(manifest) == 5
    for name, m in manifest.items():
        f = np.load(os.path.join(gu.GOLD, name + ".npz"))
        assert json.loads(str(f["meta"])) == m
        assert os.path.getsize(os.path.join(gu.GOLD, name + ".npz")) < 1 << 20
        d = m["dims"]
        assert d["R"] == lu.rank_of(d["C"], m["sparsity"])
        for tag in ("adj", "disc"):
            assert m["ref_drift"][tag]["z"] <= 2e-5 / 4 and max(m["ref_drift"][tag]["dz0"], m["ref_drift"][tag]["dtheta"]) <= 2e-4 / 4
            assert min(m["max_head_grads"][tag].values()) >= 1e3 * 2e-4
            for k in m["param_names"]:
                assert f["d%s_%s" % (k, tag)].shape == f["p_" + k].shape
