"""CPU tests of the host side: C-ABI surface (loads, exports, validation -- no compute without a GPU),
control-path mirrors, coefficient preparation known answers, argument/error behaviour of cdeint."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import golden_util as gu
import ncde_amd
from ncde_amd import _lib, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem(B=32, T=49, C=20, H=32, HH=32, nl=3, interp=0, method=2, output=0, flags=0):
    """A structurally valid problem with dummy (never dereferenced) device pointers."""
    p = _lib.NcdeProblem()
    p.abi_version = _lib.NCDE_ABI_VERSION
    p.batch, p.n_knots, p.channels, p.hidden = B, T, C, H
    p.interp, p.method, p.output, p.flags = interp, method, output, flags
    p.n_layers = nl
    for l in range(nl):
        p.layer_in[l], p.layer_out[l] = (H if l == 0 else HH), HH
        p.layer_W[l] = 0x1000 if l == 0 else 0x2000
        p.layer_b[l] = 0x1100 if l == 0 else 0x2100
    p.Wo, p.bo, p.coeffs, p.z0 = 0x3000, 0x3100, 0x4000, 0x5000
    p.coeffs_stride_b, p.coeffs_stride_t = T * C, (4 * C if interp == 1 else C)
    return p


def test_library_loads_and_exports_every_declared_symbol():
    lib = ncde_amd.lib()
    header = open(os.path.join(ROOT, "include", "ncde_hip.h")).read()
    declared = set(re.findall(r"\b(ncde_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.ncde_version() == _lib.NCDE_ABI_VERSION


def test_struct_layout_matches_header():
    # 9 int32 + n_layers + 2*8 int32, 2*8 pointers, 3 pointers, 2 int64, 1 pointer (with natural alignment);
    # ABI version 2 appends 2 int32 + 4 pointers (gated fields / input modes), version 3 one pointer + 4 int32 (general time
    # axis) -- every older struct is a prefix of the newer one
    v1 = 4 * 10 + 4 * 16 + 8 * 16 + 8 * 3 + 8 * 2 + 8
    assert _lib.NcdeProblem.field_kind.offset == v1
    assert _lib.NcdeProblem.time_plan.offset == v1 + 4 * 2 + 8 * 4
    assert ctypes.sizeof(_lib.NcdeProblem) == v1 + 4 * 2 + 8 * 4 + 8 + 4 * 4
    assert ctypes.sizeof(_lib.NcdeTimeSpec) == 4 * 2 + 8 * 3 and ctypes.sizeof(_lib.NcdeTimePlanInfo) == 4 * 4 + 8
    assert ctypes.sizeof(_lib.NcdeGrads) == 8 * (1 + 16 + 2 + 4)


def test_version1_structs_are_still_accepted():
    """A caller built against the version-1 header passes the shorter struct; the library must not read past it."""
    lib = ncde_amd.lib()
    p = _problem()
    p.abi_version = 1
    p.field_kind, p.field_input = 7, 9            # garbage where a version-1 struct simply ends
    assert lib.ncde_num_outputs(ctypes.byref(p)) == 2
    assert (lib.ncde_kernel_name(ctypes.byref(p), 0) or b"").startswith(b"ncde_fwd_fast")
    p.abi_version = 2
    assert lib.ncde_num_outputs(ctypes.byref(p)) == -1 and b"field_kind" in lib.ncde_last_error_string()
    p.field_kind, p.field_input = 0, 5
    assert lib.ncde_num_outputs(ctypes.byref(p)) == -1 and b"vector_field_type" in lib.ncde_last_error_string()
    p.field_kind, p.field_input = 1, 0
    assert lib.ncde_num_outputs(ctypes.byref(p)) == -1 and b"Wg" in lib.ncde_last_error_string()
    p.Wg, p.bg = 0x6000, 0x6100
    assert lib.ncde_kernel_name(ctypes.byref(p), 1).startswith(b"ncde_adj_tiled<gated")            # minimal gating: tiled family
    p.field_kind, p.Wr, p.br = 2, 0x7000, 0x7100
    assert lib.ncde_kernel_name(ctypes.byref(p), 1) == b"ncde_adj_variant"                           # GRU: variant kernels
    # a version-2 caller's struct ends before time_plan: garbage there must not be read
    q = _problem()
    q.abi_version = 2
    q.time_plan, q.n_t_out = 0xdead, -5
    assert lib.ncde_num_outputs(ctypes.byref(q)) == 2
    q.abi_version = 3
    assert lib.ncde_num_outputs(ctypes.byref(q)) == -1 and b"time plan" in lib.ncde_last_error_string()


def test_validation_and_error_strings_without_gpu():
    lib = ncde_amd.lib()
    p = _problem()
    assert lib.ncde_num_outputs(ctypes.byref(p)) == 2
    p.output = _lib.OUT_KNOTS
    assert lib.ncde_num_outputs(ctypes.byref(p)) == 49
    bad = _problem(T=1)
    assert lib.ncde_workspace_bytes(ctypes.byref(bad), 0) == -1
    assert b"at least 2" in lib.ncde_last_error_string()
    bad = _problem(method=7)
    assert lib.ncde_workspace_bytes(ctypes.byref(bad), 0) == -1
    assert b"Invalid method" in lib.ncde_last_error_string()
    bad = _problem()
    bad.layer_in[1] = 17
    assert lib.ncde_num_outputs(ctypes.byref(bad)) == -1
    with pytest.raises(ValueError):
        _lib.check(-1, "x")
    with pytest.raises(NotImplementedError):
        _lib.check(-2, "x")
    with pytest.raises(ncde_amd.NcdeError):
        _lib.check(-4, "x")


def test_kernel_family_selection():
    lib = ncde_amd.lib()
    name = lambda p, k: (lib.ncde_kernel_name(ctypes.byref(p), k) or b"").decode()
    p = _problem()                                    # BASELINE cfg2 shape -> specialised kernels
    assert name(p, 0).startswith("ncde_fwd_fast") and name(p, 1).startswith("ncde_adj_fast")
    assert name(_problem(flags=_lib.FLAG_FORCE_GENERIC), 0) == "ncde_fwd_generic"
    q = _problem(C=5, H=16, HH=24)                    # arbitrary small shape -> zero-padded onto the smallest register-resident set that
    # holds it: (32, 32, 8) of round 6's few-channel sets (C = 4 / 8 / 12), (32, 32, 20) above 12 channels
    assert name(q, 0).startswith("ncde_fwd_fast_bf3<H32,HH32,C8") and name(q, 1).startswith("ncde_adj_fast3<H32,HH32,C8,NL3") and "discrete" in name(q, 2)
    wq = lib.ncde_workspace_bytes(ctypes.byref(q), 1)
    q8 = _problem(C=8, H=32, HH=32)                   # the shape it is padded to: same kernels, workspace without the padded copies
    assert name(q8, 1) == name(q, 1) and 0 < lib.ncde_workspace_bytes(ctypes.byref(q8), 1) < wq
    for C, cset in ((1, 4), (4, 4), (7, 8), (9, 12), (12, 12), (13, 20), (20, 20)):
        d = _problem(C=C, H=32, HH=15)                # the reference's default hidden_hidden_dim (src/ncde/ncde.py:47)
        assert name(d, 0).startswith("ncde_fwd_fast_bf3<H32,HH32,C%d," % cset) and name(d, 1).startswith("ncde_adj_fast3<H32,HH32,C%d," % cset), (C, name(d, 0), name(d, 1))
        assert "discrete" in name(d, 2) and ("C%d," % cset) in name(d, 2)
    q.flags = _lib.FLAG_FORCE_TILED                   # ... onto the batch-tiled family (C 8, HH 32) when that is asked for, or when the
    assert name(q, 0).startswith("ncde_fwd_tiled") and name(q, 1).startswith("ncde_adj_tiled")      # shape is beyond the specialised ones
    w = _problem(C=21, H=47, HH=93)
    assert name(w, 0).startswith("ncde_fwd_tiled") and name(w, 1).startswith("ncde_adj_tiled") and name(w, 2).startswith("ncde_adj_tiled")
    w24 = _problem(C=24, H=48, HH=128)
    assert name(w24, 1) == name(w, 1) and 0 < lib.ncde_workspace_bytes(ctypes.byref(w24), 1) < lib.ncde_workspace_bytes(ctypes.byref(w), 1)
    q.flags = _lib.FLAG_FORCE_GENERIC                 # ... unless the generic family is asked for
    assert name(q, 0) == "ncde_fwd_generic" and name(q, 1) == "ncde_adj_generic"
    q.flags = _lib.FLAG_FORCE_FAST
    assert lib.ncde_workspace_bytes(ctypes.byref(q), 0) == -2
    # adjoint workspace = one |theta| partial per 16-sample workgroup
    theta = 32 * 32 + 32 + 32 * 32 + 32 + 640 * 32 + 640
    assert lib.ncde_workspace_bytes(ctypes.byref(p), 1) == 4 * 2 * theta + 256 + 256     # partials, header, range-fault words (one per workgroup, rounded up)
    un = _problem(C=80, H=128, HH=512, nl=2)          # too wide for the generic adjoint's LDS plan
    assert lib.ncde_workspace_bytes(ctypes.byref(un), 1) == -2


def test_reserved_field_of_the_problem_is_not_an_input():
    """NcdeProblem.reserved_ carries the real extents of a zero-padded problem INSIDE the library; whatever a caller
    leaves in it (an uninitialised stack struct) must be ignored, not read as row strides."""
    lib = ncde_amd.lib()
    for shape in (dict(), dict(C=5, H=16, HH=24), dict(C=21, H=47, HH=93)):
        clean, dirty = _problem(**shape), _problem(**shape)
        dirty.reserved_ = (777 << 12) | 333
        for k in (0, 1, 2):
            assert lib.ncde_kernel_name(ctypes.byref(dirty), k) == lib.ncde_kernel_name(ctypes.byref(clean), k)
            assert lib.ncde_workspace_bytes(ctypes.byref(dirty), k) == lib.ncde_workspace_bytes(ctypes.byref(clean), k)


def test_shapes_without_a_backward_kernel_are_known_before_the_forward():
    """cdeint asks the library for every pass it will need BEFORE launching the forward (solver._no_kernel_reason)
    and sends a shape no fused kernel covers to the unfused solver, instead of failing inside loss.backward()."""
    big = _problem(C=20, H=196, HH=272, nl=3)          # a hidden width beyond 256: forward only
    assert solver._no_kernel_reason(big, (0,)) is None                       # the forward exists ...
    why = solver._no_kernel_reason(big, (0, 2))                              # ... the exact discrete backward does not
    assert why is not None and "hidden=196" in why and "272" in why and "discrete backward" in why
    assert "continuous adjoint" in solver._no_kernel_reason(big, (0, 1))
    assert solver._no_kernel_reason(_problem(C=20, H=256, HH=256, nl=4), (0, 1)) is not None      # four 256-wide layers: the sweep's LDS plan ends at three
    assert solver._no_kernel_reason(_problem(), (0, 1, 2)) is None           # BASELINE cfg2: every pass
    assert solver._no_kernel_reason(_problem(C=100, H=64, HH=64), (0, 1, 2)) is None      # round 5: more than 80 channels on the batch-tiled backward
    assert solver._no_kernel_reason(_problem(C=20, H=160, HH=128), (0, 1, 2)) is None     # round 5: hidden > 128 with a last width <= 128
    # round 5: hidden widths up to 256 (zero-padded to 256 in the backward) -- the reference's hyper-parameter range
    # (configurations.json5:34-35: hidden_dim up to 256, hidden_hidden_dim up to 196), the shapes VERDICT round 4 lists
    lib = ncde_amd.lib()
    for C, H, HH, nl in ((20, 160, 128, 3), (20, 196, 196, 3), (20, 256, 196, 2), (100, 64, 64, 3), (20, 196, 196, 2), (7, 256, 160, 3)):
        q = _problem(C=C, H=H, HH=HH, nl=nl)
        assert solver._no_kernel_reason(q, (0, 1, 2)) is None, (C, H, HH, nl)
        for k in (0, 1, 2):
            name = (lib.ncde_kernel_name(ctypes.byref(q), k) or b"").decode()
            assert name and "generic" not in name, (C, H, HH, nl, k, name)


def test_cooperative_status_word_offset_is_inside_the_workspace():
    """Round 6: every pass that may launch the XCD-cooperative kernels names a status word inside the
    caller's workspace; passes that never do say so (NCDE_ERR_UNSUPPORTED), and NCDE_FLAG_NO_COOP removes it."""
    lib = ncde_amd.lib()
    big = dict(B=4096, T=799, C=80, H=128, HH=128, nl=3)
    for ps in (0, 1, 2):
        p = _problem(**big)
        off, need = lib.ncde_coop_status_offset(ctypes.byref(p), ps), lib.ncde_workspace_bytes(ctypes.byref(p), ps)
        assert 0 <= off and off % 4 == 0 and off + 4 <= need, (ps, off, need)
        q = _problem(flags=_lib.FLAG_NO_COOP, **big)
        assert lib.ncde_coop_status_offset(ctypes.byref(q), ps) == -2
        small = _problem()      # cfg2's shape: register-resident kernels, nothing cooperative
        assert lib.ncde_coop_status_offset(ctypes.byref(small), ps) == -2
    # a zero-padded problem (hidden width 120 -> 128) on the batch-tiled family: the offset counts the padded-parameter head
    pp = _problem(B=512, T=9, C=80, H=128, HH=120, nl=3)
    if b"coop" in (lib.ncde_kernel_name(ctypes.byref(pp), 1) or b""):
        off, need = lib.ncde_coop_status_offset(ctypes.byref(pp), 1), lib.ncde_workspace_bytes(ctypes.byref(pp), 1)
        assert 0 < off and off + 4 <= need


def test_dopri5_kernel_selection():
    """Round 4: the fused attempt kernels where the shape allows, the per-launch kernels elsewhere and under FORCE_GENERIC."""
    lib = ncde_amd.lib()
    name = lambda p, k: (lib.ncde_dopri5_kernel_name(ctypes.byref(p), k) or b"").decode()
    p = _problem()                                    # BASELINE cfg2 shape
    assert name(p, 0).startswith("ncde_dpf_fwd<H32") and name(p, 1).startswith("ncde_dpf_adj<H32") and name(p, 2).startswith("ncde_dpf_tape<H32")
    q = _problem(C=5, H=16, HH=24)                    # smaller: the same kernels (weights read with their real extents)
    assert [name(q, k) for k in (0, 1, 2)] == [name(p, k) for k in (0, 1, 2)]
    w = _problem(C=3, H=48, HH=64, nl=2)              # (64, 64, 4) set: forward only
    assert name(w, 0).startswith("ncde_dpf_fwd<H64") and name(w, 1).startswith("ncde_dp_stage") and name(w, 2) == "ncde_dp_tape_backward"
    n4 = _problem(nl=4)                               # four layers: the adjoint's images do not fit in LDS
    assert name(n4, 0).startswith("ncde_dpf_fwd<H32") and name(n4, 1).startswith("ncde_dp_stage")
    big = _problem(C=21, H=47, HH=93)
    assert all(name(big, k).startswith("ncde_dp_") for k in (0, 1, 2))
    assert name(_problem(flags=_lib.FLAG_FORCE_GENERIC), 0).startswith("ncde_dp_stage")
    ts = _lib.NcdeTimeSpec() if hasattr(_lib, "NcdeTimeSpec") else None
    assert lib.ncde_dopri5_kernel_name(ctypes.byref(_problem(C=80, H=128, HH=512, nl=2)), 1) is None      # beyond the adjoint's LDS plan


def test_control_paths_match_oracle_control():
    import ncde_oracle as orc
    lin = gu.data.make_rectilinear_coeffs(3, 6, 4, missing=0.3, seed=5)
    cub = gu.data.make_cubic_coeffs(3, 7, 3, seed=6)
    for coeffs, cls, kind in ((lin, ncde_amd.LinearInterpolation, "linear"), (cub, ncde_amd.NaturalCubicSpline, "cubic")):
        X, ctl = cls(torch.from_numpy(coeffs)), orc.Control(coeffs, kind)
        assert X.n_knots == ctl.n_knots and X.channels == ctl.channels
        assert torch.equal(X.evaluate(0), ctl.x0())
        assert torch.equal(X.grid_points, torch.arange(ctl.n_knots, dtype=torch.float32))
        assert torch.equal(X.interval, torch.tensor([0.0, ctl.n_knots - 1]))
        for tv in (0.0, 0.25, 1.0, 1.0 + 1 / 3, 2.5, float(ctl.n_knots - 1)):
            t = torch.tensor(tv)
            assert torch.allclose(X.derivative(t), ctl.derivative(t), rtol=0, atol=0), (kind, tv)


def test_rectilinear_preparation_known_answer():
    """Same hand example as the reference's test (modules/torchcde/test/test_linear_interpolation.py:117-152)."""
    nan = float("nan")
    x = np.array([[[0.1, 0.4], [0.2, nan], [0.9, 1.1]],
                  [[0.2, nan], [0.3, 2.0], [0.3, nan]]], dtype=np.float32)
    want = np.array([[[0.1, 0.4], [0.2, 0.4], [0.2, 0.4], [0.9, 0.4], [0.9, 1.1]],
                     [[0.2, 2.0], [0.3, 2.0], [0.3, 2.0], [0.3, 2.0], [0.3, 2.0]]], dtype=np.float32)
    got = gu.data.linear_interpolation_coeffs(x, rectilinear=0)
    assert np.array_equal(got, want)
    assert np.array_equal(gu.data.linear_interpolation_coeffs(x[:, :, ::-1].copy(), rectilinear=1), want[:, :, ::-1])
    bad = x.copy()
    bad[0, 1, 0] = nan
    with pytest.raises(AssertionError):
        gu.data.linear_interpolation_coeffs(bad, rectilinear=0)
    # interior gaps are filled linearly, all-NaN channels become 0
    y = np.array([[[0.0, nan], [nan, nan], [2.0, nan]]], dtype=np.float32)
    assert np.array_equal(gu.data.linear_interpolation_coeffs(y), np.array([[[0, 0], [1, 0], [2, 0]]], np.float32))


def test_natural_cubic_reproduces_linear_data_and_interpolates_knots():
    """Properties the reference tests for its spline (test_natural_cubic_spline.py:102-141)."""
    L, C = 9, 3
    t = np.arange(L, dtype=np.float32)[:, None]
    x = (t * np.array([0.5, -1.25, 2.0], np.float32) + np.array([1.0, 0.0, -3.0], np.float32))[None]
    X = ncde_amd.NaturalCubicSpline(torch.from_numpy(gu.data.natural_cubic_coeffs(x)))
    for tv in (0.0, 0.3, 4.0, 6.75, 8.0):
        assert torch.allclose(X.derivative(torch.tensor(tv)), torch.tensor([[0.5, -1.25, 2.0]]), atol=1e-4)
        assert torch.allclose(X.evaluate(torch.tensor(tv)), torch.from_numpy(x[:, 0] + tv * np.array([0.5, -1.25, 2.0], np.float32)), atol=1e-4)
    y = ncde_amd.data.synthetic_series(2, 12, 2, seed=3)
    Y = ncde_amd.NaturalCubicSpline(torch.from_numpy(gu.data.natural_cubic_coeffs(y)))
    for k in range(12):
        assert torch.allclose(Y.evaluate(torch.tensor(float(k))), torch.from_numpy(y[:, k]), atol=1e-5)


def test_generator_is_deterministic_and_shardable():
    a = gu.data.make_rectilinear_coeffs(8, 10, 3, missing=0.3, seed=1234)
    b = gu.data.make_rectilinear_coeffs(8, 10, 3, missing=0.3, seed=1234)
    assert np.array_equal(a, b) and not np.isnan(a).any()
    lo = gu.data.make_rectilinear_coeffs(4, 10, 3, missing=0.3, seed=1234, batch_offset=0)
    hi = gu.data.make_rectilinear_coeffs(4, 10, 3, missing=0.3, seed=1234, batch_offset=4)
    assert np.array_equal(np.concatenate([lo, hi]), a)     # rank shards tile the global batch exactly
    assert a.shape == (8, 19, 4) and np.all(np.diff(a[:, :, 0], axis=1) >= 0)


def test_module_state_dict_layout_and_weight_sharing():
    m = ncde_amd.NeuralCDE(5, 16, 3, hidden_hidden_dim=24, num_layers=4)
    keys = set(m.state_dict().keys())
    assert keys == {"initial_linear.weight", "initial_linear.bias", "final_linear.weight", "final_linear.bias",
                    "func.net_to_hh.0.weight", "func.net_to_hh.0.bias", "func.net_to_hh.2.weight", "func.net_to_hh.2.bias",
                    "func.net_to_hh.4.weight", "func.net_to_hh.4.bias", "func.net_to_hh.6.weight", "func.net_to_hh.6.bias",
                    "func.tanh_output_layer.0.weight", "func.tanh_output_layer.0.bias"}
    spec = m.func.fused_spec()
    assert len(spec.layers) == 4 and spec.layers[1][0] is spec.layers[2][0] is spec.layers[3][0]
    assert len(spec.unique_params()) == 6 and len(list(m.func.parameters())) == 6
    assert tuple(spec.Wo.shape) == (16 * 5, 24)
    assert m.func(None, torch.zeros(2, 16)).shape == (2, 16, 5) and m.nfe == 1


def test_cdeint_argument_errors_mirror_the_reference():
    X = ncde_amd.LinearInterpolation(torch.zeros(2, 5, 3))
    f = ncde_amd.OriginalVectorField(3, 4, 8, 2)
    z0 = torch.zeros(2, 4)
    with pytest.raises(ValueError, match="vector_field_type"):
        ncde_amd.cdeint(X, f, z0, X.interval, vector_field_type="bogus")
    with pytest.raises(ValueError, match="Invalid method"):
        ncde_amd.cdeint(X, f, z0, X.interval, method="rk5", options={"step_size": 1})
    with pytest.raises(NotImplementedError, match="GPU"):
        ncde_amd.cdeint(X, f, z0, X.interval)                       # the reference's default, adaptive dopri5: past the argument
    with pytest.raises(NotImplementedError, match="GPU"):            # checks, stops at the CPU tensors (no CPU fallback); so does
        ncde_amd.cdeint(X, f, z0, X.interval, adjoint=False)        # adjoint=False with dopri5 (the taped solve is built)
    with pytest.raises(NotImplementedError, match="bosh3"):
        ncde_amd.cdeint(X, f, z0, X.interval, method="bosh3")
    with pytest.raises(NotImplementedError, match="step_size"):
        ncde_amd.cdeint(X, f, z0, X.interval, method="rk4")
    with pytest.raises(ValueError, match="positive"):
        ncde_amd.cdeint(X, f, z0, X.interval, method="rk4", options={"step_size": -1})
    with pytest.raises(NotImplementedError, match="fused_spec"):
        solver._field_spec(torch.nn.Linear(4, 12))      # arbitrary Python vector fields are refused, not emulated


def test_no_cpu_fallback_product_path_fails_loudly_on_cpu_tensors():
    X = ncde_amd.LinearInterpolation(torch.zeros(2, 5, 3))
    f = ncde_amd.OriginalVectorField(3, 4, 8, 2)
    with pytest.raises(NotImplementedError, match="GPU"):
        ncde_amd.cdeint(X, f, torch.zeros(2, 4), X.interval, method="rk4", options={"step_size": 1})
    m = ncde_amd.NeuralCDE(3, 4, 1, hidden_hidden_dim=8)
    with pytest.raises(NotImplementedError):
        m(torch.zeros(2, 5, 3))
    m5 = ncde_amd.NeuralCDE(3, 4, 1, solver="dopri5")
    assert m5.cdeint_options == {"min_step": 0.5} and (m5.rtol, m5.atol) == (1e-3, 1e-5)      # src/ncde/ncde.py:130-134
    with pytest.raises(NotImplementedError):
        m5(torch.zeros(2, 5, 3))


def test_control_path_gradients_are_refused_not_dropped():
    """adjoint=False tapes the solve in the reference, so coefficients that require grad would receive one; the fused backward
    has no dL/dcoeffs, so such a call (and an explicit request through adjoint_params) is routed to the unfused torch-op solver --
    which runs on the GPU only: on CPU tensors it is refused (no CPU fallback), never silently dropped.  adjoint=True without
    listing the coefficients: the reference's warning (torchcde/solver.py:207-221).  perturb=True is not silently swallowed."""
    import warnings
    c = torch.zeros(2, 5, 3, requires_grad=True)
    X = ncde_amd.LinearInterpolation(c)
    f = ncde_amd.OriginalVectorField(3, 4, 8, 2)
    z0 = torch.zeros(2, 4)
    kw = dict(method="rk4", options={"step_size": 1})
    assert solver._unfused_reason(X, f, z0, X.interval, False, None) == "the control path requires gradients"
    assert solver._unfused_reason(X, f, z0, X.interval, True, tuple(f.parameters()) + (c,)) == "the control path requires gradients"
    assert solver._unfused_reason(X, f, z0, X.interval, True, None) is None          # the fused path, with the reference's warning
    assert solver._unfused_reason(X, torch.nn.Linear(4, 12), z0, X.interval, True, None) == "func does not expose fused_spec()"
    assert solver._unfused_reason(X, f, z0, torch.tensor([4.0, 0.0]), True, None) == "decreasing output times"
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        ncde_amd.cdeint(X, f, z0, X.interval, adjoint=False, **kw)
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        ncde_amd.cdeint(X, f, z0, X.interval, adjoint=True, adjoint_params=tuple(f.parameters()) + (c,), **kw)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with pytest.raises(NotImplementedError, match="GPU"):       # past the warning, stops at the CPU tensors
            ncde_amd.cdeint(X, f, z0, X.interval, adjoint=True, **kw)
        assert any("requires gradients" in str(x.message) for x in w)
    Xd = ncde_amd.LinearInterpolation(torch.zeros(2, 5, 3))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with pytest.raises(NotImplementedError, match="GPU"):
            ncde_amd.cdeint(Xd, f, z0, Xd.interval, method="rk4", options={"step_size": 1, "perturb": True})
        assert any("perturb" in str(x.message) for x in w)


def test_tagged_times_do_not_outlive_their_control():
    """X.interval / X.grid_points carry a weak reference to their control: a tensor kept from another (or a dead) control
    is re-validated by value instead of being trusted."""
    X = ncde_amd.LinearInterpolation(torch.zeros(2, 5, 3))
    Y = ncde_amd.LinearInterpolation(torch.zeros(2, 9, 3))
    assert solver._time_mode(X, Y.grid_points) is None          # 9 knots of another control: not X's grid_points
    kept = Y.interval
    del Y
    assert solver._time_mode(X, kept) is None                   # [0, 8] is not X's interval [0, 4]


def _c_time_plan(n_knots, method, t, step, knots=None):
    p = _lib.NcdeProblem()
    p.abi_version, p.n_knots, p.method = _lib.NCDE_ABI_VERSION, n_knots, _lib.METHOD[method]
    f64 = np.asarray(t).dtype == np.float64
    td = np.ascontiguousarray(np.asarray(t, dtype=np.float64))
    kd = None if knots is None else np.ascontiguousarray(np.asarray(knots, dtype=np.float64))
    dp = ctypes.POINTER(ctypes.c_double)
    ts = _lib.NcdeTimeSpec(n_t=len(td), time_is_f64=int(f64), t=td.ctypes.data_as(dp), step_size=step,
                           knots=None if kd is None else kd.ctypes.data_as(dp))
    info = _lib.NcdeTimePlanInfo()
    lib = ncde_amd.lib()
    rc = lib.ncde_time_plan_build(ctypes.byref(p), ctypes.byref(ts), None, 0, ctypes.byref(info))
    if rc != 0:
        return rc, None, info
    buf = np.zeros(info.bytes // 4, dtype=np.int32)
    rc = lib.ncde_time_plan_build(ctypes.byref(p), ctypes.byref(ts), buf.ctypes.data, buf.nbytes, ctypes.byref(info))
    return rc, buf, info


def test_time_plan_builder_reproduces_torch_time_arithmetic():
    """ncde_time_plan_build (host C++) against the oracle's restatement in torch's own arithmetic -- the time grid of
    solvers.py:78-87, the stage times, the knot index / fraction of interpolation_linear.py:212-219, the output
    interpolation weights and the per-interval reverse grids of adjoint.py:116-133 -- bit for bit, on the time axes of the
    reference-generated goldens g11 (fp32 and fp64 times, user knot grids) and on the default axis."""
    import json
    import ncde_oracle as orc
    for name in ("g11_times_rk4_half", "g11_times_midpoint_third", "g11_knots_rk4", "g11_knots_cubic_euler",
                 "g11_knots_interval_rk4", "g11_times_f64_rk4", "g11_times_cubic_rk4_ragged"):
        f = np.load(os.path.join(gu.GOLD, name + ".npz"))
        m = json.loads(str(f["meta"]))
        kn = f["knots"] if "knots" in f.files else None
        ctl = orc.Control(f["coeffs"], m["kind"], t=kn)
        want, n_fwd, n_adj = orc.time_plan_words(ctl, torch.from_numpy(f["t_out"]), m["method"], m["step_size"])
        rc, got, info = _c_time_plan(ctl.n_knots, m["method"], f["t_out"], m["step_size"], kn)
        assert rc == 0 and np.array_equal(got, want), name
        assert (info.n_steps_fwd, info.n_steps_adj, info.n_t_out) == (n_fwd, n_adj, len(f["t_out"]))
        S = {"rk4": 4, "midpoint": 2, "euler": 1}[m["method"]]
        assert m["nfe"] == S * (n_fwd + n_adj)          # the reference's own nfe counter (base.py:90) on the same axis
    # the default axis (knots of a 7-knot path, step 1): the plan is what the specialised kernels hard-code
    ctl = orc.Control(np.zeros((1, 7, 2), np.float32), "linear")
    for t in (torch.arange(7.0), torch.tensor([0.0, 6.0])):
        want, n_fwd, n_adj = orc.time_plan_words(ctl, t, "rk4", 1.0)
        rc, got, info = _c_time_plan(7, "rk4", t.numpy(), 1.0)
        assert rc == 0 and np.array_equal(got, want) and n_fwd == n_adj == 6
        idx = got[8:8 + 6 * 15].reshape(6, 15)[:, 3::3]
        assert np.array_equal(idx, np.array([[max(n - 1, 0), n, n, n] for n in range(6)]))     # SURVEY.md §3.1 knot-index rule
    # errors: non-monotone t, non-positive step (misc.py:336-343 asserts; here NCDE_ERR_INVALID + message)
    rc, _, _ = _c_time_plan(7, "rk4", np.array([0.0, 2.0, 1.0], np.float32), 1.0)
    assert rc == -1 and b"increasing" in ncde_amd.lib().ncde_last_error_string()
    rc, _, _ = _c_time_plan(7, "rk4", np.array([0.0, 2.0], np.float32), 0.0)
    assert rc == -1 and b"step_size" in ncde_amd.lib().ncde_last_error_string()
    rc, _, _ = _c_time_plan(3, "rk4", np.array([0.0, 2.0], np.float32), 1.0, knots=[0.0, 1.0, 1.0])
    assert rc == -1 and b"knot" in ncde_amd.lib().ncde_last_error_string()


def test_general_time_axis_dispatches_to_the_plan_driven_families():
    lib = ncde_amd.lib()
    p = _problem()                       # cfg2 shape: specialised kernels on the default axis ...
    assert (lib.ncde_kernel_name(ctypes.byref(p), 0) or b"").startswith(b"ncde_fwd_fast")
    p.output, p.time_plan, p.n_t_out, p.n_steps_fwd, p.n_steps_adj = _lib.OUT_TIMES, 0x9000, 5, 12, 14
    n0, n1 = lib.ncde_kernel_name(ctypes.byref(p), 0), lib.ncde_kernel_name(ctypes.byref(p), 1)     # ... and (round 4) their plan-walking
    assert n0.startswith(b"ncde_fwd_fast_bf3<H32") and b"time plan" in n0, n0                        # instantiations otherwise;
    assert n1.startswith(b"ncde_adj_fast3") and b"time plan" in n1, n1
    assert lib.ncde_kernel_name(ctypes.byref(p), 2).startswith(b"ncde_adj_tiled")     # the exact discrete backward: batch-tiled family
    p.flags = _lib.FLAG_FORCE_TILED
    assert lib.ncde_kernel_name(ctypes.byref(p), 0).startswith(b"ncde_fwd_tiled")     # batch-tiled where every width is a multiple
    assert lib.ncde_kernel_name(ctypes.byref(p), 1).startswith(b"ncde_adj_tiled")     # of 16 (C of 4),
    p.flags = _lib.FLAG_FORCE_GENERIC
    assert lib.ncde_kernel_name(ctypes.byref(p), 0) == b"ncde_fwd_generic"            # generic for any shape
    assert lib.ncde_kernel_name(ctypes.byref(p), 1) == b"ncde_adj_generic"
    p.flags = 0
    assert lib.ncde_num_outputs(ctypes.byref(p)) == 5
    assert lib.ncde_stage_record_bytes(ctypes.byref(p)) == 4 * 12 * 4 * 32 * 32      # bytes: steps x stages x B x H
    p.flags = _lib.FLAG_FORCE_FAST
    assert lib.ncde_workspace_bytes(ctypes.byref(p), 0) >= 0
    p.flags, p.n_steps_fwd = 0, 0
    assert lib.ncde_num_outputs(ctypes.byref(p)) == -1


def test_time_mode_detection():
    X = ncde_amd.LinearInterpolation(torch.zeros(2, 5, 3))
    assert solver._time_mode(X, X.interval) == _lib.OUT_INTERVAL
    assert solver._time_mode(X, X.grid_points) == _lib.OUT_KNOTS
    assert solver._time_mode(X, torch.tensor([0.0, 4.0])) == _lib.OUT_INTERVAL
    assert solver._time_mode(X, torch.arange(5.0)) == _lib.OUT_KNOTS
    with pytest.raises(AssertionError):
        solver._time_mode(X, torch.tensor([0.0, 2.0, 1.0]))
    assert solver._time_mode(X, torch.tensor([0.0, 2.5])) is None        # -> general time axis (time plan)
    Xk = ncde_amd.LinearInterpolation(torch.zeros(2, 5, 3), t=torch.tensor([0.0, 1.0, 2.0, 3.0, 4.5]))
    assert solver._time_mode(Xk, torch.tensor([0.0, 4.0])) is None       # user knot grid: always the plan
    assert solver._time_mode(Xk, Xk.interval) is None                     # ... also for the control's own tagged tensors
    assert solver._time_mode(Xk, Xk.grid_points) is None


def test_host_coefficient_mirrors_match_reference_golden():
    """data.py's numpy builders against outputs of the reference's torchcde builders (golden g8)."""
    import golden_util as gu
    f = np.load(os.path.join(gu.GOLD, "g8_coeffs.npz"))
    assert gu.relerr(gu.data.linear_interpolation_coeffs(f["x_missing"]), f["linear"]) <= 1e-6
    assert np.array_equal(gu.data.linear_interpolation_coeffs(f["x_missing"], rectilinear=0), f["rectilinear"])
    assert np.array_equal(gu.data.natural_cubic_coeffs(f["x_clean"]), f["cubic"])
    assert np.array_equal(gu.data.natural_cubic_coeffs(f["x_clean"][:, :2]), f["cubic_len2"])
    assert np.array_equal(gu.data.natural_cubic_coeffs(f["x_missing"]), f["cubic_missing"])   # NaN = missing values


def test_gpu_coefficient_builders_refuse_cpu_tensors():
    with pytest.raises(NotImplementedError):
        ncde_amd.linear_interpolation_coeffs(torch.zeros(2, 5, 3))
    with pytest.raises(NotImplementedError):
        ncde_amd.natural_cubic_coeffs(torch.zeros(2, 5, 3))


def test_masked_temporal_loss_ignores_finished_series():
    """Per-time-step labels with NaN after a series has ended (the reference's masking rule, metrics.py:26-46): the
    sync-free weighted formulation equals the loss over the gathered valid positions, and masked positions get no gradient."""
    preds = (torch.arange(24, dtype=torch.float32).reshape(2, 4, 3) / 7 - 1).requires_grad_(True)
    labels = (torch.arange(24, dtype=torch.float32).reshape(2, 4, 3) % 2)
    labels[0, 2:] = float("nan")
    keep_p = torch.cat([preds[0, :2].reshape(-1), preds[1].reshape(-1)])
    keep_y = torch.cat([labels[0, :2].reshape(-1), labels[1].reshape(-1)])
    for kind, ref in (("mse", torch.nn.functional.mse_loss), ("l1", torch.nn.functional.l1_loss),
                      ("bce_logits", torch.nn.functional.binary_cross_entropy_with_logits)):
        loss = ncde_amd.MaskedTemporalLoss(kind)(preds, labels)
        assert torch.allclose(loss, ref(keep_p, keep_y)), kind
        g, = torch.autograd.grad(loss, preds)
        assert float(g[0, 2:].abs().sum()) == 0.0 and float(g[1].abs().sum()) > 0 and torch.isfinite(g).all()
    rm = ncde_amd.MaskedTemporalLoss("rmse", eps=0.0)(preds, labels)
    assert torch.allclose(rm, torch.nn.functional.mse_loss(keep_p, keep_y).sqrt())
    assert float(ncde_amd.masked_mean(preds, torch.full_like(labels, float("nan")))) == 0.0
    with pytest.raises(ValueError):
        ncde_amd.MaskedTemporalLoss("hinge")
    # a non-finite prediction at a masked position is discarded, as the reference's boolean gather does (0 * inf would poison the mean)
    bad = preds.detach().clone()
    bad[0, 3, 1] = float("inf")
    bad[0, 2, 0] = float("nan")
    assert torch.allclose(ncde_amd.masked_mean(bad, labels), torch.nn.functional.mse_loss(keep_p, keep_y))
    # the reference's class names (metrics.py:26-58): same values as its gather for the criteria it is used with, and for any other one
    for crit in (torch.nn.MSELoss(), torch.nn.L1Loss(), torch.nn.BCEWithLogitsLoss(), ncde_amd.RMSELoss(), torch.nn.SmoothL1Loss()):
        got = ncde_amd.TemporalLossWrapper(crit)(preds, labels)
        assert torch.allclose(got, crit(keep_p, keep_y)), type(crit).__name__


def test_time_plan_refuses_a_grid_it_cannot_index():
    """ncde_time_plan_build: a step so small that the step tables would not fit 32-bit word offsets is an error, not an overflow
    (ADVICE round 2)."""
    X = ncde_amd.LinearInterpolation(torch.zeros(2, 5, 3))
    with pytest.raises((ValueError, AssertionError, ncde_amd._lib.NcdeError), match="more than a time plan can hold"):
        solver._time_plan(X, torch.tensor([0.0, 4.0]), "rk4", 1e-9, "cpu")


def test_dispatch_table_matches_the_recorded_one():
    """tests/golden/dispatch_table.json: rows of tools/dispatch_table.py's grid (every distinct kernel name and error text it produces),
    recorded from the library as it was before the register-resident launchers and the ABI front end were rewritten around one plan /
    one route per call.  Kernel name, workspace bytes, status-word offset and the error text of each failing query: every field of
    every row."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("dispatch_table", os.path.join(ROOT, "tools", "dispatch_table.py"))
    dt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dt)
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "dispatch_table.json")))
    assert tuple(fx["keys"]) == dt.KEYS and len(fx["rows"]) > 1000
    h = dt.load(_lib.LIB_PATH)
    nk = len(fx["keys"])
    for row in fx["rows"]:
        case = dict(zip(fx["keys"], row[:nk]))
        assert dt.query(h, case) == row[nk:], case


def test_dopri5_dispatch_table_matches_the_recorded_one():
    """tests/golden/dispatch_table_dopri5.json: the whole dopri5 grid of tools/dispatch_table.py (--dopri5), recorded from the library as it
    was before the adaptive solver's host code was rebuilt on one segment list and one LDS rule.  ncde_dopri5_kernel_name and
    ncde_dopri5_workspace_bytes of the passes 0 / 1 / 2, ncde_dopri5_record_bytes over four option sets, and the error text of each failing
    query: every field of every row, and the grid is the one the tool walks today."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("dispatch_table", os.path.join(ROOT, "tools", "dispatch_table.py"))
    dt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dt)
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "dispatch_table_dopri5.json")))
    assert tuple(fx["keys"]) == dt.DP_KEYS and tuple(fx["fields"]) == dt.DP_FIELDS
    nk = len(fx["keys"])
    assert [row[:nk] for row in fx["rows"]] == [[c[k] for k in dt.DP_KEYS] for c in dt.dp_cases()]
    h = dt.dp_load(_lib.LIB_PATH)
    for row in fx["rows"]:
        case = dict(zip(fx["keys"], row[:nk]))
        assert dt.dp_query(h, case) == row[nk:], case


def _grad_slots(g, nl):
    """Every destination of an NcdeGrads as {name: address or None}."""
    d = {"z0": g.grad_z0}
    for i in range(nl):
        d["W%d" % i], d["b%d" % i] = g.grad_layer_W[i], g.grad_layer_b[i]
    d.update({k: getattr(g, "grad_" + k) for k in ("Wo", "bo", "Wg", "bg", "Wr", "br")})
    return d


def _cpu_spec(kind="original", H=4, C=3, HH=6):
    P = lambda *s: torch.nn.Parameter(torch.zeros(*s))      # noqa: E731
    W0, b0, W1, b1, Wo, bo = P(HH, H), P(HH), P(HH, HH), P(HH), P(H * C, HH), P(H * C)
    heads = {} if kind == "original" else {"Wg": P(H * C, HH), "bg": P(H * C)}
    if kind == "gru":
        heads.update(Wr=P(H, H), br=P(H))
    return ncde_amd.FieldSpec([(W0, b0), (W1, b1), (W1, b1)], Wo, bo, kind=kind, **heads)


def test_bind_grads_shares_one_buffer_per_unique_parameter():
    """nl = 3 with layers 1 and 2 sharing one (W1, b1): both layer indices are bound to ONE buffer, every bound address is the
    buffer bind_grads hands back for that parameter, and there are as many buffers as unique parameters."""
    spec = _cpu_spec()
    bound = solver.bind_grads(spec, (5, 4), "cpu")
    g = bound.g
    assert g.grad_layer_W[1] == g.grad_layer_W[2] and g.grad_layer_W[1] != g.grad_layer_W[0]
    assert g.grad_layer_b[1] == g.grad_layer_b[2] and g.grad_layer_b[1] != g.grad_layer_b[0]
    for i, (w, b) in enumerate(spec.layers):
        assert g.grad_layer_W[i] == bound.of(w).data_ptr() and g.grad_layer_b[i] == bound.of(b).data_ptr()
    assert g.grad_Wo == bound.of(spec.Wo).data_ptr() and g.grad_bo == bound.of(spec.bo).data_ptr()
    assert g.grad_z0 == bound.grad_z0.data_ptr() and bound.grad_z0.shape == (5, 4) and bound.grad_z0.dtype == torch.float32
    assert len(bound.bufs) == len(spec.unique_params()) == 6
    assert len({buf.data_ptr() for buf in bound.bufs.values()}) == 6
    assert all(g.grad_layer_W[i] is None and g.grad_layer_b[i] is None for i in range(3, _lib.NCDE_MAX_LAYERS))


@pytest.mark.parametrize("kind,heads", [("original", ()), ("minimal", ("Wg", "bg")), ("gru", ("Wg", "bg", "Wr", "br"))])
def test_bind_grads_binds_the_heads_of_the_field_kind(kind, heads):
    spec = _cpu_spec(kind)
    bound = solver.bind_grads(spec, (5, 4), "cpu")
    for k in ("Wg", "bg", "Wr", "br"):
        addr = getattr(bound.g, "grad_" + k)
        if k in heads:
            assert addr is not None and addr == bound.of(getattr(spec, k)).data_ptr(), k
        else:
            assert addr is None, k
    assert len(bound.bufs) == 6 + len(heads)


def test_bind_grads_restricted_live_set_leaves_the_rest_null():
    """live = {Wo, b0}: exactly those two destinations and grad_z0 are bound (the dopri5 adjoint's "not in the augmented state")."""
    spec = _cpu_spec("gru")
    b0 = spec.layers[0][1]
    bound = solver.bind_grads(spec, (5, 4), "cpu", live={id(spec.Wo), id(b0)})
    slots = _grad_slots(bound.g, _lib.NCDE_MAX_LAYERS)
    assert {k for k, v in slots.items() if v is not None} == {"z0", "Wo", "b0"}
    assert slots["Wo"] == bound.of(spec.Wo).data_ptr() and slots["b0"] == bound.of(b0).data_ptr()


def test_bind_grads_fill_and_non_contiguous_parameters():
    """fill = NaN reaches every element of every buffer; the buffer of a parameter that is a transposed view is contiguous and has
    the parameter's shape (the kernels write dense rows)."""
    spec = _cpu_spec("gru")
    spec.Wo = torch.nn.Parameter(torch.zeros(6, 12)).t()
    assert not spec.Wo.is_contiguous()
    bound = solver.bind_grads(spec, (5, 4), "cpu", fill=float("nan"))
    assert len(bound.bufs) == 10
    assert all(torch.isnan(buf).all() for buf in bound.bufs.values()) and torch.isnan(bound.grad_z0).all()
    assert bound.of(spec.Wo).is_contiguous() and bound.of(spec.Wo).shape == spec.Wo.shape == (12, 6)
    plain = solver.bind_grads(spec, (5, 4), "cpu")
    assert plain.of(spec.Wo).is_contiguous() and plain.of(spec.Wo).shape == (12, 6)
