"""Online inference on the GPU: ``NeuralCDE.online`` on its fused kernel (ncde_stream_step, csrc/ncde_stream.hip) against the reference's
batch ``NeuralCDE(return_sequences=True)`` at every knot (tests/golden/g19_*, tools/gen_golden_stream.py) and against this project's
own batch ``cdeint`` on the generic family, whose stage arithmetic the kernel keeps.

Bound: forward <= 2e-5 of max |ref| (tests/test_control_grad_gpu.py:21).  Launch-shape properties (several rows per call, streams
interleaved through `active`) are compared bit for bit."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import golden_util as gu
import stream_util as su

pytestmark = pytest.mark.gpu


def _fused_steps(handle, x, static):
    """step_through with every warning an error: the fused route emits none."""
    from ncde_amd import unfused
    unfused._WARNED.clear()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = su.step_through(handle, x, static, quiet=False)
    assert not unfused._WARNED, unfused._WARNED
    return res


@pytest.mark.parametrize("name", su.CASES)
def test_every_step_matches_the_reference_batch_solve(gpu_lib, name):
    f, m = su.load(name)
    model = su.model_of(f, m, "cuda")
    x, st = su.rows(f, "cuda")
    h = su.handle_of(model, m)
    assert gpu_lib.ncde_stream_kernel_name(ctypes.byref(h._problem())) == b"ncde_stream_step"
    assert gpu_lib.ncde_stream_workspace_bytes(ctypes.byref(h._problem())) == 0
    outs, zs, lasts = _fused_steps(h, x, st)
    q = su.knot_rows(m)
    ref_out, ref_z = np.swapaxes(f["out"], 0, 1), np.swapaxes(f["hidden"][:, ::q], 0, 1)
    for k in range(x.size(0)):
        e_out, e_z = gu.relerr(outs[k], ref_out[k]), gu.relerr(zs[k], ref_z[k])
        print("%s step %d: out %.3e z %.3e" % (name, k, e_out, e_z))
        assert e_out <= su.TIGHT_Z and e_z <= su.TIGHT_Z, (k, e_out, e_z)
    assert np.array_equal(lasts, np.swapaxes(f["coeffs"][:, ::q], 0, 1))      # the fill copies: bit for bit
    assert h.count.cpu().tolist() == [x.size(0)] * m["dims"]["B"]
    # m = L - 1 rows in one call: bit-identical to L - 1 single calls
    if x.size(0) > 2:
        h2 = su.handle_of(model, m)
        first = h2.step(x[0], static=st)
        many = h2.step(x[1:])
        assert np.array_equal(first.cpu().numpy(), outs[0]) and np.array_equal(many.cpu().numpy(), outs[1:])
        assert np.array_equal(h2.z.cpu().numpy(), zs[-1])


@pytest.mark.parametrize("name", ["g19_a_rect", "g19_b_linear_ffill"])
def test_interleaved_halves_equal_each_half_alone(gpu_lib, name):
    f, m = su.load(name)
    model = su.model_of(f, m, "cuda")
    x, st = su.rows(f, "cuda")
    L, B = x.size(0), x.size(1)
    half = torch.arange(B, device="cuda") % 3 != 0
    alone = {}
    for tag, sel in (("a", half), ("b", ~half)):
        ha = su.handle_of(model, m, batch=int(sel.sum()))
        alone[tag] = _fused_steps(ha, x[:, sel].contiguous(), st)
    h = su.handle_of(model, m)
    for k in range(L):
        for tag, act in (("a", half), ("b", ~half)):
            before = h.state_dict()
            out = h.step(x[k], static=st, active=act)
            after = h.state_dict()
            for key in before:      # a stream without a row: state untouched
                assert torch.equal(before[key][~act], after[key][~act]), (k, key)
            assert np.array_equal(out[act].cpu().numpy(), alone[tag][0][k])
            assert np.array_equal(h.z[act].cpu().numpy(), alone[tag][1][k])
            if k > 0:               # ... and its output is the readout of its unchanged z: what it answered one call ago
                assert torch.equal(out[~act], prev[~act])
            prev = out
    assert h.count.cpu().tolist() == [L] * B


def _batch_hidden(model, x, static=None):
    """This project's batch solve of the same model (built with return_sequences=True, apply_final_linear=False) on the generic
    family: the hidden state at every observation, [L, B, H]."""
    import ncde_amd
    assert model.return_sequences and not model.apply_final_linear
    rect = model.interpolation == "rectilinear"
    coeffs = ncde_amd.linear_interpolation_coeffs(x.transpose(0, 1).contiguous(), rectilinear=0 if rect else None, initial_value_if_nan=0.0,
                                                  forward_fill=not rect)
    with torch.no_grad():
        return model(coeffs if static is None else (static, coeffs)).transpose(0, 1).contiguous()


@pytest.mark.parametrize("method", ["euler", "midpoint"])
@pytest.mark.parametrize("path", ["linear", "rectilinear"])
def test_euler_and_midpoint_through_the_abi(gpu_lib, method, path):
    """ncde_stream_step called directly, the first row included (count == 0: the row is filled and kept, z stays as set)."""
    import ncde_amd
    from ncde_amd import _lib
    torch.manual_seed(11)
    B, L, C, H = 19, 4, 5, 12
    model = ncde_amd.NeuralCDE(C, H, 3, hidden_hidden_dim=10, num_layers=2, interpolation=path, solver=method, return_sequences=True,
                               apply_final_linear=False, kernel_flags=_lib.FLAG_FORCE_GENERIC).cuda()
    x = torch.cumsum(torch.rand(L, B, C, device="cuda") + 0.25, dim=0)
    x[1:, :, 1:][torch.rand(L - 1, B, C - 1, device="cuda") < 0.3] = float("nan")
    ref = _batch_hidden(model, x)
    p = model.online(B)._problem()
    assert p.method == _lib.METHOD[method]
    z = ref[0].clone()
    last, pdx = torch.full((B, C), 7.0, device="cuda"), torch.full((B, C), 7.0, device="cuda")
    count = torch.zeros(B, dtype=torch.int32, device="cuda")
    z_out = torch.empty(L, B, H, device="cuda")
    s = _lib.NcdeStream()
    s.n_rows, s.rectilinear, s.time_index = L, int(path == "rectilinear"), 0
    s.x, s.x_stride_m, s.x_stride_b = x.data_ptr(), x.stride(0), x.stride(1)
    s.z, s.last_row, s.prev_dx, s.count, s.z_out = z.data_ptr(), last.data_ptr(), pdx.data_ptr(), count.data_ptr(), z_out.data_ptr()
    _lib.check(gpu_lib.ncde_stream_step(ctypes.byref(p), ctypes.byref(s), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "ncde_stream_step")
    torch.cuda.synchronize()
    err = gu.relerr(z_out.cpu().numpy(), ref.cpu().numpy())
    print("%s %s: z %.3e" % (method, path, err))
    assert err <= su.TIGHT_Z, err
    assert torch.equal(z_out[-1], z) and count.cpu().tolist() == [L] * B
    assert (ref[-1] - ref[0]).abs().max() > 1e-3


def test_odd_shape_against_the_generic_batch_solve(gpu_lib):
    """(C 7, H 20, HH 24, nl 2, B 17): every dimension padded, two tiles with a one-stream tail.  The kernel keeps the operation
    order of ncde_fwd_generic, so the bound of 2e-5 is expected to be met with 0 (DESIGN.md 5.14 records what was seen)."""
    import ncde_amd
    from ncde_amd import _lib
    torch.manual_seed(7)
    B, L, C, H = 17, 5, 7, 20
    worst = 0.0
    for path in ("rectilinear", "linear"):
        model = ncde_amd.NeuralCDE(C, H, 2, hidden_hidden_dim=24, num_layers=2, interpolation=path, return_sequences=True,
                                   apply_final_linear=False, kernel_flags=_lib.FLAG_FORCE_GENERIC).cuda()
        x = torch.cumsum(torch.rand(L, B, C, device="cuda") + 0.25, dim=0)
        x[1:, :, 1:][torch.rand(L - 1, B, C - 1, device="cuda") < 0.3] = float("nan")
        ref = _batch_hidden(model, x)
        outs, zs, _ = _fused_steps(model.online(B), x, None)
        assert np.array_equal(outs, zs)      # apply_final_linear=False: the step returns the hidden state
        err = gu.relerr(zs, ref.cpu().numpy())
        print("odd shape %s: max |z - batch| / max |batch| = %.3e" % (path, err))
        assert (ref[-1] - ref[0]).abs().max() > 1e-3
        worst = max(worst, err)
    assert worst <= su.TIGHT_Z, worst


def test_gated_field_takes_the_torch_step_and_warns(gpu_lib):
    import ncde_amd
    from ncde_amd import unfused
    torch.manual_seed(3)
    B, L, C, H = 6, 5, 4, 8
    model = ncde_amd.NeuralCDE(C, H, 2, hidden_hidden_dim=8, num_layers=2, interpolation="rectilinear", vector_field="gru",
                               return_sequences=True).cuda()
    x = torch.cumsum(torch.rand(L, B, C, device="cuda") + 0.25, dim=0)
    x[2, :, 2] = float("nan")
    coeffs = ncde_amd.linear_interpolation_coeffs(x.transpose(0, 1).contiguous(), rectilinear=0, initial_value_if_nan=0.0)
    with torch.no_grad():
        ref = model(coeffs).transpose(0, 1)
    unfused._WARNED.clear()
    h = model.online(B)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        outs = torch.stack([h.step(x[k]) for k in range(L)])
    assert sum("unfused" in str(w.message) and "online step" in str(w.message) for w in rec) == 1, [str(w.message) for w in rec]
    err = gu.relerr(outs.cpu().numpy(), ref.cpu().numpy())
    print("gru online vs its batch forward: %.3e" % err)
    assert err <= su.TIGHT_Z, err
