"""Online inference on the Hermite cubic with backward differences on the GPU: ``NeuralCDE(interpolation="cubic_hermite").online`` on
its fused kernel (ncde_stream_step_hermite, csrc/ncde_stream.hip) against (i) the same model's fp64 batch solve on the CPU on
tests/hermite_ref.py coefficients and (ii) this project's fp32 batch solve on the generic family on the GPU builder's output.

Bound: forward <= 2e-5 of max |ref| (stream_util.TIGHT_Z, the project's forward bound) for both.  Launch-shape properties (several
rows per call, streams interleaved through `active`, a state_dict round trip) are compared bit for bit.  All shapes are small."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import hermite_util as hu
import stream_edges as se
import stream_util as su

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _coeffs(x, init):
    import ncde_amd
    return ncde_amd.hermite_cubic_coefficients_with_backward_differences(x.transpose(0, 1).contiguous(), initial_value_if_nan=init, forward_fill=True)


def _batch(model, x, init, static=None):
    """This project's batch solve (the model is built with return_sequences=True and FLAG_FORCE_GENERIC) -> [L, B, ...]."""
    assert model.return_sequences
    c = _coeffs(x, init)
    with torch.no_grad():
        return model(c if static is None else (static, c)).transpose(0, 1).contiguous()


def test_every_step_against_both_references(gpu_lib):
    from ncde_amd import _lib
    s = hu.MAIN
    z_ref, o_ref = hu.main_reference()
    x = se.dev(hu.main_rows().copy(), "cuda")
    model = hu.main_model("cubic_hermite", "cuda", kernel_flags=_lib.FLAG_FORCE_GENERIC)
    zmodel = hu.main_model("cubic_hermite", "cuda", kernel_flags=_lib.FLAG_FORCE_GENERIC, apply_final_linear=False)
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in zmodel.state_dict().items())
    o_gen, z_gen = _batch(model, x, s["init"]).cpu().numpy(), _batch(zmodel, x, s["init"]).cpu().numpy()
    h = model.online(s["B"], initial_value_if_nan=s["init"])
    assert gpu_lib.ncde_stream_hermite_kernel_name(ctypes.byref(h._problem())) == b"ncde_stream_step_hermite"
    assert gpu_lib.ncde_stream_hermite_workspace_bytes(ctypes.byref(h._problem())) == 0
    with se.stepping("cuda"):
        outs, zs, lasts = su.step_through(h, x, None, quiet=False)
        _, zl, _ = su.step_through(hu.main_model("linear", "cuda").online(s["B"], initial_value_if_nan=s["init"]), x, None, quiet=False)
    for k in range(s["L"]):
        e64 = max(se.err(outs[k], o_ref[k]), se.err(zs[k], z_ref[k]))
        e32 = max(se.err(outs[k], o_gen[k]), se.err(zs[k], z_gen[k]))
        print("step %d: vs the fp64 batch solve %.3e, vs the fp32 generic batch solve %.3e" % (k, e64, e32))
        assert e64 <= su.TIGHT_Z and e32 <= su.TIGHT_Z, (k, e64, e32)
    assert np.abs(z_ref[-1] - z_ref[0]).max() > 1e-3
    e_lin = se.err(zl, z_ref)
    print("the same rows through a linear handle: %.3e of max |ref|" % e_lin)
    assert e_lin > 10 * su.TIGHT_Z, e_lin      # the case tells the cubic from the broken line
    assert lasts[0, 2, 3] == s["init"] and lasts[0, 17, 1] == s["init"] and h.count.cpu().tolist() == [s["L"]] * s["B"]
    # prev_dx is the backward difference of the last piece
    assert np.array_equal(h.prev_dx.cpu().numpy(), lasts[-1] - lasts[-2])


@pytest.mark.parametrize("method", ["euler", "midpoint"])
def test_euler_and_midpoint_through_the_abi(gpu_lib, method):
    """ncde_stream_step_hermite called directly, the first row included (count == 0: the row is filled and kept, z stays as set)."""
    import ncde_amd
    from ncde_amd import _lib
    B, L, C, H, init = 17, 4, 7, 20, -0.5
    rows = se.make_rows(6301, L, B, C)
    rows[0, 3, 2] = NAN
    x = se.dev(rows, "cuda")
    model = se.make_model(63, C, H, 3, 24, 2, "cubic_hermite", "cuda", solver=method, apply_final_linear=False, kernel_flags=_lib.FLAG_FORCE_GENERIC)
    ref32 = _batch(model, x, init)
    ref64, _ = hu.batch_reference(model, rows, None, init)
    p = model.online(B, initial_value_if_nan=init)._problem()
    assert p.method == _lib.METHOD[method] and p.interp == _lib.INTERP["cubic"]
    z = ref32[0].clone()
    last, pdx = torch.full((B, C), 7.0, device="cuda"), torch.full((B, C), 7.0, device="cuda")
    count = torch.zeros(B, dtype=torch.int32, device="cuda")
    z_out = torch.empty(L, B, H, device="cuda")
    s = _lib.NcdeStream()
    s.n_rows, s.rectilinear, s.time_index, s.initial_value_if_nan = L, 0, 0, init
    s.x, s.x_stride_m, s.x_stride_b = x.data_ptr(), x.stride(0), x.stride(1)
    s.z, s.last_row, s.prev_dx, s.count, s.z_out = z.data_ptr(), last.data_ptr(), pdx.data_ptr(), count.data_ptr(), z_out.data_ptr()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(gpu_lib.ncde_stream_step_hermite(ctypes.byref(p), ctypes.byref(s), stream), "ncde_stream_step_hermite")
    torch.cuda.synchronize()
    e32, e64 = se.err(z_out, ref32.cpu().numpy()), se.err(z_out, ref64)
    print("%s: z vs the fp32 generic batch solve %.3e, vs the fp64 batch solve %.3e" % (method, e32, e64))
    assert e32 <= su.TIGHT_Z and e64 <= su.TIGHT_Z, (e32, e64)
    knots = ncde_amd.linear_interpolation_coeffs(x.transpose(0, 1).contiguous(), initial_value_if_nan=init, forward_fill=True)
    assert torch.equal(z_out[-1], z) and count.cpu().tolist() == [L] * B
    assert torch.equal(last, knots[:, -1]) and torch.equal(pdx, knots[:, -1] - knots[:, -2])      # the state the next call reads
    assert np.abs(ref64[-1] - ref64[0]).max() > 1e-3
    # what the entry refuses: a rectilinear stream, a problem that does not say cubic; the linear entry keeps refusing a cubic problem
    s.rectilinear = 1
    assert gpu_lib.ncde_stream_step_hermite(ctypes.byref(p), ctypes.byref(s), stream) == -1
    s.rectilinear = 0
    p.interp = _lib.INTERP["linear"]
    assert gpu_lib.ncde_stream_step_hermite(ctypes.byref(p), ctypes.byref(s), stream) == -1
    assert gpu_lib.ncde_stream_hermite_kernel_name(ctypes.byref(p)) is None and gpu_lib.ncde_stream_kernel_name(ctypes.byref(p)) == b"ncde_stream_step"
    p.interp = _lib.INTERP["cubic"]
    assert gpu_lib.ncde_stream_workspace_bytes(ctypes.byref(p)) == -1 and gpu_lib.ncde_stream_kernel_name(ctypes.byref(p)) is None
    assert count.cpu().tolist() == [L] * B      # nothing refused advanced a stream


def _main_handle(model, batch=None):
    return model.online(batch or hu.MAIN["B"], initial_value_if_nan=hu.MAIN["init"])


def test_rows_in_one_call_and_state_dict_round_trip(gpu_lib):
    s = hu.MAIN
    model = hu.main_model("cubic_hermite", "cuda")
    x = se.dev(hu.main_rows().copy(), "cuda")
    with se.stepping("cuda"):
        outs, zs, _ = su.step_through(_main_handle(model), x, None, quiet=False)
        h = _main_handle(model)
        first = h.step(x[0])
        assert h._may_init is False
        many = h.step(x[1:])      # ONE launch with m = L - 1 rows
        assert np.array_equal(first.cpu().numpy(), outs[0]) and np.array_equal(many.cpu().numpy(), outs[1:])
        assert np.array_equal(h.z.cpu().numpy(), zs[-1])
        # a state_dict taken in mid-stream, loaded into a new handle: bit-equal to not interrupting
        ha, hb = _main_handle(model), _main_handle(model)
        ha.step(x[:3])
        saved = ha.state_dict()
        assert sorted(saved) == ["count", "last_row", "prev_dx", "z"] and saved["count"].tolist() == [3] * s["B"]
        hb.load_state_dict(saved)
        tail_a, tail_b = ha.step(x[3:]), hb.step(x[3:])
        assert torch.equal(tail_a, tail_b) and np.array_equal(tail_a.cpu().numpy(), outs[3:])
        for k in saved:
            assert torch.equal(ha.state_dict()[k], hb.state_dict()[k]), k


def test_interleaved_halves_equal_each_half_alone(gpu_lib):
    s = hu.MAIN
    model = hu.main_model("cubic_hermite", "cuda")
    x = se.dev(hu.main_rows().copy(), "cuda")
    half = torch.arange(s["B"], device="cuda") % 3 != 0
    with se.stepping("cuda"):
        alone = {tag: su.step_through(_main_handle(model, int(sel.sum())), x[:, sel].contiguous(), None, quiet=False) for tag, sel in (("a", half), ("b", ~half))}
        h = _main_handle(model)
        for k in range(s["L"]):
            for tag, act in (("a", half), ("b", ~half)):
                before = h.state_dict()
                out = h.step(x[k], active=act)
                after = h.state_dict()
                for key in before:      # a stream without a row: state untouched
                    assert torch.equal(before[key][~act], after[key][~act]), (k, key)
                assert np.array_equal(out[act].cpu().numpy(), alone[tag][0][k])
                assert np.array_equal(h.z[act].cpu().numpy(), alone[tag][1][k])
                if k > 0:               # ... and its output is the readout of its unchanged z: what it answered one call ago
                    assert torch.equal(out[~act], prev[~act])
                prev = out
        assert h.count.cpu().tolist() == [s["L"]] * s["B"]


def test_one_tile_holds_first_steps_and_later_steps(gpu_lib):
    """The staggered schedule of tests/stream_edges.py: at call 3 the first tile steps streams with 0, 1 and >= 2 rows behind them next
    to streams that receive nothing -- b is the stream's own difference at its first step and the previous one later, per stream.
    Every stream answers, bit for bit, what it answers alone in a handle of its own, and meets the fp64 batch solve of its own rows."""
    x_np, A = se.staggered_rows()
    se.assert_schedule(A)
    st = se.STAG
    model = se.make_model(41, st["C"], st["H"], st["n_out"], st["HH"], st["nl"], "cubic_hermite", "cuda")
    x, act = se.dev(x_np, "cuda"), se.dev(A, "cuda")
    final = {}
    with se.stepping("cuda"):
        h = model.online(st["B"], initial_value_if_nan=st["init"])
        alone = [model.online(1, initial_value_if_nan=st["init"]) for _ in range(st["B"])]
        for j in range(st["calls"]):
            before = h.state_dict()
            out = h.step(x[j], active=act[j])
            after = h.state_dict()
            for key in before:
                assert torch.equal(before[key][~act[j]], after[key][~act[j]]), (j, key)
            for b in np.nonzero(A[j])[0]:
                ob = alone[b].step(x[j, b:b + 1])
                assert torch.equal(ob[0], out[b]) and torch.equal(alone[b].z[0], h.z[b]), (j, b)
                assert torch.equal(alone[b].last_row[0], h.last_row[b]) and torch.equal(alone[b].prev_dx[0], h.prev_dx[b]), (j, b)
        assert h.count.cpu().tolist() == A.sum(axis=0).tolist()
        final = h.z.cpu().numpy()
    worst = 0.0
    for b in (0, 1, 4, 5):      # every row; joins at call 3 with NaNs in its first row; pauses; has one row behind it at call 3
        rows = np.ascontiguousarray(x_np[A[:, b], b][:, None])
        z_ref, _ = hu.batch_reference(model, rows, None, st["init"])
        worst = max(worst, se.err(final[b], z_ref[-1, 0]))
    print("staggered streams against the fp64 batch solve of their own rows: %.3e" % worst)
    assert worst <= su.TIGHT_Z, worst


@pytest.mark.parametrize("final", [True, False], ids=["final_linear", "hidden"])
def test_readout_and_start_with_static_features(gpu_lib, final):
    B, L, C, H, sd, init = 17, 4, 5, 12, 3, 0.5
    rows = se.make_rows(6401, L, B, C)
    rows[0, 1, 2] = NAN
    static_np = np.random.default_rng(64).standard_normal((B, sd)).astype(np.float32)
    model = se.make_model(65, C, H, 2, 10, 2, "cubic_hermite", "cuda", static_dim=sd, use_initial=True, apply_final_linear=final)
    z_ref, o_ref = hu.batch_reference(model, rows, static_np, init)
    x, static = se.dev(rows, "cuda"), se.dev(static_np, "cuda")
    with se.stepping("cuda"):
        outs, zs, _ = su.step_through(model.online(B, initial_value_if_nan=init), x, static, quiet=False)
    e_out, e_z = se.err(outs, o_ref), se.err(zs, z_ref)
    print("static_dim %d, apply_final_linear %s: out %.3e z %.3e" % (sd, final, e_out, e_z))
    assert e_out <= su.TIGHT_Z and e_z <= su.TIGHT_Z, (e_out, e_z)
    assert outs.shape == (L, B, 2 if final else H) and (final or np.array_equal(outs, zs))
    assert np.abs(z_ref[0]).max() > 1e-3 and np.abs(z_ref[-1] - z_ref[0]).max() > 1e-3


def _one_warning(model, x, init):
    from ncde_amd import unfused
    unfused._WARNED.clear()
    h = model.online(x.size(1), initial_value_if_nan=init)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        outs = torch.stack([h.step(x[k]) for k in range(x.size(0))])
    assert sum("unfused" in str(w.message) and "online step" in str(w.message) for w in rec) == 1, [str(w.message) for w in rec]
    return outs, h


def test_gated_field_takes_the_torch_step_behind_one_warning(gpu_lib):
    B, L, C, init = 6, 5, 4, 0.5
    rows = se.make_rows(6501, L, B, C)
    model = se.make_model(66, C, 8, 2, 8, 2, "cubic_hermite", "cuda", vector_field="gru")
    _, o_ref = hu.batch_reference(model, rows, None, init)
    outs, _ = _one_warning(model, se.dev(rows, "cuda"), init)
    e = se.err(outs, o_ref)
    print("gru on cubic_hermite, torch-op step vs the fp64 batch solve: %.3e" % e)
    assert e <= su.TIGHT_Z, e


def test_the_first_shape_the_lds_query_refuses_takes_the_torch_step(gpu_lib):
    """The LDS plan is the linear step's: H352 is the last shape it holds, H368 the first it does not (tests/stream_edges.py)."""
    held = se.wide_model("H352", "cubic_hermite", "cuda").online(se.WIDE["H352"][4])
    assert gpu_lib.ncde_stream_hermite_kernel_name(ctypes.byref(held._problem())) == b"ncde_stream_step_hermite"
    C, H, HH, nl, B, n = se.WIDE["H368"]
    model = se.wide_model("H368", "cubic_hermite", "cuda")
    assert gpu_lib.ncde_stream_hermite_workspace_bytes(ctypes.byref(model.online(B)._problem())) == -2
    assert gpu_lib.ncde_stream_hermite_kernel_name(ctypes.byref(model.online(B)._problem())) is None
    rows = se.wide_rows("H368")
    z_ref, _ = hu.batch_reference(model, rows, None, 0.0)
    outs, h = _one_warning(model, se.dev(rows, "cuda"), 0.0)
    e = se.err(outs, z_ref)
    print("H368 on cubic_hermite, torch-op step vs the fp64 batch solve: %.3e" % e)
    assert e <= su.TIGHT_Z and h.count.cpu().tolist() == [n] * B, e
