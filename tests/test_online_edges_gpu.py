"""The fused online step (ncde_stream_step, csrc/ncde_stream.hip) at its edges: streams that start, pause and restart at different
times, a per-row mask in one launch, reset(mask), the time channel, strided and expanded rows, un-shared / tied / uneven layer
stacks, LDS above 64 KiB and the shape the kernel refuses, tiny and odd dimensions, the readout through the ABI, missing data and
64 rows in one launch.

References: tests/stream_ref.py (the batch model in fp64 on the rows each stream received; validated on the reference project's
goldens by tests/test_online_edges_cpu.py) within the project's forward bound 2e-5 of max |ref| (su.TIGHT_Z), the oracle in fp64 for
the layer stacks, and -- bit for bit -- this project's batch solve on ncde_fwd_generic (FLAG_FORCE_GENERIC), whose stage arithmetic
the kernel keeps, rows per call, and streams run alone.  The cases shared with the CPU twin live in tests/stream_edges.py."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import golden_util as gu
import stream_edges as se
import stream_util as su

pytestmark = pytest.mark.gpu
PATHS = pytest.mark.parametrize("path", ["rectilinear", "linear"])
F32 = torch.float32
INVALID, UNSUPPORTED = -1, -2      # NcdeStatus (include/ncde_hip.h)


# ---- helpers -------------------------------------------------------------------------------------------------------------------------
def _state(B, C, H, z=None, fill=7.0):
    """(z, last_row, prev_dx, count) of B streams that have received nothing: z as given, the rows filled with a value that must
    never be read."""
    z = torch.zeros(B, H, device="cuda") if z is None else z.clone()
    return [z, torch.full((B, C), fill, device="cuda"), torch.full((B, C), fill, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")]


def _stream(x, state, rect, time_index=0, init=0.0, active=None, Wf=None, bf=None, out=None, z_out=None):
    from ncde_amd import _lib
    s = _lib.NcdeStream()
    s.n_rows, s.rectilinear, s.time_index = x.size(0), int(rect), time_index
    s.x, s.x_stride_m, s.x_stride_b = x.data_ptr(), x.stride(0), x.stride(1)
    s.active = None if active is None else active.data_ptr()
    s.initial_value_if_nan = init
    s.z, s.last_row, s.prev_dx, s.count = (t.data_ptr() for t in state)
    if Wf is not None:
        s.Wf, s.n_out = Wf.data_ptr(), Wf.size(0)
    s.bf = None if bf is None else bf.data_ptr()
    s.out = None if out is None else out.data_ptr()
    s.z_out = None if z_out is None else z_out.data_ptr()
    return s


def _launch(lib, p, s):
    rc = lib.ncde_stream_step(ctypes.byref(p), ctypes.byref(s), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def _ok(lib, p, s):
    from ncde_amd import _lib
    _lib.check(_launch(lib, p, s), "ncde_stream_step")


def _batch_hidden(model, x, init=0.0, time_index=0):
    """This project's batch solve of the same model (return_sequences=True, apply_final_linear=False, FLAG_FORCE_GENERIC) on the
    coefficients built from the same rows: the hidden state at every observation, [L, B, H]."""
    import ncde_amd
    from ncde_amd import _lib
    assert model.return_sequences and not model.apply_final_linear and model.kernel_flags == _lib.FLAG_FORCE_GENERIC
    rect = model.interpolation == "rectilinear"
    coeffs = ncde_amd.linear_interpolation_coeffs(x.transpose(0, 1).contiguous(), rectilinear=time_index if rect else None,
                                                  initial_value_if_nan=init, forward_fill=not rect)
    with torch.no_grad():
        return model(coeffs).transpose(0, 1).contiguous()


def _through_the_handle(model, x, **kw):
    """One call per row, no warning allowed -> z [L, B, H] as numpy."""
    with se.stepping("cuda"):
        return su.step_through(model.online(x.size(1), **kw), x, None, quiet=False)[1]


def _lds_bytes(C, H, widths):
    r16, r4 = (lambda n: (n + 15) // 16 * 16), (lambda n: (n + 3) // 4 * 4)
    return 4 * (5 * r16(H) * 16 + 2 * max(r16(w) for w in [H] + list(widths)) * 16 + 5 * r4(C) * 16 + 48)


# ---- the cases shared with the CPU twin --------------------------------------------------------------------------------------------
@PATHS
def test_staggered_streams(gpu_lib, path):
    """(a) B = 19: streams that receive every row, join late, receive one row only, never receive anything and pause, in one
    tile at one call; against the fp64 prefix reference, state of non-receivers untouched, every stream as if alone."""
    print("staggered %s: worst %.3e" % (path, se.check_staggered("cuda", F32, path)))


@PATHS
def test_per_row_mask_in_one_launch(gpu_lib, path):
    """(b) active [m, B] read per row inside one launch."""
    print("row mask %s: worst %.3e" % (path, se.check_row_mask("cuda", F32, path)))


@PATHS
def test_reset_mask_and_state_dict_on_the_device(gpu_lib, path):
    """(c)"""
    print("reset %s: worst %.3e" % (path, se.check_reset("cuda", F32, path)))


def test_time_index_last_channel(gpu_lib):
    """(d) (time in channel 2: the golden g19_e_rect_time2 through tests/test_online_gpu.py)"""
    print("time index: worst %.3e" % se.check_time_index("cuda", F32))


@PATHS
def test_strided_and_expanded_rows(gpu_lib, path):
    """(e) Found: x.expand()ed over the batch (stride 0) reached the ABI, which refuses rows closer than C floats; the handle now
    copies such an input."""
    se.check_strides("cuda", F32, path)


@PATHS
def test_missing_data(gpu_lib, path):
    """(j)"""
    print("missing %s: worst %.3e" % (path, se.check_missing("cuda", F32, path)))


# ---- (b) first rows in the middle of a launch, through the ABI -----------------------------------------------------------------------
@PATHS
def test_first_rows_arrive_mid_launch_through_the_abi(gpu_lib, path):
    """rk4, six rows and the whole staggered schedule in ONE launch, z preset to each stream's h0: a stream's first row comes at row
    0, 1, 2, 3 or 4 of the launch (or never), is filled and kept and takes no step.  Bit-identical to the handle's masked single
    calls, within the bound of the fp64 reference."""
    s_ = se.STAG
    x_np, A = se.staggered_rows()
    model = se.staggered_model(path, "cuda", F32)
    x, act = se.dev(x_np, "cuda"), se.dev(A, "cuda")
    with torch.no_grad():      # h0 of every stream from ITS first row, as the handle builds it
        filled = torch.where(torch.isnan(x), torch.full_like(x, s_["init"]), x)
        h0 = torch.stack([model.initial_linear(filled[j]) for j in range(s_["calls"])])
    z0 = torch.zeros(s_["B"], s_["H"], device="cuda")
    for b in range(s_["B"]):
        if A[:, b].any():
            z0[b] = h0[int(np.argmax(A[:, b])), b]
    state = _state(s_["B"], s_["C"], s_["H"], z0)
    out, z_out = torch.empty(s_["calls"], s_["B"], s_["n_out"], device="cuda"), torch.empty(s_["calls"], s_["B"], s_["H"], device="cuda")
    a8 = act.to(torch.uint8).contiguous()
    p = model.online(s_["B"])._problem()
    fl = model.final_linear
    _ok(gpu_lib, p, _stream(x, state, path == "rectilinear", 0, s_["init"], a8, fl.weight, fl.bias, out, z_out))
    with se.stepping("cuda"):
        h = model.online(s_["B"], initial_value_if_nan=s_["init"])
        outs, zs = [], []
        for j in range(s_["calls"]):
            outs.append(h.step(x[j], active=act[j]))
            zs.append(h.z.clone())
    seen = se.dev(np.cumsum(A, axis=0) > 0, "cuda")      # (before its first row a stream answers from the preset z here, from 0 in the handle)
    assert torch.equal(out[seen], torch.stack(outs)[seen]) and torch.equal(z_out[seen], torch.stack(zs)[seen])
    assert torch.equal(z_out[~seen], z0.expand_as(z_out)[~seen])
    got = se.dev(A.any(axis=0), "cuda")
    assert torch.equal(state[0], h.z) and torch.equal(state[3], h.count)
    stepped = se.dev(A.sum(axis=0) > 1, "cuda")
    assert torch.equal(state[1][got], h.last_row[got]) and torch.equal(state[2][stepped], h.prev_dx[stepped])
    assert bool((state[1][~got] == 7.0).all()) and bool((state[2][~stepped] == 7.0).all())      # never received / never stepped: never computed
    z_ref, o_ref = se.staggered_reference(path)
    e_out, e_z = se.err(out[seen], o_ref[seen.cpu().numpy()]), se.err(z_out[seen], z_ref[seen.cpu().numpy()])
    print("mid-launch first rows %s: out %.3e z %.3e" % (path, e_out, e_z))
    assert e_out <= su.TIGHT_Z and e_z <= su.TIGHT_Z, (e_out, e_z)


# ---- (e) what the ABI refuses --------------------------------------------------------------------------------------------------------
def test_invalid_arguments_leave_the_state_alone(gpu_lib):
    B, C, H = 19, 5, 12
    model = se.make_model(61, C, H, 3, 10, 2, "rectilinear", "cuda")
    p = model.online(B)._problem()
    x = se.dev(se.make_rows(6101, 2, B, C, missing=0.0), "cuda")
    state = _state(B, C, H, torch.randn(B, H, device="cuda"), fill=0.5)
    state[3].fill_(2)
    before = [t.clone() for t in state]
    z_out, out = torch.empty(2, B, H, device="cuda"), torch.empty(2, B, 3, device="cuda")
    fl = model.final_linear

    def edit(**kw):
        s = _stream(x, state, True, z_out=z_out)
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    bad = {"x_stride_b < C": edit(x_stride_b=C - 1), "x_stride_b 0": edit(x_stride_b=0), "n_rows 0": edit(n_rows=0),
           "time_index C": edit(time_index=C), "time_index -1": edit(time_index=-1),
           "NULL z": edit(z=None), "NULL last_row": edit(last_row=None), "NULL prev_dx": edit(prev_dx=None), "NULL count": edit(count=None),
           "NULL x": edit(x=None), "Wf without out": _stream(x, state, True, Wf=fl.weight, bf=fl.bias, z_out=z_out),
           "neither Wf nor z_out": _stream(x, state, True)}
    for name, s in bad.items():
        assert _launch(gpu_lib, p, s) == INVALID, name
        assert gpu_lib.ncde_last_error_string(), name
        for t, t0 in zip(state, before):
            assert torch.equal(t, t0), name
    _ok(gpu_lib, p, _stream(x, state, True, Wf=fl.weight, bf=fl.bias, out=out))      # ... and the same structure, completed, runs
    assert state[3].cpu().tolist() == [4] * B and not torch.equal(state[0], before[0])


# ---- (f) layer stacks ----------------------------------------------------------------------------------------------------------------
@PATHS
@pytest.mark.parametrize("method", ["rk4", "midpoint"])
@pytest.mark.parametrize("spec,H,HH", se.STACKS, ids=[se.stack_id(s) for s in se.STACKS])
def test_layer_stacks_through_the_abi(gpu_lib, spec, H, HH, method, path):
    """Un-shared, tied, eight-layer and uneven stacks (Dp > Hp with widths 93 and 128), B = 17, C = 7: z at every row bit-identical
    to ncde_fwd_generic on the coefficients built from the same rows, and within 2e-5 of the oracle in fp64."""
    import gpu_util
    import ncde_amd
    from ncde_amd import _lib
    B, C, L = (se.STACK_DIMS[k] for k in ("B", "C", "rows"))
    rect = path == "rectilinear"
    case = se.stack_case(spec, H, HH, method, path)
    x = se.dev(case["rows"], "cuda")
    coeffs = ncde_amd.linear_interpolation_coeffs(x.transpose(0, 1).contiguous(), rectilinear=0 if rect else None, initial_value_if_nan=0.0,
                                                  forward_fill=not rect)
    assert np.array_equal(coeffs.cpu().numpy(), case["coeffs"])      # the device builder on the same rows: the host's bits
    res = gpu_util.run_case(case, flags=_lib.FLAG_FORCE_GENERIC, need_grads=False)
    assert res["kernels"][0] == "ncde_fwd_generic", res["kernels"]
    p, func, keep = gpu_util.case_problem(case, _lib.FLAG_AUTO, "cuda")
    assert gpu_lib.ncde_stream_kernel_name(ctypes.byref(p)) == b"ncde_stream_step"
    state = _state(B, C, H, torch.from_numpy(case["z0"]).cuda())
    z_out = torch.empty(L, B, H, device="cuda")
    _ok(gpu_lib, p, _stream(x, state, rect, z_out=z_out))
    q = 2 if rect else 1
    got = z_out.cpu().numpy()
    assert np.array_equal(got, np.swapaxes(res["z_out"][:, ::q], 0, 1))
    assert np.array_equal(got[0], case["z0"]) and state[3].cpu().tolist() == [L] * B
    ref = np.swapaxes(se.stack_oracle(case)[:, ::q], 0, 1)
    e = gu.relerr(got, ref)
    print("stack %s %s %s: z vs fp64 oracle %.3e, vs ncde_fwd_generic 0" % (case["meta"]["topology"], method, path, e))
    assert e <= su.TIGHT_Z, e
    assert np.abs(ref[-1] - ref[0]).max() > 1e-3


# ---- (g) wide shapes and the LDS boundary --------------------------------------------------------------------------------------------
def _wide(name, path, lib):
    from ncde_amd import _lib
    model = se.wide_model(name, path, "cuda", kernel_flags=_lib.FLAG_FORCE_GENERIC)
    x = se.dev(se.wide_rows(name), "cuda")
    assert lib.ncde_stream_workspace_bytes(ctypes.byref(model.online(x.size(1))._problem())) == 0
    zs = _through_the_handle(model, x)
    assert np.array_equal(zs, _batch_hidden(model, x).cpu().numpy())
    h = model.online(x.size(1))
    with se.stepping("cuda"):
        h.step(x[0])
        assert np.array_equal(h.step(x[1:]).cpu().numpy(), zs[1:])
    e = gu.relerr(zs, se.wide_reference(name, path))
    assert np.abs(zs[-1] - zs[0]).max() > 1e-3
    return e


@PATHS
def test_wide_shape_on_the_lds_opt_in_path(gpu_lib, path):
    """(C 6, H 192, HH 192, nl 2), B = 17: about 87 KiB of LDS, beyond the 64 KiB a kernel gets without asking."""
    C, H, HH, nl, B, n = se.WIDE["H192"]
    assert _lds_bytes(C, H, [HH]) > 64 * 1024
    e = _wide("H192", path, gpu_lib)
    print("wide H192 %s (%d B of LDS): z vs fp64 %.3e, vs ncde_fwd_generic 0" % (path, _lds_bytes(C, H, [HH]), e))
    assert e <= su.TIGHT_Z, e


def test_lds_boundary(gpu_lib):
    """C = 4, HH = H, H walked upward in steps of 16: the LDS plan of the step, 4 (5 HS + 2 DS + 5 CS + 48) bytes, fits 160 KiB up
    to H = 352 (159168 B) and not at H = 368 (166336 B).  At 368 the plan of ncde_fwd_generic (165120 B) does not fit either, and
    that check, which stream_problem makes first, is the one that answers."""
    from ncde_amd import unfused
    limit, answers = 160 * 1024, {}
    for H in range(16, 417, 16):
        model = se.make_model(51, 4, H, 2, H, 2, "rectilinear", "cuda", apply_final_linear=False)
        rc = gpu_lib.ncde_stream_workspace_bytes(ctypes.byref(model.online(1)._problem()))
        answers[H] = (rc, (gpu_lib.ncde_last_error_string() or b"").decode() if rc else "")
        assert rc == (0 if _lds_bytes(4, H, [H]) <= limit else UNSUPPORTED), (H, rc)
    last_ok, first_no = max(H for H, a in answers.items() if a[0] == 0), min(H for H, a in answers.items() if a[0] != 0)
    print("LDS boundary: last accepted H %d (%d B), first refused H %d: %s" % (last_ok, _lds_bytes(4, last_ok, [last_ok]), first_no, answers[first_no][1]))
    assert (last_ok, first_no) == (352, 368)
    assert "LDS" in answers[first_no][1] and "generic forward needs 165120 B" in answers[first_no][1], answers[first_no]
    # the last accepted shape runs fused, without a warning, and matches
    e = _wide("H352", "rectilinear", gpu_lib)
    print("H352 fused: z vs fp64 %.3e, vs ncde_fwd_generic 0" % e)
    assert e <= su.TIGHT_Z, e
    # the first refused shape: the torch-op step behind exactly one warning, within the same bound
    model = se.wide_model("H368", "rectilinear", "cuda")
    x = se.dev(se.wide_rows("H368"), "cuda")
    unfused._WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        zs = su.step_through(model.online(x.size(1)), x, None, quiet=False)[1]
    said = [str(w.message) for w in rec]
    assert len(said) == 1 and "online step" in said[0] and "LDS" in said[0] and "unfused" in said[0], said
    e = gu.relerr(zs, se.wide_reference("H368", "rectilinear"))
    print("H368 torch-op step: z vs fp64 %.3e" % e)
    assert e <= su.TIGHT_Z, e


# ---- (h) small and odd dimensions ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,path", [(1, "linear"), (1, "rectilinear"), (2, "rectilinear"), (9, "linear"), (33, "rectilinear")],
                         ids=["C1_linear", "C1_rect_time_only", "C2_rect", "C9_linear", "C33_rect"])
@pytest.mark.parametrize("B", [1, 15, 16, 17, 33])
def test_small_and_odd_dimensions(gpu_lib, B, C, path):
    """Batches around one and two tiles, channel counts around the quads of the dX/dt images; C = 1 is time alone (rectilinear: the
    second piece of every step is all zero).  Bit-identical to the generic batch solve."""
    from ncde_amd import _lib
    model = se.make_model(55, C, 12, 2, 10, 2, path, "cuda", apply_final_linear=False, kernel_flags=_lib.FLAG_FORCE_GENERIC)
    x = se.dev(se.make_rows(5500 + C, 3, B, C), "cuda")
    zs = _through_the_handle(model, x)
    ref = _batch_hidden(model, x).cpu().numpy()
    print("B %d C %d %s: max |z - batch| / max |batch| = %.3e" % (B, C, path, gu.relerr(zs, ref)))
    assert np.array_equal(zs, ref)
    assert np.abs(ref[-1] - ref[0]).max() > 1e-3


# ---- (i) the readout through the ABI -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_out,bias,with_z", [(3, False, False), (1, True, False), (33, True, False), (3, True, True)],
                         ids=["no_bias", "n_out_1", "n_out_33", "Wf_and_z_out"])
def test_readout_through_the_abi(gpu_lib, n_out, bias, with_z):
    B, C, H, m = 19, 5, 12, 3
    model = se.make_model(57, C, H, 2, 10, 2, "linear", "cuda")
    p = model.online(B)._problem()
    x = se.dev(se.make_rows(5701, m, B, C), "cuda")
    g = torch.Generator().manual_seed(57)
    z0, Wf, bf = torch.randn(B, H, generator=g).cuda(), torch.randn(n_out, H, generator=g).cuda(), torch.randn(n_out, generator=g).cuda()
    plain, z_rows = _state(B, C, H, z0), torch.empty(m, B, H, device="cuda")
    _ok(gpu_lib, p, _stream(x, plain, False, z_out=z_rows))
    state, out = _state(B, C, H, z0), torch.full((m, B, n_out), float("nan"), device="cuda")
    z_too = torch.full((m, B, H), float("nan"), device="cuda") if with_z else None
    _ok(gpu_lib, p, _stream(x, state, False, Wf=Wf, bf=bf if bias else None, out=out, z_out=z_too))
    for a, b in zip(plain, state):      # the readout does not change the step
        assert torch.equal(a, b)
    assert z_too is None or torch.equal(z_too, z_rows)
    ref = z_rows.double().cpu() @ Wf.double().cpu().t() + (bf.double().cpu() if bias else 0.0)
    e = se.err(out, ref.numpy())
    print("readout n_out %d bias %s: %.3e" % (n_out, bias, e))
    assert e <= su.TIGHT_Z, e
    assert (z_rows[-1] - z_rows[0]).abs().max() > 1e-3


# ---- (k) many rows in one launch -----------------------------------------------------------------------------------------------------
@PATHS
def test_sixty_four_rows_in_one_launch(gpu_lib, path):
    """m = 64: bit-identical to 64 single calls and to the generic batch solve of the 65 observations (no fp64 bound: round-off
    accumulates over 64 or 128 steps)."""
    from ncde_amd import _lib
    B, C, m = 17, 5, 64
    model = se.make_model(59, C, 12, 2, 10, 2, path, "cuda", apply_final_linear=False, kernel_flags=_lib.FLAG_FORCE_GENERIC)
    x = se.dev(se.make_rows(5901, m + 1, B, C), "cuda")
    singles = _through_the_handle(model, x)
    h = model.online(B)
    with se.stepping("cuda"):
        first = h.step(x[0])
        many = h.step(x[1:])
    assert tuple(many.shape) == (m, B, 12)
    assert np.array_equal(first.cpu().numpy(), singles[0]) and np.array_equal(many.cpu().numpy(), singles[1:])
    assert np.array_equal(h.z.cpu().numpy(), singles[-1]) and h.count.cpu().tolist() == [m + 1] * B
    ref = _batch_hidden(model, x).cpu().numpy()
    print("64 rows %s: max |z - batch| / max |batch| = %.3e" % (path, gu.relerr(singles, ref)))
    assert np.array_equal(singles, ref)
    assert np.isfinite(ref).all() and np.abs(ref[-1] - ref[0]).max() > 1e-3
