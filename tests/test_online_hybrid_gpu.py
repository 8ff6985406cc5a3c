"""The hybrid step on the GPU (ncde_stream_step_hybrid / ncde_stream_step_field_hybrid / ncde_stream_step_lowrank_hybrid,
csrc/ncde_stream.hip): ``NeuralCDE.online(..., rectilinear_indices=R)`` on a linear model.

Reference: tests/hybrid_stream.prefix_reference (per stream and prefix, this package's batch model in fp64 on the CPU on
hybrid_ref.hybrid of the causally filled prefix, read at the stream's last kept knot) within the project's forward bound
su.TIGHT_Z = 2e-5 of max |ref|, for z and the readout at every step.  Bit for bit: rows per call, streams run alone or in halves
(a neighbour's piece B never touches a stream without one), masks, the state dict, a refused call, and R = [] against
ncde_stream_step.  Within the same bound: the torch-op step on the same GPU tensors and this package's fp32 batch forward on
linear_rectilinear_hybrid_coeffs of the filled rows.

Observed on the MI355X (max over steps of |delta| / max |ref|, z or readout, whichever is larger):
  parity, 4 pairs                        1.8e-7 .. 2.4e-7 (the same rows on a linear / a rectilinear handle: 3.8e-2 .. 5.4e-1 / 2.4e-2 .. 5.8e-1 away)
  euler / midpoint                       3.3e-7 / 4.0e-7
  shape edges, 11 cases                  1.2e-7 .. 3.3e-7 (the largest: low-rank, rank 2 of C 4)
  vs the torch-op step / the fp32 batch  1.5e-7 .. 2.6e-7 / 0 .. 2.1e-7 (0: the low-rank step sums in the batch kernel's order)
  evaluate input on the torch-op step    1.8e-7 (original), 1.3e-7 (minimal)
  LDS boundary H 352 fused / H 353 torch 1.4e-7 / 1.2e-7"""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import hybrid_stream as hs
import stream_edges as se
import stream_util as su

pytestmark = pytest.mark.gpu
F32 = torch.float32
INVALID, UNSUPPORTED = -1, -2      # NcdeStatus (include/ncde_hip.h)
S = hs.BASE
# (field, input) -> (the hybrid family, its kernel)
PAIRS = {("original", "matmul"): "hybrid", ("minimal", "matmul"): "field_hybrid", ("original", "derivative"): "field_hybrid",
         ("low-rank", "matmul"): "lowrank_hybrid"}


def _family(kind, mode):
    if kind == "low-rank":
        return "lowrank_hybrid"
    return "hybrid" if (kind, mode) == ("original", "matmul") else "field_hybrid"


# ---- helpers -------------------------------------------------------------------------------------------------------------------------
def _handle(model, B, R=S["R"], init=S["init"]):
    return model.online(B, initial_value_if_nan=init, rectilinear_indices=list(R))


def _kernel_name(lib, h):
    spec = h.model.func.fused_spec()
    family = h._kernel_entry(spec)[1][len("ncde_stream_step_"):]
    return family, getattr(lib, "ncde_stream_%s_kernel_name" % family)(ctypes.byref(h._problem()))


def _steps(model, x, R=S["R"], init=S["init"]):
    """One call per row on the fused route (any warning is an error) -> (outs, zs) as numpy, the handle."""
    with se.stepping("cuda"):
        h = _handle(model, x.size(1), R, init)
        outs, zs = hs.step_through(h, x)
    return outs, zs, h


def _check(lib, what, key, build, rows, R, init, family):
    """A model (build(device)) on `rows` through the hybrid handle against the fp64 reference of `key`."""
    z_ref, o_ref = hs.reference(key, lambda: build("cpu"), rows, R, init)
    outs, zs, h = _steps(build("cuda"), se.dev(rows, "cuda"), R, init)
    assert _kernel_name(lib, h) == (family, ("ncde_stream_step_" + family).encode())
    assert h.count.cpu().tolist() == [rows.shape[0]] * rows.shape[1]
    return hs.worst(outs, zs, z_ref, o_ref, su.TIGHT_Z, what), zs, z_ref


def _state_equal(a, b, where):
    for k in a.state_dict():
        assert torch.equal(a.state_dict()[k], b.state_dict()[k]), (where, k)


# ---- 1. parity, 2. non-vacuity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mode", list(PAIRS))
def test_parity_with_the_fp64_prefix_reference(gpu_lib, kind, mode):
    rows = hs.base_rows()
    hs.assert_rows(rows, S["R"], S["init"])
    _, zs, z_ref = _check(gpu_lib, "%s/%s" % (kind, mode), (kind, mode), lambda d: hs.model(kind, mode, d), rows, S["R"], S["init"], PAIRS[(kind, mode)])
    # the same rows on the two neighbouring paths answer otherwise
    x, scale = se.dev(rows, "cuda"), np.abs(z_ref).max()
    with se.stepping("cuda"):
        _, z_lin = hs.step_through(hs.model(kind, mode, "cuda").online(S["B"], initial_value_if_nan=S["init"]), x)
        _, z_rec = hs.step_through(hs.model(kind, mode, "cuda", path="rectilinear").online(S["B"], initial_value_if_nan=S["init"]), x)
    g_lin, g_rec = np.abs(zs - z_lin).max() / scale, np.abs(zs - z_rec).max() / scale
    print("%s/%s hybrid vs the linear handle %.3e, vs the rectilinear handle %.3e" % (kind, mode, g_lin, g_rec))
    assert g_lin > 1e-3 and g_rec > 1e-3, (g_lin, g_rec)


@pytest.mark.parametrize("method", ["euler", "midpoint"])
def test_euler_and_midpoint(gpu_lib, method):
    rows = hs.base_rows()
    _check(gpu_lib, "original/matmul %s" % method, ("method", method), lambda d: hs.model("original", "matmul", d, solver=method), rows, S["R"],
           S["init"], "hybrid")


# ---- 3. shape edges ------------------------------------------------------------------------------------------------------------------
EDGES = [      # (id, kind, mode, model dims, B, R)
    ("B1", "original", "matmul", {}, 1, (2, 4)),
    ("B16", "minimal", "matmul", {}, 16, (2, 4)),
    ("B17", "original", "derivative", {}, 17, (2, 4)),
    ("C2_time_and_one_sparse", "original", "matmul", dict(C=2), 5, (1,)),
    ("C2_field", "minimal", "matmul", dict(C=2), 5, (1,)),
    ("R_every_channel", "original", "matmul", {}, 17, (1, 2, 3, 4)),
    ("R_every_channel_derivative", "original", "derivative", {}, 5, (1, 2, 3, 4)),
    ("H7_HH24_derivative", "original", "derivative", dict(C=6, H=7, HH=24), 5, (2, 5)),      # d0 = 13: no multiple of 4 or 16
    ("H7_HH24_minimal_derivative", "minimal", "derivative", dict(C=6, H=7, HH=24), 17, (1, 3)),
    ("lowrank_rank2_of_4", "low-rank", "matmul", dict(C=4), 17, (3,)),
    ("lowrank_rank5_of_9", "low-rank", "matmul", dict(C=9), 5, (2, 5, 8)),
]


@pytest.mark.parametrize("case", EDGES, ids=[c[0] for c in EDGES])
def test_shape_edges(gpu_lib, case):
    name, kind, mode, dims, B, R = case
    C = dims.get("C", 5)
    rows = hs.make_rows(9103, 5, B, C, R, busy=B - 1)
    has = hs.piece_b(rows, R, 0.25)
    assert has[1:].any() and (~has[1:]).any() or B == 1
    model = hs.model(kind, mode, "cpu", **dims)
    if kind == "low-rank":
        assert model.func.fused_spec().rank < C
    _check(gpu_lib, name, ("edge", name), lambda d: hs.model(kind, mode, d, **dims), rows, R, 0.25, _family(kind, mode))


def test_no_sparse_channel_is_ncde_stream_step_bit_for_bit(gpu_lib):
    rows = hs.base_rows()
    x = se.dev(rows, "cuda")
    model = hs.model("original", "matmul", "cuda")
    with se.stepping("cuda"):
        ha, hb = _handle(model, S["B"], R=[]), model.online(S["B"], initial_value_if_nan=S["init"])
        assert _kernel_name(gpu_lib, ha)[1] == b"ncde_stream_step_hybrid"
        assert gpu_lib.ncde_stream_kernel_name(ctypes.byref(hb._problem())) == b"ncde_stream_step" and not hb.hybrid
        for k in range(S["rows"]):
            assert torch.equal(ha.step(x[k]), hb.step(x[k])), k
            _state_equal(ha, hb, k)
    assert (ha.z - model.online(S["B"]).z).abs().max() > 1e-3


# ---- 4. bit identities ---------------------------------------------------------------------------------------------------------------
BITS = [("original", "matmul"), ("original", "derivative"), ("low-rank", "matmul")]


@pytest.mark.parametrize("kind,mode", BITS)
def test_rows_in_one_call_alone_and_interleaved_halves(gpu_lib, kind, mode):
    """Every stream gives, alone in a handle of batch 1 and in a half of the batch, the bits it gives in the full batch: a
    neighbour's piece B never touches a stream without one (the base rows hold tile-rows with both kinds of stream)."""
    model = hs.model(kind, mode, "cuda")
    rows = hs.base_rows()
    has = hs.piece_b(rows, S["R"], S["init"])
    assert any(has[r, :16].any() and not has[r, :16].all() for r in range(1, S["rows"]))
    x = se.dev(rows, "cuda")
    with se.stepping("cuda"):
        h1, h2 = _handle(model, S["B"]), _handle(model, S["B"])
        many = torch.cat([h1.step(x[0])[None], h1.step(x[1:])])      # m = 5 rows in one launch
        singles = torch.stack([h2.step(x[k]) for k in range(S["rows"])])
        assert torch.equal(many, singles)
        _state_equal(h1, h2, "m rows in one call")
        for half in (slice(0, None, 2), slice(1, None, 2)):      # streams of one tile spread over two tiles and the reverse
            xh = x[:, half].contiguous()
            hh = _handle(model, xh.size(1))
            assert torch.equal(torch.stack([hh.step(xh[k]) for k in range(S["rows"])]), singles[:, half])
            for k in hh.state_dict():
                assert torch.equal(hh.state_dict()[k], h2.state_dict()[k][half]), k
        for b in range(S["B"]):
            hb = _handle(model, 1)
            assert torch.equal(hb.step(x[:1, b:b + 1])[0, 0], singles[0, b])
            assert torch.equal(hb.step(x[1:, b:b + 1])[:, 0], singles[1:, b]), b
            for k in hb.state_dict():
                assert torch.equal(hb.state_dict()[k][0], h2.state_dict()[k][b]), (b, k)
    assert (singles[-1] - singles[0]).abs().max() > 1e-3


@pytest.mark.parametrize("kind,mode", BITS)
def test_masks_in_one_launch_and_non_receivers(gpu_lib, kind, mode):
    """The staggered schedule of tests/stream_edges.py on the hybrid rows: non-receivers keep their state, every stream answers
    what it answers alone, and -- after an unmasked first call -- the [m, B] mask in ONE launch equals the masked single calls."""
    model = hs.model(kind, mode, "cuda")
    A = se.schedule()
    se.assert_schedule(A)
    rows = hs.base_rows().copy()
    rows[~A] = se.GARBAGE
    x, act = se.dev(rows, "cuda"), se.dev(A, "cuda")
    with se.stepping("cuda"):
        h = _handle(model, S["B"])
        alone = [_handle(model, 1) for _ in range(S["B"])]
        for j in range(S["rows"]):
            before = h.state_dict()
            out = h.step(x[j], active=act[j])
            after = h.state_dict()
            for key in before:
                assert torch.equal(before[key][~act[j]], after[key][~act[j]]), (j, key)
            for b in np.nonzero(A[j])[0]:
                ob = alone[b].step(x[j, b:b + 1])
                assert torch.equal(ob[0], out[b]) and all(torch.equal(alone[b].state_dict()[k][0], after[k][b]) for k in after), (j, b)
        assert h.count.cpu().tolist() == A.sum(axis=0).tolist()
        assert not (h.last_row == float(se.GARBAGE)).any()
        A1 = A.copy()
        A1[0] = True
        rows1 = hs.base_rows().copy()
        rows1[~A1] = se.GARBAGE
        x, act = se.dev(rows1, "cuda"), se.dev(A1, "cuda")
        h1, h2 = _handle(model, S["B"]), _handle(model, S["B"])
        first = h1.step(x[0])
        assert h1._may_init is False
        many = h1.step(x[1:], active=act[1:])
        singles = [h2.step(x[0])] + [h2.step(x[j], active=act[j]) for j in range(1, S["rows"])]
        assert torch.equal(torch.cat([first[None], many]), torch.stack(singles))
        _state_equal(h1, h2, "row mask in one launch")


@pytest.mark.parametrize("kind,mode", BITS)
def test_state_dict_round_trip_and_a_refused_call(gpu_lib, kind, mode):
    model = hs.model(kind, mode, "cuda")
    x = se.dev(hs.base_rows(), "cuda")
    with se.stepping("cuda"):
        ha, hb = _handle(model, S["B"]), _handle(model, S["B"])
        ha.step(x[:3])
        saved = ha.state_dict()
        hb.load_state_dict(saved)
        assert torch.equal(ha.step(x[3:]), hb.step(x[3:]))
        _state_equal(ha, hb, "round trip")
        # refusals through the ABI: nothing is launched, the state keeps its bits
        before = ha.state_dict()
        p = ha._problem()
        st, out, keep = ha._stream_args(x[:1], None, 1)
        entry = getattr(gpu_lib, ha._kernel_entry(model.func.fused_spec())[1])
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        mask = ctypes.c_void_p(ha.rect_mask.data_ptr())
        st.n_rows = 0
        assert entry(ctypes.byref(p), ctypes.byref(st), mask, stream) == INVALID and b"n_rows" in gpu_lib.ncde_last_error_string()
        st.n_rows = 1
        assert entry(ctypes.byref(p), ctypes.byref(st), None, stream) == INVALID and b"rectilinear_mask is NULL" in gpu_lib.ncde_last_error_string()
        st.rectilinear = 1
        assert entry(ctypes.byref(p), ctypes.byref(st), mask, stream) == INVALID and b"rectilinear must be 0" in gpu_lib.ncde_last_error_string()
        torch.cuda.synchronize()
        for k in before:
            assert torch.equal(before[k], ha.state_dict()[k]), k


# ---- 5. against the two routes that exist without the kernel ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mode", list(PAIRS))
def test_against_the_torch_step_and_the_batch_forward(gpu_lib, kind, mode):
    import ncde_amd
    model = hs.model(kind, mode, "cuda", apply_final_linear=False)
    rows = hs.base_rows()
    x = se.dev(rows, "cuda")
    _, zs, h = _steps(model, x)
    assert _kernel_name(gpu_lib, h)[1] == ("ncde_stream_step_" + PAIRS[(kind, mode)]).encode()
    # the torch-op step on the same tensors (the route this handle takes where no kernel covers it)
    ht = _handle(model, S["B"])
    ht._route[("cuda", F32)] = False
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, z_torch = hs.step_through(ht, x)
    # this package's fp32 batch forward on the hybrid coefficients of the causally filled rows, read per stream at its kept knot
    filled = se.dev(np.ascontiguousarray(np.swapaxes(hs.causal_fill(rows, S["init"]), 0, 1)), "cuda")
    coeffs, lengths = ncde_amd.linear_rectilinear_hybrid_coeffs(filled, list(S["R"]), return_lengths=True)
    has = hs.piece_b(rows, S["R"], S["init"])
    at = np.arange(S["rows"])[:, None] + np.cumsum(has, axis=0)      # [rows, B]: the last kept knot of every prefix
    assert lengths.cpu().tolist() == (at[-1] + 1).tolist()
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        z_all = model(coeffs).cpu().numpy()      # [B, T, H]
    z_batch = np.stack([z_all[np.arange(S["B"]), at[k]] for k in range(S["rows"])])
    e_torch = max(se.err(zs[k], z_torch[k]) for k in range(S["rows"]))
    e_batch = max(se.err(zs[k], z_batch[k]) for k in range(S["rows"]))
    print("%s/%s: vs the torch-op step %.3e, vs the fp32 batch forward %.3e" % (kind, mode, e_torch, e_batch))
    assert e_torch <= su.TIGHT_Z and e_batch <= su.TIGHT_Z, (e_torch, e_batch)
    assert np.abs(z_batch[-1] - z_batch[0]).max() > 1e-3


# ---- 6. the evaluate input -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["original", "minimal"])
def test_the_evaluate_input_takes_the_torch_step(gpu_lib, kind):
    from ncde_amd import unfused
    rows = hs.base_rows()
    z_ref, o_ref = hs.reference((kind, "evaluate"), lambda: hs.model(kind, "evaluate", "cpu"), rows, S["R"], S["init"])
    model = hs.model(kind, "evaluate", "cuda")
    h = _handle(model, S["B"])
    assert gpu_lib.ncde_stream_field_hybrid_workspace_bytes(ctypes.byref(h._problem())) == UNSUPPORTED
    assert gpu_lib.ncde_stream_field_hybrid_kernel_name(ctypes.byref(h._problem())) is None
    unfused._WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        outs, zs = hs.step_through(h, se.dev(rows, "cuda"))
    msgs = [str(w.message) for w in rec]
    assert len(msgs) == 1 and "unfused" in msgs[0] and "online step" in msgs[0] and "evaluate" in msgs[0], msgs
    assert h._route[("cuda", F32)] is False
    hs.worst(outs, zs, z_ref, o_ref, su.TIGHT_Z, "%s/evaluate on the torch-op step" % kind)


# ---- 7. the LDS boundary ---------------------------------------------------------------------------------------------------------------
def _wide(H, device):
    return se.make_model(95, 4, H, 2, H, 2, "linear", device, F32, apply_final_linear=False, vector_field_type="derivative")


WIDE_R = (3,)


def _wide_rows():
    rows = hs.make_rows(9108, 3, 3, 4, WIDE_R, busy=2)
    has = hs.piece_b(rows, WIDE_R, 0.0)
    assert has[1:].any() and not has[1:].all()
    return rows


def test_last_width_the_lds_plan_holds_steps_fused(gpu_lib):
    """C 4, HH = H, nl 2, derivative: H 352 is the last width the query accepts (tests/test_online_hybrid_cpu.py finds it)."""
    assert gpu_lib.ncde_stream_field_hybrid_workspace_bytes(ctypes.byref(_handle(_wide(352, "cuda"), 3, WIDE_R, 0.0)._problem())) == 0
    _check(gpu_lib, "H352 derivative", ("wide", 352), lambda d: _wide(352, d), _wide_rows(), WIDE_R, 0.0, "field_hybrid")


def test_first_width_the_lds_plan_refuses_takes_the_torch_step(gpu_lib):
    from ncde_amd import unfused
    rows = _wide_rows()
    model = _wide(353, "cuda")
    h = _handle(model, 3, WIDE_R, 0.0)
    assert gpu_lib.ncde_stream_field_hybrid_workspace_bytes(ctypes.byref(h._problem())) == UNSUPPORTED
    assert gpu_lib.ncde_stream_field_hybrid_kernel_name(ctypes.byref(h._problem())) is None
    z_ref, o_ref = hs.reference(("wide", 353), lambda: _wide(353, "cpu"), rows, WIDE_R, 0.0)
    unfused._WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        outs, zs = hs.step_through(h, se.dev(rows, "cuda"))
    msgs = [str(w.message) for w in rec]
    assert len(msgs) == 1 and "unfused" in msgs[0] and "online step" in msgs[0] and "LDS" in msgs[0], msgs
    hs.worst(outs, zs, z_ref, o_ref, su.TIGHT_Z, "H353 derivative on the torch-op step")
