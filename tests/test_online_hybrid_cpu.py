"""The online hybrid step without a GPU: the torch-op step of ``NeuralCDE.online(..., rectilinear_indices=R)`` in fp32 and fp64
against the fp64 reference of tests/hybrid_stream.py (within stream_edges.tol), its arguments, its bit identities, and the C-ABI
queries of the three hybrid entry points (ncde_stream_hybrid_* / ncde_stream_field_hybrid_* / ncde_stream_lowrank_hybrid_*), which
read the problem only.

Observed (max over steps of |delta| / max |ref|): fp32 1.4e-7 .. 2.0e-7, fp64 0 .. 1.9e-16."""
import ctypes
import re
import warnings

import numpy as np
import pytest
import torch

import hybrid_stream as hs
import stack_util as sk
import stream_edges as se
from test_online_fields_cpu import field_problem

INVALID, UNSUPPORTED = -1, -2
S = hs.BASE
# (field, input) -> the hybrid family that steps it
ACCEPTED = {("original", "matmul"): "hybrid", ("minimal", "matmul"): "field_hybrid", ("original", "derivative"): "field_hybrid",
            ("low-rank", "matmul"): "lowrank_hybrid"}
NAMES = {"hybrid": b"ncde_stream_step_hybrid", "field_hybrid": b"ncde_stream_step_field_hybrid", "lowrank_hybrid": b"ncde_stream_step_lowrank_hybrid"}


def _handle(model, B=None, R=S["R"], **kw):
    return model.online(B or S["B"], initial_value_if_nan=S["init"], rectilinear_indices=list(R), **kw)


# ---- the rows ------------------------------------------------------------------------------------------------------------------------
def test_the_rows_hold_the_six_conditions():
    rows = hs.base_rows()
    hs.assert_rows(rows, S["R"], S["init"])
    has = hs.piece_b(rows, S["R"], S["init"])
    print("piece B per row (streams of 19):", has.sum(axis=1).tolist())
    miss = np.isnan(rows[:, :, list(S["R"])]).mean()
    assert 0.65 <= miss <= 0.9, miss


# ---- the torch-op step against the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("kind,mode", list(ACCEPTED) + [("original", "evaluate"), ("gru", "matmul")])
def test_torch_step_against_the_fp64_reference(kind, mode, dtype):
    rows = hs.base_rows()
    z_ref, o_ref = hs.reference((kind, mode), lambda: hs.model(kind, mode, "cpu"), rows, S["R"], S["init"])
    with se.stepping("cpu"):
        h = _handle(hs.model(kind, mode, "cpu", dtype))
        outs, zs = hs.step_through(h, se.dev(rows, "cpu", dtype))
    hs.worst(outs, zs, z_ref, o_ref, se.tol("cpu", dtype), "torch-op hybrid %s/%s %s" % (kind, mode, dtype))
    assert h.count.tolist() == [S["rows"]] * S["B"]
    # the state after the last row: the filled row, and the last piece taken
    f, has = hs.causal_fill(rows, S["init"]), hs.piece_b(rows, S["R"], S["init"])
    assert np.array_equal(h.last_row.to(torch.float32).numpy(), f[-1])
    d = f[-1].astype(np.float64) - f[-2].astype(np.float64)
    sparse = np.isin(np.arange(S["C"]), S["R"])
    want = np.where(has[-1][:, None], np.where(sparse, d, 0.0), np.where(sparse, 0.0, d))
    assert np.allclose(h.prev_dx.double().numpy(), want, rtol=0, atol=1e-6 * np.abs(f).max())


@pytest.mark.parametrize("method", ["euler", "midpoint"])
def test_euler_and_midpoint(method):
    rows = hs.base_rows()
    z_ref, o_ref = hs.reference(("method", method), lambda: hs.model("original", "matmul", "cpu", solver=method), rows, S["R"], S["init"])
    with se.stepping("cpu"):
        outs, zs = hs.step_through(_handle(hs.model("original", "matmul", "cpu", solver=method)), se.dev(rows, "cpu"))
    hs.worst(outs, zs, z_ref, o_ref, se.tol("cpu", torch.float32), "torch-op hybrid %s" % method)


def test_the_hybrid_path_is_neither_the_linear_nor_the_rectilinear_one():
    rows = hs.base_rows()
    z_ref, _ = hs.reference(("original", "matmul"), lambda: hs.model("original", "matmul", "cpu"), rows, S["R"], S["init"])
    x = se.dev(rows, "cpu")
    with se.stepping("cpu"):
        _, z_hyb = hs.step_through(_handle(hs.model("original", "matmul", "cpu")), x)
        _, z_lin = hs.step_through(hs.model("original", "matmul", "cpu").online(S["B"], initial_value_if_nan=S["init"]), x)
        _, z_rec = hs.step_through(hs.model("original", "matmul", "cpu", path="rectilinear").online(S["B"], initial_value_if_nan=S["init"]), x)
    scale = np.abs(z_ref).max()
    print("hybrid vs linear %.3e, vs rectilinear %.3e" % (np.abs(z_hyb - z_lin).max() / scale, np.abs(z_hyb - z_rec).max() / scale))
    assert np.abs(z_hyb - z_lin).max() > 1e-3 * scale and np.abs(z_hyb - z_rec).max() > 1e-3 * scale


def test_no_sparse_channel_is_the_linear_handle_bit_for_bit():
    rows = se.dev(hs.base_rows(), "cpu")
    model = hs.model("original", "matmul", "cpu")
    with se.stepping("cpu"):
        ha, hb = _handle(model, R=[]), model.online(S["B"], initial_value_if_nan=S["init"])
        assert ha.hybrid and not ha.rect_mask.any() and not hb.hybrid
        for k in range(S["rows"]):
            assert torch.equal(ha.step(rows[k]), hb.step(rows[k])), k
            for key in ha.state_dict():
                assert torch.equal(ha.state_dict()[key], hb.state_dict()[key]), (k, key)


# ---- arguments -----------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    lin = hs.model("original", "matmul", "cpu")
    for path in ("rectilinear", "cubic_hermite"):
        with pytest.raises(ValueError, match="interpolation"):
            hs.model("original", "matmul", "cpu", path=path).online(3, rectilinear_indices=[2])
    with pytest.raises(NotImplementedError, match="channel 0"):
        lin.online(3, time_index=1, rectilinear_indices=[2])
    for bad in ([0], [0, 2], [S["C"]], [2, S["C"] + 3], [-1], [2, 2], [2, 4, 2], [1.0], [True]):
        with pytest.raises(ValueError, match="rectilinear_indices"):
            lin.online(3, rectilinear_indices=bad)
    h = lin.online(3, rectilinear_indices=[4, 1])
    assert h.rect_mask.dtype == torch.uint8 and h.rect_mask.tolist() == [0, 1, 0, 0, 1] and h.rect_mask.device == h.z.device
    assert lin.online(3, rectilinear_indices=(c for c in (2, 3))).rect_mask.tolist() == [0, 0, 1, 1, 0]
    assert lin.online(3).rect_mask is None and lin.online(3, time_index=1).hybrid is False      # None: today's handle


# ---- bit identities --------------------------------------------------------------------------------------------------------------
def test_rows_in_one_call_equal_single_calls():
    x = se.dev(hs.base_rows(), "cpu")
    model = hs.model("original", "matmul", "cpu")
    with se.stepping("cpu"):
        h1, h2 = _handle(model), _handle(model)
        many = torch.cat([h1.step(x[0])[None], h1.step(x[1:])])
        singles = torch.stack([h2.step(x[k]) for k in range(S["rows"])])
    assert torch.equal(many, singles)
    for k in h1.state_dict():
        assert torch.equal(h1.state_dict()[k], h2.state_dict()[k]), k


def test_masks_leave_the_state_of_non_receivers_untouched():
    rows = hs.base_rows()
    A = se.schedule()
    assert A.shape == rows.shape[:2]
    rows = rows.copy()
    rows[~A] = se.GARBAGE
    x, act = se.dev(rows, "cpu"), se.dev(A, "cpu")
    model = hs.model("original", "matmul", "cpu")
    with se.stepping("cpu"):
        h, moved = _handle(model), False
        for j in range(S["rows"]):
            before = h.state_dict()
            h.step(x[j], active=act[j])
            after = h.state_dict()
            for key in before:
                assert torch.equal(before[key][~act[j]], after[key][~act[j]]), (j, key)
            moved = moved or not torch.equal(before["z"][act[j]], after["z"][act[j]])
        assert moved and h.count.tolist() == A.sum(axis=0).tolist()
        assert not (h.last_row == float(se.GARBAGE)).any()


def test_state_dict_round_trip():
    x = se.dev(hs.base_rows(), "cpu")
    model = hs.model("minimal", "matmul", "cpu")
    with se.stepping("cpu"):
        ha, hb = _handle(model), _handle(model)
        ha.step(x[:3])
        saved = ha.state_dict()
        assert sorted(saved) == ["count", "last_row", "prev_dx", "z"]
        assert [tuple(saved[k].shape) for k in sorted(saved)] == [(S["B"],), (S["B"], S["C"]), (S["B"], S["C"]), (S["B"], S["H"])]
        hb.load_state_dict(saved)
        assert torch.equal(ha.step(x[3:]), hb.step(x[3:]))
        for k in saved:
            assert torch.equal(ha.state_dict()[k], hb.state_dict()[k]), k


# ---- the queries ---------------------------------------------------------------------------------------------------------------------
def _problem(kind, mode, **kw):
    return field_problem({"low-rank": "lowrank"}.get(kind, kind), mode, **kw)


def query(family, p):
    from ncde_amd import _lib
    lib = _lib.lib()
    rc = getattr(lib, "ncde_stream_%s_workspace_bytes" % family)(None if p is None else ctypes.byref(p))
    msg = (lib.ncde_last_error_string() or b"").decode()
    name = getattr(lib, "ncde_stream_%s_kernel_name" % family)(None if p is None else ctypes.byref(p))
    assert (name == NAMES[family]) == (rc == 0) and (name is None) == (rc != 0)
    return rc, msg


@pytest.mark.parametrize("kind,mode", list(ACCEPTED))
def test_queries_accept_the_four_pairs(kind, mode):
    family = ACCEPTED[(kind, mode)]
    for method in (0, 1, 2):
        assert query(family, _problem(kind, mode, method=method))[0] == 0
    model = hs.model(kind, mode, "cpu")
    h = _handle(model)
    assert h._kernel_entry(model.func.fused_spec()) == ("ncde_stream_%s_workspace_bytes" % family, "ncde_stream_step_%s" % family)
    assert query(family, h._problem())[0] == 0      # the handle's own problem


def test_queries_refuse_evaluate_gru_and_the_hermite_path():
    for kind in ("original", "minimal"):
        rc, msg = query("field_hybrid", _problem(kind, "evaluate"))
        assert rc == UNSUPPORTED and "evaluate" in msg and "knot index" in msg, msg
    for mode in ("matmul", "derivative"):
        rc, msg = query("field_hybrid", _problem("gru", mode))
        assert rc == UNSUPPORTED and "GRU" in msg, msg
    rc, msg = query("field_hybrid", _problem("original", "matmul"))
    assert rc == UNSUPPORTED and "ncde_stream_step_hybrid" in msg
    rc, msg = query("field_hybrid", _problem("low-rank", "matmul"))
    assert rc == UNSUPPORTED and "low-rank" in msg
    for kind, mode in (("minimal", "matmul"), ("original", "derivative"), ("low-rank", "matmul"), ("gru", "matmul")):
        assert query("hybrid", _problem(kind, mode))[0] == UNSUPPORTED, (kind, mode)
    for kind in ("original", "minimal", "gru"):
        rc, msg = query("lowrank_hybrid", _problem(kind, "matmul"))
        assert rc == UNSUPPORTED and "low-rank field only" in msg
    for (kind, mode), family in ACCEPTED.items():
        rc, msg = query(family, _problem(kind, mode, interp=1))
        assert rc == UNSUPPORTED and "Hermite" in msg, (family, msg)
        assert query(family, _problem(kind, mode, interp=2))[0] == INVALID
        assert query(family, _problem(kind, mode, method=3))[0] == INVALID
        assert query(family, None)[0] == INVALID
    model = hs.model("gru", "matmul", "cpu")
    assert _handle(model)._kernel_entry(model.func.fused_spec()) is None


def _bytes(family, C, H, direct=False, R=1):
    """The LDS plans of the hybrid steps (csrc/ncde_stream.hip) for HH = H, nl 2, written out: the plain step's plan plus 16 flags
    (64 words of flags and counts); the field step's without the two start rows of the evaluate input (five [Cp][16] images)."""
    ru = lambda v, m: (v + m - 1) // m * m      # noqa: E731
    HS, CS = ru(H, 16) * 16, ru(C, 4) * 16
    if family == "hybrid":
        return 4 * (5 * HS + 2 * HS + 5 * CS + 64)
    if family == "lowrank_hybrid":
        return 4 * (5 * HS + 2 * HS + 5 * CS + 64 + 16 * ru((H + C) * R, 16))
    DS = 16 * max(ru(H, 16), ru(H + C if direct else H, 16))
    return 4 * (3 * DS + 4 * HS + 5 * CS + 64)


@pytest.mark.parametrize("family,kind,mode", [("hybrid", "original", "matmul"), ("field_hybrid", "original", "derivative"),
                                              ("field_hybrid", "minimal", "matmul"), ("lowrank_hybrid", "low-rank", "matmul")])
def test_lds_boundary_by_the_query(family, kind, mode):
    last = None
    for H in range(1, 4096):
        p = _problem(kind, mode, B=3, C=4, H=H, HH=H, nl=2)
        if kind == "low-rank":
            from ncde_amd import _lib
            p.flags = _lib.FLAG_FIELD_RANK(1)
        rc, msg = query(family, p)
        if rc != 0:
            break
        last = H
    need = _bytes(family, 4, H, direct=mode == "derivative")
    print("%s %s/%s, C 4, HH = H, nl 2: last accepted H %d, first refused H %d (%s)" % (family, kind, mode, last, H, msg))
    assert rc == UNSUPPORTED and "B of LDS" in msg and H == last + 1
    said = int(re.search(r"needs (\d+) B", msg).group(1))
    assert said > 160 * 1024 and need > 160 * 1024 and _bytes(family, 4, last, direct=mode == "derivative") <= 160 * 1024
    if family == "hybrid":      # (the plain step's problem judges the batch kernel's plan first: it is the smaller one, and over as well)
        assert "generic forward" in msg and said <= need
    else:
        assert said == need


def test_the_old_entry_points_still_refuse_what_they_refused():
    from ncde_amd import _lib
    lib = _lib.lib()
    by = ctypes.byref
    assert lib.ncde_stream_field_workspace_bytes(by(_problem("gru", "matmul"))) == UNSUPPORTED
    assert lib.ncde_stream_field_workspace_bytes(by(_problem("original", "matmul"))) == UNSUPPORTED
    assert lib.ncde_stream_field_workspace_bytes(by(_problem("original", "evaluate"))) == 0      # ... and still accept the evaluate input
    assert lib.ncde_stream_field_workspace_bytes(by(_problem("original", "evaluate", interp=1))) == INVALID
    assert lib.ncde_stream_workspace_bytes(by(_problem("minimal", "matmul"))) == UNSUPPORTED
    assert lib.ncde_stream_lowrank_workspace_bytes(by(_problem("original", "matmul"))) == UNSUPPORTED
    assert lib.ncde_stream_lowrank_kernel_name(by(_problem("low-rank", "matmul", interp=1))) == b"ncde_stream_step_lowrank_hermite"
    rc, msg = sk.query([sk.dummy_problem(), sk.dummy_problem(C=20)])
    assert rc == 0
    # the launch routines judge the stream before anything is launched (no device is touched by a refusal)
    s = _lib.NcdeStream()
    s.n_rows, s.rectilinear = 1, 1
    s.x, s.x_stride_m, s.x_stride_b = 0x100, 19 * 5, 5      # (dummy pointers: never dereferenced)
    s.z, s.last_row, s.prev_dx, s.count, s.z_out = 0x200, 0x300, 0x400, 0x500, 0x600
    arr_p = (ctypes.POINTER(_lib.NcdeProblem) * 1)(ctypes.pointer(sk.dummy_problem()))
    arr_s = (ctypes.POINTER(_lib.NcdeStream) * 1)(ctypes.pointer(s))
    assert lib.ncde_stream_stack_step(arr_p, arr_s, 1, None) == INVALID and b"rectilinear must be 0" in lib.ncde_last_error_string()
    mask = ctypes.c_void_p(0x2000)
    for family, (kind, mode) in (("hybrid", ("original", "matmul")), ("field_hybrid", ("minimal", "matmul")), ("lowrank_hybrid", ("low-rank", "matmul"))):
        step = getattr(lib, "ncde_stream_step_" + family)
        p = _problem(kind, mode)
        assert step(by(p), by(s), mask, None) == INVALID and b"rectilinear must be 0" in lib.ncde_last_error_string(), family
        s.rectilinear = 0
        assert step(by(p), by(s), None, None) == INVALID and b"rectilinear_mask is NULL" in lib.ncde_last_error_string(), family
        s.time_index = 2
        assert step(by(p), by(s), mask, None) == INVALID and b"time is channel 0" in lib.ncde_last_error_string(), family
        s.time_index, s.n_rows = 0, 0
        assert step(by(p), by(s), mask, None) == INVALID and b"n_rows" in lib.ncde_last_error_string(), family
        s.n_rows, s.rectilinear = 1, 1


def test_hybrid_handle_on_cpu_tensors_takes_the_torch_step():
    from ncde_amd import unfused
    model = hs.model("original", "matmul", "cpu")
    x = se.dev(hs.base_rows(), "cpu")
    unfused._WARNED.clear()
    h = _handle(model)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = torch.stack([h.step(x[k]) for k in range(x.size(0))])
    assert sum("unfused" in str(w.message) and "not fp32 on the GPU" in str(w.message) for w in rec) == 1, [str(w.message) for w in rec]
    assert h._route[("cpu", torch.float32)] is False and torch.isfinite(out).all()
