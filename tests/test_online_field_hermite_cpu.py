"""The queries of the field step on the Hermite path (ncde_stream_field_hermite_workspace_bytes / _kernel_name), which read the
problem only and need no device, and the route of a minimal-gated ``cubic_hermite`` handle on CPU tensors.

The five pairs are those of ncde_stream_step_field (tests/test_online_fields_cpu.py, whose field_problem builds the problems here);
the LDS plan is that step's too, so the two queries must agree on every shape."""
import ctypes
import warnings

import pytest
import torch

import stream_edges as se
from test_online_fields_cpu import PAIRS, field_problem, plan_bytes

INVALID, UNSUPPORTED = -1, -2
CUBIC = 1


def query(p):
    from ncde_amd import _lib
    lib = _lib.lib()
    rc = lib.ncde_stream_field_hermite_workspace_bytes(ctypes.byref(p))
    msg = (lib.ncde_last_error_string() or b"").decode()
    name = lib.ncde_stream_field_hermite_kernel_name(ctypes.byref(p))
    assert (name == b"ncde_stream_step_field_hermite") == (rc == 0) and (name is None) == (rc != 0)
    return rc, msg


def linear_query(p):
    from ncde_amd import _lib
    return _lib.lib().ncde_stream_field_workspace_bytes(ctypes.byref(p))


@pytest.mark.parametrize("kind,mode", PAIRS)
@pytest.mark.parametrize("nl", [0, 3])
def test_query_accepts_the_five_pairs(kind, mode, nl):
    for method in (0, 1, 2):
        assert query(field_problem(kind, mode, nl=nl, method=method, interp=CUBIC))[0] == 0


def test_query_refuses():
    from ncde_amd import _lib
    for kind in ("gru", "lowrank"):
        for mode in ("matmul", "evaluate", "derivative"):
            rc, msg = query(field_problem(kind, mode, interp=CUBIC))
            assert rc == UNSUPPORTED and ("GRU" in msg if kind == "gru" else "low-rank" in msg), (kind, mode, msg)
    rc, msg = query(field_problem("original", "matmul", interp=CUBIC))
    assert rc == UNSUPPORTED and "ncde_stream_step_hermite" in msg
    for kind, mode in PAIRS:
        rc, msg = query(field_problem(kind, mode))      # linear: that is ncde_stream_step_field's
        assert rc == INVALID and "NCDE_INTERP_CUBIC" in msg
        assert query(field_problem(kind, mode, interp=2))[0] == INVALID
        assert query(field_problem(kind, mode, interp=CUBIC, method=3))[0] == INVALID
        p = field_problem(kind, mode, interp=CUBIC)
        p.layer_in[1] = p.layer_in[1] + 1
        rc, msg = query(p)
        assert rc == INVALID and "chain" in msg
        if kind != "original":
            for gone in ("Wg", "bg"):
                p = field_problem(kind, mode, interp=CUBIC)
                setattr(p, gone, None)
                rc, msg = query(p)
                assert rc == INVALID and "Wg" in msg, (kind, mode, gone)
    assert _lib.lib().ncde_stream_field_hermite_workspace_bytes(None) == INVALID


def test_the_step_refuses_a_rectilinear_stream_before_it_launches():
    """Answered on the host: no device is touched (every pointer is a dummy)."""
    from ncde_amd import _lib
    lib = _lib.lib()
    s = _lib.NcdeStream()
    s.n_rows, s.x, s.x_stride_m, s.x_stride_b = 1, 0x100, 19 * 5, 5
    s.z, s.last_row, s.prev_dx, s.count, s.z_out = 0x200, 0x300, 0x400, 0x500, 0x600
    s.rectilinear = 1
    p = field_problem("minimal", "evaluate", interp=CUBIC)
    assert lib.ncde_stream_step_field_hermite(ctypes.byref(p), ctypes.byref(s), None) == INVALID
    assert b"rectilinear must be 0" in lib.ncde_last_error_string()
    s.rectilinear, s.n_rows = 0, 0
    assert lib.ncde_stream_step_field_hermite(ctypes.byref(p), ctypes.byref(s), None) == INVALID
    assert b"n_rows" in lib.ncde_last_error_string()


GRID_H = (1, 7, 16, 17, 100, 336, 337, 341, 348, 349, 352, 353, 368)


@pytest.mark.parametrize("kind,mode", PAIRS)
def test_query_agrees_with_the_field_query_across_its_boundary(kind, mode):
    """The stage image takes the DXB slot: exactly the shapes ncde_stream_field_workspace_bytes accepts, refused with its bytes."""
    seen = set()
    for C in (1, 4, 5, 9):
        for H in GRID_H:
            for widths in ("HH=H", 24, 400):
                HH = H if widths == "HH=H" else widths
                rc, msg = query(field_problem(kind, mode, B=3, C=C, H=H, HH=HH, nl=2, interp=CUBIC))
                assert rc == linear_query(field_problem(kind, mode, B=3, C=C, H=H, HH=HH, nl=2)), (C, H, HH)
                need = plan_bytes(C, H, [HH, HH], mode != "matmul")
                assert (rc == 0) == (need <= 160 * 1024) and rc in (0, UNSUPPORTED), (C, H, HH, need)
                assert rc == 0 or (str(need) in msg and "LDS" in msg)
                seen.add(rc)
    assert seen == {0, UNSUPPORTED}


def test_lds_boundary_for_the_evaluate_input():
    assert query(field_problem("original", "evaluate", B=3, C=4, H=352, HH=352, nl=2, interp=CUBIC))[0] == 0
    rc, msg = query(field_problem("original", "evaluate", B=3, C=4, H=353, HH=353, nl=2, interp=CUBIC))
    assert rc == UNSUPPORTED and str(plan_bytes(4, 353, [353, 353], True)) in msg


def test_the_old_queries_still_refuse_the_five_pairs_at_cubic():
    from ncde_amd import _lib
    lib = _lib.lib()
    for kind, mode in PAIRS:
        p = field_problem(kind, mode, interp=CUBIC)
        assert lib.ncde_stream_hermite_workspace_bytes(ctypes.byref(p)) == UNSUPPORTED, (kind, mode)
        assert lib.ncde_stream_hermite_kernel_name(ctypes.byref(p)) is None
        assert lib.ncde_stream_field_workspace_bytes(ctypes.byref(p)) == INVALID, (kind, mode)
        assert lib.ncde_stream_field_kernel_name(ctypes.byref(p)) is None
        assert lib.ncde_stream_workspace_bytes(ctypes.byref(p)) == INVALID, (kind, mode)
        assert lib.ncde_stream_lowrank_workspace_bytes(ctypes.byref(p)) == UNSUPPORTED, (kind, mode)


def test_minimal_hermite_handle_on_cpu_tensors_takes_the_torch_step():
    from ncde_amd import unfused
    B, C = 3, 4
    model = se.make_model(7, C, 6, 2, 5, 2, "cubic_hermite", vector_field="minimal")
    x = se.dev(se.make_rows(71, 3, B, C), "cpu")
    unfused._WARNED.clear()
    h = model.online(B)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = torch.stack([h.step(x[k]) for k in range(x.size(0))])
    assert sum("unfused" in str(w.message) and "not fp32 on the GPU" in str(w.message) for w in rec) == 1, [str(w.message) for w in rec]
    assert h._route[("cpu", torch.float32)] is False and torch.isfinite(out).all() and h.count.tolist() == [3] * B
    p = h._problem()      # the handle's problem says cubic and carries the gate head: the new query accepts it
    assert p.interp == CUBIC and p.Wg and p.bg and query(p)[0] == 0
    assert h._kernel_entry(model.func.fused_spec()) == ("ncde_stream_field_hermite_workspace_bytes", "ncde_stream_step_field_hermite")
    gru = se.make_model(7, C, 6, 2, 5, 2, "cubic_hermite", vector_field="gru").online(B)      # pinned to the torch-op step
    assert gru._kernel_entry(gru.model.func.fused_spec()) is None
