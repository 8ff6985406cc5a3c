"""The field step's C-ABI queries (ncde_stream_field_workspace_bytes / ncde_stream_field_kernel_name), which read the problem only
and need no device, and the route of a minimal-gated handle on CPU tensors.

The five pairs of ncde_stream_step_field: the original field with the evaluate / derivative input, the minimal-gated field with
the matmul / evaluate / derivative input."""
import ctypes
import warnings

import pytest
import torch

import stack_util as sk
import stream_edges as se

INVALID, UNSUPPORTED = -1, -2
PAIRS = [("original", "evaluate"), ("original", "derivative"), ("minimal", "matmul"), ("minimal", "evaluate"), ("minimal", "derivative")]


def field_problem(kind, mode, B=19, C=5, H=20, HH=15, nl=3, **kw):
    """stack_util.dummy_problem with the field's enums, the gate head of a gated field and a layer chain that starts at d0."""
    from ncde_amd import _lib
    p = sk.dummy_problem(B=B, C=C, H=H, HH=HH, nl=nl, **kw)
    p.field_kind, p.field_input = _lib.FIELD_KIND[kind], _lib.FIELD_INPUT[mode]
    if nl and mode != "matmul":
        p.layer_in[0] = H + C
    if kind != "original":
        p.Wg, p.bg = 0x4000, 0x4100
    if kind == "gru":
        p.Wr, p.br = 0x5000, 0x5100
    if kind == "lowrank":
        p.flags = _lib.FLAG_FIELD_RANK(2)
    return p


def query(p):
    from ncde_amd import _lib
    lib = _lib.lib()
    rc = lib.ncde_stream_field_workspace_bytes(ctypes.byref(p))
    msg = (lib.ncde_last_error_string() or b"").decode()
    name = lib.ncde_stream_field_kernel_name(ctypes.byref(p))
    assert (name == b"ncde_stream_step_field") == (rc == 0) and (name is None) == (rc != 0)
    return rc, msg


@pytest.mark.parametrize("kind,mode", PAIRS)
@pytest.mark.parametrize("nl", [0, 3])
def test_query_accepts_the_five_pairs(kind, mode, nl):
    assert query(field_problem(kind, mode, nl=nl))[0] == 0
    for method in (0, 1, 2):
        assert query(field_problem(kind, mode, nl=nl, method=method))[0] == 0


def test_query_refuses():
    for kind in ("gru", "lowrank"):
        for mode in ("matmul", "evaluate", "derivative"):
            rc, msg = query(field_problem(kind, mode))
            assert rc == UNSUPPORTED and msg, (kind, mode)
    rc, msg = query(field_problem("original", "matmul"))
    assert rc == UNSUPPORTED and "ncde_stream_step" in msg and "ncde_stream_step_field" not in msg
    for kind, mode in PAIRS:
        assert query(field_problem(kind, mode, interp=1))[0] == INVALID      # cubic: the Hermite path has no field step
        assert query(field_problem(kind, mode, method=3))[0] == INVALID
        p = field_problem(kind, mode)
        p.layer_in[1] = p.layer_in[1] + 1
        rc, msg = query(p)
        assert rc == INVALID and "chain" in msg
        p = field_problem(kind, mode)
        p.layer_in[0] = p.layer_in[0] + (1 if mode == "matmul" else -p.channels)      # (a direct input: the matmul chain, from H)
        rc, msg = query(p)
        assert rc == INVALID and "chain" in msg, (kind, mode)
        if kind != "original":
            for gone in ("Wg", "bg"):
                p = field_problem(kind, mode)
                setattr(p, gone, None)
                rc, msg = query(p)
                assert rc == INVALID and "Wg" in msg, (kind, mode, gone)
    from ncde_amd import _lib
    assert _lib.lib().ncde_stream_field_workspace_bytes(None) == INVALID


def test_the_linear_step_still_refuses_the_five_pairs():
    from ncde_amd import _lib
    lib = _lib.lib()
    for kind, mode in PAIRS:
        p = field_problem(kind, mode)
        assert lib.ncde_stream_workspace_bytes(ctypes.byref(p)) == UNSUPPORTED, (kind, mode)
        assert lib.ncde_stream_kernel_name(ctypes.byref(p)) is None
        p.interp = 1
        assert lib.ncde_stream_hermite_workspace_bytes(ctypes.byref(p)) == UNSUPPORTED, (kind, mode)


def plan_bytes(C, H, widths, direct):
    """The LDS plan of the field step (csrc/ncde_stream.hip), written out: three [Dp][16] images (field input, two activations),
    four [Hp][16] (K1, K2, KO, z), seven [Cp][16] (three dX/dt, two start rows, last row, previous dX/dt), 48 words of flags."""
    ru = lambda v, m: (v + m - 1) // m * m      # noqa: E731
    d0 = H + C if direct else H
    Dp = max([ru(H, 16), ru(d0, 16)] + [ru(v, 16) for v in widths])
    return 4 * (3 * Dp * 16 + 4 * ru(H, 16) * 16 + 7 * ru(C, 4) * 16 + 48)


def lds_boundary():
    """(last accepted H, first refused H, its message) for the evaluate input with C 4, HH = H, nl 2, found by the query."""
    last = None
    for H in range(1, 4096):
        rc, msg = query(field_problem("original", "evaluate", B=3, C=4, H=H, HH=H, nl=2))
        if rc != 0:
            return last, H, rc, msg
        last = H
    raise AssertionError("no width refused")


def test_lds_boundary_by_the_query():
    last, first, rc, msg = lds_boundary()
    print("field step, evaluate, C 4, HH = H, nl 2: last accepted H %d (%d B), first refused H %d (%s)"
          % (last, plan_bytes(4, last, [last, last], True), first, msg))
    assert rc == UNSUPPORTED and "B of LDS" in msg and first == last + 1
    need = plan_bytes(4, first, [first, first], True)
    assert str(need) in msg and need > 160 * 1024
    assert plan_bytes(4, last, [last, last], True) <= 160 * 1024
    for kind, mode in PAIRS:      # the plan depends on the input's width only: every pair is held at the last width
        assert query(field_problem(kind, mode, B=3, C=4, H=last, HH=last, nl=2))[0] == 0, (kind, mode)


def test_minimal_handle_on_cpu_tensors_takes_the_torch_step():
    from ncde_amd import unfused
    B, C = 3, 4
    model = se.make_model(7, C, 6, 2, 5, 2, "linear", vector_field="minimal")
    x = se.dev(se.make_rows(71, 3, B, C), "cpu")
    unfused._WARNED.clear()
    h = model.online(B)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = torch.stack([h.step(x[k]) for k in range(x.size(0))])
    assert sum("unfused" in str(w.message) and "not fp32 on the GPU" in str(w.message) for w in rec) == 1, [str(w.message) for w in rec]
    assert h._route[("cpu", torch.float32)] is False and torch.isfinite(out).all() and h.count.tolist() == [3] * B
    p = h._problem()      # the handle's problem carries the gate head: the field step's query accepts it
    assert p.Wg and p.bg and query(p)[0] == 0
