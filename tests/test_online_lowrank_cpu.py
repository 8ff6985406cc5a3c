"""The low-rank step's C-ABI queries (ncde_stream_lowrank_workspace_bytes / ncde_stream_lowrank_kernel_name), which read the problem
only and need no device, and the route of a low-rank handle on CPU tensors."""
import ctypes
import warnings

import pytest
import torch

import stack_util as sk
import stream_edges as se

INVALID, UNSUPPORTED = -1, -2
LINEAR, CUBIC = 0, 1
NAMES = {LINEAR: b"ncde_stream_step_lowrank", CUBIC: b"ncde_stream_step_lowrank_hermite"}


def lowrank_problem(B=19, C=5, H=20, HH=15, nl=3, R=2, **kw):
    """stack_util.dummy_problem as a low-rank field: the rank in the top byte of flags, M_o in Wg / bg."""
    from ncde_amd import _lib
    p = sk.dummy_problem(B=B, C=C, H=H, HH=HH, nl=nl, **kw)
    p.field_kind, p.field_input = _lib.FIELD_KIND["lowrank"], _lib.FIELD_INPUT["matmul"]
    p.Wg, p.bg = 0x4000, 0x4100
    p.flags = _lib.FLAG_FIELD_RANK(R)
    return p


def query(p):
    from ncde_amd import _lib
    lib = _lib.lib()
    rc = lib.ncde_stream_lowrank_workspace_bytes(ctypes.byref(p))
    msg = (lib.ncde_last_error_string() or b"").decode()
    name = lib.ncde_stream_lowrank_kernel_name(ctypes.byref(p))
    assert (name is None) == (rc != 0) and (rc != 0 or name == NAMES[p.interp])
    return rc, msg


@pytest.mark.parametrize("interp", [LINEAR, CUBIC])
def test_query_accepts_both_paths_and_every_method(interp):
    for method in (0, 1, 2):
        for nl in (1, 3):
            assert query(lowrank_problem(interp=interp, method=method, nl=nl))[0] == 0
    assert query(lowrank_problem(interp=interp, C=5, R=5))[0] == 0      # R = C, above the ranks held in registers


def test_query_refuses():
    from ncde_amd import _lib
    for kind in ("original", "minimal", "gru"):
        p = lowrank_problem()
        p.field_kind = _lib.FIELD_KIND[kind]
        rc, msg = query(p)
        assert rc == UNSUPPORTED and "low-rank field only" in msg, (kind, msg)
    for mode in ("evaluate", "derivative"):
        p = lowrank_problem()
        p.field_input = _lib.FIELD_INPUT[mode]
        rc, msg = query(p)
        assert rc == UNSUPPORTED and "matmul input only" in msg, (mode, msg)
    for R in (0, 6):      # the batch family's range: 1 .. channels
        rc, msg = query(lowrank_problem(C=5, R=R))
        assert rc == INVALID and "rank %d" % R in msg, (R, msg)
    rc, msg = query(lowrank_problem(nl=0))
    assert rc == INVALID and "at least one inner layer" in msg, msg
    for interp in (LINEAR, CUBIC):
        p = lowrank_problem(interp=interp)
        p.layer_in[1] = p.layer_in[1] + 1
        rc, msg = query(p)
        assert rc == INVALID and "chain" in msg
        p = lowrank_problem(interp=interp)
        p.layer_in[0] = p.layer_in[0] + p.channels      # the chain starts at H: the field has no direct input
        rc, msg = query(p)
        assert rc == INVALID and "chain" in msg
        for gone in ("Wo", "bo", "Wg", "bg"):
            p = lowrank_problem(interp=interp)
            setattr(p, gone, None)
            rc, msg = query(p)
            assert rc == INVALID and "Wo/bo" in msg and "Wg/bg" in msg, (gone, msg)
        p = lowrank_problem(interp=interp)
        p.layer_W[2] = None
        rc, msg = query(p)
        assert rc == INVALID and "layer 2" in msg
        assert query(lowrank_problem(interp=interp, method=3))[0] == INVALID
    assert query(lowrank_problem(interp=2))[0] == INVALID      # quintic: not causal
    assert _lib.lib().ncde_stream_lowrank_workspace_bytes(None) == INVALID
    assert _lib.lib().ncde_stream_lowrank_kernel_name(None) is None


def test_the_step_refuses_a_bad_stream_before_it_launches():
    """What stream_launch rejects about NcdeStream, answered on the host: no device is touched (every pointer is a dummy)."""
    from ncde_amd import _lib
    lib = _lib.lib()

    def stream(**kw):
        s = _lib.NcdeStream()
        s.n_rows, s.x, s.x_stride_m, s.x_stride_b = 1, 0x100, 19 * 5, 5
        s.z, s.last_row, s.prev_dx, s.count, s.z_out = 0x200, 0x300, 0x400, 0x500, 0x600
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def step(p, s):
        rc = lib.ncde_stream_step_lowrank(ctypes.byref(p), None if s is None else ctypes.byref(s), None)
        return rc, (lib.ncde_last_error_string() or b"").decode()

    for interp in (LINEAR, CUBIC):
        p = lowrank_problem(interp=interp)
        assert step(p, None)[0] == INVALID
        for kw, token in ((dict(n_rows=0), "n_rows"), (dict(z=None), "NULL"), (dict(count=None), "NULL"), (dict(x_stride_b=4), "strides"),
                          (dict(z_out=None), "readout"), (dict(Wf=0x700, n_out=0), "readout")):
            rc, msg = step(p, stream(**kw))
            assert rc == INVALID and token in msg, (kw, msg)
    rc, msg = step(lowrank_problem(interp=LINEAR), stream(rectilinear=1, time_index=5))
    assert rc == INVALID and "Time index" in msg
    rc, msg = step(lowrank_problem(interp=CUBIC), stream(rectilinear=1))
    assert rc == INVALID and "rectilinear must be 0" in msg
    rc, msg = step(lowrank_problem(R=0), stream())      # the problem is judged first
    assert rc == INVALID and "rank 0" in msg


def plan_bytes(C, H, R, widths):
    """The LDS plan of the low-rank step (csrc/ncde_stream.hip), written out: five [Hp][16] images (stage input, K1, K2, KO, z), two
    [Dp][16] activations, five [Cp][16] (three dX/dt, last row, previous dX/dt), 48 words of flags, and PQ, the stacked heads'
    output, [ru16((H + C) R)][16]."""
    ru = lambda v, m: (v + m - 1) // m * m      # noqa: E731
    Dp = max([ru(H, 16)] + [ru(v, 16) for v in widths])
    return 4 * (5 * ru(H, 16) * 16 + 2 * Dp * 16 + 5 * ru(C, 4) * 16 + 48 + 16 * ru((H + C) * R, 16))


def lds_boundary(C, R, interp=LINEAR):
    """(last accepted H, first refused H, its status, its message) with HH = H, nl 2, found by the query."""
    last = None
    for H in range(1, 4096):
        rc, msg = query(lowrank_problem(B=3, C=C, H=H, HH=H, nl=2, R=R, interp=interp))
        if rc != 0:
            return last, H, rc, msg
        last = H
    raise AssertionError("no width refused")


@pytest.mark.parametrize("C,R", [(4, 1), (5, 3)])
def test_lds_boundary_by_the_query(C, R):
    last, first, rc, msg = lds_boundary(C, R)
    print("low-rank step, C %d, R %d, HH = H, nl 2: last accepted H %d (%d B), first refused H %d (%s)"
          % (C, R, last, plan_bytes(C, last, R, [last, last]), first, msg))
    assert rc == UNSUPPORTED and "B of LDS" in msg and first == last + 1
    need = plan_bytes(C, first, R, [first, first])
    assert str(need) in msg and need > 160 * 1024
    assert plan_bytes(C, last, R, [last, last]) <= 160 * 1024
    assert lds_boundary(C, R, CUBIC)[:3] == (last, first, rc)      # the Hermite image takes the DXB slot: the same plan
    if (C, R) == (4, 1):      # the two widths tests/test_online_lowrank_gpu.py steps
        assert (last, first) == (304, 305)


def test_plan_counts_the_widest_layer_and_the_stacked_rows():
    """Below the limit the query says nothing about the plan, so the restatement is held against it where each term decides: a wide
    inner layer and a large rank each push a shape over the limit that is accepted without them."""
    assert query(lowrank_problem(B=3, C=4, H=64, HH=64, nl=2, R=1))[0] == 0
    seen = set()
    for HH in (1056, 1057):      # 2 Dp 16 floats: HH 1056 fits, 1057 (Dp 1072) does not
        rc, msg = query(lowrank_problem(B=3, C=4, H=64, HH=HH, nl=2, R=1))
        need = plan_bytes(4, 64, 1, [HH, HH])
        assert (rc == 0) == (need <= 160 * 1024), (HH, need, msg)
        assert rc == 0 or str(need) in msg
        seen.add(rc)
    assert seen == {0, UNSUPPORTED}
    seen = set()
    for R in range(1, 65):      # 16 ru16((H + C) R) floats
        rc, msg = query(lowrank_problem(B=3, C=64, H=192, HH=64, nl=2, R=R))
        need = plan_bytes(64, 192, R, [64, 64])
        assert (rc == 0) == (need <= 160 * 1024), (R, need, msg)
        assert rc == 0 or str(need) in msg
        seen.add(rc)
    assert seen == {0, UNSUPPORTED}


def test_the_old_queries_still_refuse_the_low_rank_field():
    from ncde_amd import _lib
    lib = _lib.lib()
    for interp, fns in ((LINEAR, ("ncde_stream_workspace_bytes", "ncde_stream_field_workspace_bytes")),
                        (CUBIC, ("ncde_stream_hermite_workspace_bytes", "ncde_stream_field_hermite_workspace_bytes"))):
        for fn in fns:
            assert getattr(lib, fn)(ctypes.byref(lowrank_problem(interp=interp))) == UNSUPPORTED, fn
    arr = (ctypes.POINTER(_lib.NcdeProblem) * 1)(ctypes.pointer(lowrank_problem()))
    assert lib.ncde_stream_stack_workspace_bytes(arr, 1) == UNSUPPORTED
    assert lib.ncde_stream_kernel_name(ctypes.byref(lowrank_problem())) is None


@pytest.mark.parametrize("path", ["linear", "rectilinear", "cubic_hermite"])
def test_low_rank_handle_on_cpu_tensors_takes_the_torch_step(path):
    from ncde_amd import _lib, unfused
    B, C = 3, 5
    model = se.make_model(7, C, 6, 2, 5, 2, path, vector_field="low-rank", sparsity=0.5)
    x = se.dev(se.make_rows(71, 3, B, C), "cpu")
    unfused._WARNED.clear()
    h = model.online(B)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = torch.stack([h.step(x[k]) for k in range(x.size(0))])
    assert sum("unfused" in str(w.message) and "not fp32 on the GPU" in str(w.message) for w in rec) == 1, [str(w.message) for w in rec]
    assert h._route[("cpu", torch.float32)] is False and torch.isfinite(out).all() and h.count.tolist() == [3] * B
    p = h._problem()      # the handle's problem carries the rank and M_o: the low-rank query accepts it
    assert p.flags >> 24 == 3 == model.func.rank and p.Wg and p.bg and p.interp == (CUBIC if path == "cubic_hermite" else LINEAR)
    assert query(p)[0] == 0
    assert h._kernel_entry(model.func.fused_spec()) == ("ncde_stream_lowrank_workspace_bytes", "ncde_stream_step_lowrank")
