"""Checks of a fused online step that do not depend on the field, shared by tests/test_online_lowrank_gpu.py and
tests/test_online_field_hermite_gpu.py.  Helper only: no test functions.

A model is a function build(device) (built on the CPU under its seed, then moved).  The reference is the batch model in fp64 on the
CPU: stream_ref.prefix_reference on a linear or rectilinear path, hermite_util.batch_reference on the Hermite path (every stream
receives every row there).  The bound is su.TIGHT_Z = 2e-5 of max |ref|, for z and the readout at every step."""
import ctypes
import warnings

import numpy as np
import torch

import hermite_util as hu
import stream_edges as se
import stream_ref as sr
import stream_util as su

F32 = torch.float32
INVALID, UNSUPPORTED = -1, -2      # NcdeStatus (include/ncde_hip.h)


def reference(key, build, rows, init, ti=0, received=None):
    """(z, out) in fp64: computed once per key, shared, never modified."""
    def make():
        model = build("cpu")
        if model.interpolation == "cubic_hermite":
            assert received is None
            return hu.batch_reference(model, rows, None, init)
        return sr.prefix_reference(model, rows, received, None, init, ti)
    return se.reference(key, make)


def steps(model, x, init, ti=0):
    """One call per row on the fused route (any warning is an error) -> (outs, zs) as numpy, the handle."""
    with se.stepping("cuda"):
        h = model.online(x.size(1), initial_value_if_nan=init, time_index=ti)
        outs, zs, _ = su.step_through(h, x, None, quiet=False)
    return outs, zs, h


def worst(outs, zs, z_ref, o_ref, what):
    top = 0.0
    for k in range(outs.shape[0]):
        e_out, e_z = se.err(outs[k], o_ref[k]), se.err(zs[k], z_ref[k])
        print("%s step %d: out %.3e z %.3e" % (what, k, e_out, e_z))
        assert e_out <= su.TIGHT_Z and e_z <= su.TIGHT_Z, (what, k, e_out, e_z)
        top = max(top, e_out, e_z)
    assert np.abs(z_ref[-1] - z_ref[0]).max() > 1e-3      # the state moved: not a vacuous pass
    print("%s: worst %.3e" % (what, top))
    return top


def check(name_fn, expect, what, key, build, rows, init, ti=0):
    """A model on `rows` through the handle against the fp64 reference of `key`; name_fn(problem) is the kernel-name query."""
    z_ref, o_ref = reference(key, build, rows, init, ti)
    outs, zs, h = steps(build("cuda"), se.dev(rows, "cuda"), init, ti)
    assert name_fn(ctypes.byref(h._problem())) == expect
    assert h.count.cpu().tolist() == [rows.shape[0]] * rows.shape[1]
    return worst(outs, zs, z_ref, o_ref, what), zs, z_ref


def state_equal(a, b, where):
    for k in a.state_dict():
        assert torch.equal(a.state_dict()[k], b.state_dict()[k]), (where, k)


def rows_in_one_call_and_interleaved_halves(model, x, init):
    n, B = x.size(0), x.size(1)
    with se.stepping("cuda"):
        h1, h2 = model.online(B, initial_value_if_nan=init), model.online(B, initial_value_if_nan=init)
        many = torch.cat([h1.step(x[0])[None], h1.step(x[1:])])      # m = n - 1 rows in one launch
        singles = torch.stack([h2.step(x[k]) for k in range(n)])
        assert torch.equal(many, singles)
        state_equal(h1, h2, "m rows in one call")
        for half in (slice(0, None, 2), slice(1, None, 2)):      # streams of one tile spread over two tiles and the reverse
            xh = x[:, half].contiguous()
            hh = model.online(xh.size(1), initial_value_if_nan=init)
            assert torch.equal(torch.stack([hh.step(xh[k]) for k in range(n)]), singles[:, half])
            for k in hh.state_dict():
                assert torch.equal(hh.state_dict()[k], h2.state_dict()[k][half]), k
    assert (singles[-1] - singles[0]).abs().max() > 1e-3


def masks_and_a_tile_of_mixed_counts(build, key, what):
    """The staggered schedule of tests/stream_edges.py: at call 3 one tile holds streams with 0, 1 and >= 2 rows behind them next to
    streams that receive nothing.  Every stream answers what it answers alone in a handle of batch 1, non-receivers keep their state,
    and -- after an unmasked first call -- the [m, B] mask in ONE launch equals the masked single calls.  On a linear or rectilinear
    path every call is also held against the fp64 reference (the Hermite reference has no masks)."""
    s = se.STAG
    x_np, A = se.staggered_rows()
    se.assert_schedule(A)
    model = build("cuda")
    ref = None if model.interpolation == "cubic_hermite" else reference(key, build, x_np, s["init"], 0, A)
    x, act = se.dev(x_np, "cuda"), se.dev(A, "cuda")
    with se.stepping("cuda"):
        h = model.online(s["B"], initial_value_if_nan=s["init"])
        alone = [model.online(1, initial_value_if_nan=s["init"]) for _ in range(s["B"])]
        for j in range(s["calls"]):
            before = h.state_dict()
            out = h.step(x[j], active=act[j])
            after = h.state_dict()
            for k in before:
                assert torch.equal(before[k][~act[j]], after[k][~act[j]]), (j, k)
            if ref is not None:
                e_out, e_z = se.err(out, ref[1][j]), se.err(h.z, ref[0][j])
                print("staggered %s call %d: out %.3e z %.3e" % (what, j, e_out, e_z))
                assert e_out <= su.TIGHT_Z and e_z <= su.TIGHT_Z, (j, e_out, e_z)
            if j == 0:
                z_first = h.z[0].clone()
            for b in np.nonzero(A[j])[0]:
                ob = alone[b].step(x[j, b:b + 1])
                assert torch.equal(ob[0], out[b]) and all(torch.equal(alone[b].state_dict()[k][0], after[k][b]) for k in after), (j, b)
        assert h.count.cpu().tolist() == A.sum(axis=0).tolist()
        assert (h.z[0] - z_first).abs().max() > 1e-3      # stream 0 (a row at every call) moved
        # the [m, B] mask in one launch
        x_np, A = se.staggered_rows(first_all=True)
        x, act = se.dev(x_np, "cuda"), se.dev(A, "cuda")
        h1, h2 = model.online(s["B"], initial_value_if_nan=s["init"]), model.online(s["B"], initial_value_if_nan=s["init"])
        first = h1.step(x[0])
        assert h1._may_init is False
        many = h1.step(x[1:], active=act[1:])
        singles = [h2.step(x[0])] + [h2.step(x[j], active=act[j]) for j in range(1, s["calls"])]
        assert torch.equal(torch.cat([first[None], many]), torch.stack(singles))
        state_equal(h1, h2, "row mask in one launch")


def state_dict_round_trip_and_a_refused_call(lib, entry, model, x, init):
    with se.stepping("cuda"):
        B = x.size(1)
        ha, hb = model.online(B, initial_value_if_nan=init), model.online(B, initial_value_if_nan=init)
        ha.step(x[:3])
        saved = ha.state_dict()
        hb.load_state_dict(saved)
        assert torch.equal(ha.step(x[3:]), hb.step(x[3:]))
        state_equal(ha, hb, "round trip")
        # a refusal through the ABI: nothing is launched, the state keeps its bits
        before = ha.state_dict()
        p = ha._problem()
        st, out, keep = ha._stream_args(x[:1], None, 1)
        st.n_rows = 0
        rc = getattr(lib, entry)(ctypes.byref(p), ctypes.byref(st), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == INVALID and b"n_rows" in lib.ncde_last_error_string()
        for k in before:
            assert torch.equal(before[k], ha.state_dict()[k]), k


def against_the_torch_step(model, x, init, what):
    """The fused step against the torch-op step on the same tensors (the route the handle took before the kernel existed)
    -> (zs of the kernel, the worst relative gap)."""
    _, zs, h = steps(model, x, init)
    ht = model.online(x.size(1), initial_value_if_nan=init)
    ht._route[("cuda", F32)] = False
    _, z_torch, _ = su.step_through(ht, x, None)
    gap = max(se.err(zs[k], z_torch[k]) for k in range(x.size(0)))
    print("%s: vs the torch-op step %.3e" % (what, gap))
    assert gap <= su.TIGHT_Z, gap
    assert np.abs(z_torch[-1] - z_torch[0]).max() > 1e-3
    return zs, h


def torch_step_behind_one_lds_warning(model, rows, init, z_ref, o_ref, what):
    from ncde_amd import unfused
    unfused._WARNED.clear()
    h = model.online(rows.shape[1], initial_value_if_nan=init)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        outs, zs, _ = su.step_through(h, se.dev(rows, "cuda"), None, quiet=False)
    msgs = [str(w.message) for w in rec]
    assert len(msgs) == 1 and "unfused" in msgs[0] and "online step" in msgs[0] and "LDS" in msgs[0], msgs
    return worst(outs, zs, z_ref, o_ref, what)
