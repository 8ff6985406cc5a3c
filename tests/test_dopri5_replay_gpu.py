"""The adaptive dopri5 kernels on designed, irregular step sequences against the fp64 oracle (tests/dopri5_cases.py): every kernel set of
the three entry points -- fused attempt kernels (H32 and H64 forward sets, fused adjoint, fused taped sweep), the per-launch kernels and
the routes that mix them -- replays a list with rejects, dt from 2^-5 to 3.5, steps over three knots and steps holding 0 .. 5 outputs,
on the default grid and on a user knot grid.  Bars: the project's TIGHT_Z (z) and E2E_G (every gradient), |delta| / max |ref|; the fp32
oracle itself lies within a quarter of them (tests/test_dopri5_replay_cpu.py).  Each test prints its errors before it asserts."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import dopri5_cases as dc

pytestmark = pytest.mark.gpu


def _control(a):
    import ncde_amd
    coeffs = torch.from_numpy(a["coeffs"]).cuda()
    kn = None if a["knots"] is None else torch.from_numpy(a["knots"]).cuda()
    return (ncde_amd.LinearInterpolation if a["interp"] == "linear" else ncde_amd.NaturalCubicSpline)(coeffs, t=kn)


def _solve(a, adjoint):
    """cdeint on the case with its lists replayed and traced, and the backward -> dict(z_out, dz0, grads, trace_fwd, trace_bwd, nfe_fwd,
    nfe_bwd, stats{forward / backward: (nfe, accepted, rejected) as the library reported them}).  Any warning is an error: the fused
    route emits none."""
    import gpu_util
    import ncde_amd
    from ncde_amd import solver
    func = gpu_util.CaseField(a["params"], a["layers"], "cuda")
    z0 = torch.from_numpy(a["z0"]).cuda().requires_grad_(True)
    real, seen = solver._dopri5_call, {}

    def spy(name, cfg, *args, **kw):
        seen["cfg"] = cfg
        return real(name, cfg, *args, **kw)
    solver._dopri5_call = spy
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            out = ncde_amd.cdeint(_control(a), func, z0, torch.from_numpy(a["t"]).cuda(), adjoint=adjoint, method="dopri5", rtol=dc.RTOL,
                                  atol=dc.ATOL, kernel_flags=a["flags"], options={"first_step": a["fwd"][0][0], "_replay": a["fwd"], "_trace": 256},
                                  adjoint_options={"first_step": a["bwd"][0][0], "_replay": a["bwd"], "_trace": 256})
            res = {"z_out": out.detach().cpu().numpy(), "nfe_fwd": func.nfe, "trace_fwd": np.array(func.dopri5_trace)}
            (out * torch.from_numpy(a["grad_out"]).cuda()).sum().backward()
            torch.cuda.synchronize()
    finally:
        solver._dopri5_call = real
    cfg = seen["cfg"]
    res.update(dz0=z0.grad.cpu().numpy(), grads={n: func.p[n].grad.cpu().numpy() for n in a["names"]}, nfe_bwd=func.nfe - res["nfe_fwd"],
               trace_bwd=np.array(func.dopri5_trace_backward) if adjoint else None,
               stats={k: cfg.get("stats_" + k) for k in ("forward", "backward")})
    return res


def _grads(res):
    return {"dz0": res["dz0"], **res["grads"]}


def _same_rows(trace, rows, t_start):
    """The kernel's trace against the list: dt and the accept flag of every row, and t0 -- the exact sum of the accepted dt so far."""
    assert trace.shape == (len(rows), 4), (trace.shape, len(rows))
    t0 = t_start
    for got, (dt, acc) in zip(trace, rows):
        assert got[0] == t0 and got[1] == dt and got[2] == float(acc), (got, t0, dt, acc)
        if acc:
            t0 += dt


@pytest.mark.parametrize("cid", dc.case_ids())
def test_dopri5_designed_sequence_vs_fp64_oracle(cid, gpu_lib):
    import gpu_util
    from ncde_amd import _lib, solver
    a, ref = dc.arrays(cid), dc.reference(cid)
    n_acc, n_rej = sum(r[1] for r in a["fwd"]), sum(1 - r[1] for r in a["fwd"])
    # the route
    func = gpu_util.CaseField(a["params"], a["layers"], "cuda")
    prob = solver.build_problem(torch.from_numpy(a["coeffs"]).cuda(), a["interp"], torch.from_numpy(a["z0"]).cuda(), func.fused_spec(), "rk4",
                                _lib.OUT_INTERVAL, a["flags"])
    kn = [(_lib.lib().ncde_dopri5_kernel_name(ctypes.byref(prob), k) or b"?").decode() for k in (0, 1, 2)]
    assert all(k.startswith(want) for k, want in zip(kn, a["route"])), (kn, a["route"])
    # 1. forward (no gradient asked for: the plain solve)
    import ncde_amd
    func = gpu_util.CaseField(a["params"], a["layers"], "cuda")
    with torch.no_grad():
        out = ncde_amd.cdeint(_control(a), func, torch.from_numpy(a["z0"]).cuda(), torch.from_numpy(a["t"]).cuda(), adjoint=True, method="dopri5",
                              rtol=dc.RTOL, atol=dc.ATOL, kernel_flags=a["flags"],
                              options={"first_step": a["fwd"][0][0], "_replay": a["fwd"], "_trace": 256})
    fwd = {"z_out": out.cpu().numpy()}
    # 2. adjoint=True, both lists; 3. adjoint=False, the forward list
    adj, tape = _solve(a, True), _solve(a, False)
    errs = dc.errors({"z_out": fwd["z_out"], "adj": _grads(adj), "tape": _grads(tape)}, ref)
    errs["z_adj"], errs["z_tape"] = dc.errors(adj, ref)["z"], dc.errors(tape, ref)["z"]
    print("dopri5-replay %s %s | z %.2e adj %.2e tape %.2e |" % ((cid, kn[0].split("<")[0] + "/" + kn[1].split("<")[0]) + dc.worst(errs)),
          " ".join("%s %.1e" % kv for kv in errs.items()))
    _same_rows(np.array(func.dopri5_trace), a["fwd"], a["t"][0])
    assert func.nfe == 1 + 6 * len(a["fwd"]) == ref["nfe_fwd"]
    for r in (adj, tape):
        _same_rows(r["trace_fwd"], a["fwd"], a["t"][0])
        assert r["nfe_fwd"] == ref["nfe_fwd"]
        assert r["stats"]["forward"] == (ref["nfe_fwd"], n_acc, n_rej), r["stats"]      # what the library reports: the list's counts
    assert ref["steps_fwd"] == (n_acc, n_rej)
    assert adj["stats"]["backward"] == (ref["nfe_bwd"],) + ref["steps_bwd"] and tape["stats"]["backward"] is None, (adj["stats"], tape["stats"])
    assert np.array_equal(adj["trace_fwd"][:, :3], ref["trace_fwd"]) and np.array_equal(adj["trace_bwd"][:, :3], ref["trace_bwd"])
    assert adj["nfe_bwd"] == ref["nfe_bwd"]
    assert tape["nfe_bwd"] == 0                                   # the taped sweep evaluates no vector field the reference counts
    assert fwd["z_out"].shape == ref["z_out"].shape
    assert errs["z"] <= dc.TIGHT_Z and errs["z_adj"] <= dc.TIGHT_Z and errs["z_tape"] <= dc.TIGHT_Z, errs
    assert all(v <= dc.E2E_G for k, v in errs.items() if not k.startswith("z")), errs


@pytest.mark.parametrize("cid", ["h32-Cc-end-B21", "h32_pad_nl1-A-early-B21"])
def test_dopri5_designed_sequence_on_the_fused_route_is_reproducible(cid, gpu_lib):
    """The fused attempt kernels twice on one case: bit-identical outputs and gradients, adjoint=True and adjoint=False."""
    a = dc.arrays(cid)
    assert a["route"][1] == "ncde_dpf_adj"
    for adjoint in (True, False):
        r1, r2 = _solve(a, adjoint), _solve(a, adjoint)
        assert np.array_equal(r1["z_out"], r2["z_out"]) and np.array_equal(r1["dz0"], r2["dz0"]), adjoint
        assert all(np.array_equal(r1["grads"][n], r2["grads"][n]) for n in a["names"]), adjoint
        assert np.isfinite(r1["dz0"]).all()
