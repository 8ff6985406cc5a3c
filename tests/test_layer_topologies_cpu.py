"""The expectations of the layer-topology cases (tests/layer_topologies.py), pinned on the CPU before a GPU kernel is judged by them:
the oracle's `acc` accumulation over repeated tensors and libncde_cpu.so's parameter slots had only ever seen the reference's three
stacks ([W0], [W0, W1], [W0, W1, W1, ...]).

  (a) oracle (fp32, hand-written VJPs) against torch autograd in fp64 through the same fixed-step solve;
  (b) oracle against the C++ restatement behind the C ABI (forward, ncde_adjoint, ncde_backward);
  (c) a tied tensor's gradient = the sum of the gradients of equal-valued un-tied copies, one per layer: exact algebra, so an
      expectation from this oracle FAILS a kernel that drops (or overwrites) one layer's share of a tied tensor.
"""
import numpy as np
import pytest

import golden_util as gu
import layer_topologies as lt
from test_gpu_parity import TIGHT_G, TIGHT_Z      # (importing that module runs nothing on a GPU)

C, H, HH, B, L = 3, 8, 8, 5, 4
SETTINGS = [("linear", "rk4", True), ("cubic", "midpoint", False)]
SPECS = list(lt.TOPOLOGIES) + [(w[0], tuple(w[1])) for w in lt.WIDTHS]      # a name, or (H, widths)
_IDS = list(lt.TOPOLOGIES) + [lt.widths_id(w) for w in lt.WIDTHS]


def _case(spec, setting):
    interp, method, seq = setting
    seed = 300 + 7 * SETTINGS.index(setting)
    if isinstance(spec, str):
        return lt.cached_case(spec, C, H, HH, interp, method, seq, B, L, seed)
    return lt.cached_case(spec[1], C, spec[0], None, interp, method, seq, B, L, seed)      # a WIDTHS stack brings its own H


def _cpu(case):
    import cpu_lib_util
    m = case["meta"]
    return cpu_lib_util.CpuCase(case["coeffs"], m["kind"], case["z0"], case["params"], case["layers"], m["method"], m["sequence"])


def _fp32_distance_from_fp64(case):
    """-> {route: worst relative error of its discrete-backward gradients (dz0 and every parameter) against fp64 autograd}.  The
    restatement runs on ONE thread here: its per-thread partial sums are added in arrival order, and a yardstick must not move from
    run to run."""
    import cpu_lib_util
    m, ex = case["meta"], case["expect"]
    _z, dz64, g64 = lt.autograd64(case, ex["grad_out"])
    cpu = _cpu(case)
    prev = cpu_lib_util.cpu_lib().ncde_cpu_set_threads(1)
    try:
        _zc, rec = cpu.forward(record=True)
        cdz0, cg = cpu.backward(rec, ex["grad_out"], discrete=True)
    finally:
        cpu_lib_util.cpu_lib().ncde_cpu_set_threads(prev)
    return {"oracle": max([gu.relerr(ex["bp_dz0"], dz64)] + [gu.relerr(ex["bp_d" + n], g64[n]) for n in m["param_names"]]),
            "restatement": max([gu.relerr(cdz0, dz64)] + [gu.relerr(cg[n], g64[n]) for n in m["param_names"]])}


_YARD = {}


def _yardstick(spec, setting):
    """Both fp32 routes against fp64 on `ref_shared3`, computed once per size and setting.  Named stacks: at the file's sizes,
    (H, HH) = (8, 8), as they run.  A WIDTHS stack brings its own H and widths (up to 47 and 128 against 8), and fp32 rounding grows
    with the length of the dot products: measured at (8, 8) the yardstick would say 7e-7 .. 1e-6 about a computation whose own
    rounding is 2e-6 (H47_93x15x47 sits at 1.65e-6).  DEVIATION, stated: for a WIDTHS stack ref_shared3 is measured at that stack's
    H and its largest width, so that yardstick and stack round alike; the factor 4 stays."""
    interp, method, seq = setting
    h, hh = (H, HH) if isinstance(spec, str) else (spec[0], max(spec[1]))
    if (h, hh, setting) not in _YARD:
        _YARD[(h, hh, setting)] = _fp32_distance_from_fp64(lt.cached_case("ref_shared3", C, h, hh, interp, method, seq, B, L, 300 + 7 * SETTINGS.index(setting)))
    return _YARD[(h, hh, setting)]


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "%s_%s_%s" % (s[0], s[1], "seq" if s[2] else "final"))
@pytest.mark.parametrize("spec", SPECS, ids=_IDS)
def test_oracle_discrete_backward_vs_fp64_autograd(spec, setting):
    """(a) orc.solve_discrete_backward (fp32) against torch autograd in fp64 through orc.solve_forward on the same stack; the forward
    too.  The bound is the fp32 rounding of this computation, not a constant: both fp32 routes (the oracle, the C++ restatement)
    are run against the same fp64 result on `ref_shared3` -- the stack on which the oracle is pinned to the reference -- at the sizes
    of the stack under test, and every stack is allowed 4 x the larger of the two errors (same sizes, same number of steps; the
    deepest stack has 8 / 3 of its layers).  Measured, relative, max over dL/dz0 and every parameter: ref_shared3 at (H, HH) = (8, 8)
    oracle 2.06e-7 / restatement 3.47e-7 for linear + rk4 (bound 1.39e-6), 1.82e-7 / 3.30e-7 for cubic + midpoint (bound 1.32e-6); the
    other named stacks 2e-8 .. 5.8e-7.  WIDTHS stacks (yardstick at their own sizes, see _yardstick): yardstick 1.9e-7 .. 5.4e-7, the
    stacks 4.6e-8 .. 1.65e-6 (H47_93x15x47, cubic: b1 1.65e-6 against 2.14e-6; it would miss the (8, 8) yardstick's 1.32e-6)."""
    case = _case(spec, setting)
    yard = _yardstick(spec, setting)
    bound = 4.0 * max(yard.values())
    m, ex = case["meta"], case["expect"]
    z64, dz64, g64 = lt.autograd64(case, ex["grad_out"])
    errs = {"z": gu.relerr(ex["z_out"], z64), "dz0": gu.relerr(ex["bp_dz0"], dz64)}
    errs.update({n: gu.relerr(ex["bp_d" + n], g64[n]) for n in m["param_names"]})
    print(m["topology"], setting, "yardstick", {k: "%.2e" % v for k, v in yard.items()}, {k: "%.2e" % v for k, v in errs.items()})
    assert sorted(g64) == sorted(m["param_names"])       # every tensor of the case is in the stack, none twice
    assert bound <= TIGHT_G                              # the yardstick itself is fp32 rounding
    assert all(v <= bound for v in errs.values()), (bound, errs)


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "%s_%s_%s" % (s[0], s[1], "seq" if s[2] else "final"))
@pytest.mark.parametrize("spec", SPECS, ids=_IDS)
def test_oracle_vs_cpp_restatement(spec, setting):
    """(b) libncde_cpu.so -- forward, recorded forward, ncde_adjoint on the oracle's z_out, ncde_backward on the oracle's stage
    record -- against the oracle, at the tight bounds of the GPU suite."""
    case = _case(spec, setting)
    m, ex = case["meta"], case["expect"]
    cpu = _cpu(case)
    z = cpu.forward()
    zr, rec = cpu.forward(record=True)
    assert np.array_equal(z, zr)
    assert gu.relerr(z, ex["z_out"]) <= TIGHT_Z
    assert gu.relerr(rec.reshape(case["stage_record"].shape), case["stage_record"]) <= TIGHT_Z
    for prefix, src, disc in (("", ex["z_out"], False), ("bp_", case["stage_record"], True)):
        dz0, g = cpu.backward(src, ex["grad_out"], discrete=disc)
        errs = {"dz0": gu.relerr(dz0, ex[prefix + "dz0"])}
        errs.update({n: gu.relerr(g[n], ex[prefix + "d" + n]) for n in m["param_names"]})
        assert all(v <= TIGHT_G for v in errs.values()), (prefix, errs)


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "%s_%s_%s" % (s[0], s[1], "seq" if s[2] else "final"))
@pytest.mark.parametrize("spec", lt.TIED)
def test_tied_gradient_is_the_sum_over_untied_copies(spec, setting):
    """(c) for the oracle (continuous adjoint and discrete backward) and for the C++ restatement: dL/d(tied tensor) equals the sum
    over the layers that use it of dL/d(that layer's own equal-valued copy); and every single share is non-negligible, so dropping
    one is visible at the bound."""
    import ncde_oracle as orc
    case = _case(spec, setting)
    m, ex = case["meta"], case["expect"]
    un, origin = lt.untied(case)
    field, ctl = gu.oracle_field(un), orc.Control(un["coeffs"], m["kind"])
    names = un["meta"]["param_names"]
    _, gp = orc.solve_adjoint(ctl, field, ex["z_out"], ex["grad_out"], m["method"], m["sequence"])
    _, bgp = orc.solve_discrete_backward(ctl, field, un["z0"], ex["grad_out"], m["method"], m["sequence"])
    cpu = _cpu(un)
    _, cg = cpu.backward(ex["z_out"], ex["grad_out"], discrete=False)
    _, cbg = cpu.backward(case["stage_record"], ex["grad_out"], discrete=True)
    for prefix, parts in (("", dict(zip(names, (g.numpy() for g in gp)))), ("bp_", dict(zip(names, (g.numpy() for g in bgp)))),
                          ("", cg), ("bp_", cbg)):
        total = lt.sum_over_copies(parts, origin, m["param_names"])
        for n in m["param_names"]:
            assert gu.relerr(total[n], ex[prefix + "d" + n]) <= TIGHT_G, (prefix, n, gu.relerr(total[n], ex[prefix + "d" + n]))
            copies = [c for c, o in origin.items() if o == n]
            for c in copies if len(copies) > 1 else []:      # the expectation without this layer's share misses the bound by far
                assert gu.relerr(total[n] - parts[c], ex[prefix + "d" + n]) >= 100 * TIGHT_G, (prefix, n, c)


def test_names_follow_unique_params_order():
    """param_names of a case = Field.unique_params() order of the oracle = FieldSpec.unique_params() order of the package."""
    import torch
    from ncde_amd import solver
    for spec in SPECS:
        case = lt.bare_case(spec, C, H, HH, "linear", "rk4", False, 2, 3, 1) if isinstance(spec, str) else \
            lt.bare_case(list(spec[1]), C, spec[0], None, "linear", "rk4", False, 2, 3, 1)
        field = gu.oracle_field(case)
        t = {id(v): k for k, v in zip(case["meta"]["param_names"], field.unique_params())}
        assert len(t) == len(case["params"]) == len(case["meta"]["param_names"])
        for (w, b), (tw, tb) in zip(case["layers"], field.layers):
            assert t[id(tw)] == w and t[id(tb)] == b
        q = {k: torch.nn.Parameter(torch.from_numpy(v)) for k, v in case["params"].items()}
        fs = solver.FieldSpec([(q[w], q[b]) for w, b in case["layers"]], q["Wo"], q["bo"])
        assert [k for p_ in fs.unique_params() for k, v in q.items() if v is p_] == case["meta"]["param_names"]
