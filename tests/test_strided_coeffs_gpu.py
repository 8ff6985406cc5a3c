"""Every kernel family on non-contiguous control-path coefficients.

NcdeProblem takes the control path as a pointer and two element strides (include/ncde_hip.h), the Python host forwards whatever
strides torch gives it, and every kernel family has its own copy of the address arithmetic (staging blocks, one-row-ahead prefetch,
zero-padded channel counts, plan-walking reads).  Each test here runs ONE call twice -- on a view carved out of a NaN-filled buffer
(tests/strided_views.py, pinned on the CPU by tests/test_strided_coeffs_cpu.py) and on `view.contiguous()` -- and asserts

  (a) the kernel name is the same for both and is the one the row expects: dispatch does not depend on strides;
  (b) every output (z_out, dz0, every parameter gradient) is finite and BIT-IDENTICAL between the two: the arithmetic does not depend on
      addresses, and every family is asserted bit-reproducible from launch to launch elsewhere, so no tolerance is involved;
  (c) the contiguous run meets test_gpu_parity.py's bounds against the oracle (imported, not restated).

The forward goes through cdeint (gpu_util.run_case), the continuous adjoint and the exact discrete backward through the C-ABI on the
oracle's own z_out / stage record (gpu_util.run_adjoint_direct), as tests/test_adj_relu_masks_gpu.py does.  Shapes are the smallest
that take every path: B = 17 where one workgroup is one sample tile (a full tile and a one-sample tile), B = 37 on the batch-tiled
family (ragged last workgroup for NS2 / NS4), raw length 3 (5 rectilinear knots) / a 4-knot cubic.  The `broadcast` and `overlap`
layouts constrain the values, so their cases (and oracle expectations) are built from what the view holds; z0 still differs per sample.
`far` (an 8 GiB buffer) runs once per row, on the row's first (interp, method).
"""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

import golden_util as gu
import strided_views as sv
from test_gpu_parity import (COOP_FLIP_ROWS, E2E_G, TIGHT_G, TIGHT_Z, TOL_DZ0, _check_rows_with_one_flip, _grad_errors, _rows_off,
                             _seeded_case)

pytestmark = pytest.mark.gpu

LIN, CUB, EUL = ("linear", "rk4", False), ("cubic", "midpoint", True), ("linear", "euler", True)
FT, NS1, NS2, NS4, GENERIC = 0x8000, 0x1000, 0x2000, 0x4000, 1
FP32_MFMA, SPLIT_BF16, V1, V2, V4 = 4, 0x40, 8, 0x10, 0x20
SHARED = ("broadcast", "overlap")          # layouts whose samples share storage: the case follows from the layout
COOP_LAYOUTS = ("time_prefix", "batch_slice", "far")

# id: (C, H, HH, nl), B, field kind, field input, flags, combos, (forward, adjoint, discrete) name fragments, layouts (None = all)
F3 = ("ncde_fwd_fast_bf3<H32,HH32,C20", "fp16x2")
ROWS = {
    # 1. register-resident sets
    "fast3": ((20, 32, 32, 3), 17, "original", "matmul", 0, (LIN, CUB, EUL), (F3, ("ncde_adj_fast3<H32,HH32,C20,NL3",), ("ncde_adj_fast3<", "discrete")), None),
    "fast3_fp32": ((20, 32, 32, 3), 17, "original", "matmul", FP32_MFMA, (LIN, CUB), (("ncde_fwd_fast<H32,HH32,C20",), ("ncde_adj_fast3<",), ("ncde_adj_fast3<", "discrete")), None),
    "fast3_bf16": ((20, 32, 32, 3), 17, "original", "matmul", SPLIT_BF16, (LIN, CUB), (("ncde_fwd_fast_bf3<", "bf16x3"), ("ncde_adj_fast3<", "chain+grad,bf16x3"), ("ncde_adj_fast3<", "bf16x3,discrete")), None),
    "adj_v1": ((20, 32, 32, 3), 17, "original", "matmul", V1, (LIN, CUB), (F3, ("ncde_adj_fast<H32,HH32,C20,NL3",), ("ncde_adj_fast3<", "discrete")), None),
    "adj_v2": ((20, 32, 32, 3), 17, "original", "matmul", V2, (LIN, CUB), (F3, ("ncde_adj_fast2<H32,HH32,C20,NL3",), ("ncde_adj_fast3<", "discrete")), None),
    "adj_v4": ((20, 32, 32, 3), 17, "original", "matmul", V4, (LIN, CUB), (F3, ("ncde_adj_fast4<H32,HH32,C20,NL3",), ("ncde_adj_fast4<", "discrete")), None),
    "fast_nl2": ((20, 32, 32, 2), 17, "original", "matmul", 0, (LIN, CUB), (F3, ("ncde_adj_fast3<H32,HH32,C20,NL2",), ("ncde_adj_fast3<H32,HH32,C20,NL2", "discrete")), None),
    "h64": ((4, 64, 64, 3), 17, "original", "matmul", 0, (LIN, CUB), (("ncde_fwd_fast_bf3<H64,HH64,C4",), ("ncde_adj_h64<H64,HH64,NS1",), ("ncde_adj_h64<H64,HH64,NS1", "discrete")), None),
    "h64_ns2": ((4, 64, 64, 3), 17, "original", "matmul", NS2, (LIN, CUB), (("ncde_fwd_fast_bf3<H64,HH64,C4",), ("ncde_adj_h64<H64,HH64,NS2",), ("ncde_adj_h64<H64,HH64,NS2", "discrete")), None),
    "fast_c8": ((8, 32, 32, 3), 17, "original", "matmul", 0, (LIN, CUB), (("ncde_fwd_fast_bf3<H32,HH32,C8",), ("ncde_adj_fast3<H32,HH32,C8,NL3",), ("ncde_adj_fast3<H32,HH32,C8", "discrete")), None),
    "fwd_only_c40": ((40, 32, 32, 3), 17, "original", "matmul", 0, (LIN, CUB), (("ncde_fwd_fast_bf3<H32,HH32,C40",), ("ncde_adj_tiled<",), ("ncde_adj_tiled<", "discrete")), None),
    "fast_padded": ((18, 30, 30, 3), 17, "original", "matmul", 0, (LIN, CUB), (F3, ("ncde_adj_fast3<H32,HH32,C20,NL3",), ("ncde_adj_fast3<", "discrete")), None),
    # 3. batch-tiled family
    "tiled_ns1": ((8, 48, 64, 2), 37, "original", "matmul", FT | NS1, (LIN, CUB), (("ncde_fwd_tiled<NS1",), ("ncde_adj_tiled<",), ("ncde_adj_tiled<", "discrete")), None),
    "tiled_ns2": ((8, 48, 64, 2), 37, "original", "matmul", FT | NS2, (LIN, CUB), (("ncde_fwd_tiled<NS2>",), ("ncde_adj_tiled<",), ("ncde_adj_tiled<", "discrete")), None),
    "tiled_ns4": ((8, 48, 64, 2), 37, "original", "matmul", FT | NS4, (LIN, CUB), (("ncde_fwd_tiled<NS4>",), ("ncde_adj_tiled<",), ("ncde_adj_tiled<", "discrete")), None),
    "tiled_resident": ((16, 64, 64, 2), 37, "original", "matmul", 0, (LIN, CUB), (("ncde_fwd_tiled<NS1",), ("ncde_adj_tiled<",), ("ncde_adj_tiled<", "discrete")), None),
    "tiled_wide": ((20, 160, 128, 3), 37, "original", "matmul", 0, (LIN, CUB), (("ncde_fwd_tiled<NS1",), ("ncde_adj_tiled<wide",), ("ncde_adj_tiled<wide,discrete",)), None),
    "tiled_padded": ((5, 47, 93, 2), 37, "original", "matmul", 0, (LIN, CUB), (("ncde_fwd_tiled<NS1",), ("ncde_adj_tiled<",), ("ncde_adj_tiled<", "discrete")), None),
    "tiled_minimal": ((12, 32, 32, 3), 37, "minimal", "matmul", 0, (LIN, CUB), (("ncde_fwd_tiled<NS1,gated",), ("ncde_adj_tiled<gated",), ("ncde_adj_tiled<gated,discrete",)), None),
    # 4. cooperative output phase (the shapes of test_cooperative_timeout_is_reexecuted_not_nan, no fault injection)
    "coop_256": ((20, 128, 128, 3), 256, "original", "matmul", 0, (CUB,), (("ncde_fwd_tiled<", "coop"), ("ncde_adj_tiled<coop",), ("ncde_adj_tiled<coop,discrete",)), COOP_LAYOUTS),
    "coop_123": ((40, 64, 128, 2), 123, "original", "matmul", 0, (LIN,), (("ncde_fwd_tiled<", "coop"), ("ncde_adj_tiled<coop",), ("ncde_adj_tiled<coop,discrete",)), COOP_LAYOUTS),
    # ... and its batch-chunk rebasing (coop_chunk_args: c.coeffs = a.coeffs + 16 t0 cs_b, t0 > 0 only with more sample tiles than CUs):
    # the case of test_cooperative_kernels_on_more_sample_tiles_than_cus, 288 tiles = 256 + 32, on a time_prefix view
    "coop_chunked": ((80, 128, 128, 3), 4608, "original", "matmul", 0, (LIN,), (("ncde_fwd_tiled<", "coop"), ("ncde_adj_tiled<coop",), ("ncde_adj_tiled<coop,discrete",)), ("time_prefix",)),
    # 5. generic and variant kernels; the evaluate / derivative inputs (evaluate reads the `a` columns: X(t) itself)
    "generic": ((3, 7, 15, 1), 17, "original", "matmul", GENERIC, (LIN, CUB), (("ncde_fwd_generic",), ("ncde_adj_generic",), ("ncde_adj_generic<discrete>",)), None),
    "gru": ((8, 32, 32, 2), 17, "gru", "matmul", 0, (LIN, CUB), (("ncde_fwd_variant",), ("ncde_adj_variant",), ("ncde_adj_variant<discrete>",)), None),
    "tiled_evaluate": ((8, 32, 48, 3), 37, "original", "evaluate", 0, (LIN, CUB), (("ncde_fwd_tiled<NS1,direct",), ("ncde_adj_tiled<direct",), ("ncde_adj_tiled<direct,discrete",)), None),
    "tiled_derivative": ((8, 32, 48, 3), 37, "original", "derivative", 0, (LIN, CUB), (("ncde_fwd_tiled<NS1,direct",), ("ncde_adj_tiled<direct",), ("ncde_adj_tiled<direct,discrete",)), None),
    "variant_evaluate": ((8, 32, 48, 3), 17, "minimal", "evaluate", GENERIC, (LIN, CUB), (("ncde_fwd_variant",), ("ncde_adj_variant",), ("ncde_adj_variant<discrete>",)), None),
    "variant_derivative": ((8, 32, 48, 3), 17, "original", "derivative", GENERIC, (LIN, CUB), (("ncde_fwd_variant",), ("ncde_adj_variant",), ("ncde_adj_variant<discrete>",)), None),
}


def _params(rows):
    out = []
    for rid, row in rows.items():
        for i, combo in enumerate(row[5]):
            for layout in (row[7] or sv.layouts(combo[0])):
                if layout == "far" and i:      # the 8 GiB layout: once per row (every kernel name of the row sees it)
                    continue
                out.append(pytest.param(rid, combo, layout, id="%s-%s-%s-%s" % (rid, combo[0], combo[1], layout)))
    return out


def _with_expectations(case, coeffs):
    """`case` on other coefficient values: the oracle's forward solution, both gradients and the stage record (as _seeded_case)."""
    import ncde_oracle as orc
    m = case["meta"]
    case = dict(case, coeffs=coeffs)
    names, method, seq = m["param_names"], m["method"], m["sequence"]
    field, ctl = gu.oracle_field(case), orc.Control(coeffs, m["kind"])
    z = orc.solve_forward(ctl, field, case["z0"], method, seq)
    gout = (gu.data.normal(77, z.numel(), stream=1).reshape(z.shape) / np.sqrt(z.shape[1])).astype(np.float32)
    dz0, gp = orc.solve_adjoint(ctl, field, z, gout, method, seq)
    ex = {"z_out": z.numpy(), "grad_out": gout, "dz0": dz0.numpy()}
    ex.update({"d" + n: g.numpy() for n, g in zip(names, gp)})
    bdz0, bgp = orc.solve_discrete_backward(ctl, field, case["z0"], gout, method, seq)
    ex["bp_dz0"] = bdz0.numpy()
    ex.update({"bp_d" + n: g.numpy() for n, g in zip(names, bgp)})
    case["expect"] = ex
    case["stage_record"] = orc.stage_record(ctl, field, case["z0"], method).numpy()
    return case


@functools.lru_cache(maxsize=None)
def _case(rid, combo, shared):
    """The row's case on one (interp, method, output) -- computed once, shared by the layouts, never modified.  shared: None, or the
    layout ("broadcast" / "overlap") whose view the coefficients must fit."""
    (C, H, HH, nl), B, kind, mode, _flags, _combos, _names, _layouts = ROWS[rid]
    interp, method, seq = combo
    L = {"coop_123": 4, "coop_256": 3, "coop_chunked": 2}.get(rid, 4 if interp == "cubic" else 3)
    seed = {"coop_256": 940 + C, "coop_123": 940 + C, "coop_chunked": 960}.get(rid, 5000 + 7 * C + H + nl)
    if rid == "coop_chunked":
        torch.set_num_threads(min(16, len(__import__("os").sched_getaffinity(0))))
    if mode == "matmul" and shared is None:
        return _seeded_case(interp, method, seq, B=B, L=L, C=C, H=H, HH=HH, nl=nl, seed=seed, kind=kind)
    if mode == "matmul":
        base = _case(rid, combo, None)
    else:      # the direct input modes: layer 0 reads [z, X(t)] / [z, dX/dt], the heads have H rows
        coeffs = gu.data.make_cubic_coeffs(B, L, C - 1, seed=seed) if interp == "cubic" else gu.data.make_rectilinear_coeffs(B, L, C - 1, missing=0.3, seed=seed)
        p = gu.data.make_variant_weights(H, HH, C, seed=seed + 1, kind=kind, mode=mode)
        names = [n for n in ("W0", "b0", "W1", "b1", "Wr", "br", "Wg", "bg", "Wo", "bo") if n in p]
        base = {"meta": {"kind": interp, "method": method, "sequence": seq, "param_names": names, "field_kind": kind, "field_mode": mode,
                         "dims": {"C": C, "H": H, "HH": HH, "nl": nl}, "field": "original"},
                "coeffs": coeffs, "z0": (gu.data.normal(seed + 3, B * H, stream=2).reshape(B, H) * 0.5).astype(np.float32), "params": p,
                "layers": [("W0", "b0")] + [("W1", "b1")] * (nl - 1), "H": H, "C": C}
    return _with_expectations(base, sv.logical(base["coeffs"], shared) if shared else base["coeffs"])


def _differing(a, b):
    pairs = [(k, a[k], b[k]) for k in ("z_out", "dz0") if k in a] + [(k, a["grads"][k], b["grads"][k]) for k in a.get("grads", {})]
    return {k: float(np.abs(x.astype(np.float64) - y).max()) for k, x, y in pairs if not np.array_equal(x, y, equal_nan=False)}


def _finite(r):
    return all(np.isfinite(r[k]).all() for k in ("z_out", "dz0") if k in r) and all(np.isfinite(g).all() for g in r.get("grads", {}).values())


def _view(coeffs_np, layout):
    try:
        return sv.make_view(coeffs_np, layout, "cuda")
    except sv.FarLayoutNeedsMemory as e:
        pytest.skip(str(e))


def _named(name, fragments):
    return name.startswith(fragments[0]) and all(f in name for f in fragments[1:])


@pytest.mark.parametrize("rid,combo,layout", _params(ROWS))
def test_default_axis_kernels_read_through_the_strides(rid, combo, layout, gpu_lib):
    """Rows 1, 3, 4 and 5 of the issue: forward, continuous adjoint and exact discrete backward of one kernel row on one layout."""
    import gpu_util
    flags, want = ROWS[rid][4], ROWS[rid][6]
    case = _case(rid, combo, layout if layout in SHARED else None)
    ex = case["expect"]
    view = _view(case["coeffs"], layout)
    cont = view.contiguous()
    assert cont.is_contiguous() and (layout == "contiguous") == view.is_contiguous()
    runs = {}
    for tag, dev in (("view", view), ("contiguous", cont)):
        names = gpu_util.kernel_names(case, flags, coeffs=dev)
        runs[tag] = (names, gpu_util.run_case(case, flags=flags, need_grads=False, coeffs=dev),
                     gpu_util.run_adjoint_direct(case, ex["z_out"], flags=flags, coeffs=dev),
                     gpu_util.run_adjoint_direct(case, ex["z_out"], flags=flags, stages=case["stage_record"], coeffs=dev))
    (nv, fv, av, dv), (nc, fc, ac, dc) = runs["view"], runs["contiguous"]
    assert nv == nc and av["kernel"] == ac["kernel"] == nc[1] and dv["kernel"] == dc["kernel"] == nc[2], (nv, nc)      # (a)
    assert all(_named(n, w) for n, w in zip(nc, want)), (nc, want)
    for what, v, c_ in (("forward", fv, fc), ("adjoint", av, ac), ("discrete backward", dv, dc)):                      # (b)
        assert _finite(v) and _finite(c_), (what, nc)
        assert not _differing(v, c_), (what, layout, nc, _differing(v, c_))
    ez = gu.relerr(fc["z_out"], ex["z_out"])                                                                            # (c)
    assert ez <= TIGHT_Z, ("forward", nc[0], ez)
    if rid.startswith("coop"):
        # Against the oracle per ROW of dL/dz0: a batch of hundreds of samples meets ReLU gates within rounding of zero, where two fp32
        # implementations may disagree and THAT sample's row moves (and the batch sums with it).  The two small batches are held as the
        # plan-walking test holds its 37 samples (at most one such row: _check_rows_with_one_flip), the 4608-sample one as
        # test_cooperative_kernels_on_more_sample_tiles_than_cus holds it (COOP_FLIP_ROWS rows within TOL_DZ0, the sums at E2E_G).  On top,
        # not instead: the per-workgroup sweep (NCDE_FLAG_NO_COOP) at the bound each of those tests has for it.
        from ncde_amd import _lib
        names = case["meta"]["param_names"]
        for pre, r, kw in (("", ac, {}), ("bp_", dc, {"stages": case["stage_record"]})):
            old = gpu_util.run_adjoint_direct(case, ex["z_out"], flags=flags | _lib.FLAG_NO_COOP, coeffs=cont, **kw)
            assert "coop" not in old["kernel"], old["kernel"]
            if rid == "coop_chunked":
                n_off, worst = _rows_off(r["dz0"], ex[pre + "dz0"])
                assert n_off <= COOP_FLIP_ROWS and worst <= TOL_DZ0, (r["kernel"], n_off, worst)
                for k, e in _grad_errors(case, r, pre).items():
                    assert k == "dz0" or e <= E2E_G, (pre or "adjoint", r["kernel"], k, e)
                n_off, worst = _rows_off(r["dz0"], old["dz0"])
                assert n_off <= COOP_FLIP_ROWS and worst <= TOL_DZ0, (old["kernel"], n_off, worst)
                for k in old["grads"]:
                    assert gu.relerr(r["grads"][k], old["grads"][k]) <= E2E_G, (r["kernel"], k)
            else:
                _check_rows_with_one_flip(r, torch.from_numpy(ex[pre + "dz0"]), [ex[pre + "d" + n] for n in names], names, 1, (rid, pre or "adjoint"))
                assert gu.relerr(r["dz0"], old["dz0"]) <= TIGHT_G, (r["kernel"], gu.relerr(r["dz0"], old["dz0"]))
                for k in old["grads"]:
                    assert gu.relerr(r["grads"][k], old["grads"][k]) <= TIGHT_G, (r["kernel"], k)
        return
    for pre, r in (("", ac), ("bp_", dc)):
        for k, e in _grad_errors(case, r, pre).items():
            assert e <= TIGHT_G, (pre or "adjoint", r["kernel"], k, e)


# ---- 2. plan-walking instantiations (the sd.idx sites): step 0.5, off-grid output times, a user knot grid on the linear path -----------
PLAN_ROWS = {      # id: (C, H, HH, nl), flags, (forward, adjoint, discrete) name fragments
    "plan_fast": ((20, 32, 32, 3), 0, (("ncde_fwd_fast_bf3<H32", "time plan"), ("ncde_adj_fast3<", "time plan"), ("ncde_adj_tiled<", "discrete"))),
    "plan_tiled": ((8, 48, 64, 2), FT, (("ncde_fwd_tiled<",), ("ncde_adj_tiled<",), ("ncde_adj_tiled<", "discrete"))),
    "plan_generic": ((20, 32, 32, 3), GENERIC, (("ncde_fwd_generic",), ("ncde_adj_generic",), ("ncde_adj_generic<discrete>",))),
    "plan_generic_48": ((8, 48, 64, 2), GENERIC, (("ncde_fwd_generic",), ("ncde_adj_generic",), ("ncde_adj_generic<discrete>",))),
}


@functools.lru_cache(maxsize=None)
def _plan_case(rid, interp, method, shared):
    """Inputs as test_general_time_axis_on_the_specialised_kernels_vs_oracle takes them, and the oracle's general-time results."""
    import ncde_oracle as orc
    (C, H, HH, nl), _flags, _names = PLAN_ROWS[rid]
    B, L, step = 37, 9, 0.5
    rng = np.random.RandomState(7)
    x = (gu.data.normal(61, B * L * C, stream=3).reshape(B, L, C) * 0.5).astype(np.float32)
    if interp == "linear":      # user knot grid, spacing 0.6 .. 1.4
        kn = np.cumsum(np.concatenate([[0.0], 0.6 + 0.8 * rng.rand(L - 1)])).astype(np.float32)
        x[:, :, 0] = kn[None, :]
        coeffs = x
    else:
        kn = np.arange(L, dtype=np.float32)
        x[:, :, 0] = kn[None, :]
        coeffs = gu.data.natural_cubic_coeffs(x)
    if shared:
        coeffs = sv.logical(coeffs, shared)
    p = gu.data.make_field_weights(H, HH, C, seed=29)
    z0 = (gu.data.normal(63, B * H, stream=2).reshape(B, H) * 0.5).astype(np.float32)
    tout = np.array([kn[0], 0.5 * (kn[1] + kn[2]), kn[4], kn[6] + 0.05, kn[-1] - 0.125], np.float32)
    field = orc.Field.variant(p, H, C, nl, "original", "matmul")
    ctl = orc.Control(coeffs, interp, t=kn if interp == "linear" else None)
    z = orc.solve_forward_times(ctl, field, z0, tout, method, step)
    gout = (gu.data.normal(25, z.numel(), stream=1).reshape(z.shape) / 2.0).astype(np.float32)
    g = {"coeffs": coeffs, "z0": z0, "t_out": tout, "grad_out": gout}
    if interp == "linear":
        g["knots"] = kn
    names = [n for n in ("W0", "b0", "W1", "b1", "Wo", "bo") if n in p]
    return {"g": g, "p": p, "kn": kn, "names": names, "z": z.numpy(), "meta": {"kind": interp, "method": method, "step_size": step, "dims": {"nl": nl}},
            "adjoint": orc.solve_adjoint_times(ctl, field, tout, z, gout, method, step),
            "discrete": orc.solve_discrete_backward_times(ctl, field, z0, tout, gout, method, step)}


def _plan_params():
    out = []
    for rid in PLAN_ROWS:
        for i, (interp, method) in enumerate((("linear", "rk4"), ("cubic", "midpoint"))):
            out += [pytest.param(rid, interp, method, layout, id="%s-%s-%s-%s" % (rid, interp, method, layout))
                    for layout in sv.layouts(interp) if not (layout == "far" and i)]
    return out


@pytest.mark.parametrize("rid,interp,method,layout", _plan_params())
def test_plan_walking_kernels_read_through_the_strides(rid, interp, method, layout, gpu_lib):
    """Row 2 of the issue, end to end through cdeint (run_times_case): forward + continuous adjoint, recording forward + discrete
    backward.  (c) is the bound of test_general_time_axis_on_the_specialised_kernels_vs_oracle: z at TIGHT_Z; every dL/dz0 row within
    E2E_G but at most one (a ReLU mask within rounding of zero flips between two fp32 implementations), the batch-summed gradients
    within E2E_G when no row flipped."""
    import gpu_util
    import ncde_amd
    from ncde_amd import _lib, solver
    (C, H, HH, nl), flags, want = PLAN_ROWS[rid]
    pc = _plan_case(rid, interp, method, layout if layout in SHARED else None)
    g, p, meta = pc["g"], pc["p"], pc["meta"]
    view = _view(g["coeffs"], layout)
    func = gpu_util.CaseField(p, [("W0", "b0")] + [("W1", "b1")] * (nl - 1), "cuda")
    res = {}
    for tag, dev in (("view", view), ("contiguous", view.contiguous())):
        X = (ncde_amd.LinearInterpolation if interp == "linear" else ncde_amd.NaturalCubicSpline)(dev, t=torch.from_numpy(pc["kn"]).cuda() if interp == "linear" else None)
        plan = solver._time_plan(X, torch.from_numpy(g["t_out"]), method, meta["step_size"], dev.device)
        prob = solver.build_problem(dev, interp, torch.from_numpy(g["z0"]).cuda(), func.fused_spec(), method, _lib.OUT_TIMES, flags, plan)
        names = tuple((_lib.lib().ncde_kernel_name(ctypes.byref(prob), k) or b"?").decode() for k in (0, 1, 2))
        res[tag] = (names, gpu_util.run_times_case(g, meta, adjoint=True, params=p, flags=flags, coeffs=dev),
                    gpu_util.run_times_case(g, meta, adjoint=False, params=p, flags=flags, coeffs=dev))
    (nv, av, dv), (nc, ac, dc) = res["view"], res["contiguous"]
    assert nv == nc and all(_named(n, w) for n, w in zip(nc, want)), (nv, nc, want)                                    # (a)
    for what, v, c_ in (("adjoint", av, ac), ("discrete", dv, dc)):                                                     # (b)
        assert _finite(v) and _finite(c_), (what, nc)
        assert not _differing(v, c_), (what, layout, nc, _differing(v, c_))
        assert v["nfe"] == c_["nfe"]
    for what, r, (want_dz0, want_gp) in (("adjoint", ac, pc["adjoint"]), ("discrete", dc, pc["discrete"])):             # (c)
        assert gu.relerr(r["z_out"], pc["z"]) <= TIGHT_Z, (what, gu.relerr(r["z_out"], pc["z"]))
        _check_rows_with_one_flip(r, want_dz0, want_gp, pc["names"], 1, (what, layout))


# ---- 6. dopri5 -------------------------------------------------------------------------------------------------------------------
DP_ROWS = {      # id: (C, H, HH, nl), (forward, adjoint, taped backward) name fragments
    "dopri5_fused_32": ((20, 32, 32, 3), (("ncde_dpf_fwd<H32",), ("ncde_dpf_adj<H32",), ("ncde_dpf_tape<H32",))),
    "dopri5_fused_64": ((4, 64, 64, 2), (("ncde_dpf_fwd<H64",), ("ncde_dp_stage",), ("ncde_dp_tape_backward",))),
    "dopri5_per_launch": ((7, 24, 40, 2), (("ncde_dp_stage",), ("ncde_dp_stage",), ("ncde_dp_tape_backward",))),
}
DP_OPTS = {"first_step": 0.75, "min_step": 0.75, "max_step": 0.75}      # the forced step sequence: no controller decision involved


class _GateWatch:
    """While active, every ReLU pre-activation the ORACLE forms (oracle/ncde_oracle.py: Field._net) is compared with the fp32
    rounding bound of the dot product behind it, (n + 1) 2^-24 (|b| + |x| . |w|) for n terms in any order of summation.  `worst` is the
    smallest |pre-activation| / bound met: below 1 the sign of that pre-activation -- the ReLU gate, an O(1) factor on the cotangent --
    is not decided by the inputs in fp32, and two correct fp32 implementations may disagree on it."""

    def __enter__(self):
        import ncde_oracle as orc
        self.orc, self.real, self.worst = orc, orc.Field._net, float("inf")
        watch = self

        def net(field, u):
            x = u
            for w, b in field.layers:
                bound = (w.shape[1] + 1) * 2.0 ** -24 * (b.abs() + x.abs() @ w.abs().t())
                watch.worst = min(watch.worst, float((torch.addmm(b, x, w.t()).abs() / bound).min()))
                x = torch.relu(torch.addmm(b, x, w.t()))
            return watch.real(field, u)
        orc.Field._net = net
        return self

    def __exit__(self, *exc):
        self.orc.Field._net = self.real


DP_SEEDS = range(95, 95 + 2 * 40, 2)      # the first pair (95, 96) is the one test_dopri5_every_kernel_set_forced_sequence_vs_oracle uses


@functools.lru_cache(maxsize=None)
def _dp_case(rid, interp, shared):
    """Inputs as test_dopri5_every_kernel_set_forced_sequence_vs_oracle takes them (B = 17, the shortest paths here), from the first seed
    of DP_SEEDS on which the oracle itself is a yardstick at E2E_G: every ReLU gate its three solves meet is decided beyond the fp32
    rounding of its own dot product (_GateWatch; a property of the inputs and the oracle alone, no kernel is consulted).
    (One gate at 1e-8 is enough: the adaptive adjoint of one sample then lands on either side of it, and its gradients move by 5e-4.)"""
    import ncde_oracle as orc
    (C, H, HH, nl), _names = DP_ROWS[rid]
    B = 17
    p = gu.data.make_field_weights(H, HH, C, seed=9)
    rw = gu.data.make_readin_weights(H, C, 1, seed=9)
    for seed in DP_SEEDS:
        if interp == "linear":
            coeffs = gu.data.make_rectilinear_coeffs(B, 3, C - 1, missing=0.3, seed=seed)
            x0 = coeffs[:, 0]
        else:
            coeffs = gu.data.make_cubic_coeffs(B, 4, C - 1, seed=seed + 1)
            x0 = coeffs[:, 0, :C]
        if shared:
            coeffs = sv.logical(coeffs, shared)
        z0 = (x0 @ rw["Wi"].T + rw["bi"]).astype(np.float32)
        field, ctl = orc.Field.original(p, H, C, nl), orc.Control(coeffs, interp)
        tt = torch.arange(ctl.n_knots, dtype=torch.float32)
        with _GateWatch() as gates:
            z = orc.dopri5_forward(ctl, field, z0, tt, 1e-3, 1e-5, DP_OPTS)
            gout = (gu.data.normal(31, z.numel(), stream=1).reshape(z.shape) / np.sqrt(z.shape[1])).astype(np.float32)
            dz0, gp = orc.dopri5_adjoint(ctl, field, tt, z, gout, 1e-3, 1e-5, DP_OPTS)
            _zb, bdz0, bgp = orc.dopri5_discrete_backward(ctl, field, z0, tt, gout, 1e-3, 1e-5, DP_OPTS)
        if gates.worst > 1.0:
            break
    else:
        raise AssertionError("no seed of DP_SEEDS gives a case whose gates are all decided in fp32")
    return {"coeffs": coeffs, "p": p, "z0": z0, "z": z.numpy(), "gout": gout, "names": ["W0", "b0", "W1", "b1", "Wo", "bo"],
            "seed": seed, "gate_margin": gates.worst, True: (dz0, gp), False: (bdz0, bgp)}


def _dp_params():
    out = []
    for rid in DP_ROWS:
        for i, interp in enumerate(("linear", "cubic")):
            out += [pytest.param(rid, interp, layout, id="%s-%s-%s" % (rid, interp, layout)) for layout in sv.layouts(interp) if not (layout == "far" and i)]
    return out


@pytest.mark.parametrize("rid,interp,layout", _dp_params())
def test_dopri5_kernels_read_through_the_strides(rid, interp, layout, gpu_lib):
    """Row 6 of the issue: forward, adaptive adjoint and taped backward on the forced step sequence; besides (a) - (c) the step
    sequences (accepted / rejected attempts, forward and backward) and nfe are the same for the view and the contiguous tensor.
    (c) is the bound of test_dopri5_every_kernel_set_forced_sequence_vs_oracle: TIGHT_Z, E2E_G.
    The inputs are conditioned on the oracle alone (_dp_case, _GateWatch): no ReLU gate within fp32 rounding of zero."""
    import gpu_util
    import ncde_amd
    from ncde_amd import _lib, solver
    (C, H, HH, nl), want = DP_ROWS[rid]
    dc = _dp_case(rid, interp, layout if layout in SHARED else None)
    view = _view(dc["coeffs"], layout)
    layers = [("W0", "b0")] + [("W1", "b1")] * (nl - 1)
    res = {}
    for tag, dev in (("view", view), ("contiguous", view.contiguous())):
        X = (ncde_amd.LinearInterpolation if interp == "linear" else ncde_amd.NaturalCubicSpline)(dev)
        func = gpu_util.CaseField(dc["p"], layers, "cuda")
        prob = solver.build_problem(dev, interp, torch.from_numpy(dc["z0"]).cuda(), func.fused_spec(), "rk4", _lib.OUT_INTERVAL, 0)
        names = tuple((_lib.lib().ncde_dopri5_kernel_name(ctypes.byref(prob), k) or b"?").decode() for k in (0, 1, 2))
        out = {}
        for adjoint in (True, False):
            func = gpu_util.CaseField(dc["p"], layers, "cuda")
            z0 = torch.from_numpy(dc["z0"]).cuda().requires_grad_(True)
            z = ncde_amd.cdeint(X, func, z0, X.grid_points, adjoint=adjoint, method="dopri5", rtol=1e-3, atol=1e-5, options=dict(DP_OPTS, _trace=256))
            (z * torch.from_numpy(dc["gout"]).cuda()).sum().backward()
            torch.cuda.synchronize()
            tr = [np.asarray(getattr(func, a)) for a in ("dopri5_trace", "dopri5_trace_backward") if getattr(func, a, None) is not None]
            out[adjoint] = {"z_out": z.detach().cpu().numpy(), "dz0": z0.grad.cpu().numpy(), "nfe": func.nfe, "trace": tr,
                            "grads": {k: v.grad.cpu().numpy() for k, v in func.p.items() if v.grad is not None}}
        res[tag] = (names, out)
    (nv, ov), (nc, oc) = res["view"], res["contiguous"]
    assert nv == nc and all(_named(n, w) for n, w in zip(nc, want)), (nv, nc, want)                                    # (a)
    for adjoint in (True, False):
        v, c_ = ov[adjoint], oc[adjoint]
        assert _finite(v) and _finite(c_) and not _differing(v, c_), (adjoint, layout, nc, _differing(v, c_))           # (b)
        assert v["nfe"] == c_["nfe"] and len(v["trace"]) == len(c_["trace"]) >= 1
        for tv, tc in zip(v["trace"], c_["trace"]):      # rows of (t0, dt, accepted, error ratio): the same attempts, accepted and rejected
            assert tv.shape == tc.shape and np.array_equal(tv, tc)
        want_dz0, want_gp = dc[adjoint]                                                                                 # (c)
        assert gu.relerr(c_["z_out"], dc["z"]) <= TIGHT_Z
        assert gu.relerr(c_["dz0"], want_dz0) <= E2E_G
        for n_, g_ in zip(dc["names"], want_gp):
            assert gu.relerr(c_["grads"][n_], g_) <= E2E_G, (adjoint, n_)


# ---- 7. the control-gradient route (ncde_backward_control through cdeint(adjoint=False)) -----------------------------------------------
@pytest.mark.parametrize("path", ["linear", "cubic", "smoothed"])
@pytest.mark.parametrize("layout", [l for l in sv.layouts() if l != "far"])
def test_control_gradient_through_a_view(layout, path, gpu_lib):
    """coeffs = a view of `base`, base.requires_grad_(): dL/dcoeffs (dense inside the library) is bit-identical to the contiguous call's,
    base.grad is exactly zero outside the view and holds the view's gradient inside (summed where samples share storage: the batch sum
    for `broadcast`); nothing runs unfused.  The cubic-smoothed path reads refined rows the class builds contiguous (asserted)."""
    import gpu_util
    import ncde_amd
    from ncde_amd import solver, unfused
    B, C, H, HH, nl = 37, 8, 32, 32, 2
    interp = "cubic" if path == "cubic" else "linear"
    raw = gu.data.make_cubic_coeffs(B, 4, C - 1, seed=81) if interp == "cubic" else gu.data.make_rectilinear_coeffs(B, 3, C - 1, missing=0.3, seed=81)
    coeffs = sv.logical(raw, layout)
    p = gu.data.make_field_weights(H, HH, C, seed=82)
    z0n = (gu.data.normal(83, B * H, stream=2).reshape(B, H) * 0.5).astype(np.float32)
    view0, base0 = sv.carve(coeffs, layout, "cuda")

    def control(c):
        if path == "smoothed":
            return ncde_amd.SmoothLinearInterpolation(c, gradient_matching_eps=0.5)
        return (ncde_amd.NaturalCubicSpline if interp == "cubic" else ncde_amd.LinearInterpolation)(c)

    def run(leaf, c):
        unfused._WARNED.clear()
        seen, dense, real = [], [], solver.build_problem
        c.register_hook(lambda g_: dense.append(g_.detach().clone()))

        def spy(cf, *a, **k):
            seen.append((tuple(cf.shape), cf.stride(), cf.is_contiguous()))
            return real(cf, *a, **k)
        solver.build_problem = spy
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                X = control(c)
                func = gpu_util.CaseField(p, [("W0", "b0")] + [("W1", "b1")] * (nl - 1), "cuda")
                z0 = torch.from_numpy(z0n).cuda().requires_grad_(True)
                out = ncde_amd.cdeint(X, func, z0, X.grid_points, adjoint=False, method="rk4", options={"step_size": 1})
                gout = torch.from_numpy((gu.data.normal(85, out.numel(), stream=1).reshape(out.shape) / 2.0).astype(np.float32)).cuda()
                (out * gout).sum().backward()
            torch.cuda.synchronize()
        finally:
            solver.build_problem = real
        assert not unfused._WARNED, unfused._WARNED
        return {"z_out": out.detach().cpu().numpy(), "dz0": z0.grad.cpu().numpy(), "dcoeffs": dense[0].cpu().numpy(), "leaf": leaf.grad,
                "grads": {k: v.grad.cpu().numpy() for k, v in func.p.items()}, "seen": seen}

    base = base0.detach().clone().requires_grad_(True)
    v = run(base, base.as_strided(view0.shape, view0.stride(), view0.storage_offset()))
    cont = view0.detach().contiguous().requires_grad_(True)
    c_ = run(cont, cont)
    assert v["seen"] and c_["seen"]
    if path == "smoothed":      # the refined rows: built contiguous whatever the caller's strides
        assert all(s[2] for s in v["seen"]) and [s[0] for s in v["seen"]] == [s[0] for s in c_["seen"]]
    else:                       # the kernels were handed the caller's strides
        assert all(s[1] == tuple(view0.stride()) for s in v["seen"]) and all(s[2] for s in c_["seen"]), (v["seen"], view0.stride())
    assert _finite(v) and not _differing(v, c_), _differing(v, c_)
    assert np.isfinite(v["dcoeffs"]).all() and np.array_equal(v["dcoeffs"], c_["dcoeffs"]) and np.any(v["dcoeffs"])
    assert np.array_equal(c_["leaf"].cpu().numpy(), c_["dcoeffs"])
    grad = v["leaf"].cpu()
    inside = sv.inside_mask(view0, base0)
    assert not grad[~inside].any() and torch.isfinite(grad).all()                     # exactly zero outside the view
    got = grad.as_strided(view0.shape, view0.stride(), view0.storage_offset()).numpy()
    if layout not in SHARED:
        assert np.array_equal(got, v["dcoeffs"])
    else:      # shared storage: the sum over the samples that point at an element, to fp32 summation (at most B terms)
        d64 = torch.from_numpy(v["dcoeffs"]).double()
        Bv, R, K = view0.shape
        sb, st, _ = view0.stride()
        idx = (view0.storage_offset() + sb * torch.arange(Bv)[:, None, None] + st * torch.arange(R)[None, :, None] + torch.arange(K)).reshape(-1)
        want = torch.zeros(base0.numel(), dtype=torch.double).index_add_(0, idx, d64.reshape(-1))
        mag = torch.zeros(base0.numel(), dtype=torch.double).index_add_(0, idx, d64.abs().reshape(-1))
        assert bool(((grad.double() - want).abs() <= Bv * 2.0 ** -23 * mag).all())
        if layout == "broadcast":
            assert np.allclose(got[0], v["dcoeffs"].astype(np.float64).sum(0), rtol=0, atol=float(Bv * 2.0 ** -23 * np.abs(v["dcoeffs"]).sum(0).max()))


# ---- the host: a time stride smaller than the row is copied, not rejected --------------------------------------------------------------
@pytest.mark.parametrize("adjoint", [True, False])
def test_constant_path_expanded_over_time_solves(adjoint, gpu_lib):
    """x0.unsqueeze(1).expand(B, T, C) has stride(1) == 0 and unit stride in C: the host copies it (the C-ABI keeps rejecting such a
    stride, tests/test_smooth_gpu.py), the solve equals the materialised tensor's bit for bit and warns nothing -- also on the
    control-gradient route (adjoint=False, coefficients that require grad)."""
    import gpu_util
    import ncde_amd
    B, T, C, H, HH, nl = 17, 5, 20, 32, 32, 3
    x0 = torch.from_numpy((gu.data.normal(91, B * C, stream=3).reshape(B, C) * 0.5).astype(np.float32)).cuda()
    p = gu.data.make_field_weights(H, HH, C, seed=92)
    z0n = (gu.data.normal(93, B * H, stream=2).reshape(B, H) * 0.5).astype(np.float32)
    res = []
    for materialise in (False, True):
        for leaf in ((False, True) if not adjoint else (False,)):
            src = x0.clone().requires_grad_(leaf)
            coeffs = src.unsqueeze(1).expand(B, T, C)
            assert coeffs.stride() == (C, 0, 1)
            coeffs = coeffs.contiguous() if materialise else coeffs
            func = gpu_util.CaseField(p, [("W0", "b0")] + [("W1", "b1")] * (nl - 1), "cuda")
            z0 = torch.from_numpy(z0n).cuda().requires_grad_(True)
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                X = ncde_amd.LinearInterpolation(coeffs)
                out = ncde_amd.cdeint(X, func, z0, X.grid_points, adjoint=adjoint, method="rk4", options={"step_size": 1})
                out.square().sum().backward()
            torch.cuda.synchronize()
            res.append((materialise, leaf, {"z_out": out.detach().cpu().numpy(), "dz0": z0.grad.cpu().numpy(),
                                            "grads": dict({k: v.grad.cpu().numpy() for k, v in func.p.items()},
                                                          **({"x0": src.grad.cpu().numpy()} if leaf else {}))}))
    for leaf in {r[1] for r in res}:
        (a,), (b,) = [[r[2] for r in res if r[0] == m and r[1] == leaf] for m in (False, True)]
        assert _finite(a) and not _differing(a, b), (leaf, _differing(a, b))
    assert gu.relerr(res[0][2]["z_out"][:, -1], z0n) <= TIGHT_Z      # a constant path: dX/dt = 0, the state does not move


# ---- piecewise-quintic rows (6C columns): batch-tiled, generic and variant kernels -------------------------------------------------
QUINTIC_ROWS = {      # id: golden of tests/test_smooth_gpu.py, flags, (forward, adjoint, discrete) name fragments
    "quintic_tiled": ("g14_e_quintic_eps05_rk4", 0, (("ncde_fwd_tiled<",), ("ncde_adj_tiled<",), ("ncde_adj_tiled<", "discrete"))),
    "quintic_tiled_c20": ("g14_h_quintic_eps05_rk4_half_c20", 0, (("ncde_fwd_tiled<",), ("ncde_adj_tiled<",), ("ncde_adj_tiled<", "discrete"))),
    "quintic_generic": ("g14_e_quintic_eps05_rk4", GENERIC, (("ncde_fwd_generic",), ("ncde_adj_generic",), ("ncde_adj_generic<discrete>",))),
    "quintic_variant": ("g14_g_quintic_eps1_gru_evaluate", 0, (("ncde_fwd_variant",), ("ncde_adj_variant",), ("ncde_adj_variant<discrete>",))),
}


@pytest.mark.parametrize("layout", sv.layouts("quintic"))
@pytest.mark.parametrize("rid", list(QUINTIC_ROWS))
def test_quintic_rows_read_through_the_strides(rid, layout, gpu_lib):
    """A quintic path as tests/test_smooth_gpu.py builds it -- SmoothLinearInterpolation(match_second_derivatives=True), whose refined
    rows a | b | 2c | 3d | 4e | 5f the kernels read -- with those rows handed over as a view: cdeint forward + continuous adjoint and
    recording forward + discrete backward, through that file's own `_run`.  (a) and (b) as everywhere; (c) is that file's bound against
    the reference's golden (TIGHT_Z, E2E_G).  `broadcast` and `overlap` change the values, for which no reference exists (the oracle
    has no quintic control): there (a) and (b) only."""
    import test_smooth_gpu as ts
    from ncde_amd import _lib
    name, flags, want = QUINTIC_ROWS[rid]
    f, m = ts._load(name)
    X0 = ts._control(f, m)
    rows = sv.logical(X0.fused_coeffs.cpu().numpy(), layout)
    assert rows.shape[2] == 6 * m["dims"]["C"]
    view = _view(rows, layout)
    res = {}
    for tag, dev in (("view", view), ("contiguous", view.contiguous())):
        out = []
        for adjoint in (True, False):
            X = ts._control(f, m)
            key = X.fused_coeffs is not None and X._fused[0]
            X._fused = (key, dev)                      # the refined rows the solver hands to the kernels: this tensor, strides and all
            probs = []
            out.append(ts._run(f, m, adjoint, flags, X=X, capture=probs))
            assert probs and all((p.coeffs, p.coeffs_stride_b, p.coeffs_stride_t) == (dev.data_ptr(), dev.stride(0), dev.stride(1)) and
                                 p.interp == _lib.INTERP["quintic"] for p in probs)
        names = tuple((_lib.lib().ncde_kernel_name(ctypes.byref(probs[-1]), k) or b"?").decode() for k in (0, 1, 2))
        res[tag] = (names, out)
    (nv, ov), (nc, oc) = res["view"], res["contiguous"]
    assert nv == nc and all(_named(n, w) for n, w in zip(nc, want)), (nv, nc, want)                                    # (a)
    for v, c_ in zip(ov, oc):                                                                                           # (b)
        assert _finite(v) and _finite(c_) and not _differing(v, c_), (layout, nc, _differing(v, c_))
        assert v["nfe"] == c_["nfe"]
    if layout in SHARED:
        return
    ra, rd = oc                                                                                                         # (c)
    errs = {"z": gu.relerr(ra["z_out"], f["z_out"]), "dz0": gu.relerr(ra["dz0"], f["dz0"]), "bp_dz0": gu.relerr(rd["dz0"], f["bp_dz0"])}
    for n in m["param_names"]:
        errs["d" + n], errs["bp_d" + n] = gu.relerr(ra["grads"][n], f["d" + n]), gu.relerr(rd["grads"][n], f["bp_d" + n])
    assert errs["z"] <= ts.TIGHT_Z and np.array_equal(rd["z_out"], ra["z_out"]), errs
    assert all(e <= ts.E2E_G for k, e in errs.items() if k != "z"), errs
