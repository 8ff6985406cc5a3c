"""Coefficient builders without a GPU: the float64 reference of tests/coeff_ref64.py and the fp32 host mirrors of
oracle/coeff_oracle.py against the reference's own output (goldens g8, g14, g15), and the case table of tests/prepare_cases.py
against the launch decision of csrc/ncde_prepare.hip (``ncde_prepare_kernel_name``, a host function)."""
import json
import os

import numpy as np
import pytest

import golden_util as gu
import coeff_ref64 as ref64
import prepare_cases as pc

F32 = 2.0 ** -24      # fp32 unit round-off

# What the reference's own fp32 output may differ from exact arithmetic by, per series and section, relative to the section or --
# where that is smaller -- to the series' own values (floor = 1: an fp32 golden does not resolve a section below its own absolute
# error; the small sections are pinned by the float64 golden g15, whose bound resolves 1e-12 of the data):
#   NaN fill  x_p + ratio * (x_q - x_p): four roundings (ratio, difference, product, sum), each <= F32 relative to at most
#             twice the section's largest value -> 8 F32
#   spline    a diagonally dominant tridiagonal solve, condition <= 3 h_max / h_min (<= 17 for spacings in [0.3, 1.7]), a few F32 per
#             row operation, and the 2c / 3d rows subtract knot derivatives from slopes (cancellation up to ~ 10 x): 17 * 10 * F32 ~ 1e-5
LINEAR_F32, CUBIC_F32 = 8 * F32, 1e-5


def _g8():
    return np.load(os.path.join(gu.GOLD, "g8_coeffs.npz")), np.load(os.path.join(gu.GOLD, "g8_coeffs_user_grid.npz"))


def test_ref64_against_the_fp32_goldens_of_the_reference():
    g, gt = _g8()
    xm, xc, t = g["x_missing"], g["x_clean"], gt["t"]
    assert np.array_equal(ref64.linear(xm, rectilinear=0).astype(np.float32), g["rectilinear"])
    for f, tt in ((g, None), (gt, t)):
        e = pc.case_errors(f["linear"], ref64.linear(xm, t=tt), 1, floor=1.0)
        print("linear", "user grid" if tt is not None else "default grid", e)
        assert (e <= LINEAR_F32).all(), e
        for key, x, tk in (("cubic", xc, tt), ("cubic_missing", xm, tt), ("cubic_len2", xc[:, :2], None if tt is None else tt[:2])):
            e = pc.case_errors(f[key], ref64.natural_cubic(x, t=tk), 4, floor=1.0)
            print(key, "user grid" if tt is not None else "default grid", e)
            assert (e <= CUBIC_F32).all(), (key, e)


@pytest.mark.parametrize("name", ["g14_a_cubic_eps1_rk4", "g14_b_cubic_eps05_rk4", "g14_c_cubic_eps02_rk4_quarter", "g14_d_quintic_eps1_midpoint",
                                  "g14_e_quintic_eps05_rk4", "g14_f_quintic_eps03_euler_tenth", "g14_g_quintic_eps1_gru_evaluate",
                                  "g14_h_quintic_eps05_rk4_half_c20"])
def test_ref64_smooth_against_the_matching_coefficients_of_the_reference(name):
    """g14 holds the reference's fp32 matching coefficients and ``coeff_drift``, their distance (max abs) from the reference's own
    float64 ones: the closed forms of coeff_ref64.smooth must sit at that distance too, up to float64 round-off."""
    f = np.load(os.path.join(gu.GOLD, name + ".npz"))
    m = json.loads(str(f["meta"]))
    x, order = f["coeffs"], 5 if m["scheme"] == "quintic" else 3
    B, T, C = x.shape
    rows = ref64.smooth(x, m["eps"], order).reshape(B, -1, order + 1, C)
    match = rows[:, 1::2] if m["eps"] < 1 else rows[:, 1:]
    mc = f["matching_coeffs"].astype(np.float64)                                        # [B, T-2, C, order+1], highest power first
    err = max(float(np.abs(match[:, :, q] / max(q, 1) - mc[..., order - q]).max()) for q in range(order + 1))
    print(name, "err %.3e coeff_drift %.3e" % (err, m["coeff_drift"]))
    assert err <= m["coeff_drift"] * (1 + 1e-6) + 1e-12
    lin = rows[:, 0::2] if m["eps"] < 1 else rows[:, :1]
    assert not lin[:, :, 2:].any()


def test_ref64_against_the_float64_golden_of_the_reference():
    """g15: torchcde's builders in float64 on every gap pattern, default and user grid (oracle/gen_golden_prepare.py).  Two float64
    algorithms for one spline: 1e3 x the figure the generator observed, ~1e5 below fp32 resolution."""
    f = np.load(os.path.join(gu.GOLD, "g15_coeffs_f64.npz"))
    with open(os.path.join(gu.GOLD, "MANIFEST_prepare.json")) as fh:
        man = json.load(fh)
    bound = man["bound_factor"] * man["ref64_vs_reference_worst"]
    assert 0 < bound < 1e-3 * F32
    for s in man["sets"]:
        x, t = f[s["name"] + "_x"], f[s["name"] + "_t"]
        assert x.shape == (s["B"], s["L"], s["C"]) and np.isnan(x).any()
        for grid, tt in (("", None), ("_t", t)):
            for what, got, ns in (("linear", ref64.linear(x, t=tt), 1), ("cubic", ref64.natural_cubic(x, t=tt), 4)):
                want = f["%s_%s%s" % (s["name"], what, grid)]
                assert want.dtype == np.float64 and got.shape == want.shape
                e = float(pc.case_errors(got, want, ns, floor=1.0).max())
                print(s["name"], what + grid, "%.3e" % e)
                assert e <= bound, (s["name"], what, grid, e, bound)
                # a (series, section) the reference makes exactly zero (two knots, one or no observation) is exactly zero here
                N, T = want.shape[0], want.shape[1]
                gs, ws = (np.abs(a.reshape(N, T, ns, -1)).max(axis=1) for a in (got, want))
                assert (ws == 0).any() and not gs[ws == 0].any()


def test_host_mirrors_with_a_user_grid_are_the_reference_bit_for_bit():
    g, gt = _g8()
    xm, xc, t = g["x_missing"], g["x_clean"], gt["t"]
    data = gu.data
    assert np.array_equal(data.linear_interpolation_coeffs(xm), g["linear"])
    assert np.array_equal(data.linear_interpolation_coeffs(xm, t=t), gt["linear"])
    assert np.array_equal(data.natural_cubic_coeffs(xc, t=t), gt["cubic"])
    assert np.array_equal(data.natural_cubic_coeffs(xc[:, :2], t=t[:2]), gt["cubic_len2"])
    assert np.array_equal(data.natural_cubic_coeffs(xm, t=t), gt["cubic_missing"])
    # t = the integer grid is the default grid
    L = xm.shape[1]
    assert np.array_equal(data.natural_cubic_coeffs(xm, t=np.arange(L, dtype=np.float32)), g["cubic_missing"])
    assert np.array_equal(data.natural_cubic_coeffs(xc, t=np.arange(L, dtype=np.float32)), g["cubic"])


def test_two_knot_series_are_exactly_linear_in_mirror_and_ref64():
    """Ends-only observations: the reference's length-2 branch, b = dx / dt and 2c = 3d = 0 exactly (interpolation_cubic.py:16-20)."""
    for L in (3, 4, 12, 40):
        x = np.full((1, L, 2), np.nan, np.float32)
        x[0, 0], x[0, -1] = (0.3, -1.25), (1.7, 2.5)
        t = np.cumsum(0.3 + 1.4 * gu.data.uniform01(5, L, stream=3)).astype(np.float32)
        for tt in (None, t):
            for out in (gu.data.natural_cubic_coeffs(x, t=tt), ref64.natural_cubic(x, t=tt)):
                assert not out[0, :, 4:].any()
                assert (out[0, :, 2:4] == out[0, 0, 2:4]).all()


def test_case_table_reaches_the_launch_paths_it_names():
    """Every case of the GPU table against the dispatch of ncde_prepare.hip -- a case that means the global-memory kernel and lands on
    the LDS one would test nothing.  Together the cases reach every path."""
    import ncde_amd
    lib = ncde_amd.lib()
    assert len(set(pc.IDS)) == len(pc.IDS)
    for case in pc.CASES:
        assert pc.kernel_name(lib, case) == case[8], (case[0], pc.kernel_name(lib, case))
        if case[1] == "smooth":
            B, T, C, eps = case[2], case[3], case[4], case[9]
            P = lib.ncde_smooth_pieces(T, eps)
            assert P == ref64.smooth_pieces(T, eps)
            assert (B * P * C > pc.SMOOTH_GRID_ELEMS) == case[0].endswith("_big"), case[0]
    paths = {c[8] for c in pc.CASES}
    assert {pc.LDS, pc.V1, pc.CUB, pc.SMOOTH, pc._cl(1)} <= paths and len([p for p in paths if p.startswith("ncde_cubic_coeffs_lds")]) >= 6
    # the query refuses what the builders refuse
    for bad in ((0, 0, 5, 3, 0, -1), (0, 2, 1, 3, 0, -1), (1, 2, 5, 0, 0, -1), (0, 2, 5, 3, 0, 3), (2, 2, 5, 3, 0, -1), (7, 2, 5, 3, 0, -1)):
        assert lib.ncde_prepare_kernel_name(*bad) is None, bad


@pytest.mark.parametrize("case", pc.CASES, ids=pc.IDS)
def test_case_inputs_and_mirrors(case):
    """The inputs hold the gap patterns the case names; the fp32 mirror of the linear builders sits within fp32 distance of the
    float64 reference (the bound of the goldens above).  Spline and smooth: E_mirror is printed -- it is the yardstick of the GPU
    test, not a claim of its own (the big smooth cases are left to the GPU run)."""
    x, t = pc.make_input(case)
    name, builder, B, L, C, grid, rect, gaps = case[:8]
    assert x.shape == (B, L, C) and x.dtype == np.float32 and (t is None) == (not grid)
    if gaps == "edges":
        ps = pc.pattern_series(case)
        obs = {p: np.nonzero(~np.isnan(x[b, :, c]))[0] for p, (b, c) in ps.items()}
        assert obs["all_nan"].size == 0 and list(obs["ends_only"]) == sorted({0, L - 1})
        assert list(obs["one_first"]) == [0] and list(obs["one_middle"]) == [L // 2] and list(obs["one_last"]) == [L - 1]
        assert obs["leading"][0] == max(1, L // 3) and obs["trailing"][-1] == L - max(1, L // 3) - 1
        if rect is not None:
            assert not np.isnan(x[:, :, rect]).any()
    elif gaps == "samples_3_41":
        assert sorted(set(np.nonzero(np.isnan(x).any(axis=(1, 2)))[0])) == [3, 41]
    else:
        assert not np.isnan(x).any()
    if t is not None:
        d = np.diff(t.astype(np.float64))
        assert d.min() >= 0.3 - 1e-6 and d.max() <= 1.7 + 1e-6
    if builder == "smooth" and B * L * C > 100000:
        return
    mir, want = pc.mirror(case, x, t), pc.reference64(case, x, t)
    assert mir.shape == want.shape and mir.dtype == np.float32 and np.isfinite(mir).all()
    e = pc.case_errors(mir, want, pc.sections(case), floor=1.0 if builder == "linear" else 2.0 ** -24)
    print(name, "E_mirror", e)
    if builder == "rect":
        assert np.array_equal(mir, want.astype(np.float32))
    elif builder == "linear":
        assert (e <= LINEAR_F32).all(), e
