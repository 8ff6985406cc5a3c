"""The batch-tiled kernels at the edges of their bookkeeping (tests/tiled_cases.py) against the fp64 oracle: one live lane / one exact
tile / one exact tile pair / a one-sample unpaired tile / uneven tile ownership of the pass-B waves / two part-groups; one- and
two-step solves; degenerate time plans on the family's own plan walk with time-window hand-overs on and beside the end of a reverse
solve; range faults of the split-fp16 forward.  Every case asserts the instantiation it runs on (ncde_kernel_name), the project's
bounds (TIGHT_Z on z; TIGHT_G on a backward kernel fed the oracle's own z / stage record rounded to fp32; E2E_G end to end) and no
per-row ReLU-flip allowance: the cases are screened on the CPU instead (tests/test_tiled_edges_cpu.py)."""
import numpy as np
import pytest
import torch

import golden_util as gu
import tiled_cases as tc

pytestmark = pytest.mark.gpu
HEADS = ("Wo", "bo", "Wg", "bg")
WINDOW_SUM = 2e-6      # head gradients of a windowed run: summation order only (one pass-B partial per window)


def _L():
    from ncde_amd import _lib
    return _lib


def _same(a, b):
    return torch.equal(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b)))


def _assert_names(name, got):
    for ps, (g, w) in enumerate(zip(got, tc.want_names(name))):
        assert tc.name_matches(g, w), (name, ps, g, w)


def _finite(res):
    return np.isfinite(res["dz0"]).all() and all(np.isfinite(v).all() for v in res["grads"].values())


def _iso(name, case, ex, flags, passes=("adjoint", "discrete"), tag=""):
    """The backward kernels fed the fp64 oracle's z_out / stage record rounded to fp32 -> {pass: result}; TIGHT_G on every gradient."""
    import gpu_util
    out = {}
    for ps in passes:
        stages = ex["stages"].astype(np.float32) if ps == "discrete" else None
        res = gpu_util.run_adjoint_direct(case, ex["z_out"].astype(np.float32), flags=flags, stages=stages)
        assert res["kernel"].startswith("ncde_adj_tiled"), (name, ps, res["kernel"])
        tc.check("%s %s%s on the oracle's %s [%s]" % (name, ps, tag, "record" if stages is not None else "z", res["kernel"]),
                 tc.errors(res, ex[ps], tc.names_of(name)), tc.TIGHT_G)
        out[ps] = res
    return out


def _default_axis(name):
    """Forward + continuous adjoint + adjoint=False end to end, and both backward kernels in isolation, under the set's own flags."""
    import gpu_util
    case, ex, names, flags = tc.golden_case(name), tc.expect(name), tc.names_of(name), tc.flags_of(name)
    res = gpu_util.run_case(case, flags=flags)
    _assert_names(name, res["kernels"])
    assert np.isfinite(res["z_out"]).all() and res["z_out"].shape == ex["z_out"].shape
    tc.check(name + " end to end, adjoint", tc.errors(res, ex["adjoint"], names, (res["z_out"], ex["z_out"])), tc.E2E_G)
    resd = gpu_util.run_case(case, flags=flags, adjoint=False)
    assert np.array_equal(resd["z_out"], res["z_out"])      # recording does not change the solution
    tc.check(name + " end to end, discrete", tc.errors(resd, ex["discrete"], names), tc.E2E_G)
    return res, resd, _iso(name, case, ex, flags)


def _assert_window_run_equals(label, got, want):
    """A run under forced time windows against the single-window run: dL/dz0 and the hidden-layer gradients bit for bit (the carried
    (y, a) and the hidden-layer partial are exact hand-overs), the head gradients to summation order."""
    assert _finite(got), label
    assert _same(got["dz0"], want["dz0"]), label
    for k in want["grads"]:
        if k in HEADS:
            assert gu.relerr(got["grads"][k], want["grads"][k]) <= WINDOW_SUM, (label, k, gu.relerr(got["grads"][k], want["grads"][k]))
        else:
            assert _same(got["grads"][k], want["grads"][k]), (label, k)


def _assert_repeats(label, got, want):
    assert _same(got["dz0"], want["dz0"]) and all(_same(got["grads"][k], want["grads"][k]) for k in want["grads"]), label


@pytest.mark.parametrize("kset", tc.BATCH_SETS)
def test_batch_edges(kset, gpu_lib):
    """B = 1, 16, 17, 32, 33, 97, 129, each against fp64 (default flags, and every backward under NCDE_FLAG_FP32_MFMA: fp32 records
    and ncde_dwo_tiled on every set); sample independence of the forward, bitwise: rows [0:16] / [0:32] / 128 of the B = 129 run are
    the B = 16 / 32 / 1 runs; at B = 17 and 97 the forward's other instantiations (two and four sample tiles per workgroup: ragged
    workgroups with empty tiles; all split-bf16; fp32-input MFMA); at B = 97 and 129 a second backward launch repeats the first bit
    for bit (the partials of every part-group are written, not accumulated)."""
    import gpu_util
    L = _L()
    own = tc.SETS[kset][6]
    z1 = {}
    for B in tc.BATCH_SIZES:
        name = "batch_%s_B%d" % (kset, B)
        case, ex = tc.golden_case(name), tc.expect(name)
        _, _, iso = _default_axis(name)
        _iso(name, case, ex, own | L.FLAG_FP32_MFMA, tag=" fp32 MFMA")
        if B in (129, 16, 32, 1):
            r = gpu_util.run_case(case, flags=own | L.FLAG_TILED_NS1, need_grads=False)
            tc.check("%s forward NS1 [%s]" % (name, r["kernels"][0]), {"z": gu.relerr(r["z_out"], ex["z_out"])}, tc.TIGHT_G)
            z1[B] = r["z_out"]
        if B in (17, 97):
            bf = "bf16" if tc.SETS[kset][2] in (32, 64, 128) else "NS1"      # (a last width of 16 has no split output tiles)
            for fl, tag in ((L.FLAG_TILED_NS2, "NS2"), (L.FLAG_TILED_NS4, "NS4"), (L.FLAG_SPLIT_BF16, bf), (L.FLAG_FP32_MFMA, "NS1")):
                r = gpu_util.run_case(case, flags=own | fl, need_grads=False)
                assert tag in r["kernels"][0] and "fp16x2" not in r["kernels"][0], (name, tag, r["kernels"])
                tc.check("%s forward %s [%s]" % (name, tag, r["kernels"][0]), {"z": gu.relerr(r["z_out"], ex["z_out"])}, tc.TIGHT_G)
        if B in (97, 129):
            again = _iso(name, case, ex, own, tag=" again")
            for ps in again:
                _assert_repeats((name, ps), again[ps], iso[ps])
    assert _same(z1[129][:16], z1[16]) and _same(z1[129][:32], z1[32]) and _same(z1[129][128:], z1[1])


@pytest.mark.parametrize("B", tc.EULER_SIZES)
def test_batch_edges_odd_fragment_count(B, gpu_lib):
    """Euler over three steps on the fp32-record set: the only stage count at which a wave of ncde_dwo_tiled steps through an odd
    number of fragments, and so consumes the zero-cotangent fragment it fetched past the end (tiled_cases)."""
    _default_axis("batch_T16_euler_B%d" % B)


@pytest.mark.parametrize("name", tc.BY_GROUP["steps"])
def test_short_solves(name, gpu_lib):
    """One and two steps on every set: the prologue is the whole solve / the sweep hands over once.  Default flags against fp64, and
    windows of one step against the default run (T = 3: two windows)."""
    L = _L()
    _, _, iso = _default_axis(name)
    case, ex = tc.golden_case(name), tc.expect(name)
    win = _iso(name, case, ex, tc.flags_of(name) | L.FLAG_TILED_WINDOW_STEPS(1), tag=" window 1")
    for ps in win:
        _assert_window_run_equals((name, ps), win[ps], iso[ps])


@pytest.mark.parametrize("name", tc.BY_GROUP["plan"])
def test_plan_edges(name, gpu_lib):
    """Degenerate time plans on the family's own plan walk: the planned forward, the planned continuous sweep and the planned
    discrete backward against fp64 -- with the default window (the larger of the two step counts) and with forced windows of 1 and 2
    reverse steps, whose boundaries fall on / beside the end of a reverse solve (tiled_cases.PLAN_WINDOWS) -- and, plans (c) and (f),
    bit for bit the same on coefficients whose never-read pieces are poisoned.  Plan (f) runs with an fp64 t."""
    import gpu_util
    L = _L()
    own = tc.flags_of(name)
    _assert_names(name, tc.kernel_names(name, device="cuda"))
    ex, names, params = tc.expect(name), tc.names_of(name), tc.arrays(name)["params"]
    f, meta, kind, mode = tc.times_case(name)
    assert f["t_out"].dtype == (np.float64 if name.split("_")[1] == "f" else np.float32)
    base = {}
    for w in (0, 1, 2):
        flags = own | (L.FLAG_TILED_WINDOW_STEPS(w) if w else 0)
        for adjoint, ps in ((True, "adjoint"), (False, "discrete")):
            res = gpu_util.run_times_case(f, meta, adjoint=adjoint, params=params, flags=flags, kind=kind, mode=mode)
            assert res["z_out"].shape == ex["z_out"].shape and np.isfinite(res["z_out"]).all()
            tc.check("%s %s window %d" % (name, ps, w), tc.errors(res, ex[ps], names, (res["z_out"], ex["z_out"])), tc.E2E_G)
            if w == 0:
                base[ps] = res
            else:
                assert _same(res["z_out"], base[ps]["z_out"]), (name, ps, w)
                _assert_window_run_equals((name, ps, w), res, base[ps])
            if name.split("_")[1] in ("c", "f") and w in (0, 2):      # the first and the last piece are never read
                fp, _, _, _ = tc.times_case(name, tc.poisoned(name))
                got = gpu_util.run_times_case(fp, meta, adjoint=adjoint, params=params, flags=flags, kind=kind, mode=mode)
                assert _same(got["z_out"], res["z_out"]), (name, ps, w)
                _assert_repeats((name, ps, w, "poisoned"), got, res)


@pytest.mark.parametrize("name", tc.BY_GROUP["fault"])
def test_range_faults_of_the_forward(name, gpu_lib):
    """A tile whose operands leave the fp16 range only from step 2 on (its earlier rows were already written by the split-fp16
    kernel), and a fault in a tail tile holding ONE sample: every row of the faulted tile is the split-bf16 run's, bit for bit, the
    other tiles' rows are those of the run without the outlier, all rows meet the fp64 bound (per sample: the outlier is 1e5 x the
    rest).  The backward of this family does not speculate on range: it is held to fp64 on the clean batch."""
    import gpu_util
    L = _L()
    c, a, ex, own = tc.CASES[name], tc.arrays(name), tc.expect(name), tc.flags_of(name)
    s = c["outlier"][0]
    lo, hi = 16 * (s // 16), min(16 * (s // 16) + 16, c["B"])
    case, clean_case = tc.golden_case(name), tc.golden_case(name, a["clean_coeffs"], a["clean_z0"])
    plain = gpu_util.run_case(clean_case, flags=own, need_grads=False)
    r16 = gpu_util.run_case(case, flags=own, need_grads=False)
    rbf = gpu_util.run_case(case, flags=own | L.FLAG_SPLIT_BF16, need_grads=False)
    _assert_names(name, r16["kernels"])
    assert "fp16x2" in r16["kernels"][0] and "bf16" in rbf["kernels"][0], (r16["kernels"], rbf["kernels"])
    assert np.isfinite(r16["z_out"]).all()
    assert _same(r16["z_out"][lo:hi], rbf["z_out"][lo:hi])                                  # the re-executed tile, early rows included
    rest = np.r_[0:lo, hi:c["B"]]
    assert _same(r16["z_out"][rest], plain["z_out"][rest])
    assert not _same(plain["z_out"][rest], rbf["z_out"][rest])      # the two kernels differ in the last bits: the tile above came from the second
    others = np.r_[lo:s, s + 1:hi]
    if len(others):
        assert not _same(r16["z_out"][others], plain["z_out"][others])                      # ... and the fault happened
    scale = np.abs(ex["z_out"]).max(axis=(1, 2), keepdims=True)
    err = float((np.abs(r16["z_out"] - ex["z_out"]) / scale).max())
    print(name, "z per sample %.2e" % err)
    assert err <= tc.TIGHT_Z
    _iso(name, clean_case, tc.expect(name, clean=True), own, tag=" clean")
