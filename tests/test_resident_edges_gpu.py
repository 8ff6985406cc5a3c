"""The register-resident kernels at the edges of their bookkeeping (tests/resident_cases.py) against the fp64 oracle: ring phases of
the dX/dt ring (1 .. 6 pieces), one-record discrete backwards, slot words of the zero-quad skip on short rectilinear paths, one
live lane / one full tile / a one-sample tail tile, degenerate time plans, range faults that appear late or in a one-sample tile.
Every case asserts the instantiation it runs on (ncde_kernel_name), the project's bounds (TIGHT_Z on z; TIGHT_G on a backward
kernel fed the oracle's own z / stage record rounded to fp32; E2E_G end to end) and no per-row ReLU-flip allowance: the cases are
screened on the CPU instead (tests/test_resident_edges_cpu.py)."""
import numpy as np
import pytest
import torch

import golden_util as gu
import resident_cases as rc

pytestmark = pytest.mark.gpu


def _flags():
    from ncde_amd import _lib
    return _lib


def _same(a, b):
    return torch.equal(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b)))


def _assert_names(name, got):
    want = rc.want_names(name)
    for ps, (g, w) in enumerate(zip(got, want)):
        assert rc.name_matches(g, w), (name, ps, g, w)


def _iso(name, case, ex, flags=0, passes=("adjoint", "discrete"), tag=""):
    """The backward kernels fed the fp64 oracle's z_out / stage record rounded to fp32 -> {pass: result}; TIGHT_G on every gradient."""
    import gpu_util
    out = {}
    for ps in passes:
        stages = ex["stages"].astype(np.float32) if ps == "discrete" else None
        res = gpu_util.run_adjoint_direct(case, ex["z_out"].astype(np.float32), flags=flags, stages=stages)
        rc.check("%s %s%s on the oracle's %s [%s]" % (name, ps, tag, "record" if stages is not None else "z", res["kernel"]),
                 rc.errors(res, ex[ps], rc.names_of(name)), rc.TIGHT_G)
        out[ps] = res
    return out


def _default_axis(name, flags=0, iso_passes=("adjoint", "discrete")):
    """Forward + continuous adjoint + adjoint=False end to end, and both backward kernels in isolation."""
    import gpu_util
    case, ex, names = rc.golden_case(name), rc.expect(name), rc.names_of(name)
    res = gpu_util.run_case(case, flags=flags)
    if flags == 0:
        _assert_names(name, res["kernels"])
    assert np.isfinite(res["z_out"]).all() and res["z_out"].shape == ex["z_out"].shape
    rc.check(name + " end to end, adjoint", rc.errors(res, ex["adjoint"], names, (res["z_out"], ex["z_out"])), rc.E2E_G)
    resd = gpu_util.run_case(case, flags=flags, adjoint=False)
    assert np.array_equal(resd["z_out"], res["z_out"])      # recording does not change the solution
    rc.check(name + " end to end, discrete", rc.errors(resd, ex["discrete"], names), rc.E2E_G)
    iso = _iso(name, case, ex, flags, iso_passes)
    return res, resd, iso


@pytest.mark.parametrize("name", [n for n in rc.BY_GROUP["ring"] if rc.CASES[n]["set"] == "R20"])
def test_ring_phases_on_the_unrolled_set(name, gpu_lib):
    """(32, 32, 20), three layers: T = 2 .. 7 knots x path x method x output mode on the unrolled forward and ncde_adj_fast3,
    continuous and discrete, and the backward's other instantiations (single-role, fp32 chain, decoupled waves, all split-bf16,
    fp32-input MFMA, dense channels) on the oracle's z / stage record.  At T = 2 and T = 4 a second launch must repeat the first
    bit for bit (the prologue is the whole solve / the ring wraps once)."""
    import gpu_util
    L = _flags()
    res, resd, iso = _default_axis(name)
    case, ex = rc.golden_case(name), rc.expect(name)
    for fl, tag in ((L.FLAG_SPLIT_BF16, "split-bf16"), (L.FLAG_FP32_MFMA, "fp32 MFMA")):
        r = gpu_util.run_case(case, flags=fl, need_grads=False)
        rc.check("%s forward %s [%s]" % (name, tag, r["kernels"][0]), {"z": gu.relerr(r["z_out"], ex["z_out"])}, rc.TIGHT_G)
    for fl, tag in ((L.FLAG_ADJOINT_V1, " V1"), (L.FLAG_ADJOINT_V2, " V2"), (L.FLAG_ADJOINT_V4, " V4"), (L.FLAG_SPLIT_BF16, " split-bf16"),
                    (L.FLAG_FP32_MFMA, " fp32 MFMA"), (L.FLAG_DENSE_CHANNELS, " dense")):
        _iso(name, case, ex, fl, tag=tag)
    if rc.CASES[name]["T"] in (2, 4):
        again = _iso(name, case, ex)
        for ps in again:
            assert _same(again[ps]["dz0"], iso[ps]["dz0"]), (name, ps)
            assert all(_same(again[ps]["grads"][k], iso[ps]["grads"][k]) for k in iso[ps]["grads"]), (name, ps)


@pytest.mark.parametrize("name", [n for n in rc.BY_GROUP["ring"] if rc.CASES[n]["set"] != "R20"])
def test_ring_phases_on_the_other_sets(name, gpu_lib):
    """T = 2 and T = 4 on the other layer counts, the few-channel sets, the forward-only set (its backward wherever the dispatcher
    sends it), (64, 64, 4) with one and two sample tiles per workgroup, and the zero-padded shapes (row width != kernel width)."""
    L = _flags()
    _default_axis(name)
    if rc.CASES[name]["set"] in ("R64", "pad3"):
        case, ex = rc.golden_case(name), rc.expect(name)
        for fl, tag in ((L.FLAG_TILED_NS1, " NS1"), (L.FLAG_TILED_NS2, " NS2")):
            _iso(name, case, ex, fl, tag=tag)


@pytest.mark.parametrize("name", rc.BY_GROUP["skip"])
def test_slot_words_on_short_rectilinear_paths(name, gpu_lib):
    """Raw length 2, 3, 4: the slot words of the zero-quad skip change owner on every step and, at 3 and 5 knots, are never cleared
    in the steady state.  Against fp64, and the default run against the NCDE_FLAG_DENSE_CHANNELS run: equal up to the sign of a zero."""
    L = _flags()
    c, a = rc.CASES[name], rc.arrays(name)
    d = a["coeffs"][:, 1:, 1:] - a["coeffs"][:, :-1, 1:]
    narrow = [q for q in range(d.shape[1]) if not np.any(d[:, q, 3:])]
    if c["bump"] is None:
        assert 0 < len(narrow) < d.shape[1], (name, narrow)
    else:      # the only time-only piece of the three-knot path: one sample sends its tile wide on it
        s, _, ch, _ = c["bump"]
        q = a["bump_piece"]
        assert d[s, q, ch - 1] != 0 and np.count_nonzero(d[:, q]) == 1 and narrow == []
    skip = _default_axis(name)
    dense = _default_axis(name, flags=L.FLAG_DENSE_CHANNELS)
    for (s_, d_), what in zip(zip(skip[:2], dense[:2]), ("adjoint", "discrete")):
        assert s_["kernels"] == d_["kernels"]
        assert _same(s_["z_out"], d_["z_out"]) and _same(s_["dz0"], d_["dz0"]), (name, what)
        assert all(_same(s_["grads"][k], d_["grads"][k]) for k in s_["grads"]), (name, what)
    for ps in skip[2]:
        assert _same(skip[2][ps]["dz0"], dense[2][ps]["dz0"]), (name, ps)
        assert all(_same(skip[2][ps]["grads"][k], dense[2][ps]["grads"][k]) for k in skip[2][ps]["grads"]), (name, ps)


@pytest.mark.parametrize("T", [2, 4])
@pytest.mark.parametrize("kset", rc.BATCH_SETS)
def test_batch_edges_and_sample_independence(kset, T, gpu_lib):
    """B = 1 (one live lane), B = 16 (one full tile, no tail), B = 33 (a one-sample tail tile): each against fp64, and bitwise on
    z: the first 16 rows of the B = 33 run are the B = 16 run, its row 32 is the B = 1 run of that sample."""
    z = {}
    for B in (33, 16, 1):
        name = "batch_%s_T%d_B%d" % (kset, T, B)
        z[B] = _default_axis(name)[0]["z_out"]
    assert _same(z[33][:16], z[16]) and _same(z[33][32:], z[1])


@pytest.mark.parametrize("name", rc.BY_GROUP["plan"])
def test_plan_edges(name, gpu_lib):
    """Degenerate time plans on the planned instantiations: forward, continuous adjoint and adjoint=False, all split-bf16 and default."""
    import gpu_util
    L = _flags()
    _assert_names(name, rc.kernel_names(name, device="cuda")[0])
    ex, names = rc.expect(name), rc.names_of(name)
    f, meta = rc.times_case(name)
    for flags in (L.FLAG_SPLIT_BF16, 0):
        res = gpu_util.run_times_case(f, meta, adjoint=True, params=rc.arrays(name)["params"], flags=flags)
        assert res["z_out"].shape == ex["z_out"].shape and np.isfinite(res["z_out"]).all()
        rc.check("%s adjoint flags %#x" % (name, flags), rc.errors(res, ex["adjoint"], names, (res["z_out"], ex["z_out"])), rc.E2E_G)
        resd = gpu_util.run_times_case(f, meta, adjoint=False, params=rc.arrays(name)["params"], flags=flags)
        rc.check("%s discrete flags %#x" % (name, flags), rc.errors(resd, ex["discrete"], names, (resd["z_out"], ex["z_out"])), rc.E2E_G)
        if name.split("_")[1] in ("c", "f"):      # the first and the last piece are never read: poisoned, bit for bit the same results
            fp, _ = rc.times_case(name, rc.poisoned(name))
            for adjoint, want in ((True, res), (False, resd)):
                got = gpu_util.run_times_case(fp, meta, adjoint=adjoint, params=rc.arrays(name)["params"], flags=flags)
                assert _same(got["z_out"], want["z_out"]) and _same(got["dz0"], want["dz0"]), (name, flags, adjoint)
                assert all(_same(got["grads"][k], want["grads"][k]) for k in want["grads"]), (name, flags, adjoint)


@pytest.mark.parametrize("name", rc.BY_GROUP["fault"])
def test_range_faults_at_the_edges(name, gpu_lib):
    """A tile whose operands leave the fp16 range only from step 2 on (its earlier rows were already written by the split-fp16
    kernel), and a fault in a tail tile holding ONE sample: every row of the faulted tile is the split-bf16 run's, bit for bit, the
    other tiles' rows are those of the run without the outlier, all rows meet the fp64 bound (per sample: the outlier is 1e5 x
    the rest), and the parameter gradients of both backward kernels meet fp64 -- a faulted workgroup's partial is replaced, not
    added twice.  The tail outlier carries a full cotangent and 5 - 28 % of dW1, db1, dWo, dbo (resident_cases.arrays); the late one
    carries none, there the partial of the tile's other fifteen samples is what must be counted once."""
    import gpu_util
    L = _flags()
    c, a, ex = rc.CASES[name], rc.arrays(name), rc.expect(name)
    s = c["outlier"][0]
    lo, hi = 16 * (s // 16), min(16 * (s // 16) + 16, c["B"])
    case = rc.golden_case(name)
    plain = gpu_util.run_case(rc.golden_case(name, a["clean_coeffs"], a["clean_z0"]), need_grads=False)
    r16 = gpu_util.run_case(case, need_grads=False)
    rbf = gpu_util.run_case(case, flags=L.FLAG_SPLIT_BF16, need_grads=False)
    _assert_names(name, r16["kernels"])
    assert "fp16x2" in r16["kernels"][0] and "bf16x3" in rbf["kernels"][0], (r16["kernels"], rbf["kernels"])
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
    assert err <= rc.TIGHT_Z
    # the backward kernels on the oracle's z / stage record: the same re-execution, asserted the same way
    clean_case, exc = rc.golden_case(name, a["clean_coeffs"], a["clean_z0"]), rc.expect(name, clean=True)
    isoc = _iso(name, clean_case, exc, tag=" clean")
    iso = _iso(name, case, ex)
    isob = _iso(name, case, ex, L.FLAG_SPLIT_BF16, tag=" split-bf16")
    for ps in iso:
        assert np.isfinite(iso[ps]["dz0"]).all() and all(np.isfinite(v).all() for v in iso[ps]["grads"].values()), (name, ps)
        assert _same(iso[ps]["dz0"][lo:hi], isob[ps]["dz0"][lo:hi]), (name, ps)                  # the re-executed tile
        assert _same(iso[ps]["dz0"][rest], isoc[ps]["dz0"][rest]), (name, ps)                    # the other tiles: as without the outlier
        assert not _same(isoc[ps]["dz0"][rest], isob[ps]["dz0"][rest]), (name, ps)               # (the two kernels differ in the last bits)
        if len(others):
            assert not _same(iso[ps]["dz0"][others], isoc[ps]["dz0"][others]), (name, ps)        # ... and the backward faulted
    if c["outlier"][1] == "z0":
        # the one-sample tile's partial is no zero: a partial added twice, or not replaced, moves these tensors by >= 0.05 of their maximum
        share = rc.outlier_share(name)
        assert all(share[ps][n] >= 0.05 for ps in share for n in rc.names_of(name) if n not in ("W0", "b0")), share
        assert np.abs(ex["adjoint"]["dz0"][s]).max() >= rc.MIN_GRAD
