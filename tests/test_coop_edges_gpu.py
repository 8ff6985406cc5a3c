"""The XCD-cooperative kernels at the edges of their bookkeeping (tests/coop_cases.py) against the fp64 oracle: every group size below
cfg5's, several groups in one launch, a launch of one group behind a launch of 64, and the power-of-two scales on inputs of mixed
magnitude.  Every case runs the forward, the continuous adjoint on the oracle's z and the exact discrete backward on the oracle's
stage record, and asserts: "coop" in the three kernel names; the cooperative status word 0 after each pass (a run that timed out and
was redone by the per-workgroup kernels does not count); z within TIGHT_Z, dL/dz0 and every parameter gradient within TIGHT_G of fp64;
NaN-filled gradient buffers come back finite; a second call repeats the first bit for bit.  No per-row ReLU-flip allowance: the cases
are screened on the CPU instead (tests/test_coop_edges_cpu.py)."""
import numpy as np
import pytest
import torch

import coop_cases as cc
import golden_util as gu

pytestmark = pytest.mark.gpu
WINDOW_DZ0, WINDOW_THETA = 1e-6, 2e-6      # a windowed run against the single-window run (test_cooperative_output_phase_vs_oracle)
PASSES = ("adjoint", "discrete")


def _L():
    from ncde_amd import _lib
    return _lib


def _same(a, b):
    return torch.equal(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b)))


def _finite(res):
    return np.isfinite(res["dz0"]).all() and all(np.isfinite(v).all() for v in res["grads"].values())


def _backward(name, ps, flags=0, tag=""):
    """One backward kernel sequence fed the fp64 oracle's z_out / stage record rounded to fp32; name, status word, finiteness."""
    import gpu_util
    case, ex = cc.golden_case(name), cc.expect(name)
    stages = ex["stages"].astype(np.float32) if ps == "discrete" else None
    res = gpu_util.run_adjoint_direct(case, ex["z_out"].astype(np.float32), flags=flags, stages=stages)
    assert gpu_util.coop_status_word(case, 2 if ps == "discrete" else 1, flags=flags) == 0, (name, ps, tag)
    assert "coop" in res["kernel"] and "ncde_dwo_h2" in res["kernel"] and ("discrete" in res["kernel"]) == (ps == "discrete"), res["kernel"]
    assert _finite(res), (name, ps, tag)      # (the buffers went in NaN-filled: gpu_util.prepare_adjoint)
    return res


def _run(name, per_row=False, windows=(0,)):
    """The three passes of a case -> (z, {pass: result}).  per_row: dL/dz0 row by row, each relative to its own maximum in fp64
    (PER_ROW_G), the parameter gradients relative to the tensor's maximum as everywhere."""
    import gpu_util
    L = _L()
    case, ex, names = cc.golden_case(name), cc.expect(name), cc.names_of(name)
    got = gpu_util.kernel_names(case)
    assert all("coop" in k for k in got), (name, got)
    fw = gpu_util.run_case(case, need_grads=False)
    assert gpu_util.coop_status_word(case, 0) == 0, name
    assert fw["z_out"].shape == ex["z_out"].shape and np.isfinite(fw["z_out"]).all()
    cc.check("%s forward [%s]" % (name, fw["kernels"][0]), {"z": gu.relerr(fw["z_out"], ex["z_out"])}, cc.TIGHT_G)
    assert _same(gpu_util.run_case(case, need_grads=False)["z_out"], fw["z_out"]), name
    out = {}
    for ps in PASSES:
        for w in windows:
            tag = " window %d" % w if w else ""
            res = _backward(name, ps, L.FLAG_TILED_WINDOW_STEPS(w) if w else 0, tag)
            errs = cc.errors(res, ex[ps], names)
            if per_row:
                errs["dz0 per row"] = cc.row_err(res["dz0"], ex[ps]["dz0"])
                assert cc.PER_ROW_G == cc.TIGHT_G
            cc.check("%s %s%s [%s]" % (name, ps, tag, res["kernel"]), errs, cc.TIGHT_G)
            if w == 0:
                out[ps] = res
                again = _backward(name, ps, 0, " again")
                assert _same(again["dz0"], res["dz0"]) and all(_same(again["grads"][k], res["grads"][k]) for k in res["grads"]), (name, ps)
            elif ps == "adjoint" or per_row:      # against the single-window run
                e = {k: gu.relerr(res["grads"][k], out[ps]["grads"][k]) for k in res["grads"]}
                print(name, ps, tag, "vs one window: dz0 %.2e" % gu.relerr(res["dz0"], out[ps]["dz0"]), e)
                if not per_row:
                    assert gu.relerr(res["dz0"], out[ps]["dz0"]) <= WINDOW_DZ0 and all(v <= WINDOW_THETA for v in e.values()), (name, ps, e)
    return fw["z_out"], out


@pytest.mark.parametrize("name", cc.BY_GROUP["size"])
def test_group_sizes(name, gpu_lib):
    """M = 4, 12, 16, 20, 24, 28 with one group each, H = 16 .. 128, one to three layers, three ragged batches; uneven my_n at M = 12
    (2, 2, 1, 1) and M = 20 .. 28.  M = 12 and M = 20 also in two time windows (NCDE_FLAG_TILED_WINDOW_STEPS(1)): within 1e-6 (dz0) /
    2e-6 (parameters) of the single-window run."""
    _run(name, windows=(0, 1) if name in cc.WINDOWED else (0,))


def test_several_groups_and_sample_independence(gpu_lib):
    """G = 6 groups of 4 (parts = 8: the XCD-mapped branch of ncde_dwo_h2, nrg = 5) and G = 2 groups of 12 (my_n = 2, 2, 2, 2, 1, 1,
    1, 1) in one launch; their row subsets as one group: z and dL/dz0 of the shared rows against each other's fp64 rows (the same
    numbers), each within TIGHT_Z / TIGHT_G."""
    for big, small in (("groups_M4_B384", "groups_M4_B64"), ("groups_M12_B384", "size_M12_C80_H48")):
        lo, hi = cc.CASES[small]["rows"]
        zb, rb = _run(big)
        zs, rs = _run(small)
        eb, es = cc.expect(big), cc.expect(small)
        assert np.array_equal(eb["z_out"][lo:hi], es["z_out"])
        errs = {"z": max(gu.relerr(zb[lo:hi], es["z_out"]), gu.relerr(zs, eb["z_out"][lo:hi]))}
        for ps in PASSES:
            assert np.array_equal(eb[ps]["dz0"][lo:hi], es[ps]["dz0"])
            errs[ps + " dz0"] = max(gu.relerr(rb[ps]["dz0"][lo:hi], es[ps]["dz0"]), gu.relerr(rs[ps]["dz0"], eb[ps]["dz0"][lo:hi]))
        cc.check("%s rows %d:%d vs %s" % (big, lo, hi, small), errs, cc.TIGHT_G)


def test_chunk_tail_at_the_smallest_width(gpu_lib):
    """260 tiles of C 80 / H 16 / one layer: a launch of 256 tiles (64 groups) and one of 4 (one group; thirty of its 32 pass-B
    workgroups per row group have no pair).  dL/dz0 per row in the measure of test_cooperative_kernels_on_more_sample_tiles_than_cus
    -- with ZERO rows off: the CPU screening (ii) leaves no pre-activation within rounding of zero, so the COOP_FLIP_ROWS allowance
    of that test is not used here -- and per row relative to the row's own maximum; the last 64 samples against the B = 64 case of
    the group-size table (the same inputs); the recording forward's z bit for bit the plain forward's."""
    import gpu_util
    big, small = "tail_M4_B4160", "size_M4_C80_H16"
    lo, hi = cc.CASES[small]["rows"]
    zb, rb = _run(big, per_row=True)
    eb, es = cc.expect(big), cc.expect(small)
    for ps in PASSES:
        n_off, worst = cc.rows_off(rb[ps]["dz0"], eb[ps]["dz0"])
        print(big, ps, "rows of dz0 beyond TIGHT_G: %d, worst %.2e" % (n_off, worst))
        assert n_off == 0 and worst <= cc.TIGHT_G, (ps, n_off, worst)
    zs, rs = _run(small)
    errs = {"z": max(gu.relerr(zb[lo:hi], es["z_out"]), gu.relerr(zs, eb["z_out"][lo:hi]))}
    for ps in PASSES:
        errs[ps + " dz0"] = max(gu.relerr(rb[ps]["dz0"][lo:hi], es[ps]["dz0"]), gu.relerr(rs[ps]["dz0"], eb[ps]["dz0"][lo:hi]))
    cc.check("%s rows %d:%d vs %s" % (big, lo, hi, small), errs, cc.TIGHT_G)
    case = cc.golden_case(big)
    fd = gpu_util.run_case(case, adjoint=False, need_grads=False)
    assert _same(fd["z_out"], zb)


@pytest.mark.parametrize("name", cc.BY_GROUP["scale"])
def test_scales(name, gpu_lib):
    """Cotangents of 2^-30 .. 2^20 across the samples of a tile and of 2^-20 .. 2^12 across the output times (sd per sample, sigma
    per window: one and two windows), states and paths of mixed binades (sx, sd, u_T), (Wo, bo) x 2^-8 and x the largest passing
    power of two (sw), a sample without a cotangent and one whose path does not move (the zero branch of coop_pow2_scale): dL/dz0
    per row, each row relative to its own fp64 maximum; a row that is exactly zero in fp64 is exactly zero."""
    c = cc.CASES[name]
    z, out = _run(name, per_row=True, windows=(0, 1) if c["var"][0] in ("gout_times", "gout_rows", "zeros") else (0,))
    if c["var"][0] == "zeros":
        ex = cc.expect(name)
        scale = np.abs(ex["z_out"]).max(axis=(1, 2), keepdims=True)
        assert float((np.abs(z - ex["z_out"]) / scale).max()) <= cc.TIGHT_Z
        for ps in PASSES:
            assert not np.any(out[ps]["dz0"][cc.ZERO_GOUT]) and np.isfinite(out[ps]["dz0"]).all()
    if c["var"][0] == "state_path":      # z per sample as well: the states differ by 2^4
        ex = cc.expect(name)
        scale = np.abs(ex["z_out"]).max(axis=(1, 2), keepdims=True)
        err = float((np.abs(z - ex["z_out"]) / scale).max())
        print(name, "z per sample %.2e" % err)
        assert err <= cc.TIGHT_Z
