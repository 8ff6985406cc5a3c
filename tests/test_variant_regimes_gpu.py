"""The variant kernels (ncde_fwd_variant / ncde_adj_variant) in every regime of their LDS plan and of the register weight-gradient
rule, at widths that are no multiple of 16, on one- and 17-sample tail tiles and on general time axes (tests/variant_cases.py; the
regimes are asserted without a GPU in tests/test_variant_plan_cpu.py).

Every case: the fused fp32 solve through ncde_amd.cdeint with warnings as errors, the library naming the variant kernels for the
captured problem, against the package's unfused torch-op solver in fp64 on the same inputs (which must emit its one warning).  The
reference runs the UNTIED stack -- each layer its own equal-valued tensors -- and a shared tensor's gradient is compared with the fp64
sum over its uses.  Tolerances are the project's: forward <= 2e-5, dL/dz0 and every parameter gradient <= 2e-4, as |delta| relative
to max |ref|; every gradient of the reference has a maximum >= 1e3 x the tolerance.  Then each launch on its own through the C ABI:
the recording forward equals the plain one bit for bit, a backward writes every element of NaN-filled buffers, and a second backward
gives the same bits."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import variant_cases as vc
from ncde_amd import _lib

pytestmark = pytest.mark.gpu

RUNS = [(n, m) for n in vc.WITH_BACKWARD for m in vc.ALL_MODES]


@functools.lru_cache(maxsize=None)
def _reference(name, mode):
    """The unfused solver in fp64 on the untied stack: computed once, shared, never modified."""
    return vc.solve(name, mode, torch.float64, "cuda", untie=True)


@functools.lru_cache(maxsize=None)
def _flags(name):
    """What pins the case to the variant family: nothing where the default dispatch already picks it (every GRU field), else
    FLAG_FORCE_GENERIC (original / minimal with the evaluate / derivative input may be zero-padded onto the batch-tiled family)."""
    default = vc.Direct(name).kernel_names()
    print(name, "default dispatch:", default)
    flags = 0 if default == vc.VARIANT_NAMES else _lib.FLAG_FORCE_GENERIC
    assert vc.Direct(name, flags).kernel_names() == vc.VARIANT_NAMES
    if vc.CASES[name]["kind"] == "gru":
        assert flags == 0, default
    return flags


def _bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


@pytest.mark.parametrize("name,mode", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_variant_regimes_vs_fp64(name, mode, gpu_lib):
    """Forward at 2e-5, dL/dz0 and every parameter gradient at 2e-4 of the fp64 unfused solve, end to end, on the continuous adjoint
    and on the exact discrete backward; the family under test is the one that ran."""
    assert vc.regime_of(name) == vc.CASES[name]["regime"]
    probs = []
    res = vc.solve(name, mode, torch.float32, "cuda", capture=probs, flags=_flags(name))
    a = vc.arrays(name)
    for p in probs:
        assert [(gpu_lib.ncde_kernel_name(ctypes.byref(p), ps) or b"?").decode() for ps in (0, 1, 2)] == vc.VARIANT_NAMES
    p = probs[-1]
    assert (p.batch, p.hidden, p.channels, p.n_layers) == (vc.CASES[name]["B"], vc.CASES[name]["H"], vc.CASES[name]["C"], len(a["layers"]))
    assert [(int(p.layer_out[l]), int(p.layer_in[l])) for l in range(p.n_layers)] == a["dims"]
    if name.startswith("K_"):
        assert p.output == _lib.OUT_TIMES and p.time_plan and p.n_steps_fwd >= 4
    assert set(res["grads"]) == set(a["names"])
    vc.check("%s %s" % (name, mode), res, _reference(name, mode), a["names"])


@pytest.mark.parametrize("name", vc.WITH_BACKWARD)
def test_variant_launches_in_isolation(name, gpu_lib):
    """One launch at a time through the C ABI: the forward that writes the stage record equals the plain forward bit for bit; each
    backward finds every gradient buffer filled with NaN and leaves it finite (each parameter written once and in full: no tail tile
    or padded row leaks in, none is left out) and within the tolerances of the fp64 solve; a second call gives the same bits,
    whether the partial lives in LDS or in global memory (one wave per address)."""
    d = vc.Direct(name, _flags(name))
    assert d.kernel_names() == vc.VARIANT_NAMES
    a = vc.arrays(name)
    out, none = d.forward()
    rec_out, stages = d.forward(record=True)
    assert none is None and stages is not None and bool(torch.isfinite(out).all()) and bool(torch.isfinite(stages).all())
    assert _bits(out.cpu().numpy(), rec_out.cpu().numpy())
    for mode, src in (("adjoint", None), ("discrete", stages)):
        first = d.backward(out, src)
        assert np.isfinite(first["dz0"]).all(), (mode, "dz0")
        for k in a["names"]:
            assert first["grads"][k].shape == a["params"][k].shape and np.isfinite(first["grads"][k]).all(), (mode, k)
        vc.check("%s %s (isolated)" % (name, mode), dict(first, z_out=out.cpu().numpy()), _reference(name, mode), a["names"])
        again = d.backward(out, src)
        assert _bits(first["dz0"], again["dz0"]), mode
        for k in a["names"]:
            assert _bits(first["grads"][k], again["grads"][k]), (mode, k)


def test_variant_samples_are_independent_across_tiles(gpu_lib):
    """Case B at B = 33 (two full tiles and a one-sample tail) restricted to its first 16 samples equals the run at B = 16 bit for
    bit, in the solution and in dL/dz0 of both backwards: no tile reads or writes another tile's samples."""
    name = "B_gru_evaluate_d72"
    full, one = vc.Direct(name, _flags(name)), vc.Direct(name, _flags(name), samples=16)
    assert (full.p.batch, one.p.batch) == (33, 16)
    zf, sf = full.forward(record=True)
    zo, so = one.forward(record=True)
    assert _bits(zf[:16].cpu().numpy(), zo.cpu().numpy())
    for src_f, src_o in ((None, None), (sf, so)):
        gf, go = full.backward(zf, src_f), one.backward(zo, src_o)
        assert _bits(gf["dz0"][:16], go["dz0"])
        assert not _bits(gf["grads"]["Wr"], go["grads"]["Wr"])      # (the parameter gradients do sum over all 33 samples)


@pytest.mark.parametrize("name", sorted(vc.FORWARD_ONLY))
def test_variant_forward_only_shapes(name, gpu_lib):
    """gru / matmul at H 96 and 112, HH 96: the forward's plan fits (the shared layer, then every layer streamed from L2) and is
    checked against fp64; the backward's plan passes 160 KB, so ncde_workspace_bytes answers NCDE_ERR_UNSUPPORTED for both backward
    passes and cdeint with gradients runs on the unfused solver behind exactly one warning, within the tolerances."""
    plan = vc.plan_of(name)
    assert (plan.ok_fwd, plan.ok_adj) == (True, False) and plan.res_fwd == vc.FORWARD_ONLY[name]
    d = vc.Direct(name)
    assert d.kernel_names()[0] == "ncde_fwd_variant"
    assert [gpu_lib.ncde_workspace_bytes(ctypes.byref(d.p), ps) for ps in (1, 2)] == [-2, -2]
    assert gpu_lib.ncde_workspace_bytes(ctypes.byref(d.p), 0) > 0
    out, _ = d.forward()
    ref = _reference(name, "discrete")
    err = vc.gu.relerr(out.cpu().numpy(), ref["z_out"])
    print("%s fused forward z %.2e" % (name, err))
    assert err <= vc.TIGHT_Z, err
    for mode in vc.ALL_MODES:
        probs = []
        res = vc.solve(name, mode, torch.float32, "cuda", capture=probs, refused=True)
        assert probs and gpu_lib.ncde_workspace_bytes(ctypes.byref(probs[-1]), 1 if mode == "adjoint" else 2) == -2
        vc.check("%s %s (unfused fp32)" % (name, mode), res, _reference(name, mode), vc.arrays(name)["names"])
