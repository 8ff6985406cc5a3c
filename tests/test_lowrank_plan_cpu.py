"""Without a GPU: the Python restatement of the low-rank kernels' LDS plan (lowrank_util.lr_plan) against
what the library answers around the 160 KB boundary; the test-side stack field against the restated formula; and every case of
tests/lowrank_cases.py validated on the CPU -- the unfused solver in fp32 against itself in fp64 within the project's tolerances, with
every gradient tensor of the fp64 reference far above the tolerance."""
import ctypes

import numpy as np
import pytest
import torch

import golden_util as gu
import layer_topologies as lt
import lowrank_cases as lc
import lowrank_util as lu
import ncde_amd
from ncde_amd import _lib

UNSUPPORTED = -2


def _problem(H, C, R, HH, nl, B=20, T=9):
    """The reference's stack (layer 0, then ONE shared layer) with dummy device pointers, as in tests/test_lowrank_cpu.py."""
    p = _lib.NcdeProblem()
    p.abi_version = _lib.NCDE_ABI_VERSION
    p.batch, p.n_knots, p.channels, p.hidden = B, T, C, H
    p.interp, p.method, p.output = 0, 2, 0
    p.flags = _lib.FLAG_FIELD_RANK(R)
    p.n_layers = nl
    for l in range(nl):
        p.layer_in[l], p.layer_out[l] = (H if l == 0 else HH), HH
        p.layer_W[l] = 0x1000 if l == 0 else 0x2000
        p.layer_b[l] = 0x1100 if l == 0 else 0x2100
    p.Wo, p.bo, p.coeffs, p.z0 = 0x3000, 0x3100, 0x4000, 0x5000
    p.Wg, p.bg = 0x6000, 0x6100
    p.field_kind, p.field_input = 3, 0
    p.coeffs_stride_b, p.coeffs_stride_t = T * C, C
    return p


def _restated(H, C, R, HH, nl):
    layers, dims = lt.stack_of("ref_shared3", H, HH)
    layers, dims = ([layers[0]] + [layers[1]] * (nl - 1)), ([dims[0]] + [dims[1]] * (nl - 1))
    return lu.lr_plan(H, C, R, dims, layers)


def _library(H, C, R, HH, nl):
    lib = ncde_amd.lib()
    rc = [lib.ncde_workspace_bytes(ctypes.byref(_problem(H, C, R, HH, nl)), ps) for ps in (0, 1, 2)]
    assert all(r > 0 or r == UNSUPPORTED for r in rc), (rc, lib.ncde_last_error_string())
    return [r > 0 for r in rc]


# H, C, HH; R and the layer count are swept
GRID = [(H, C, HH) for H in (64, 96, 128) for C in (8, 24, 64, 128) for HH in (64, 128)]


def test_plan_restatement_agrees_with_the_library_across_the_boundary():
    """ok of the restatement == (ncde_workspace_bytes != NCDE_ERR_UNSUPPORTED) for passes 0, 1, 2 on a grid of shapes; the grid has
    accepted and refused shapes for the forward and for the backward, and shapes where only the backward is refused."""
    seen = set()
    for H, C, HH in GRID:
        for R in sorted(set(r for r in (1, 2, 4, 8, 12, 16, 24, 32, 64, 128) if r <= C)):
            for nl in (1, 2, 5, 8):
                ok_fwd, ok_adj = _restated(H, C, R, HH, nl)[:2]
                assert _library(H, C, R, HH, nl) == [ok_fwd, ok_adj, ok_adj], (H, C, R, HH, nl)
                seen.add((ok_fwd, ok_adj))
    assert seen == {(True, True), (True, False), (False, False)}


def test_documented_point_is_accepted_and_its_nearest_neighbours_are_refused():
    """H 64, C 24, R 8, HH 64, two layers (149 KB with streamed heads) is accepted; growing the layer count, or the rank,
    one step at a time, library and restatement change their answer at the same step."""
    H, C, R, HH, nl = 64, 24, 8, 64, 2
    assert _library(H, C, R, HH, nl) == [True, True, True]
    assert _restated(H, C, R, HH, nl) == (True, True, False, False, False)
    first = {}
    for key, walk in (("layers", [(R, n) for n in range(nl, 9)]), ("rank", [(r, nl) for r in range(R, C + 1)])):
        for r, n in walk:
            ok = _restated(H, C, r, HH, n)[:2]
            assert _library(H, C, r, HH, n) == [ok[0], ok[1], ok[1]], (key, r, n)
            if not ok[1] and key not in first:
                first[key] = (r, n)
    print("first refused backward:", first)
    assert first == {"layers": (8, 6), "rank": (10, 2)}
    assert lc.REFUSED == dict(H=H, C=C, R=10, HH=HH, nl=2) and lc.plan_of("refused_rank10")[:2] == (True, False)


@pytest.mark.parametrize("spec,H,HH", [("tied_first_last", 12, 12), ((93, 15, 47), 47, None)], ids=["tied_first_last", "H47_93x15x47"])
def test_stack_field_forward_is_the_restated_formula(spec, H, HH):
    """lowrank_util.StackField.forward (what the unfused reference integrates) against restated_forward on a layer list, in fp64."""
    C, R = 5, 3
    layers, dims = lt.stack_of(spec if isinstance(spec, str) else list(spec), H, HH)
    p = {k: v for k, v in lt.make_weights(layers, dims, C, H, 9).items() if k not in ("Wo", "bo")}
    p.update(lu.head_weights(gu.data, H, C, R, dims[-1][0], 9))
    z = (gu.data.normal(5, 7 * H, stream=2).reshape(7, H) * 0.7).astype(np.float32)
    ref = lu.restated_forward(p, z, H, C, R, len(layers), layers)
    f = lu.StackField(p, layers, H, C, R, dtype=torch.float64)
    out = f(0.0, torch.from_numpy(z).double())
    assert out.shape == (7, H, C) and f.nfe == 1 and float(ref.abs().max()) > 0.01
    assert gu.relerr(out.detach().numpy(), ref.numpy()) <= 1e-13
    spec_ = f.fused_spec()
    assert (spec_.kind, spec_.mode, spec_.rank) == ("lowrank", "matmul", R)
    assert len(spec_.unique_params()) == len(set(n for wb in layers for n in wb)) + 4
    assert spec_.Wo is f.p["Wh"] and spec_.Wg is f.p["Wq"]


def test_regime_cases_are_in_their_regimes():
    for name, regime in lc.REGIMES.items():
        assert lc.plan_of(name) == (True, True) + regime, name
    # every other case: everything LDS-resident (the regime the existing goldens run), so the three above are the new ones
    for name in lc.CASES:
        if name not in lc.REGIMES and name != "refused_rank10":
            assert lc.plan_of(name) == (True, True, True, True, True), name


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_case_is_well_posed_on_the_cpu(name):
    """The unfused solver in fp32 against itself in fp64 (the untied stack, gradients summed over the copies) on the CPU, on every
    backward the case runs: within the tolerances, and every gradient of the fp64 reference has a maximum >= 1e3 x the tolerance."""
    a = lc.arrays(name)
    for mode in lc.CASES[name]["modes"]:
        probe = {}
        ref = lc.solve(name, mode, torch.float64, "cpu", untie=True,
                       field_probe=lambda f, z: probe.update(share=lc.saturated_share(f, z)))
        res = lc.solve(name, mode, torch.float32, "cpu")
        lc.check("%s %s fp32 vs fp64 (cpu)" % (name, mode), res, ref, a["names"])
        if name == "edge_saturated_heads":
            print("share of |M| > 0.99: %.3f" % probe["share"])
            assert probe["share"] >= lc.SATURATED_SHARE
