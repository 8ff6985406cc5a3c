"""Without a GPU: the Python restatement of the variant kernels' LDS plan (variant_util.vr_plan) against what
the library answers on a grid of shapes and across the backward's 160 KB boundary; every case of tests/variant_cases.py in the regime
it is there for; the test-side field against the oracle's; and every case validated on the CPU -- the unfused solver in fp32 against
itself in fp64 within the project's tolerances, every gradient of the fp64 reference far above the tolerance, no ReLU mask at a
knife edge."""
import ctypes

import numpy as np
import pytest
import torch

import golden_util as gu
import variant_cases as vc
import variant_util as vu
import ncde_amd
from ncde_amd import _lib

UNSUPPORTED = -2
PAIRS = [(k, m) for k in ("original", "minimal", "gru") for m in ("matmul", "evaluate", "derivative") if (k, m) != ("original", "matmul")]


def _problem(kind, mode, C, H, dims, layers, B=20, T=9):
    """Dummy device pointers (one per distinct tensor name) behind FLAG_FORCE_GENERIC: the variant family's own answer."""
    p = _lib.NcdeProblem()
    p.abi_version = _lib.NCDE_ABI_VERSION
    p.batch, p.n_knots, p.channels, p.hidden = B, T, C, H
    p.interp, p.method, p.output = 0, 2, 0
    p.flags = _lib.FLAG_FORCE_GENERIC
    p.n_layers = len(dims)
    ptr = {}
    for l, ((w, b), (dout, din)) in enumerate(zip(layers, dims)):
        p.layer_in[l], p.layer_out[l] = din, dout
        p.layer_W[l] = ptr.setdefault(w, 0x10000 * (len(ptr) + 1))
        p.layer_b[l] = ptr.setdefault(b, 0x10000 * (len(ptr) + 1))
    p.Wo, p.bo, p.coeffs, p.z0 = 0x3000, 0x3100, 0x4000, 0x5000
    p.Wg, p.bg, p.Wr, p.br = 0x6000, 0x6100, 0x7000, 0x7100
    p.field_kind, p.field_input = _lib.FIELD_KIND[kind], _lib.FIELD_INPUT[mode]
    p.coeffs_stride_b, p.coeffs_stride_t = T * C, C
    return p


def _library(kind, mode, C, H, dims, layers):
    lib = ncde_amd.lib()
    rc = [lib.ncde_workspace_bytes(ctypes.byref(_problem(kind, mode, C, H, dims, layers)), ps) for ps in (0, 1, 2)]
    assert all(r > 0 or r == UNSUPPORTED for r in rc), (rc, lib.ncde_last_error_string())
    return [r > 0 for r in rc]


def _both(kind, mode, C, H, HH, nl):
    layers, dims = vu.ref_stack(mode, C, H, HH, nl)
    plan = vu.vr_plan(kind, mode, C, H, dims, layers)
    assert _library(kind, mode, C, H, dims, layers) == [plan.ok_fwd, plan.ok_adj, plan.ok_adj], (kind, mode, C, H, HH, nl, plan)
    return plan.ok_fwd, plan.ok_adj


def test_plan_restatement_agrees_with_the_library_on_the_grid():
    """ok of the restatement == (ncde_workspace_bytes != NCDE_ERR_UNSUPPORTED) for passes 0, 1, 2 on the reference's stack over every
    kind / mode pair of the family, C in {3, 8, 20}, H in {7 .. 128}, HH in {15 .. 128}, one to three layers.  On that grid the
    forward is never refused (its plan, 7 DS + 4 HS + 16 Cp floats, stays below 27,000 at H + C = 148 and no last width passes 128), so
    the third outcome -- both passes refused -- comes from the points BEYOND: a last width of 129 or 144 (nine column tiles) and widths whose
    forward plan passes 160 KB (first at H = 225)."""
    seen = set()
    for kind, mode in PAIRS:
        for C in (3, 8, 20):
            for H in (7, 16, 32, 47, 64, 80, 96, 112, 128):
                for HH in (15, 32, 64, 93, 112, 128):
                    for nl in (1, 2, 3):
                        seen.add(_both(kind, mode, C, H, HH, nl))
    assert seen == {(True, True), (True, False)}
    beyond = set()
    for kind, mode in PAIRS:
        for C, H, HH, nl in ((3, 16, 144, 1), (3, 16, 129, 2), (8, 64, 144, 2), (3, 384, 64, 1), (3, 16, 368, 2), (3, 225, 64, 1)):
            beyond.add(_both(kind, mode, C, H, HH, nl))
    assert beyond == {(False, False)}
    # the last accepted points next to them: a last width of 128, and H = 224 (176 x 224 + 16 ru4(C) floats)
    assert _both("gru", "matmul", 3, 16, 128, 1) == (True, True) and _both("minimal", "matmul", 3, 224, 64, 1) == (True, False)


# the first refused backward of gru / matmul at C 2, H 16, HH 128 along the layer count (DESIGN.md section 5.4 quotes it)
FIRST_REFUSED = dict(C=2, H=16, HH=128, nl=2, floats=42368)


def test_backward_boundary_walk():
    """gru / matmul at C 2, H 16, HH 128: one layer is accepted at 38,272 floats (case D), the second layer adds 2 DS = 4,096 floats
    and the backward's plan passes 40,960 -- library and restatement flip at the same step, and the forward stays accepted.  The
    widths DESIGN.md used to promise ("<= 128") are refused long before: H 96, HH 96, two layers."""
    first = None
    for nl in (1, 2):
        ok = _both("gru", "matmul", 2, 16, 128, nl)
        assert ok[0]
        if not ok[1] and first is None:
            first = nl
    layers, dims = vu.ref_stack("matmul", 2, 16, 128, 2)
    plan = vu.vr_plan("gru", "matmul", 2, 16, dims, layers)
    print("first refused backward: nl", first, "floats", plan.floats_adj)
    assert dict(C=2, H=16, HH=128, nl=first, floats=plan.floats_adj) == FIRST_REFUSED
    assert vc.plan_of("D_gru_matmul_dlast128").floats_adj == 38272 and vc.plan_of("D_gru_matmul_dlast128").ok_adj
    assert _both("gru", "matmul", 4, 96, 96, 2) == (True, False) and _both("gru", "matmul", 4, 16, 128, 2) == (True, False)


def test_cases_are_in_their_regimes():
    """Every case sits where its comment says (a change of the plan cannot silently move it), and together the cases hold every
    regime: the partial in LDS and in global memory; register weight gradients at the 16-tile bound, refused by size, refused by
    topology; everything, nothing and part of the weights resident in the backward; a streamed reset gate in front of a resident
    layer."""
    held = set()
    for name in vc.WITH_BACKWARD:
        plan = vc.plan_of(name)
        assert plan.ok_fwd and plan.ok_adj, name
        assert vc.regime_of(name) == vc.CASES[name]["regime"], (name, vc.regime_of(name))
        held.add((plan.gacc_in_lds, plan.dw_why, vu.pattern(plan.res_adj)))
    assert {g for g, _, _ in held} == {True, False}
    assert {w for _, w, _ in held} == {"registers", "size", "topology"}
    assert {r for _, _, r in held} == {"all", "none", "mixed"}
    assert (False, "topology", "mixed") in held      # J: refused by topology WITH the partial in global memory
    tiles = lambda n, k: -(-n // 16) * -(-k // 16)      # noqa: E731
    # C: every matrix of the register path at exactly 16 tiles
    c = vc.arrays("C_gru_matmul_16tiles")
    assert [tiles(*d) for d in c["dims"]] == [16, 16] and tiles(64, 64) == vu.DW_REG_TILES
    # B: the reset gate alone refuses the register path, and it is streamed in front of a resident layer 0
    b, pb = vc.arrays("B_gru_evaluate_d72"), vc.plan_of("B_gru_evaluate_d72")
    assert all(tiles(*d) <= 16 for d in b["dims"]) and tiles(72, 72) == 25
    assert pb.res_adj["r"] is False and pb.res_adj["layers"][0] is True
    # A: forward with both heads streamed;  F: forward all resident with a backward that keeps nothing;  the figures of the table
    assert vc.plan_of("A_gru_matmul_H80").res_fwd == {"r": True, "layers": [True, True], "o": False, "g": False}
    pf = vc.plan_of("F_original_derivative_odd")
    assert vu.pattern(pf.res_fwd) == "all" and vu.pattern(pf.res_adj) == "none" and pf.floats_adj == 40384
    assert vc.plan_of("G_gru_derivative_d37").floats_adj == 39872
    assert vc.arrays("D_gru_matmul_dlast128")["dims"][-1][0] == vu.MAX_DLAST
    for name, res_fwd in vc.FORWARD_ONLY.items():
        plan = vc.plan_of(name)
        assert (plan.ok_fwd, plan.ok_adj) == (True, False) and plan.res_fwd == res_fwd and plan.res_adj is None, (name, plan)
        c_ = vc.CASES[name]
        assert _both(c_["kind"], c_["mode"], c_["C"], c_["H"], c_["HH"], c_["nl"]) == (True, False)
    # one-sample and 17-sample tail tiles
    assert {vc.CASES[n]["B"] % 16 for n in vc.WITH_BACKWARD} >= {1, 3, 5} and vc.CASES["B_gru_evaluate_d72"]["B"] == 33
    assert {vc.CASES[n]["method"] for n in vc.WITH_BACKWARD} == {"rk4", "midpoint", "euler"}
    assert {vc.CASES[n]["interp"] for n in vc.WITH_BACKWARD} == {"linear", "cubic"}


@pytest.mark.parametrize("name", sorted(vc.CASES))
def test_case_is_well_posed_on_the_cpu(name):
    """The unfused solver in fp32 against itself in fp64 (the untied stack, gradients summed over the copies) on the CPU, on the
    continuous adjoint and the exact discrete backward: within the tolerances, every gradient of the fp64 reference -- reset gate,
    both heads, every inner layer, dL/dz0 -- has a maximum >= 1e3 x the tolerance, and no ReLU pre-activation of the reference, in the
    forward or in either backward, lies closer to zero than fp32 can decide (layer_topologies.ReluMargin; a case that fails this is
    re-seeded in variant_cases.py).  The forward-only cases too: their gradients are what the unfused fall-back is checked on."""
    a = vc.arrays(name)
    for mode in vc.ALL_MODES:
        ref = vc.solve(name, mode, torch.float64, "cpu", untie=True, observe=True)
        res = vc.solve(name, mode, torch.float32, "cpu")
        vc.check("%s %s fp32 vs fp64 (cpu)" % (name, mode), res, ref, a["names"])
        print("relu margin %.2f" % ref["relu_margin"])
        assert ref["relu_margin"] >= 1.0, (name, mode, ref["relu_margin"])


@pytest.mark.parametrize("kind,mode,nl", [("gru", "evaluate", 3), ("minimal", "derivative", 2), ("gru", "matmul", 2)])
def test_stack_field_is_the_oracles_field(kind, mode, nl):
    """variant_util.StackField.forward (what the unfused reference integrates) against ncde_oracle.Field.variant in fp64 on one batch
    of states, with variant_util.make_weights' shapes (d0 = H + C inputs, H-row heads, a d0 x d0 reset gate)."""
    import ncde_oracle as orc
    C, H, HH, B = 5, 13, 22, 7
    layers, dims = vu.ref_stack(mode, C, H, HH, nl)
    p = vu.make_weights(layers, dims, kind, mode, C, H, 9)
    d0, rows = vu.field_dims(mode, C, H)
    assert p["W0"].shape == (HH, d0) and p["Wo"].shape == (rows, HH) and (kind != "gru" or p["Wr"].shape == (d0, d0))
    z = (gu.data.normal(5, B * H, stream=2).reshape(B, H) * 0.7)
    cin = gu.data.normal(6, B * C, stream=3).reshape(B, C)
    field = orc.Field.variant({k: torch.from_numpy(v).double() for k, v in p.items()}, H, C, nl, kind, mode)
    ref = field.g(torch.from_numpy(z), torch.from_numpy(cin))
    f = vu.StackField(p, layers, H, C, kind, mode, dtype=torch.float64)
    u = torch.from_numpy(z if mode == "matmul" else np.concatenate([z, cin], axis=1))
    out = f(0.0, u)
    if mode == "matmul":
        assert out.shape == (B, H, C)
        out = (out @ torch.from_numpy(cin).unsqueeze(-1)).squeeze(-1)
    assert out.shape == (B, H) and f.nfe == 1 and float(ref.abs().max()) > 0.01
    assert gu.relerr(out.detach().numpy(), ref.numpy()) <= 1e-13
    spec = f.fused_spec()
    assert (spec.kind, spec.mode) == (kind, mode) and len(spec.unique_params()) == len(vu.param_names(layers, kind)) == len(p)
