"""Without a GPU: every case of tests/tiled_cases.py validated before a kernel sees it -- the acceptance conditions (i) - (iii) of
resident_cases' docstring (on the gated sets also for the sigmoid head's tensors), the instantiation each (case, pass) is dispatched
to (ncde_kernel_name, a host-side query), the backward's workspace against the restated part-group / window rules, the C time-plan
builder against the oracle's plan words and where the forced time windows cut each plan, and the default-axis original-field cases
through the C++ restatement behind the same C ABI (oracle/_build/libncde_cpu.so)."""
import numpy as np
import pytest
import torch

import golden_util as gu
import resident_cases as rc
import tiled_cases as tc

PLANNED = [n for n, c in sorted(tc.CASES.items()) if tc.is_planned(c)]
CPU_LIB = [n for n, c in sorted(tc.CASES.items()) if not tc.is_planned(c) and tc.SETS[c["set"]][4:6] == ("original", "matmul")]


def test_the_table_holds_what_it_is_there_for():
    """The axes of the table: seven batch sizes on four sets (and the odd-fragment Euler pair), one- and two-step solves on every
    set, plans (a) - (g) on five sets, a late and a tail-tile range fault on two; nothing larger than B = 129, T = 7, width 64 (the
    two wide sets apart, which stay out of the batch group)."""
    batch = [tc.CASES[n] for n in tc.BY_GROUP["batch"]]
    assert {(c["set"], c["B"]) for c in batch if c["method"] == "rk4"} == {(s, B) for s in tc.BATCH_SETS for B in (1, 16, 17, 32, 33, 97, 129)}
    assert {(c["set"], c["B"]) for c in batch if c["method"] != "rk4"} == {("T16", 97), ("T16", 129)}
    assert all((c["T"], c["path"], c["out"]) == (4, "linear", "knots") for c in batch) and len(batch) == 4 * 7 + 2
    assert tc.BATCH_SETS == ("T16", "T32r2", "T48", "G32") and sorted(tc.BATCH_SIZES) == [1, 16, 17, 32, 33, 97, 129]
    for c in batch:      # a row subset is what it says: rows of the B = 129 case, its own row count
        if c["base"] is not None:
            assert tc.CASES[c["base"]]["B"] == 129 and c["rows"][1] - c["rows"][0] == c["B"] and tc.CASES[c["base"]]["set"] == c["set"]
    assert tc.CASES["batch_T48_B1"]["rows"] == (128, 129)
    steps = [tc.CASES[n] for n in tc.BY_GROUP["steps"]]
    assert {(c["set"], c["T"], c["path"], c["method"], c["out"]) for c in steps} == {
        (s, T) + v for s in tc.SETS for T in (2, 3) for v in (("linear", "rk4", "interval"), ("cubic", "midpoint", "knots"))}
    assert len(steps) == 4 * len(tc.SETS) == 44 and {c["B"] for c in steps} == {17}
    plan = [tc.CASES[n] for n in tc.BY_GROUP["plan"]]
    assert len(plan) == 5 * 13 and {c["set"] for c in plan} == {"T32r2", "T48", "G32", "D32", "W160"} and {c["B"] for c in plan} == {19}
    assert {n.split("_")[1] for n in tc.BY_GROUP["plan"]} == set("abcdefg") and tc.PLANS is rc.PLANS
    assert not [c for c in plan if c["knots"] is not None and c["path"] == "cubic"]
    fault = {(c["set"], c["B"]) + c["outlier"] for c in map(tc.CASES.get, tc.BY_GROUP["fault"])}
    assert fault == {(s,) + v for s in ("T48", "G32") for v in ((33, 32, "z0", rc.FAULT_Z0), (37, 21, "dx", rc.FAULT_DX))}
    assert sum(map(len, tc.BY_GROUP.values())) == len(tc.CASES)
    for c in tc.CASES.values():
        C, H, HH = tc.SETS[c["set"]][:3]
        assert c["B"] <= 129 and c["T"] <= 7 and (max(H, HH) <= 64 or c["set"] in ("W160", "W256")), c["name"]
        assert c["set"] != "W256" or c["group"] == "steps"
    assert max((c["B"], tc.SETS[c["set"]][1], c["T"]) for c in batch) == (129, 48, 4)
    assert (tc.TIGHT_Z, tc.TIGHT_G, tc.E2E_G) == (2e-5, 2e-5, 2e-4) == (rc.TIGHT_Z, rc.TIGHT_G, rc.E2E_G)


@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_case_is_accepted(name):
    """(i) fp32 oracle vs fp64 oracle within half of each bound (end to end within E2E_G / 2 and TIGHT_Z / 2; the continuous adjoint
    fed the fp64 z rounded to fp32 within TIGHT_G / 2), (ii) the ReLU margin, (iii) the gradient magnitudes -- and the kernel names."""
    c, ex, o32, names = tc.CASES[name], tc.expect(name), tc.oracle32(name), tc.names_of(name)
    assert ("Wg" in names and "bg" in names) == (tc.SETS[c["set"]][4] == "minimal")
    e_adj = tc.errors(o32["adjoint"], ex["adjoint"], names, (o32["z_out"], ex["z_out"]))
    e_dis = tc.errors(o32["discrete"], ex["discrete"], names)
    e_iso = tc.errors(o32["adjoint_iso"], ex["adjoint"], names)
    print(name, "fp32 oracle: z %.2e adjoint %.2e discrete %.2e adjoint on fp64 z %.2e" %
          (e_adj["z"], max(v for k, v in e_adj.items() if k != "z"), max(e_dis.values()), max(e_iso.values())))
    if c["outlier"] is None:
        assert e_adj["z"] <= tc.TIGHT_Z / 2, e_adj
    else:      # per sample: the outlier is 1e5 x the rest
        scale = np.abs(ex["z_out"]).max(axis=(1, 2), keepdims=True)
        assert float((np.abs(o32["z_out"] - ex["z_out"]) / scale).max()) <= tc.TIGHT_Z / 2
    assert all(v <= tc.E2E_G / 2 for k, v in e_adj.items() if k != "z"), e_adj
    assert all(v <= tc.E2E_G / 2 for v in e_dis.values()), e_dis
    assert all(v <= tc.TIGHT_G / 2 for v in e_iso.values()), e_iso
    # (ii)
    if c["outlier"] is None:
        margin = float(ex["margin"].min())
    else:
        margin = min(float(tc.expect(name, clean=True)["margin"].min()), tc.outlier_margin(name))
    print("relu margin %.2e" % margin)
    assert margin >= tc.RELU_MARGIN, (name, margin)
    # (iii)
    for ps in ("adjoint", "discrete"):
        assert float(np.abs(ex[ps]["dz0"]).max()) >= tc.MIN_GRAD, (name, ps, "dz0")
        for n in names:
            assert float(np.abs(ex[ps]["grads"][n]).max()) >= tc.MIN_GRAD, (name, ps, n, float(np.abs(ex[ps]["grads"][n]).max()))
    # the instantiation of every pass
    for ps, (g, w) in enumerate(zip(tc.kernel_names(name), tc.want_names(name))):
        assert tc.name_matches(g, w), (name, ps, g, w)


def test_the_streamed_set_needs_no_force_flag():
    """(8, 48, 64, 2) has no shape-specialised kernel set to be padded onto: the same kernels with and without NCDE_FLAG_FORCE_TILED."""
    for name in ("steps_T48_T3_linear_rk4_interval", "plan_b_T48_linear_rk4"):
        assert tc.kernel_names(name, flags=0) == tc.kernel_names(name)


@pytest.mark.parametrize("name", tc.BY_GROUP["batch"])
def test_backward_workspace_is_the_restated_plan(name):
    """ncde_workspace_bytes of both backward passes equals the restated tiled_adj_plan (part-groups, window, float layout), with the
    set's flags, under NCDE_FLAG_FP32_MFMA (fp32 records on every set) and under a forced one-step window; the tile, pair and
    part-group counts the batch sizes are there for: B <= 112 one part-group, B = 129 two, nine tiles, five pairs."""
    c = tc.CASES[name]
    own = tc.flags_of(name)
    for flags in (None, own | tc.FP32_MFMA, own | (1 << 16)):
        for ps in (1, 2):
            assert tc.workspace_bytes(name, ps, flags) == tc.expected_workspace_bytes(name, flags), (name, flags, ps)
    plan = tc.adj_plan(name)
    assert plan["parts"] == (1 if c["B"] <= 112 else 2) and plan["window"] == 3 and plan["bf"] == (c["set"] != "T16")
    assert not tc.adj_plan(name, own | tc.FP32_MFMA)["bf"] and tc.adj_plan(name, own | (1 << 16))["window"] == 1
    assert (plan["n_st"], plan["pairs"]) == {1: (1, 1), 16: (1, 1), 17: (2, 1), 32: (2, 1), 33: (3, 2), 97: (7, 4), 129: (9, 5)}[c["B"]]


@pytest.mark.parametrize("name", PLANNED)
def test_time_plan_builder_and_where_the_windows_cut(name):
    """ncde_time_plan_build on the case's axis, bit for bit the oracle's restatement in torch's arithmetic (fp32 or fp64 t); and for
    the forced windows of 1 and 2 reverse steps, whether a boundary between two windows falls on the step that ends a reverse solve is
    what tiled_cases.PLAN_WINDOWS says."""
    import ncde_oracle as orc
    c, a = tc.CASES[name], tc.arrays(name)
    ctl = rc._control(c, a["coeffs"], torch.float32)
    want, n_fwd, n_adj = orc.time_plan_words(ctl, torch.from_numpy(tc.t_out(c)), c["method"], c["step"])
    _, got, _keep = tc.problem_of(name)
    assert got.dtype == np.int32 and np.array_equal(got, want), name
    assert (int(got[2]), int(got[3]), int(got[4])) == (n_fwd, n_adj, len(c["out"]))
    assert tc.t_out(c).dtype == (np.float64 if c["t64"] else np.float32)
    t_adj, t_fwd, on = tc.PLAN_WINDOWS[name.split("_")[1]]
    assert (n_adj, n_fwd) == (t_adj, t_fwd), (name, n_adj, n_fwd)
    assert {w: tc.window_on_reset(got, w) for w in (1, 2)} == on, name
    if tc.SETS[c["set"]][5] == "matmul":      # the window: the larger step count unless forced
        for w, steps in ((0, max(n_adj, n_fwd)), (1, 1), (2, 2)):
            flags = tc.flags_of(name) | (w << 16)
            assert tc.adj_plan(name, flags, steps=max(n_adj, n_fwd))["window"] == steps
            for ps in (1, 2):
                assert tc.workspace_bytes(name, ps, flags) == 4 * tc.adj_plan(name, flags, steps=max(n_adj, n_fwd))["total"], (name, w, ps)


@pytest.mark.parametrize("name", [n for n in tc.BY_GROUP["plan"] if n.split("_")[1] in ("c", "f")])
def test_plans_c_and_f_never_read_the_first_and_the_last_piece(name):
    """The oracle on the poisoned coefficients (tiled_cases.poisoned) gives the same solution and gradients, bit for bit."""
    a, ex = tc.arrays(name), tc.expect(name)
    x = tc.poisoned(name)
    assert np.all(np.abs(x[:, 0]) == tc.POISON) and np.all(np.abs(x[:, -1]) == tc.POISON) and np.array_equal(x[:, 1:-1], a["coeffs"][:, 1:-1])
    w = tc.walk(name, x, a["z0"], a["grad_out"], torch.float64)
    assert np.array_equal(w["z"].numpy(), ex["z_out"])
    for ps in ("adjoint", "discrete"):
        assert np.array_equal(w[ps][0].numpy(), ex[ps]["dz0"])
        assert all(np.array_equal(g.numpy(), ex[ps]["grads"][n]) for n, g in zip(tc.names_of(name), w[ps][1]))


@pytest.mark.parametrize("name", tc.BY_GROUP["fault"])
def test_fault_cases_leave_the_fp16_range_where_they_say(name):
    """The outlier's state passes NCDE_H2_LIMIT (6e4) -- in the late case from the stages of step 2 on, with an ordinary z0 and
    ordinary states through step 1 -- and no other sample comes near it; the tail outlier is alone in its tile."""
    c, a, ex = tc.CASES[name], tc.arrays(name), tc.expect(name)
    s, what, mag = c["outlier"]
    assert mag > 6.0e4 / np.abs(a["params"]["W0"]).sum(axis=1).max()
    S = tc.STAGES[c["method"]]
    per_step = np.abs(ex["stages"]).max(axis=2).reshape(c["T"] - 1, S, c["B"]).max(axis=1)      # [step, sample]
    assert np.delete(per_step, s, axis=1).max() < 100.0
    if what == "dx":
        assert np.abs(a["z0"]).max() < 10.0 and per_step[0, s] < 100.0 and (per_step[2:, s] > 6.0e4).all(), per_step[:, s]
        assert s // 16 == 1 and c["B"] == 37 and not np.any(a["grad_out"][s])
    else:
        assert per_step[0, s] > 6.0e4 and s == 32 and c["B"] == 33
        pre = a["params"]["W0"].astype(np.float64) @ a["z0"][s] + a["params"]["b0"]
        assert pre.max() < -100.0      # every unit of layer 0 switched off: the head stays unsaturated (resident_cases.arrays)
    assert np.any(a["grad_out"][s - 1])
    assert np.array_equal(np.delete(a["z0"], s, axis=0), np.delete(a["clean_z0"], s, axis=0))
    assert np.array_equal(np.delete(a["coeffs"], s, axis=0), np.delete(a["clean_coeffs"], s, axis=0))


@pytest.mark.parametrize("name", CPU_LIB)
def test_default_axis_case_through_the_cpu_library(name):
    """The C++ restatement (fp32) on the case's own arrays: forward, stage record, continuous adjoint on the fp64 z, discrete
    backward on the fp64 record -- within the bounds the kernels are held to."""
    import cpu_lib_util as cu
    c, ex, names = tc.CASES[name], tc.expect(name), tc.names_of(name)
    g = tc.golden_case(name)
    cc = cu.CpuCase(g["coeffs"], g["meta"]["kind"], g["z0"], g["params"], g["layers"], c["method"], c["out"] == "knots")
    z, rec = cc.forward(record=True)
    assert rec.size == ex["stages"].size == (c["T"] - 1) * tc.STAGES[c["method"]] * c["B"] * tc.SETS[c["set"]][1]
    scale = np.abs(ex["z_out"]).max(axis=(1, 2), keepdims=True) if c["outlier"] is not None else np.abs(ex["z_out"]).max()
    assert float((np.abs(z - ex["z_out"]) / scale).max()) <= tc.TIGHT_Z
    if c["outlier"] is None:
        assert gu.relerr(rec.reshape(ex["stages"].shape), ex["stages"]) <= tc.TIGHT_Z
    assert np.array_equal(cc.forward(), z)
    for ps in ("adjoint", "discrete"):
        src = ex["stages"] if ps == "discrete" else ex["z_out"]
        dz0, bufs = cc.backward(src, g["expect"]["grad_out"], discrete=ps == "discrete")
        errs = tc.errors({"dz0": dz0, "grads": bufs}, ex[ps], names)
        print(name, ps, " ".join("%s %.2e" % kv for kv in errs.items()))
        assert all(v <= tc.TIGHT_G for v in errs.values()), (name, ps, errs)
