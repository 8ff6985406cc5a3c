"""Without a GPU: every case of tests/resident_cases.py validated before a kernel sees it -- the acceptance conditions (i) - (iii) of
that module's docstring, the instantiation each (case, pass) is dispatched to (ncde_kernel_name, a host-side query), the C time-plan
builder against the oracle's plan words for every planned case, and the default-axis cases through the C++ restatement behind the
same C ABI (oracle/_build/libncde_cpu.so): layouts, shared layers, record shapes."""
import numpy as np
import pytest
import torch

import golden_util as gu
import resident_cases as rc

DEFAULT_AXIS = [n for n, c in sorted(rc.CASES.items()) if not rc.is_planned(c)]
PLANNED = [n for n, c in sorted(rc.CASES.items()) if rc.is_planned(c)]


def test_the_table_holds_what_it_is_there_for():
    """The axes of the table: ring phases 1 .. 6 pieces on the unrolled set in the full cross, T = 2 / 4 on every other set, short
    rectilinear paths on three channel sets, B in {1, 16, 33}, plans (a) - (g) on three sets, late and tail-tile range faults."""
    ring20 = [rc.CASES[n] for n in rc.BY_GROUP["ring"] if rc.CASES[n]["set"] == "R20"]
    assert len(ring20) == 60 and {c["T"] for c in ring20} == {2, 3, 4, 5, 7} and {c["B"] for c in ring20} == {17}
    assert {(c["path"], c["method"], c["out"]) for c in ring20} == {(p, m, o) for p in ("linear", "cubic") for m in ("rk4", "midpoint", "euler")
                                                                     for o in ("interval", "knots")}
    others = [rc.CASES[n] for n in rc.BY_GROUP["ring"] if rc.CASES[n]["set"] != "R20"]
    assert {c["set"] for c in others} == set(rc.SETS) - {"R20"} and len(others) == 4 * (len(rc.SETS) - 1)
    assert {(c["set"], c["T"]) for c in map(rc.CASES.get, rc.BY_GROUP["skip"])} >= {(s, T) for s in ("R20", "Rc8", "Rc12") for T in (3, 5, 7)}
    assert {(c["set"], c["T"], c["B"]) for c in map(rc.CASES.get, rc.BY_GROUP["batch"])} == {(s, T, B) for s in rc.BATCH_SETS for T in (2, 4)
                                                                                           for B in (1, 16, 33)}
    assert len(rc.BY_GROUP["plan"]) == 3 * 13 and len(rc.BY_GROUP["fault"]) == 4
    assert all(c["B"] <= 37 and c["T"] <= 7 and max(rc.SETS[c["set"]][1:3]) <= 64 for c in rc.CASES.values())
    # plan (b): no output on the grid steps [1.5, 2] and [2, 2.5];  plan (a): one forward step
    import ncde_oracle as orc
    for k, n_fwd, cnts, kinds in (("a", 1, [3], [0, 2, 2, 1]), ("b", 6, [1, 0, 1, 0, 0, 1], [0, 1, 1, 1]), ("c", 3, [1, 0, 1], [0, 1, 1]),
                                  ("f", 3, [1, 0, 1], [0, 1, 1]), ("e", 8, [0, 0, 1, 0, 0, 0, 0, 1], [0, 2, 1])):
        T, step, t, _, f64 = rc.PLANS[k]
        ctl = orc.Control(np.zeros((1, T, 2), np.float32), "linear")
        words, nf, na = orc.time_plan_words(ctl, torch.tensor(t, dtype=torch.float64 if f64 else torch.float32), "rk4", step)
        steps = words[8:8 + nf * 15].reshape(nf, 15)
        assert nf == n_fwd and list(steps[:, 2]) == cnts, (k, nf)
        assert list(words[words[6]:words[6] + 2 * len(t)].reshape(-1, 2)[:, 0]) == kinds, k      # output kinds: on t0, on t1, interpolated
        if k == "a":      # every reverse solve a single step
            assert na == len(t) - 1
        if k in ("c", "f"):      # five knots: only pieces 1 and 2 are ever named, forwards and in the reverse solves
            assert T == 5 and set(steps[:, 3::3].ravel()) | set(words[words[7]:].reshape(na, 15)[:, 3::3].ravel()) == {1, 2}
    # plan (d): a step whose stages sit in different pieces
    words, nf, _ = orc.time_plan_words(orc.Control(np.zeros((1, 7, 2), np.float32), "linear"), torch.tensor(rc.PLANS["d"][2]), "rk4", 2.5)
    assert any(len(set(row[3::3])) >= 3 for row in words[8:8 + nf * 15].reshape(nf, 15))


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_case_is_accepted(name):
    """(i) fp32 oracle vs fp64 oracle within half of each bound (end to end within E2E_G / 2 and TIGHT_Z / 2; the continuous adjoint
    fed the fp64 z rounded to fp32 within TIGHT_G / 2), (ii) the ReLU margin, (iii) the gradient magnitudes -- and the kernel names."""
    c, ex, o32, names = rc.CASES[name], rc.expect(name), rc.oracle32(name), rc.names_of(name)
    e_adj = rc.errors(o32["adjoint"], ex["adjoint"], names, (o32["z_out"], ex["z_out"]))
    e_dis = rc.errors(o32["discrete"], ex["discrete"], names)
    e_iso = rc.errors(o32["adjoint_iso"], ex["adjoint"], names)
    print(name, "fp32 oracle: z %.2e adjoint %.2e discrete %.2e adjoint on fp64 z %.2e" %
          (e_adj["z"], max(v for k, v in e_adj.items() if k != "z"), max(e_dis.values()), max(e_iso.values())))
    if c["outlier"] is None:
        assert e_adj["z"] <= rc.TIGHT_Z / 2, e_adj
    else:      # per sample: the outlier is 1e5 x the rest
        scale = np.abs(ex["z_out"]).max(axis=(1, 2), keepdims=True)
        assert float((np.abs(o32["z_out"] - ex["z_out"]) / scale).max()) <= rc.TIGHT_Z / 2
    assert all(v <= rc.E2E_G / 2 for k, v in e_adj.items() if k != "z"), e_adj
    assert all(v <= rc.E2E_G / 2 for v in e_dis.values()), e_dis
    assert all(v <= rc.TIGHT_G / 2 for v in e_iso.values()), e_iso
    # (ii)
    if c["outlier"] is None:
        margin = float(ex["margin"].min())
    else:
        margin = min(float(rc.expect(name, clean=True)["margin"].min()), rc.outlier_margin(name))
    print("relu margin %.2e" % margin)
    assert margin >= rc.RELU_MARGIN, (name, margin)
    # (iii)
    for ps in ("adjoint", "discrete"):
        assert float(np.abs(ex[ps]["dz0"]).max()) >= rc.MIN_GRAD, (name, ps, "dz0")
        for n in names:
            assert float(np.abs(ex[ps]["grads"][n]).max()) >= rc.MIN_GRAD, (name, ps, n)
    # the instantiation of every pass
    got, _ = rc.kernel_names(name)
    for ps, (g, w) in enumerate(zip(got, rc.want_names(name))):
        assert rc.name_matches(g, w), (name, ps, g, w)


@pytest.mark.parametrize("name", [n for n in rc.BY_GROUP["plan"] if n.split("_")[1] in ("c", "f")])
def test_plans_c_and_f_never_read_the_first_and_the_last_piece(name):
    """The oracle on the poisoned coefficients (resident_cases.poisoned) gives the same solution and gradients, bit for bit."""
    c, a, ex = rc.CASES[name], rc.arrays(name), rc.expect(name)
    x = rc.poisoned(name)
    assert np.all(np.abs(x[:, 0]) == rc.POISON) and np.all(np.abs(x[:, -1]) == rc.POISON) and np.array_equal(x[:, 1:-1], a["coeffs"][:, 1:-1])
    w = rc._walk(c, rc._field64(c, a["params"]), rc._control(c, x, torch.float64), torch.from_numpy(a["z0"]).double(),
                 torch.from_numpy(a["grad_out"]).double())
    assert np.array_equal(w["z"].numpy(), ex["z_out"])
    for ps in ("adjoint", "discrete"):
        assert np.array_equal(w[ps][0].numpy(), ex[ps]["dz0"])
        assert all(np.array_equal(g.numpy(), ex[ps]["grads"][n]) for n, g in zip(rc.names_of(name), w[ps][1]))


@pytest.mark.parametrize("name", rc.BY_GROUP["fault"])
def test_fault_cases_leave_the_fp16_range_where_they_say(name):
    """The outlier's state passes NCDE_H2_LIMIT (6e4) -- in the late case from the stages of step 2 on, with an ordinary z0 and
    ordinary states through step 1 -- and no other sample comes near it.  The tail outlier, alone in its tile, carries a cotangent
    and a share of at least 5 % of dW1, db1, dWo, dbo: its tile's partial is no zero."""
    c, a, ex, names_ = rc.CASES[name], rc.arrays(name), rc.expect(name), rc.names_of(name)
    s, what, mag = c["outlier"]
    assert mag > 6.0e4 / np.abs(a["params"]["W0"]).sum(axis=1).max()
    S = rc.STAGES[c["method"]]
    per_step = np.abs(ex["stages"]).max(axis=2).reshape(c["T"] - 1, S, c["B"]).max(axis=1)      # [step, sample]
    rest = np.delete(per_step, s, axis=1)
    assert rest.max() < 100.0
    if what == "dx":
        assert np.abs(a["z0"]).max() < 10.0 and per_step[0, s] < 100.0 and (per_step[2:, s] > 6.0e4).all(), per_step[:, s]
        assert s // 16 == 1 and c["B"] == 37
    else:
        assert per_step[0, s] > 6.0e4 and s == 32 and c["B"] == 33
    assert np.any(a["grad_out"][s - 1])
    share = rc.outlier_share(name)
    print(name, share)
    if what == "dx":
        assert not np.any(a["grad_out"][s])
    else:
        assert np.abs(a["grad_out"][s]).max() >= 0.5 * np.abs(a["grad_out"]).max()
        assert all(share[ps][n] >= 0.05 for ps in share for n in names_ if n not in ("W0", "b0")), share
        assert min(np.abs(ex[ps]["dz0"][s]).max() for ps in share) >= rc.MIN_GRAD


@pytest.mark.parametrize("name", PLANNED)
def test_time_plan_builder_equals_the_oracles_plan_words(name):
    """ncde_time_plan_build on the case's axis, bit for bit the oracle's restatement in torch's arithmetic (fp32 or fp64 t): the
    GPU test then compares arithmetic, not grids."""
    import ncde_oracle as orc
    c, a = rc.CASES[name], rc.arrays(name)
    ctl = rc._control(c, a["coeffs"], torch.float32)
    want, n_fwd, n_adj = orc.time_plan_words(ctl, torch.from_numpy(rc.t_out(c)), c["method"], c["step"])
    _, got = rc.kernel_names(name)
    assert got.dtype == np.int32 and np.array_equal(got, want), name
    assert (int(got[2]), int(got[3]), int(got[4])) == (n_fwd, n_adj, len(c["out"]))
    assert rc.t_out(c).dtype == (np.float64 if c["t64"] else np.float32)


@pytest.mark.parametrize("name", DEFAULT_AXIS)
def test_default_axis_case_through_the_cpu_library(name):
    """The C++ restatement (fp32) on the case's own arrays: forward, stage record, continuous adjoint on the fp64 z, discrete
    backward on the fp64 record -- within the bounds the kernels are held to."""
    import cpu_lib_util as cu
    c, ex, names = rc.CASES[name], rc.expect(name), rc.names_of(name)
    g = rc.golden_case(name)
    cc = cu.CpuCase(g["coeffs"], g["meta"]["kind"], g["z0"], g["params"], g["layers"], c["method"], c["out"] == "knots")
    z, rec = cc.forward(record=True)
    S = rc.STAGES[c["method"]]
    assert rec.size == ex["stages"].size == (c["T"] - 1) * S * c["B"] * rc.SETS[c["set"]][1]
    if c["outlier"] is None:
        assert gu.relerr(z, ex["z_out"]) <= rc.TIGHT_Z and gu.relerr(rec.reshape(ex["stages"].shape), ex["stages"]) <= rc.TIGHT_Z
    else:
        scale = np.abs(ex["z_out"]).max(axis=(1, 2), keepdims=True)
        assert float((np.abs(z - ex["z_out"]) / scale).max()) <= rc.TIGHT_Z
    assert np.array_equal(cc.forward(), z)
    for ps in ("adjoint", "discrete"):
        src = ex["stages"] if ps == "discrete" else ex["z_out"]
        dz0, bufs = cc.backward(src, g["expect"]["grad_out"], discrete=ps == "discrete")
        errs = rc.errors({"dz0": dz0, "grads": bufs}, ex[ps], names)
        print(name, ps, " ".join("%s %.2e" % kv for kv in errs.items()))
        assert all(v <= rc.TIGHT_G for v in errs.values()), (name, ps, errs)
