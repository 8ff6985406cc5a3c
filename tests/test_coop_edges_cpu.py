"""Without a GPU: every case of tests/coop_cases.py validated before a kernel sees it -- the acceptance conditions (i) - (iii) of
resident_cases' docstring (per row where the GPU test checks per row), the cooperative instantiation of every pass (ncde_kernel_name,
a host-side query; tiled_device_cus() answers 256 without a device) and its absence under NCDE_FLAG_NO_COOP, the status word inside the
workspace, the restated plan (group size, chunks, part count, the pairs every pass-B workgroup walks) against what the table says
each case is there for, and the acceptance boundary of tiled_coop_plan on a grid of shapes and tile counts."""
import ctypes

import numpy as np
import pytest
import torch

import coop_cases as cc
import resident_cases as rc


def test_the_table_holds_what_it_is_there_for():
    """Group sizes 4 .. 28 on nine shapes with B = 16 M (three of them ragged by one sample), H = 16 .. 128 in steps of 16 except 128's
    neighbours 144+ (refused), one to three layers; two launches of several groups with their row subsets; the chunk tail; the scale
    cases on the M = 4 (C 20, H 64) and M = 12 (C 80, H 48) shapes; T = 2 .. 4, rk4 on linear and midpoint on cubic paths in turn."""
    size = {(cc.GROUP_SIZE[c["set"]],) + cc.SETS[c["set"]] + (c["B"],) for c in map(cc.CASES.get, cc.BY_GROUP["size"])}
    assert size == {(4, 80, 16, 1, 64), (4, 20, 64, 2, 64), (4, 40, 32, 2, 64), (12, 80, 48, 2, 192), (12, 40, 96, 3, 191),
                    (16, 40, 128, 2, 256), (20, 80, 80, 2, 320), (24, 80, 96, 1, 384), (28, 80, 112, 2, 447)}
    assert {cc.SETS[c["set"]][1] for c in cc.CASES.values()} == {16, 32, 48, 64, 80, 96, 112, 128}
    for kset, (C, H, nl) in cc.SETS.items():
        assert cc.GROUP_SIZE[kset] == (H // 4) * (C // 4) // 20 and (H // 4) * (C // 4) % 20 == 0
    for c in cc.CASES.values():
        assert 2 <= c["T"] <= 4 and (c["path"], c["method"]) in (("linear", "rk4"), ("cubic", "midpoint")), c["name"]
        if c["base"] is not None:
            b = cc.CASES[c["base"]]
            assert c["rows"][1] - c["rows"][0] == c["B"] <= b["B"] and (b["set"], b["T"], b["path"], b["method"], b["out"]) == \
                (c["set"], c["T"], c["path"], c["method"], c["out"]), c["name"]
    plain = [c for c in cc.CASES.values() if c["group"] != "scale"]
    assert {(c["path"], c["method"]) for c in plain} == {("linear", "rk4"), ("cubic", "midpoint")}
    assert abs(sum(c["path"] == "linear" for c in plain) - sum(c["path"] == "cubic" for c in plain)) <= 1
    g = {n: (cc.CASES[n]["set"], cc.CASES[n]["B"]) for n in cc.BY_GROUP["groups"]}
    assert g == {"groups_M4_B384": ("M4s", 384), "groups_M4_B64": ("M4s", 64), "groups_M12_B384": ("M12a", 384)}
    assert cc.CASES["size_M12_C80_H48"]["base"] == "groups_M12_B384" and cc.CASES["groups_M4_B64"]["base"] == "groups_M4_B384"
    assert cc.CASES["size_M4_C80_H16"]["base"] == "tail_M4_B4160" and cc.CASES["size_M4_C80_H16"]["rows"] == (4096, 4160)
    assert (cc.CASES["tail_M4_B4160"]["B"], cc.CASES["tail_M4_B4160"]["T"], cc.SETS["M4s"]) == (4160, 2, (80, 16, 1))
    kinds = {(c["set"], c["var"][0]) for c in map(cc.CASES.get, cc.BY_GROUP["scale"])}
    assert kinds == {(s, v) for s in ("M4a", "M12a") for v in ("gout_rows", "gout_times", "zeros", "state_path", "weights")}
    for c in map(cc.CASES.get, cc.BY_GROUP["scale"]):
        assert c["B"] == 16 * cc.GROUP_SIZE[c["set"]] and c["out"] == "knots" and c["T"] == 3, c["name"]
    assert min(cc.GOUT_ROWS) == -30 and max(cc.GOUT_ROWS) == 20 and cc.GOUT_TIMES["up"] == (-20, 0, 12)
    assert set(cc.WINDOWED) == {"size_M12_C80_H48", "size_M20_C80_H80"} and all(cc.CASES[n]["T"] == 3 for n in cc.WINDOWED)
    assert sum(map(len, cc.BY_GROUP.values())) == len(cc.CASES) == len(cc.FACTS)
    assert (cc.TIGHT_Z, cc.TIGHT_G, cc.E2E_G, cc.PER_ROW_G) == (2e-5, 2e-5, 2e-4, 2e-5) == (rc.TIGHT_Z, rc.TIGHT_G, rc.E2E_G, rc.TIGHT_G)


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_case_is_accepted(name):
    """(i) fp32 oracle vs fp64 oracle within half of each bound (end to end within E2E_G / 2 and TIGHT_Z / 2; the continuous adjoint
    fed the fp64 z rounded to fp32 within TIGHT_G / 2; where the GPU test checks dL/dz0 per row, per row within PER_ROW_G / 2),
    (ii) the ReLU margin, (iii) the gradient magnitudes -- and "coop" in every kernel name, in none under NCDE_FLAG_NO_COOP."""
    ex, o32, names = cc.expect(name), cc.oracle32(name), cc.names_of(name)
    e_adj = cc.errors(o32["adjoint"], ex["adjoint"], names, (o32["z_out"], ex["z_out"]))
    e_dis = cc.errors(o32["discrete"], ex["discrete"], names)
    e_iso = cc.errors(o32["adjoint_iso"], ex["adjoint"], names)
    print(name, "fp32 oracle: z %.2e adjoint %.2e discrete %.2e adjoint on fp64 z %.2e" %
          (e_adj["z"], max(v for k, v in e_adj.items() if k != "z"), max(e_dis.values()), max(e_iso.values())))
    assert e_adj["z"] <= cc.TIGHT_Z / 2, e_adj
    assert all(v <= cc.E2E_G / 2 for k, v in e_adj.items() if k != "z"), e_adj
    assert all(v <= cc.E2E_G / 2 for v in e_dis.values()), e_dis
    assert all(v <= cc.TIGHT_G / 2 for v in e_iso.values()), e_iso
    if name in cc.PER_ROW:
        rows = (cc.row_err(o32["adjoint_iso"]["dz0"], ex["adjoint"]["dz0"]), cc.row_err(o32["discrete"]["dz0"], ex["discrete"]["dz0"]))
        print("fp32 oracle, dz0 per row: adjoint on fp64 z %.2e discrete %.2e" % rows)
        assert max(rows) <= cc.PER_ROW_G / 2, rows
    margin = float(ex["margin"].min())
    print("relu margin %.2e" % margin)
    assert margin >= cc.RELU_MARGIN, (name, margin)
    for ps in ("adjoint", "discrete"):
        assert float(np.abs(ex[ps]["dz0"]).max()) >= cc.MIN_GRAD, (name, ps, "dz0")
        for n in names:
            assert float(np.abs(ex[ps]["grads"][n]).max()) >= cc.MIN_GRAD, (name, ps, n, float(np.abs(ex[ps]["grads"][n]).max()))
    got = cc.kernel_names(name)
    assert all("coop" in k for k in got) and got[0].startswith("ncde_fwd_tiled<") and "ncde_dwo_h2" in got[1] and "discrete" in got[2], got
    assert not any("coop" in k for k in cc.kernel_names(name, flags=cc.NO_COOP)), name
    for ps in (0, 1, 2):
        for flags in (0, 1 << 16):
            off, need = cc.status_window(name, ps, flags)
            assert 0 <= off and off % 4 == 0 and off + 4 <= need, (name, ps, flags, off, need)
        assert cc.status_window(name, ps, cc.NO_COOP)[0] < 0


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_restated_plan_holds_what_the_table_says(name):
    """coop_plan (tiled_coop_plan, the part count of tiled_adj_plan, the chunks of tiled_adj_run, my_n of ncde_dwo_h2) on the case
    against coop_cases.FACTS; and from my_n alone, the pairs the workgroups of a launch walk are every pair of the launch once."""
    M, parts, mapped, launches = cc.FACTS[name]
    plan = cc.plan_of(name)
    assert plan is not None and (plan["M"], plan["parts"], plan["xcd_mapped"]) == (M, parts, mapped), plan
    assert [(la["G"], la["n_pair"], la["my_n"]) for la in plan["launches"]] == launches
    assert M == cc.GROUP_SIZE[cc.CASES[name]["set"]] and plan["nrg"] * 16 == 20 * M and plan["chunk"] == min(plan["n_tiles"], 256 // M * M)
    for la in plan["launches"]:
        assert la["tiles"] == la["G"] * M and len(la["my_n"]) == parts and sum(la["my_n"]) == la["n_pair"] == la["tiles"] // 2
        assert cc.pairs_walked(la, parts) == list(range(la["n_pair"]))
    assert sum(la["tiles"] for la in plan["launches"]) == plan["n_tiles"] == (cc.CASES[name]["B"] + 15) // 16


def test_the_plan_edges_the_table_is_there_for():
    """Uneven my_n on both branches of the workgroup-id mapping, idle workgroups and a last chunk smaller than the one `parts` was
    sized for, several groups with nrg = 5 on the XCD-mapped branch."""
    my_n = lambda n, k=0: cc.plan_of(n)["launches"][k]["my_n"]      # noqa: E731
    assert my_n("size_M12_C80_H48") == [2, 2, 1, 1] and not cc.plan_of("size_M12_C80_H48")["xcd_mapped"]
    assert my_n("size_M20_C80_H80") == [2, 2, 1, 1, 1, 1, 1, 1] and cc.plan_of("size_M20_C80_H80")["xcd_mapped"]
    assert my_n("groups_M12_B384") == [2, 2, 2, 2, 1, 1, 1, 1] and cc.plan_of("groups_M12_B384")["launches"][0]["G"] == 2
    g4 = cc.plan_of("groups_M4_B384")
    assert (g4["launches"][0]["G"], g4["parts"], g4["xcd_mapped"], g4["nrg"]) == (6, 8, True, 5)
    tail = cc.plan_of("tail_M4_B4160")
    assert (tail["n_tiles"], tail["chunk"], tail["parts"]) == (260, 256, 32) and [la["tiles"] for la in tail["launches"]] == [256, 4]
    assert my_n("tail_M4_B4160", 1).count(0) == 30 and tail["launches"][1]["G"] == 1 and tail["launches"][0]["G"] == 64
    assert all(max(my_n(n)) == 1 for n in cc.CASES if cc.GROUP_SIZE[cc.CASES[n]["set"]] == 4 and cc.CASES[n]["B"] == 64)


@pytest.mark.parametrize("C", (16, 20, 24, 40, 80))
def test_acceptance_boundary_of_the_cooperative_plan(C):
    """C x H = 16 .. 144 x n_tiles in {M - 1, M, M + 1, 2 M} (M: the group size the shape would have, at least 1) x one to three layers:
    the library names the cooperative kernels in every pass exactly where the restatement accepts, and in no pass elsewhere."""
    n_coop = 0
    for H in range(16, 145, 16):
        m = max(1, (H // 4) * (C // 4) // 20)
        for n_tiles in sorted({m - 1, m, m + 1, 2 * m} - {0}):
            for nl in (1, 2, 3):
                for B in (16 * n_tiles, 16 * n_tiles - 1):
                    want = cc.coop_plan(C, H, nl, B) is not None
                    got = cc.bare_names(cc.bare_problem(C, H, nl, B))
                    assert all(("coop" in k) == want for k in got), (C, H, nl, B, want, got)
                    assert not any("coop" in k for k in cc.bare_names(cc.bare_problem(C, H, nl, B, flags=cc.NO_COOP)))
                    n_coop += want
    assert (n_coop > 0) == (C in (20, 40, 80))
    if C == 20:      # the issue's examples: M = 2 and M = 6 are refused, M = 4 and M = 8 accepted
        for H, ok in ((32, False), (96, False), (64, True), (128, True)):
            M = (H // 4) * 5 // 20
            assert (cc.coop_plan(20, H, 2, 16 * M) is not None) == ok == all("coop" in k for k in cc.bare_names(cc.bare_problem(20, H, 2, 16 * M)))


def test_scale_cases_are_what_they_say():
    """The cotangent cases are exact images of their base case in fp64 (the adjoint is linear in the cotangent: row s x 2^k(s)); the
    zero-cotangent row is exactly zero; the constant path leaves z at z0 and dX/dt at exactly 0; state / path exponents of the kept
    samples span the declared spreads; the weight cases scale (Wo, bo) alone."""
    for kset, base in cc.SCALE_BASE.items():
        b, eb = cc.arrays(base), cc.expect(base)
        a, e = cc.arrays("scale_%s_gout_rows" % kset), cc.expect("scale_%s_gout_rows" % kset)
        assert set(a["exps"]) == set(cc.GOUT_ROWS) and np.array_equal(a["grad_out"], b["grad_out"] * (2.0 ** a["exps"])[:, None, None])
        for ps in ("adjoint", "discrete"):
            assert np.array_equal(e[ps]["dz0"], eb[ps]["dz0"] * (2.0 ** a["exps"])[:, None]), (kset, ps)
        for k, exps in cc.GOUT_TIMES.items():
            a = cc.arrays("scale_%s_gout_times_%s" % (kset, k))
            assert np.array_equal(a["grad_out"], b["grad_out"] * (2.0 ** np.asarray(exps, np.float64))[None, :, None])
        a, e = cc.arrays("scale_%s_zeros" % kset), cc.expect("scale_%s_zeros" % kset)
        assert not np.any(a["grad_out"][cc.ZERO_GOUT]) and np.any(a["grad_out"][cc.ZERO_GOUT - 1]) and np.any(a["grad_out"][cc.CONST_PATH])
        ctl = rc._control(cc.CASES[base], a["coeffs"], torch.float64)
        for t in (0.0, 0.5, 1.25, 2.0):
            dx = ctl.derivative(torch.tensor(t, dtype=torch.float64))
            assert not dx[cc.CONST_PATH].any() and dx[cc.CONST_PATH - 1].any() and dx[cc.ZERO_GOUT].any()
        assert np.array_equal(e["z_out"][cc.CONST_PATH], np.broadcast_to(a["z0"][cc.CONST_PATH].astype(np.float64), e["z_out"][cc.CONST_PATH].shape))
        for ps in ("adjoint", "discrete"):
            assert not np.any(e[ps]["dz0"][cc.ZERO_GOUT]) and np.all(np.isfinite(e[ps]["dz0"]))
            assert np.array_equal(e[ps]["dz0"][cc.CONST_PATH], a["grad_out"][cc.CONST_PATH].astype(np.float64).sum(axis=0))
        rest = np.r_[0:cc.CONST_PATH, cc.CONST_PATH + 1:len(a["z0"])]
        assert np.array_equal(a["coeffs"][rest], b["coeffs"][rest]) and np.array_equal(a["z0"], b["z0"])
        a = cc.arrays("scale_%s_state_path" % kset)
        ez, ex = cc.SPREAD[kset]
        assert set(a["exps"][:, 0]) == set(ez) and set(a["exps"][:, 1]) == set(ex) and max(ez) - min(ez) >= 1 and max(ex) - min(ex) >= 2
        assert len({tuple(r) for r in a["exps"].tolist()}) == len(ez) * len(ex)      # every combination ...
        assert all(len({tuple(r) for r in a["exps"][t:t + 16].tolist()}) >= 3 for t in range(0, len(a["exps"]), 16))      # ... and a mix inside every sample tile
        for tag, k in (("down", cc.WO_DOWN),) + ((("up", cc.WO_UP[kset]),) if kset in cc.WO_UP else ()):
            n = "scale_%s_wo_%s" % (kset, tag)
            w, w1 = cc.arrays(n)["params"], cc._weights(n, cc.CASES[n]["seed"])      # (its own seed: the unscaled draw)
            assert np.array_equal(w["Wo"], w1["Wo"] * np.float32(2.0 ** k)) and np.array_equal(w["bo"], w1["bo"] * np.float32(2.0 ** k))
            assert all(np.array_equal(w[q], w1[q]) for q in w if q not in ("Wo", "bo")) and k != 0
            assert np.abs(w["Wo"]).max() / np.abs(b["params"]["Wo"]).max() > 2.0 ** (k - 1)
