"""The oracle's `replay` option (the mirror of the library's options["_replay"]) and the designed dopri5 cases of
tests/dopri5_cases.py, on the CPU.

  * the oracle replaying the REFERENCE's recorded step sequences (goldens g10 / g12: `trace_fwd`, `trace_bwd`) reproduces the reference:
    z within 1e-6, the adaptive adjoint's and the taped sweep's gradients within 1e-5 (|delta| / max |ref|);
  * what makes the fp64 oracle a fair reference for the fp32 kernels on the designed sequences: both precisions read the same control
    piece at every stage of every attempt, and the fp32 oracle lies within a QUARTER of the project's bars (TIGHT_Z, E2E_G) of the fp64 one;
  * every list is consumed exactly."""
import numpy as np
import pytest
import torch

import dopri5_cases as dc
import golden_util as gu
import ncde_oracle as orc
from test_oracle_golden import DOPRI5_CASES, DOPRI5_TAPED_CASES, load_dopri5_case

REPLAY_Z, REPLAY_G = 1e-6, 1e-5


def _rows(trace):
    return [(r[1], r[2]) for r in trace]


@pytest.mark.parametrize("name", DOPRI5_CASES + DOPRI5_TAPED_CASES)
def test_oracle_replays_the_reference_forward_sequence(name):
    f, m, field, ctl, t = load_dopri5_case(name)
    st = {}
    z = orc.dopri5_forward(ctl, field, f["z0"], t, m["rtol"], m["atol"], dict(m["options"], replay=_rows(m["trace_fwd"])), stats=st)
    e = gu.relerr(z, f["z_out"])
    print(name, "z %.2e" % e)
    assert len(st["trace"]) == len(m["trace_fwd"]) and st["nfe"] == m["nfe_fwd"] and [st["accepted"], st["rejected"]] == m["steps_fwd"]
    assert [(r[0], r[1], r[2]) for r in st["trace"]] == [(r[0], r[1], bool(r[2])) for r in m["trace_fwd"]]
    assert e <= REPLAY_Z, e


@pytest.mark.parametrize("name", DOPRI5_CASES)
def test_oracle_replays_the_reference_adjoint_sequence(name):
    """vjp="autograd": the stage VJP as the reference computes it; the list runs on across the per-interval solves."""
    f, m, field, ctl, t = load_dopri5_case(name)
    st = {}
    dz0, gp = orc.dopri5_adjoint(ctl, field, t, f["z_out"], f["grad_out"], m["rtol"], m["atol"], dict(m["options"], replay=_rows(m["trace_bwd"])),
                                 stats=st, vjp="autograd")
    errs = {"dz0": gu.relerr(dz0, f["dz0"]), **{n: gu.relerr(g, f["d" + n]) for n, g in zip(m["param_names"], gp)}}
    print(name, {k: "%.1e" % v for k, v in errs.items()})
    assert len(st["trace"]) == len(m["trace_bwd"]) and st["nfe"] == m["nfe_bwd"]
    assert [(r[0], r[1], r[2]) for r in st["trace"]] == [(r[0], r[1], bool(r[2])) for r in m["trace_bwd"]]
    assert max(errs.values()) <= REPLAY_G, errs


@pytest.mark.parametrize("name", DOPRI5_TAPED_CASES)
def test_oracle_replays_the_reference_sequence_under_the_taped_backward(name):
    """The first step size stays the initial-step rule's (the list's first dt is that very number), so its gradient stays active."""
    f, m, field, ctl, t = load_dopri5_case(name)
    st = {}
    z, dz0, gp = orc.dopri5_discrete_backward(ctl, field, f["z0"], t, f["grad_out"], m["rtol"], m["atol"],
                                              dict(m["options"], replay=_rows(m["trace_fwd"])), stats=st)
    errs = {"dz0": gu.relerr(dz0, f["bp_dz0"]), **{n: gu.relerr(g, f["bp_d" + n]) for n, g in zip(m["param_names"], gp)}}
    print(name, {k: "%.1e" % v for k, v in errs.items()})
    assert len(st["trace"]) == len(m["trace_fwd"]) and st["delta_active"] == m["first_step_differentiable"]
    assert gu.relerr(z, f["z_out"]) <= REPLAY_Z and max(errs.values()) <= REPLAY_G, errs


def test_replay_overrides_the_controller_and_then_runs_free():
    """Rows force dt AND the decision (a reject the error ratio would accept, an accept past max_step); attempts beyond the list run
    free; replay=None changes nothing."""
    f, m, field, ctl, t = load_dopri5_case("g10_ncde_dopri5_rect_final")
    free, forced, again = {}, {}, {}
    z = orc.dopri5_forward(ctl, field, f["z0"], t, m["rtol"], m["atol"], dict(m["options"]), stats=free)
    rows = [(0.0625, 0), (0.0625, 1), (3.0, 1)]
    orc.dopri5_forward(ctl, field, f["z0"], t, m["rtol"], m["atol"], dict(m["options"], max_step=2.0, replay=rows), stats=forced)
    tr = forced["trace"]
    assert [(r[1], r[2]) for r in tr[:3]] == [(0.0625, False), (0.0625, True), (3.0, True)] and tr[2][0] == 0.0625
    assert len(tr) > 3 and all(r[1] <= 2.0 for r in tr[3:]) and tr[3][0] == 3.0625
    z2 = orc.dopri5_forward(ctl, field, f["z0"], t, m["rtol"], m["atol"], dict(m["options"], replay=None), stats=again)
    assert torch.equal(z, z2) and again["trace"] == free["trace"]


@pytest.mark.parametrize("axis,variant", [(a, v) for a in dc.AXES for v in dc.VARIANTS[a]])
def test_designed_sequences_hold_what_they_are_there_for(axis, variant):
    dc.design_check(axis, variant)


@pytest.mark.parametrize("cid", dc.case_ids())
def test_designed_case_is_a_fair_fp64_reference(cid):
    """Same control pieces in both precisions at every stage of every attempt, forward and adjoint; the fp32 oracle within a quarter of
    the bars of the fp64 one -- also from a z0 moved at the level two fp32 solves differ by anyway (dopri5_cases.SHAKE): no ReLU mask of
    the case sits on a knife edge (a seed on which one does is replaced in dopri5_cases.SEEDS)."""
    r64, r32 = dc.reference(cid), dc.run_oracle(cid, torch.float32)
    a = dc.arrays(cid)
    n_f, n_b = len(a["fwd"]), len(a["bwd"])
    assert len(r64["pieces_fwd"]) == 1 + 6 * n_f and len(r64["pieces_adj"]) >= (len(a["t"]) - 1) + 6 * n_b
    assert r32["pieces_fwd"] == r64["pieces_fwd"] and r32["pieces_adj"] == r64["pieces_adj"]
    assert len({p for p in r64["pieces_fwd"][1 + 6 * 6:1 + 6 * 7]} | {r64["pieces_fwd"][6 * 6]}) >= 3      # attempt 7: three or more pieces
    assert np.array_equal(r32["trace_fwd"], r64["trace_fwd"]) and np.array_equal(r32["trace_bwd"], r64["trace_bwd"])
    assert r64["nfe_fwd"] == 1 + 6 * n_f and r64["steps_fwd"] == (sum(r[1] for r in a["fwd"]), sum(1 - r[1] for r in a["fwd"]))
    errs = dc.errors(r32, r64)
    print(cid, " ".join("%s %.1e" % kv for kv in errs.items()))
    z, g_adj, g_tape = dc.worst(errs)
    assert z <= dc.TIGHT_Z / 4, errs
    assert g_adj <= dc.E2E_G / 4 and g_tape <= dc.E2E_G / 4, errs
    for k in dc.SHAKES:
        se = dc.errors(dc.run_oracle(cid, torch.float32, shake=k), r64)
        assert dc.worst(se)[1] <= dc.E2E_G / 4 and dc.worst(se)[2] <= dc.E2E_G / 4, (k, se)
    for mode in ("adj", "tape"):      # a wrong gradient cannot hide in a near-zero tensor
        assert all(float(np.abs(v).max()) >= 1e3 * dc.E2E_G for v in r64[mode].values()), mode


@pytest.mark.parametrize("cid", ["h32_pad_nl1-A-end-B21", "h32_pad_nl1-Cc-early-B21"])
def test_a_list_that_is_one_row_short_or_long_is_refused(cid):
    a = dc.arrays(cid)
    for kw in ({"fwd": a["fwd"][:-1]}, {"bwd": a["bwd"][:-1]}, {"fwd": a["fwd"] + ((0.5, 1),)}, {"bwd": a["bwd"] + ((0.5, 1),)}):
        with pytest.raises(AssertionError, match="attempts for a list of"):
            dc.run_oracle(cid, torch.float32, **kw)


def test_cases_cover_every_route_and_batch():
    ids = dc.case_ids()
    assert len(ids) == len(set(ids)) and {dc.parse(c)[0] for c in ids} == set(dc.SHAPES)
    assert {dc.parse(c)[3] for c in ids if dc.parse(c)[0] in ("h32", "h40")} == {1, 21, 50}
    assert set(dc.SEEDS) <= set(ids)
