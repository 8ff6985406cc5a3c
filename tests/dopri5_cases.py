"""Seeded cases for the adaptive dopri5 kernels on DESIGNED, irregular step sequences: every kernel set of the three entry points
(forward, adaptive continuous adjoint, taped backward) is made to take a hand-written list of (dt, accepted) attempts through
options["_replay"], and the oracle (oracle/ncde_oracle.py, `replay`) takes the same list in float64 on float64 copies of the inputs.

What a sequence holds that the pinned sequences (first_step = min_step = max_step) never do: a rejected first attempt, two rejects in
a row, a reject right after a step that emitted outputs, a step of 2^-5, a step across three knots (its stage times on three or more
control pieces), steps with 0 / 1 / 2 / 5 outputs, outputs exactly on a step's t1, on knots and between knots, a last step that runs past
the final output (and, in the `end` variant, past the last knot: the clamp of dp_stage_desc), a user knot grid, a start inside the
first piece; the adjoint lists hold a reject, a step of 2^-5 and a step past the interval end in EVERY output interval, the last one
running before the first knot.  Every knot, output time and dt is a multiple of 1/32: t0 accumulates exactly in fp32 and in fp64, and
no stage time t0 + alpha dt lies on a knot (design_check), so both precisions read the same control pieces
(tests/test_dopri5_replay_cpu.py holds that, and the fp32 oracle within a quarter of the bars of the fp64 one).

Bars: the project's TIGHT_Z (z) and E2E_G (every gradient), |delta| / max |ref|, against the fp64 oracle.

Seeds: an adaptive adjoint of ~40 attempts forms ~5e5 ReLU pre-activations per case; where one of a sample lies within fp32 round-off of
zero its mask is undecided, and two correct fp32 solves part by 1e-4 .. 1e-2 on that sample's gradients (seen here between the fp32
and the fp64 oracle, and reproduced by moving the fp32 oracle's z0 by 4e-6).  Such a case measures nothing: each case takes the first
seed pair on which the fp32 oracle, plain and from three shaken z0, stays within a quarter of the bars (SEEDS, run_oracle).

Measured on an MI355X, worst over the variants and batches of a shape and axis, z / adjoint=True gradients / adjoint=False gradients:
    h32          A 2.3e-06/2.9e-06/1.7e-06   B 2.9e-06/2.8e-06/5.1e-06   Cl 4.2e-06/2.7e-06/1.8e-06   Cc 2.7e-06/2.8e-06/2.3e-06
    h32_pad_nl1  A 2.0e-06/2.1e-06/9.1e-07   B 1.7e-06/2.1e-06/2.2e-06   Cl 2.7e-06/2.6e-06/8.8e-07   Cc 2.2e-06/2.3e-06/1.1e-06
    h32_nl2      A 2.4e-06/3.4e-06/8.9e-07   B 2.3e-06/2.6e-06/2.7e-06   Cl 2.3e-06/2.3e-06/1.1e-06   Cc 2.8e-06/2.1e-06/1.1e-06
    h32_nl4      A 2.3e-06/2.1e-06/7.9e-07   B 2.8e-06/3.2e-06/3.0e-06   Cl 2.5e-06/3.2e-06/2.0e-06   Cc 2.5e-06/6.0e-06/2.1e-06
    h64          A 2.7e-06/3.0e-06/7.2e-07   B 2.6e-06/3.0e-06/1.3e-06   Cl 2.9e-06/4.9e-06/9.1e-07   Cc 4.4e-06/3.7e-06/1.4e-06
    h64_pad      A 3.1e-06/2.3e-06/4.5e-07   B 3.1e-06/3.1e-06/1.4e-06   Cl 2.4e-06/3.2e-06/6.7e-07   Cc 3.0e-06/3.1e-06/7.3e-07
    h40          A 2.8e-06/3.3e-06/8.3e-07   B 2.8e-06/2.9e-06/2.7e-06   Cl 3.2e-06/3.6e-06/1.4e-06   Cc 2.8e-06/8.5e-06/1.9e-06
    h32_generic  A 2.2e-06/2.9e-06/6.9e-07   B 3.1e-06/3.2e-06/4.2e-06   Cl 2.7e-06/4.1e-06/1.7e-06   Cc 2.0e-06/2.5e-06/2.5e-06
(bars 2e-5 / 2e-4 / 2e-4).  No kernel had to be changed.

Helper only: no test functions."""
import functools
from fractions import Fraction

import numpy as np
import torch

import golden_util as gu
import ncde_oracle as orc

TIGHT_Z, E2E_G = 2e-5, 2e-4
RTOL, ATOL = 1e-3, 1e-5

# ---- shapes: (C, H, HH, nl), kernel_flags, the kernel name each pass must start with --------------------------------------------------
_FUSED = ("ncde_dpf_adj", "ncde_dpf_tape")
_LAUNCH = ("ncde_dp_stage", "ncde_dp_tape_backward")
SHAPES = {
    "h32": ((20, 32, 32, 3), 0, ("ncde_dpf_fwd<H32",) + _FUSED),
    "h32_pad_nl1": ((5, 16, 24, 1), 0, ("ncde_dpf_fwd<H32",) + _FUSED),
    "h32_nl2": ((6, 24, 32, 2), 0, ("ncde_dpf_fwd<H32",) + _FUSED),      # the NL = 2 instantiations of the fused adjoint and sweep
    "h32_nl4": ((20, 32, 32, 4), 0, ("ncde_dpf_fwd<H32",) + _LAUNCH),
    "h64": ((4, 64, 64, 3), 0, ("ncde_dpf_fwd<H64",) + _LAUNCH),
    "h64_pad": ((3, 48, 64, 2), 0, ("ncde_dpf_fwd<H64",) + _LAUNCH),
    "h40": ((7, 40, 40, 2), 0, ("ncde_dp_stage",) + _LAUNCH),
    "h32_generic": ((20, 32, 32, 3), 1, ("ncde_dp_stage",) + _LAUNCH),      # kernel_flags = 1: FLAG_FORCE_GENERIC
}
BATCH = 21                                   # two 16-sample workgroups, the second one ragged
BATCH_EXTRA = {"h32": (1, 50), "h40": (1, 50)}

# ---- time axes -------------------------------------------------------------------------------------------------------------------------
_D = 1.0 / 32
USER_KNOTS = (0.25, 0.75, 2.0, 2.75, 4.75, 5.25, 6.0, 7.25, 9.25)      # spacings 0.5, 1.25, 0.75, 2.0, 0.5, 0.75, 1.25, 2.0
AXES = {      # name: (interpolation, knot grid or None = the default integer grid 0 .. 8)
    "A": ("linear", None),          # rectilinear data with missing values, linear evaluation
    "B": ("cubic", None),
    "Cl": ("linear", USER_KNOTS),
    "Cc": ("cubic", USER_KNOTS),
}
VARIANTS = {"A": ("end", "early"), "B": ("end", "early"), "Cl": ("end", "early", "inside"), "Cc": ("end", "early")}
N_KNOTS = 9

# output times and forward attempts (dt, accepted); in the comments: t0 -> t1 and the outputs the step holds
_T_DEFAULT = (0.0, 13 * _D, 0.75, 2.0, 2.5, 3.28125, 4.0, 4.5, 6.0, 6.25, 7.40625, 8.0)
_F_DEFAULT = (
    (2.0, 0), (1.5, 0),          # a rejected first attempt, two rejects in a row
    (0.75, 1),                   # 0 -> 0.75: outputs 13/32 and 0.75 = t1
    (1.5, 0),                    # a reject right after a step that held outputs
    (_D, 1),                     # 0.75 -> 0.78125: 2^-5, no output
    (0.71875, 1),                # -> 1.5: no output (two accepted steps without one)
    (3.25, 1),                   # 1.5 -> 4.75 over the knots 2, 3, 4: outputs 2.0, 2.5, 3.28125, 4.0, 4.5; stages on pieces 1, 2, 4
    (4.0, 0),                    # 4.75 -> 8.75 rejected: stage times past the last knot
    (0.5, 1),                    # -> 5.25: no output, after a reject
    (0.5, 0),
    (1.0, 1),                    # 5.25 -> 6.25: outputs 6.0 (a knot) and 6.25 = t1
    (0.25, 1),                   # -> 6.5: no output
    (2.25, 1),                   # 6.5 -> 8.75: outputs 7.40625 and 8.0 = the last knot; runs past it
)
_T_USER = (0.25, 0.5, 0.75, 1.0, 2.0, 2.5, 3.28125, 4.75, 4.875, 6.0, 6.5, 7.40625, 9.25)
_F_USER = (
    (2.0, 0), (1.5, 0),
    (0.75, 1),                   # 0.25 -> 1.0: outputs 0.5, 0.75 (a knot), 1.0 = t1
    (1.5, 0),
    (_D, 1),                     # 1.0 -> 1.03125
    (0.46875, 1),                # -> 1.5
    (3.5, 1),                    # 1.5 -> 5.0 over the knots 2.0, 2.75, 4.75: outputs 2.0, 2.5, 3.28125, 4.75, 4.875; stages on pieces 1, 2, 3, 4
    (4.5, 0),                    # 5.0 -> 9.5 rejected: past the last knot
    (0.5, 1),                    # -> 5.5 across the knot 5.25
    (0.5, 0),
    (1.0, 1),                    # 5.5 -> 6.5: outputs 6.0 (a knot), 6.5 = t1
    (0.25, 1),                   # -> 6.75
    (2.75, 1),                   # 6.75 -> 9.5: outputs 7.40625 and 9.25 = the last knot; runs past it
)


def times(axis, variant):
    """-> (output times, forward attempts) of the axis' variant.  end: the last output is the last knot, the last step runs past it.
    early: the last output (and the last step's t1) lie strictly inside the path.  inside (user grid): t[0] strictly inside the first piece."""
    t, f = (_T_DEFAULT, _F_DEFAULT) if AXES[axis][1] is None else (_T_USER, _F_USER)
    t, f = list(t), [list(r) for r in f]
    if variant == "early":
        t = t[:-1]
        f[-1][0] = 1.25 if AXES[axis][1] is None else 2.0      # 6.5 -> 7.75 < 8 / 6.75 -> 8.75 < 9.25
    elif variant == "inside":
        t[0] = 13 * _D                                         # 0.40625 in (0.25, 0.75)
        f[2][0] = 1.0 - 13 * _D                                # -> 1.0 as before
    else:
        assert variant == "end"
    return tuple(t), tuple((float(a), int(b)) for a, b in f)


def _stage_on_knot(t0, dt, sign, knots):
    """Does a stage time t0 + alpha dt (exact arithmetic; sign -1: negated time) lie on a knot?"""
    for al in (Fraction(1, 5), Fraction(3, 10), Fraction(4, 5), Fraction(8, 9)):
        if sign * (Fraction(t0) + al * Fraction(dt)) in knots:
            return True
    return False


def _knot_set(axis):
    kn = AXES[axis][1]
    return {Fraction(k) for k in (kn if kn is not None else range(N_KNOTS))}


@functools.lru_cache(maxsize=None)
def adjoint_replay(axis, variant):
    """The adjoint's attempts in negated time, concatenated in the order the solve consumes them (interval n-1 first).  Per output
    interval of length L: a reject, a step of 2^-5, and a last step that runs `over` past the interval end -- in interval 1 before the
    first knot.  It overshoots by 1/4 (even intervals and interval 1) or 1/8."""
    t, _ = times(axis, variant)
    knots = _knot_set(axis)
    rows = []
    for i in range(len(t) - 1, 0, -1):
        s0, L = -t[i], t[i] - t[i - 1]
        assert L >= 2 * _D
        if i % 2 == 0:
            head = [(L + 0.5, 0), (_D, 1)]
        else:
            h = max(_D, int(16 * L) * _D)      # about half the interval
            head = [(_D, 1), (2 * L, 0)] + ([(h, 1)] if L - _D - h >= 2 * _D else [])
        done = 0.0
        for dt, acc in head:      # (a dt grows by 1/32 while one of its stage times would lie on a knot; 2^-5 itself never does)
            while _stage_on_knot(s0 + done, dt, -1, knots):
                dt += _D
            assert not acc or done + dt < L
            rows.append((dt, acc))
            done += dt if acc else 0.0
        dt = L - done + (0.25 if i % 2 == 0 or i == 1 else 0.125)
        while _stage_on_knot(s0 + done, dt, -1, knots):
            dt += _D
        rows.append((dt, 1))
    return tuple((float(a), int(b)) for a, b in rows)


def walk(t, rows, sign=1):
    """The attempts of one forward solve as the controller walks them -> list of (t0, dt, accepted, outputs held)."""
    out, t0, j = [], Fraction(t[0]) * sign, 1
    for dt, acc in rows:
        held = []
        if acc:
            t1 = t0 + Fraction(dt)
            while j < len(t) and Fraction(t[j]) <= t1:
                held.append(t[j])
                j += 1
        out.append((float(t0), dt, acc, held))
        if acc:
            t0 = t1
    assert j == len(t), "the list ends before the last output"
    return out


def design_check(axis, variant):
    """The properties the sequences are there for, asserted from the lists alone."""
    t, fwd = times(axis, variant)
    kn = AXES[axis][1] if AXES[axis][1] is not None else tuple(float(k) for k in range(N_KNOTS))
    knots = _knot_set(axis)
    assert 12 <= len(fwd) <= 30
    assert all(Fraction(v) % Fraction(1, 32) == 0 for v in list(t) + list(kn) + [r[0] for r in fwd] + [r[0] for r in adjoint_replay(axis, variant)])
    w = walk(t, fwd)
    assert w[-1][2] and w[-1][3] and w[-1][3][-1] == t[-1], "the last row is the step that holds the last output"
    acc = [r for r in w if r[2]]
    assert not w[0][2] and not w[1][2]                                                        # a rejected first attempt, two rejects in a row
    assert any(a[2] and a[3] and not b[2] for a, b in zip(w[:-1], w[1:]))                     # a reject right after a step with outputs
    assert any(not a[2] and b[2] and not b[3] for a, b in zip(w[:-1], w[1:]))                 # a step without outputs right after a reject
    assert any(r[1] == _D for r in acc)
    assert any(sum(r[0] < k < r[0] + r[1] for k in kn) >= 3 for r in acc)                     # a step across three knots
    assert any(len(r[3]) >= 3 for r in acc) and any(len(r[3]) == 2 for r in acc)
    assert any(r[3] and r[3][-1] == r[0] + r[1] for r in acc)                                 # an output exactly at t1
    assert any(not a[3] and not b[3] for a, b in zip(acc[:-1], acc[1:]))                      # two accepted steps in a row without an output
    assert any(x in kn for x in t[1:]) and any(x not in kn for x in t[1:])
    last = acc[-1]
    assert last[0] + last[1] > t[-1]                                                          # the last step overshoots the last output
    if variant == "early":
        assert t[-1] < kn[-1] and last[0] + last[1] < kn[-1]
    else:
        assert t[-1] == kn[-1] and last[0] + last[1] > kn[-1]
    assert any(not r[2] and r[0] + r[1] > kn[-1] for r in w)                                  # a rejected attempt past the last knot
    assert (kn[0] < t[0] < kn[1]) if variant == "inside" else t[0] == kn[0]
    for t0, dt, _, _ in w:
        assert not _stage_on_knot(t0, dt, 1, knots), (t0, dt)
    # adjoint: per interval a reject, a 2^-5 step, a last step past the interval end; interval 1 ends before the first knot
    rows, k = adjoint_replay(axis, variant), 0
    for i in range(len(t) - 1, 0, -1):
        s, seen_rej, seen_short = Fraction(-t[i]), False, False
        while True:
            dt, a = rows[k]
            k += 1
            assert not _stage_on_knot(s, dt, -1, knots)
            seen_rej |= not a
            seen_short |= bool(a) and dt == _D
            if a:
                s += Fraction(dt)
                if s >= -t[i - 1]:
                    break
        assert seen_rej and seen_short and s > -t[i - 1], i
        if i == 1:
            assert -s < kn[0]
    assert k == len(rows)


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def case_ids(shapes=None, extra_batches=True):
    ids = []
    for sh in (shapes or SHAPES):
        for ax in AXES:
            for v in VARIANTS[ax]:
                ids.append("%s-%s-%s-B%d" % (sh, ax, v, BATCH))
            if extra_batches:
                ids += ["%s-%s-end-B%d" % (sh, ax, b) for b in BATCH_EXTRA.get(sh, ())]
    return ids


def parse(cid):
    sh, ax, v, b = cid.split("-")
    return sh, ax, v, int(b[1:])


# case id -> (data seed, weight seed): the first pair of SEED_PAIRS on which the fp32 ORACLE, plain and from every shaken z0 (run_oracle),
# stays within a quarter of the bars of the fp64 oracle -- a property of the inputs and the oracle alone, no kernel is consulted
# (tests/test_dopri5_replay_cpu.py holds it for every case).  Cases not listed take the first pair.
SEED_PAIRS = [(d, w) for w in range(9, 21) for d in (95, 97)]
SEEDS = {
    "h32-A-end-B50": (95, 11), "h32-B-end-B21": (97, 9), "h32-B-early-B21": (97, 9), "h32-B-end-B50": (97, 9), "h32-Cl-end-B21": (95, 11),
    "h32-Cl-early-B21": (95, 11), "h32-Cl-inside-B21": (97, 10), "h32-Cl-end-B50": (97, 12), "h32-Cc-end-B21": (97, 10),
    "h32-Cc-early-B21": (97, 10), "h32-Cc-end-B50": (97, 11), "h32_pad_nl1-B-end-B21": (97, 9), "h32_pad_nl1-B-early-B21": (97, 9),
    "h32_pad_nl1-Cl-inside-B21": (97, 9), "h32_nl2-Cl-inside-B21": (97, 9), "h32_nl2-Cc-early-B21": (95, 10),
    "h32_nl4-A-end-B21": (95, 10), "h32_nl4-B-end-B21": (97, 9), "h32_nl4-B-early-B21": (97, 9),
    "h32_nl4-Cl-end-B21": (97, 9), "h32_nl4-Cl-early-B21": (97, 9), "h32_nl4-Cl-inside-B21": (97, 10), "h64-A-end-B21": (97, 14),
    "h64-A-early-B21": (97, 10), "h64-B-end-B21": (97, 10), "h64-B-early-B21": (97, 9), "h64-Cl-end-B21": (97, 9), "h64-Cl-early-B21": (97, 9),
    "h64-Cl-inside-B21": (95, 10), "h64-Cc-end-B21": (97, 10), "h64-Cc-early-B21": (97, 10), "h64_pad-A-end-B21": (97, 9),
    "h64_pad-A-early-B21": (97, 9), "h64_pad-B-end-B21": (97, 9), "h64_pad-B-early-B21": (97, 9), "h64_pad-Cc-early-B21": (95, 10),
    "h40-A-end-B21": (97, 9), "h40-A-early-B21": (97, 9), "h40-A-end-B50": (95, 11), "h40-B-end-B21": (97, 10), "h40-B-end-B50": (97, 10),
    "h40-Cl-end-B50": (97, 16), "h40-Cc-end-B50": (95, 17), "h32_generic-B-end-B21": (97, 9), "h32_generic-B-early-B21": (97, 9),
    "h32_generic-Cl-end-B21": (95, 11), "h32_generic-Cl-early-B21": (95, 11), "h32_generic-Cl-inside-B21": (97, 10),
    "h32_generic-Cc-end-B21": (97, 10), "h32_generic-Cc-early-B21": (97, 10),
}


@functools.lru_cache(maxsize=None)
def arrays(cid):
    """The case's inputs as fp32 / host arrays (built once; callers do not modify them)."""
    sh, ax, v, B = parse(cid)
    (C, H, HH, nl), flags, route = SHAPES[sh]
    interp, kn = AXES[ax]
    dseed, wseed = SEEDS.get(cid, SEED_PAIRS[0])
    t, fwd = times(ax, v)
    knots = None if kn is None else np.asarray(kn, dtype=np.float32)
    if ax == "A":
        coeffs = gu.data.make_rectilinear_coeffs(B, (N_KNOTS + 1) // 2, C - 1, missing=0.3, seed=dseed)
    elif ax == "B":
        coeffs = gu.data.make_cubic_coeffs(B, N_KNOTS, C - 1, seed=dseed + 1)
    else:      # the user grid: the series observed at the knots (its time channel = the knots), missing values for the linear path
        x = gu.data.synthetic_series(B, N_KNOTS, C - 1, missing=0.3 if interp == "linear" else 0.0, seed=dseed + 2)
        x[..., 0] = knots
        coeffs = gu.data.linear_interpolation_coeffs(x, t=knots) if interp == "linear" else gu.data.natural_cubic_coeffs(x, t=knots)
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float32)
    assert coeffs.shape[1] == (N_KNOTS if interp == "linear" else N_KNOTS - 1) and not np.isnan(coeffs).any()
    p = gu.data.make_field_weights(H, HH, C, seed=wseed)
    if nl == 1:
        p = {k: a for k, a in p.items() if k not in ("W1", "b1")}
    rw = gu.data.make_readin_weights(H, C, 1, seed=wseed)
    z0 = (coeffs[:, 0, :C] @ rw["Wi"].T + rw["bi"]).astype(np.float32)
    gout = (gu.data.normal(31, B * len(t) * H, stream=1).reshape(B, len(t), H) / np.sqrt(len(t))).astype(np.float32)
    return {"C": C, "H": H, "HH": HH, "nl": nl, "B": B, "flags": flags, "route": route, "interp": interp, "knots": knots, "coeffs": coeffs,
            "params": p, "names": [n for n in ("W0", "b0", "W1", "b1", "Wo", "bo") if n in p], "z0": z0, "grad_out": gout,
            "layers": [("W0", "b0")] + [("W1", "b1")] * (nl - 1), "t": np.asarray(t, dtype=np.float64), "fwd": fwd,
            "bwd": adjoint_replay(ax, v)}


class _Control(orc.Control):
    """The oracle's control path keeping the piece of every call."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.pieces = []

    def piece(self, t):
        idx = super().piece(t)
        self.pieces.append(idx)
        return idx


SHAKE = 4e-6      # of max |z0|: how far the fp32 oracle's z sits from the fp64 oracle's on these cases (1.2e-6 .. 3.9e-6)
SHAKES = (0, 1, 2)


def run_oracle(cid, dtype, fwd=None, bwd=None, shake=None):
    """The oracle in `dtype` on the case's inputs cast to it, replaying the case's lists (or `fwd` / `bwd`) -> dict of arrays, traces,
    nfe and the control pieces read, per solve.  Raises unless every list is consumed exactly: one trace row per list row.
    shake = k: z0 moved by seeded noise of SHAKE max |z0| -- the level at which two correct fp32 solves differ anyway.  A case is a fair
    yardstick only if its gradients do not care: where a ReLU pre-activation of some sample lies within that of zero, the mask -- an O(1)
    factor on that sample's cotangent -- is undecided in fp32, and the gradients of two correct implementations part by 1e-4 .. 1e-2."""
    a = arrays(cid)
    fwd = a["fwd"] if fwd is None else fwd
    bwd = a["bwd"] if bwd is None else bwd
    cast = lambda x: torch.from_numpy(np.asarray(x)).to(dtype)      # noqa: E731
    pt = {k: cast(v) for k, v in a["params"].items()}
    field = orc.Field([(pt[w], pt[b]) for w, b in a["layers"]], pt["Wo"], pt["bo"], a["H"], a["C"])
    ctl = _Control(cast(a["coeffs"]), a["interp"], None if a["knots"] is None else cast(a["knots"]))
    t, z0, gout = torch.from_numpy(a["t"]), cast(a["z0"]), cast(a["grad_out"])
    if shake is not None:
        noise = 2 * torch.rand(z0.shape, generator=torch.Generator().manual_seed(shake), dtype=torch.float64) - 1
        z0 = z0 + (SHAKE * float(z0.abs().max()) * noise).to(dtype)
    of = {"first_step": fwd[0][0], "replay": fwd}
    ob = {"first_step": bwd[0][0], "replay": bwd}
    res, sf, sa, sd = {}, {}, {}, {}
    z = orc.dopri5_forward(ctl, field, z0, t, RTOL, ATOL, of, stats=sf)
    res["pieces_fwd"], ctl.pieces = ctl.pieces, []
    dz0, gp = orc.dopri5_adjoint(ctl, field, t, z, gout, RTOL, ATOL, ob, stats=sa)
    res["pieces_adj"], ctl.pieces = ctl.pieces, []
    zt, bdz0, bgp = orc.dopri5_discrete_backward(ctl, field, z0, t, gout, RTOL, ATOL, of, stats=sd)
    assert torch.equal(zt, z) and not sd["delta_active"]
    for name, st, rows in (("forward", sf, fwd), ("adjoint", sa, bwd), ("taped", sd, fwd)):
        assert len(st["trace"]) == len(rows), "%s: %d attempts for a list of %d rows" % (name, len(st["trace"]), len(rows))
        assert [bool(r[2]) for r in st["trace"]] == [bool(r[1]) for r in rows] and [r[1] for r in st["trace"]] == [r[0] for r in rows], name
    res.update(z_out=z.numpy(), adj={"dz0": dz0.numpy(), **{n: g.numpy() for n, g in zip(a["names"], gp)}},
               tape={"dz0": bdz0.numpy(), **{n: g.numpy() for n, g in zip(a["names"], bgp)}},
               trace_fwd=np.asarray([r[:3] for r in sf["trace"]], dtype=np.float64),
               trace_bwd=np.asarray([r[:3] for r in sa["trace"]], dtype=np.float64), nfe_fwd=sf["nfe"], nfe_bwd=sa["nfe"],
               steps_fwd=(sf["accepted"], sf["rejected"]), steps_bwd=(sa["accepted"], sa["rejected"]))
    return res


@functools.lru_cache(maxsize=None)
def reference(cid):
    """The fp64 oracle's results (computed once per case and shared; callers do not modify them)."""
    return run_oracle(cid, torch.float64)


def errors(res, ref):
    """res / ref: {z_out, adj{...}, tape{...}} -> {z, adj: worst gradient error, tape: ...} and the per-tensor figures."""
    out = {"z": gu.relerr(res["z_out"], ref["z_out"])}
    for mode in ("adj", "tape"):
        if mode in res:
            for k, v in ref[mode].items():
                out["%s_d%s" % (mode, k if k != "dz0" else "z0")] = gu.relerr(res[mode][k], v)
    return out


def worst(errs):
    return (errs["z"], max([v for k, v in errs.items() if k.startswith("adj_")] or [0.0]),
            max([v for k, v in errs.items() if k.startswith("tape_")] or [0.0]))
