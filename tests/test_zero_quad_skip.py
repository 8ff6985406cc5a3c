"""Narrow stages of the register-resident adjoint: ncde_adj_fast3 (continuous adjoint and exact discrete
backward) runs channel quad 0 of the output layer only on a stage whose dX is zero in every channel >= 4 for the whole 16-sample
tile -- the time-only pieces of a rectilinear path.  A skipped term is dP = 0 (or tanh(.) * 0) added to an accumulator, so nothing
but the sign of a zero may change: every case runs the default path and the NCDE_FLAG_DENSE_CHANNELS path (all quads on every stage)
on the same inputs and requires torch.equal of z at all knots, every parameter gradient and grad_z0.  (The forward kernel has no
narrow stages; its z is compared all the same, as the input both backward passes start from.)

Base shape: B = 40 (three tiles, the last half empty), raw length 6 (11 rectilinear knots), C = 20, H = HH = 32, three layers.
"""
import functools

import numpy as np
import pytest
import torch

import golden_util as gu

pytestmark = pytest.mark.gpu

B, L, H, HH, NL = 40, 6, 32, 32, 3
MID = 20      # a sample of the middle tile (samples 16 .. 31)


def _case(coeffs, method, C, seed=6100):
    p = dict(gu.data.make_field_weights(H, HH, C, seed=seed + 1))
    rw = gu.data.make_readin_weights(H, C, 1, seed=seed + 1)
    z0 = (coeffs[:, 0] @ rw["Wi"].T + rw["bi"]).astype(np.float32)
    names = ["W0", "b0", "W1", "b1", "Wo", "bo"]
    T = coeffs.shape[1]
    gout = (gu.data.normal(seed + 2, B * T * H, stream=1).reshape(B, T, H) / np.sqrt(T)).astype(np.float32)
    return {"meta": {"kind": "linear", "method": method, "sequence": True, "param_names": names, "field_kind": "original", "field_mode": "matmul",
                     "dims": {"C": C, "H": H, "HH": HH, "nl": NL}, "field": "original"},
            "coeffs": np.ascontiguousarray(coeffs.astype(np.float32)), "z0": z0, "params": p,
            "layers": [("W0", "b0")] + [("W1", "b1")] * (NL - 1), "H": H, "C": C, "expect": {"grad_out": gout}}


@functools.lru_cache(maxsize=None)
def _rect(C=20):
    c = gu.data.make_rectilinear_coeffs(B, L, C - 1, missing=0.3, seed=6000 + C)
    assert c.shape == (B, 2 * L - 1, C)
    c.setflags(write=False)
    return c


def _time_only_pieces(c):
    """Pieces on which no data channel of any sample moves."""
    d = c[:, 1:, 1:] - c[:, :-1, 1:]
    return [p for p in range(d.shape[1]) if not np.any(d[:, p])]


def _piece():
    """A time-only piece in the middle of the base path, with pieces that move the values on both sides."""
    c = _rect()
    narrow = _time_only_pieces(c)
    assert len(narrow) >= L - 1 and len(narrow) < c.shape[1] - 1, narrow      # the path alternates
    p = [q for q in narrow if 3 <= q <= 6][0]
    return p


def _same(a, b):
    return torch.equal(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b)))


def _check(case, adjoint, C=20):
    import gpu_util
    from ncde_amd import _lib
    skip = gpu_util.run_case(case, adjoint=adjoint)
    dense = gpu_util.run_case(case, flags=_lib.FLAG_DENSE_CHANNELS, adjoint=adjoint)
    k = skip["kernels"]
    assert k == dense["kernels"], (k, dense["kernels"])      # the same kernels, under the same names
    assert k[0].startswith("ncde_fwd_fast_bf3<H32,HH32,C%d," % C), k
    bwd = k[1] if adjoint else k[2]
    assert bwd.startswith("ncde_adj_fast3<H32,HH32,C%d,NL3" % C) and ("discrete" in bwd) == (not adjoint), k
    assert np.isfinite(skip["z_out"]).all() and np.isfinite(skip["dz0"]).all()
    bad = []
    if not _same(skip["z_out"], dense["z_out"]):
        bad.append("z")
    if not _same(skip["dz0"], dense["dz0"]):
        bad.append("grad_z0")
    assert set(skip["grads"]) == set(case["params"])
    for name in skip["grads"]:
        if not _same(skip["grads"][name], dense["grads"][name]):
            bad.append(name)
    assert not bad, (case["meta"]["method"], "adjoint" if adjoint else "discrete", bad)
    return skip


@pytest.mark.parametrize("adjoint", [True, False])
@pytest.mark.parametrize("method", ["rk4", "midpoint", "euler"])
def test_rectilinear_path(method, adjoint, gpu_lib):
    """Alternating narrow / wide steps: the clear of a ring word at S = 4, 2, 1, forwards and on the backwards walk."""
    _check(_case(_rect(), method, 20), adjoint)


@pytest.mark.parametrize("adjoint", [True, False])
@pytest.mark.parametrize("method", ["rk4", "euler"])
def test_every_channel_moves_on_every_piece(method, adjoint, gpu_lib):
    """A plain linear path: never narrow (a word that was wrongly cleared would drop terms)."""
    c = gu.data.make_linear_coeffs(B, 2 * L - 1, 19, seed=6020)
    assert np.all(c[:, 1:] != c[:, :-1])
    _check(_case(c, method, 20), adjoint)


@pytest.mark.parametrize("adjoint", [True, False])
@pytest.mark.parametrize("method", ["rk4", "euler"])
def test_only_time_ever_moves(method, adjoint, gpu_lib):
    """Data constant in time: narrow on every step (a word that is never set)."""
    c = gu.data.make_linear_coeffs(B, 2 * L - 1, 19, seed=6021).copy()
    c[:, :, 1:] = c[:, :1, 1:]
    assert len(_time_only_pieces(c)) == c.shape[1] - 1
    _check(_case(c, method, 20), adjoint)


@pytest.mark.parametrize("adjoint", [True, False])
@pytest.mark.parametrize("channel", [19, 4, 3])
def test_one_sample_moves_one_channel_on_a_time_only_piece(channel, adjoint, gpu_lib):
    """One sample of the middle tile gets a delta in one data channel on a time-only piece: channel 19 / channel 4 send that tile wide
    on that step while its neighbours stay narrow; channel 3 belongs to quad 0, the tile stays narrow and must still be right."""
    p = _piece()
    c = _rect().copy()
    c[MID, p + 1:, channel] += 0.25
    d = c[:, p + 1] - c[:, p]
    assert d[MID, channel] != 0 and not np.any(np.delete(d, MID, axis=0)[:, 1:]) and np.count_nonzero(d[MID, 1:]) == 1
    for method in ("rk4", "euler"):
        _check(_case(c, method, 20), adjoint)


@pytest.mark.parametrize("adjoint", [True, False])
def test_negative_zero_deltas_count_as_zero(adjoint, gpu_lib):
    """dX = (-0.0) - (+0.0) = -0.0 in every channel >= 4 of a time-only piece."""
    p = _piece()
    c = _rect().copy()
    c[:, p, 4:] = 0.0
    c[:, p + 1, 4:] = -0.0
    d = c[:, p + 1, 4:] - c[:, p, 4:]
    assert not np.any(d) and np.signbit(d).all()
    _check(_case(c, "rk4", 20), adjoint)


@pytest.mark.parametrize("adjoint", [True, False])
@pytest.mark.parametrize("C", [8, 12])
def test_few_channel_sets(C, adjoint, gpu_lib):
    """The CQ = 2 / 3 instantiations (C = 8 / 12)."""
    for method in ("rk4", "euler"):
        _check(_case(_rect(C), method, C), adjoint, C)


@pytest.mark.parametrize("adjoint", [True, False])
def test_range_faulted_tile_is_reexecuted_on_the_same_branches(adjoint, gpu_lib):
    """One sample of the middle tile leaves the fp16 range: the split-bf16 instantiations that re-execute that tile (only_faulted)
    take the same narrow / wide branches."""
    case = _case(_rect(), "rk4", 20)
    case["z0"] = case["z0"].copy()
    case["z0"][MID + 1] *= 4.0e5
    _check(case, adjoint)


def test_rectilinear_adjoint_twenty_times(gpu_lib):
    """The reproducibility contract of the chain + gradient-wave adjoint with narrow stages in it: twenty
    launches on one forward solution, bit-identical gradients every time."""
    import gpu_util
    case = _case(_rect(), "rk4", 20)
    z = gpu_util.run_case(case, need_grads=False)["z_out"]
    first = gpu_util.run_adjoint_direct(case, z)
    assert np.isfinite(first["dz0"]).all()
    for i in range(19):
        again = gpu_util.run_adjoint_direct(case, z)
        assert _same(first["dz0"], again["dz0"]), i
        for name in first["grads"]:
            assert _same(first["grads"][name], again["grads"][name]), (i, name)
