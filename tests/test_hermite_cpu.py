"""The Hermite cubic with backward differences on the CPU: the properties that define the float64 restatement of tests/hermite_ref.py
(the vendored torchcde does not hold the scheme, so no golden exists), the new names of the public surface, and the torch-op step of
``NeuralCDE(interpolation="cubic_hermite").online`` against the same model's fp64 batch solve on hermite_ref coefficients.

Bounds: the step against the batch solve <= 2e-5 of max |ref| in fp32 (stream_util.TIGHT_Z, the project's forward bound) and <= 1e-10
in fp64 (tests/test_online_cpu.py); the end of a piece against the next knot, and its end slope against its own difference, <= 256 ulp
of fp64 at the size of the series (max |knot| + max |difference|): a dozen rounded operations on terms of up to ~10 x that size."""
import warnings

import numpy as np
import pytest
import torch

import golden_util as gu
import hermite_ref as hr
import hermite_util as hu
import stream_edges as se
import stream_util as su

NAN = float("nan")


def _series(seed, shape, missing=0.3):
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.standard_normal(shape), axis=-2).astype(np.float32)
    x[rng.random(shape) < missing] = NAN
    return x


GRIDS = {"integer": None, "user": np.cumsum(np.random.default_rng(7).uniform(0.3, 1.7, 9))}


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("causal", [False, True], ids=["fill_both_ways", "causal"])
def test_pieces_meet_the_knots_with_the_backward_differences(grid, causal):
    t = GRIDS[grid]
    x = _series(1, (4, 9, 3))
    kw = dict(initial_value_if_nan=-0.5, forward_fill=True) if causal else {}
    k, c = hr.knots(x, t, **kw), hr.coeffs(x, t, **kw)
    h, d, dprev = hr.differences(k, t)
    assert c.shape == (4, 8, 12) and c.dtype == np.float64 and np.isfinite(c).all()
    assert np.array_equal(c[..., :3], k[:, :-1]) and np.array_equal(c[..., 3:6], dprev)
    tol = 256 * 2.0 ** -52 * (np.abs(k).max() + np.abs(d).max())
    for i in range(8):
        hi = float(h[i, 0])
        assert np.abs(hr.evaluate(c, i, hi) - k[:, i + 1]).max() <= tol, i                          # the piece ends at the next knot
        assert np.array_equal(hr.derivative(c, i, 0.0), dprev[:, i])                                # starts with the slope before it
        assert np.abs(hr.derivative(c, i, hi) - d[:, i]).max() <= tol, i                            # ends with its own
    assert not c[:, 0, 6:].any()                                                                    # the first piece is exactly linear
    assert np.abs(c[:, 1:, 6:]).max() > 0.1


@pytest.mark.parametrize("grid", list(GRIDS))
def test_pieces_before_knot_k_do_not_see_later_rows(grid):
    """Causal options on: pieces 0..k-1 are bit-identical when x[k+1:] changes; without them they are not."""
    t = GRIDS[grid]
    x = _series(2, (3, 9, 4))
    x[:, 0, 1] = NAN
    x[1, 2:5, 2] = NAN
    base = hr.coeffs(x, t, 0.25, True)
    for k in range(1, 8):
        y = x.copy()
        y[:, k + 1:] = _series(100 + k, (3, 8 - k, 4), missing=0.5) + 3.0
        other = hr.coeffs(y, t, 0.25, True)
        assert np.array_equal(other[:, :k], base[:, :k]), k
        assert not np.array_equal(other[:, k:], base[:, k:])
    y = x.copy()
    y[:, 5:] += 1.0
    assert not np.array_equal(hr.coeffs(y, t)[:, :2], hr.coeffs(x, t)[:, :2])      # the two-sided fill looks ahead


def test_fill_and_knots_follow_the_linear_builder():
    x = np.array([[[NAN, 1.0], [2.0, NAN], [NAN, NAN], [5.0, 4.0], [NAN, NAN]]], dtype=np.float32)
    assert np.array_equal(hr.knots(x)[0], [[2, 1], [2, 2], [3.5, 3], [5, 4], [5, 4]])
    assert np.array_equal(hr.knots(x, None, 9.0, True)[0], [[9, 1], [2, 1], [2, 1], [5, 4], [5, 4]])
    assert np.array_equal(hr.knots(x, np.array([0.0, 1.0, 3.0, 4.0, 5.0]))[0, 2], [4.0, 3.25])
    assert np.isnan(x).any()      # the argument is not written


def test_public_names():
    import ncde_amd
    from ncde_amd import coefficients
    assert ncde_amd.CubicSpline is ncde_amd.NaturalCubicSpline
    assert ncde_amd.hermite_cubic_coefficients_with_backward_differences is coefficients.hermite_cubic_coefficients_with_backward_differences
    model = ncde_amd.NeuralCDE(4, 8, 2, interpolation="cubic_hermite")
    assert model.spline is ncde_amd.NaturalCubicSpline and model.interpolation == "cubic_hermite"
    X = ncde_amd.CubicSpline(torch.from_numpy(hr.coeffs(_series(3, (2, 5, 4), 0.0))))
    assert X.interp_name == "cubic" and X.n_knots == 5 and X.channels == 4
    for bad in (torch.zeros(2, 5, 3), torch.zeros(2, 5, 3, dtype=torch.float64)):      # no CPU route, as for the other builders
        with pytest.raises(NotImplementedError, match="fp32 CUDA"):
            ncde_amd.hermite_cubic_coefficients_with_backward_differences(bad)
    with pytest.raises(TypeError, match="forward_fill"):
        ncde_amd.hermite_cubic_coefficients_with_backward_differences(torch.zeros(2, 5, 3), forward_fill=1)


def test_online_accepts_the_hermite_path_and_still_refuses_the_others():
    import ncde_amd
    h = ncde_amd.NeuralCDE(3, 8, 2, interpolation="cubic_hermite").online(4, initial_value_if_nan=0.5)
    assert h.hermite and not h.rectilinear and sorted(h.state_dict()) == ["count", "last_row", "prev_dx", "z"]
    with pytest.raises(ValueError, match="causal control path: interpolation 'linear' or 'rectilinear', not 'cubic'"):
        ncde_amd.NeuralCDE(3, 8, 2, interpolation="cubic").online(4)
    with pytest.raises(ValueError, match="causal"):
        ncde_amd.NeuralCDE(3, 8, 2, interpolation="linear_cubic_smoothing", interpolation_eps=0.5).online(4)
    with pytest.raises(ValueError, match="fixed steps"):
        ncde_amd.NeuralCDE(3, 8, 2, interpolation="cubic_hermite", solver="dopri5").online(4)
    assert not ncde_amd.NeuralCDE(3, 8, 2, interpolation="linear").online(4).hermite


# rk4 on every field and input mode (the list of tests/test_online_cpu.py plus the fused kernel's own); the other solvers on the two
# input forms of the piece (dX/dt and X)
FIELDS = [("original", "matmul"), ("gru", "matmul"), ("minimal", "derivative"), ("original", "evaluate"), ("low-rank", "matmul")]
STEPS = [(f, m, "rk4") for f, m in FIELDS] + [("original", m, s) for s in ("midpoint", "euler") for m in ("matmul", "evaluate")]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("field,mode,method", STEPS)
def test_torch_step_matches_the_batch_solve_at_every_knot(field, mode, method, dtype):
    """Every field and input mode, NaNs in the first row and later: the step against the fp64 batch solve on hermite_ref
    coefficients at every knot; m rows in one call equal m single calls bit for bit."""
    import ncde_amd
    torch.manual_seed(5)
    B, L, C, init = 5, 6, 4, 0.5
    model = ncde_amd.NeuralCDE(C, 8, 2, hidden_hidden_dim=8, num_layers=2, interpolation="cubic_hermite", vector_field=field, solver=method,
                               vector_field_type=mode, sparsity=0.5 if field == "low-rank" else None, return_sequences=True)
    rows = se.make_rows(6201, L, B, C)
    rows[0, 1, 2] = NAN
    z_ref, o_ref = hu.batch_reference(model, rows, None, init)
    model = model.to(dtype)
    x = torch.from_numpy(rows).to(dtype)
    bound = su.TIGHT_Z if dtype == torch.float32 else 1e-10
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a, b = model.online(B, initial_value_if_nan=init), model.online(B, initial_value_if_nan=init)
        one = []
        for k in range(L):
            one.append(a.step(x[k]))
            e_out, e_z = gu.relerr(one[-1].numpy(), o_ref[k]), gu.relerr(a.z.numpy(), z_ref[k])
            print("%s %s %s %s knot %d: out %.3e z %.3e" % (field, mode, method, dtype, k, e_out, e_z))
            assert e_out <= bound and e_z <= bound, (k, e_out, e_z)
        many = b.step(x)
    assert torch.equal(torch.stack(one), many) and all(torch.equal(a.state_dict()[k], b.state_dict()[k]) for k in a.state_dict())
    assert float(a.last_row[1, 2]) != init and a.count.tolist() == [L] * B and np.abs(z_ref[-1] - z_ref[0]).max() > 1e-3


def test_the_curvature_matters_in_the_main_case():
    """The case of tests/test_online_hermite_gpu.py, on the torch-op route: the Hermite handle meets the fp64 reference, the same
    rows through a linear handle of the same weights miss it by more than 10 x the bound -- so a step that ignored 2c and 3d could
    not pass there.  (This is where the case's seeds were chosen.)"""
    z_ref, o_ref = hu.main_reference()
    x = torch.from_numpy(hu.main_rows().copy())
    s = hu.MAIN
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, zs, lasts = su.step_through(hu.main_model("cubic_hermite").online(s["B"], initial_value_if_nan=s["init"]), x, None)
        _, zl, _ = su.step_through(hu.main_model("linear").online(s["B"], initial_value_if_nan=s["init"]), x, None)
    e_h, e_l = gu.relerr(zs, z_ref), gu.relerr(zl, z_ref)
    print("main case: hermite step %.3e, linear step %.3e of max |ref|" % (e_h, e_l))
    assert e_h <= su.TIGHT_Z and e_l > 10 * su.TIGHT_Z, (e_h, e_l)
    assert np.abs(z_ref[-1] - z_ref[0]).max() > 1e-3
    assert lasts[0, 2, 3] == s["init"] and lasts[0, 17, 1] == s["init"]
