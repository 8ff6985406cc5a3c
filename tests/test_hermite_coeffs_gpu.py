"""``hermite_cubic_coefficients_with_backward_differences`` on the GPU (ncde_hermite_coeffs, csrc/ncde_prepare.hip) against the float64
restatement of tests/hermite_ref.py.

The rule of tests/test_prepare_gpu.py: per series and section  E = max_t |got - ref64| / max(max_t |ref64|, 2^-24 max_t |a|), and
per section the worst series of the GPU result is within 4 x the worst series of the fp32 mirror -- the same formulas, in the same
order, in fp32 torch ops on the CPU, on knots filled in fp32 on the host (hybrid_ref's fills, coeff_oracle's NaN interpolation).
A (series, section) that the reference and the mirror make exactly zero is exactly zero; ``a`` is the linear builder's output bit
for bit; a second call gives the same bits.  The output goes into ``torch.empty`` behind a NaN-poisoned allocator state and is checked
finite in full, so an element no thread wrote cannot pass."""
import numpy as np
import pytest
import torch

import coeff_oracle
import hermite_ref as hr
import hybrid_ref
import prepare_cases as pc

pytestmark = pytest.mark.gpu
NAN = np.float32("nan")


def _x(seed, shape, gaps):
    """Random walks [..., L, C]; gaps: none | interior (30 % NaN, first and last row observed) | edges (leading and trailing gaps, a
    series without observation, one with a single observation, NaNs in the first row)."""
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.standard_normal(shape), axis=-2).astype(np.float32)
    L = shape[-2]
    if gaps == "interior" and L > 2:
        x[..., 1:-1, :][rng.random(x[..., 1:-1, :].shape) < 0.3] = NAN
    if gaps == "edges":
        flat = x.reshape(-1, L, shape[-1])
        flat[rng.random(flat.shape) < 0.2] = NAN
        flat[0, :max(1, L // 3), 0] = NAN            # a leading gap
        flat[0, -max(1, L // 3):, -1] = NAN          # a trailing gap
        flat[-1, :, 0] = NAN                         # never observed
        if flat.shape[0] > 1:
            flat[1, :, -1] = NAN
            flat[1, L // 2, -1] = 1.5                # a single observation
    return x


def _t(seed, L):
    return np.cumsum(np.random.default_rng(seed).uniform(0.3, 1.7, L)).astype(np.float32)


def _mirror(x, t, init, ffill):
    """The definition in fp32 torch ops on the CPU."""
    f = np.asarray(x, np.float32)
    if init is not None:
        f = hybrid_ref._set_initial(f, init)
    if ffill:
        f = hybrid_ref.forward_fill(f)
    k = torch.from_numpy(coeff_oracle.linear_interpolation_coeffs(f, t=t))
    L = k.size(-2)
    h = torch.ones(L - 1, 1) if t is None else (torch.from_numpy(t)[1:] - torch.from_numpy(t)[:-1]).unsqueeze(-1)
    diff = k[..., 1:, :] - k[..., :-1, :]
    d = diff / h
    dprev = torch.cat([d[..., :1, :], d[..., :-1, :]], dim=-2)
    a, b = k[..., :-1, :], dprev
    two_c = 2 * (3 * (diff / h - b) - d + dprev) / h
    three_d = (1 / h ** 2) * (d - b) - two_c / h
    out = torch.cat([a, b, two_c, three_d], dim=-1)
    assert out.dtype == torch.float32
    return out.numpy()


def _run(xd, td, init, ffill, n_out):
    import ncde_amd
    poison = [torch.full((n,), float("nan"), device="cuda") for n in (n_out, n_out // 2 + 1, 3 * n_out)]
    del poison
    out = ncde_amd.hermite_cubic_coefficients_with_backward_differences(xd, t=td, initial_value_if_nan=init, forward_fill=ffill)
    torch.cuda.synchronize()
    return out


# name -> (shape, gaps, user grid, initial_value_if_nan, forward_fill)
CASES = {
    "two_knots":        ((3, 2, 1), "none", False, None, False),
    "odd":              ((4, 5, 7), "none", False, None, False),
    "odd_interior":     ((4, 5, 7), "interior", False, None, False),
    "odd_edges":        ((4, 5, 7), "edges", False, None, False),
    "odd_edges_grid":   ((4, 5, 7), "edges", True, None, False),
    "odd_causal":       ((4, 5, 7), "edges", False, -0.5, True),
    "odd_causal_grid":  ((4, 5, 7), "edges", True, 0.25, True),
    "initial_only":     ((4, 5, 7), "edges", False, 2.0, False),
    "ffill_only":       ((4, 5, 7), "edges", False, None, True),
    "long":             ((2, 300, 3), "interior", False, None, False),      # several workgroups
    "long_grid_causal": ((2, 300, 3), "edges", True, 0.0, True),
    "leading_shape":    ((2, 3, 6, 4), "interior", True, None, False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_builder_against_the_float64_reference(gpu_lib, name):
    import ncde_amd
    shape, gaps, grid, init, ffill = CASES[name]
    L, C = shape[-2:]
    assert gpu_lib.ncde_prepare_hermite_kernel_name(int(np.prod(shape[:-2])), L, C) == b"ncde_hermite_coeffs"
    x = _x(sum(shape) + len(name), shape, gaps)
    t = _t(L, L) if grid else None
    want, mir = hr.coeffs(x, t, init, ffill), _mirror(x, t, init, ffill)
    xd, td = torch.from_numpy(x).cuda(), None if t is None else torch.from_numpy(t).cuda()
    keep = xd.clone()
    out = _run(xd, td, init, ffill, want.size)
    got = out.cpu().numpy()
    assert got.shape == want.shape == shape[:-2] + (L - 1, 4 * C) and got.dtype == np.float32
    assert np.isfinite(got).all(), (name, "unwritten or non-finite elements", int((~np.isfinite(got)).sum()))
    assert torch.equal(_run(xd, td, init, ffill, want.size), out), (name, "two calls, different bits")
    assert torch.equal(xd.nan_to_num(nan=-7.0), keep.nan_to_num(nan=-7.0)) and torch.equal(torch.isnan(xd), torch.isnan(keep))      # x is not written
    # a is the linear builder's output, bit for bit
    knots = ncde_amd.linear_interpolation_coeffs(xd, t=td, initial_value_if_nan=init, forward_fill=ffill)
    assert torch.equal(out[..., :C], knots[..., :-1, :])
    # per section against the float64 reference
    B = int(np.prod(shape[:-2]))
    g3, w3, m3 = got.reshape(B, L - 1, 4 * C), want.reshape(B, L - 1, 4 * C), mir.reshape(B, L - 1, 4 * C)
    (eg, size), (em, _) = pc.section_errors(g3, w3, 4), pc.section_errors(m3, w3, 4)
    E_gpu, E_mirror = eg.max(axis=(0, 2)), em.max(axis=(0, 2))
    print("%-18s E_mirror %s E_gpu %s bit-identical to the mirror: %s" % (name, " ".join("%.2e" % e for e in E_mirror),
                                                                          " ".join("%.2e" % e for e in E_gpu), np.array_equal(got, mir)))
    assert (E_gpu <= 4 * E_mirror).all(), (name, "E_gpu", E_gpu.tolist(), "E_mirror", E_mirror.tolist())
    zero = (size == 0) & (np.abs(m3.reshape(B, L - 1, 4, C)).max(axis=1) == 0)          # [B, 4, C]
    g4 = np.abs(g3.reshape(B, L - 1, 4, C)).max(axis=1)
    assert not g4[zero].any(), (name, "a section the reference makes exactly zero is not", np.argwhere(zero & (g4 != 0))[:4].tolist())
    assert not g3[:, 0, 2 * C:].any()      # the first piece is exactly linear
    if gaps == "edges" and init is None and not ffill:
        assert zero[-1, :, 0].all()        # the series without observation: every section zero
    if L > 2 and gaps != "edges":
        assert np.abs(g3[:, 1:, 2 * C:]).max() > 0.1


def test_non_contiguous_view(gpu_lib):
    import ncde_amd
    x = torch.from_numpy(_x(11, (4, 9, 10), "interior")).cuda()
    view = x[:, ::2, 1:8:2]
    assert not view.is_contiguous() and tuple(view.shape) == (4, 5, 4)
    t = torch.from_numpy(_t(5, 5)).cuda()
    for kw in (dict(), dict(t=t), dict(initial_value_if_nan=0.5, forward_fill=True)):
        a = ncde_amd.hermite_cubic_coefficients_with_backward_differences(view, **kw)
        b = ncde_amd.hermite_cubic_coefficients_with_backward_differences(view.contiguous(), **kw)
        assert torch.equal(a, b) and torch.isfinite(a).all() and tuple(a.shape) == (4, 4, 16)


@pytest.mark.parametrize("grid", [False, True], ids=["integer", "user"])
def test_causality_bit_for_bit(gpu_lib, grid):
    """Both causal options on: pieces 0..k-1 keep their bits when x[k+1:] changes."""
    import ncde_amd
    L = 9
    x = _x(21, (3, L, 4), "edges")
    td = torch.from_numpy(_t(3, L)).cuda() if grid else None
    base = ncde_amd.hermite_cubic_coefficients_with_backward_differences(torch.from_numpy(x).cuda(), t=td, initial_value_if_nan=0.25, forward_fill=True)
    for k in range(1, L - 1):
        y = x.copy()
        y[:, k + 1:] = _x(200 + k, (3, L - 1 - k, 4), "none") + 3.0
        other = ncde_amd.hermite_cubic_coefficients_with_backward_differences(torch.from_numpy(y).cuda(), t=td, initial_value_if_nan=0.25, forward_fill=True)
        assert torch.equal(other[:, :k], base[:, :k]), k
        assert not torch.equal(other[:, k:], base[:, k:])


def test_argument_errors(gpu_lib):
    import ncde_amd
    f = ncde_amd.hermite_cubic_coefficients_with_backward_differences
    x = torch.zeros(2, 5, 3, device="cuda")
    with pytest.raises(NotImplementedError, match="fp32 CUDA"):
        f(x.double())
    with pytest.raises(ValueError, match="at least 2"):
        f(x[:, :1])
    with pytest.raises(ValueError, match="monotonically"):
        f(x, t=torch.tensor([0.0, 1.0, 1.0, 2.0, 3.0]))
    with pytest.raises(ValueError, match="length of t"):
        f(x, t=torch.tensor([0.0, 1.0, 2.0]))
    with pytest.raises(TypeError, match="initial_value_if_nan"):
        f(x, initial_value_if_nan="0")
    assert gpu_lib.ncde_prepare_hermite_kernel_name(1, 1, 3) is None
    assert gpu_lib.ncde_prepare_hermite(None, None, 2, 5, 3, None, None) == -1


def test_the_model_takes_the_cubic_routes(gpu_lib):
    """NeuralCDE(interpolation="cubic_hermite") on the builder's output is the cubic model on the same tensor: the kernel the batch
    solve picks and its result are those of interpolation="cubic", bit for bit."""
    import ncde_amd
    torch.manual_seed(9)
    x = torch.from_numpy(_x(31, (6, 7, 4), "interior")).cuda()
    coeffs = ncde_amd.hermite_cubic_coefficients_with_backward_differences(x, initial_value_if_nan=0.0, forward_fill=True)
    outs = {}
    for name in ("cubic_hermite", "cubic"):
        torch.manual_seed(9)
        model = ncde_amd.NeuralCDE(4, 16, 2, hidden_hidden_dim=16, num_layers=2, interpolation=name, return_sequences=True).cuda()
        with torch.no_grad():
            outs[name] = model(coeffs)
    assert torch.equal(outs["cubic_hermite"], outs["cubic"]) and torch.isfinite(outs["cubic"]).all() and tuple(outs["cubic"].shape) == (6, 7, 2)
