"""The causal control-path builders on the GPU (csrc/ncde_prepare.hip: ncde_fill, ncde_hybrid_count / _max / _write) against the
goldens g18_* of the imported reference and the host restatement tests/hybrid_ref.py (pinned to the goldens by test_hybrid_cpu.py).

Rules of comparison:
  * shapes and kept counts equal the golden exactly: the keep decisions compare copied values;
  * the time channel, the rectilinear channels and every linear series without a NaN are copies: bit-identical with the golden;
  * linear series with NaNs go through the existing NaN fill: whole-tensor relerr <= 1e-6 against the fp32 restatement, the rule
    tests/test_prepare_gpu.py applies to that kernel;
  * a second call gives the same bits, and everything is finite.
Outputs come from ``torch.empty``: every call goes into an allocator state poisoned with NaN and is compared in full shape.
"""
import functools

import numpy as np
import pytest
import torch

import golden_util as gu
import hybrid_ref as hr
import strided_views as sv

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _poison(n_out):
    junk = [torch.full((max(n, 1),), NAN, device="cuda") for n in (n_out, n_out // 2 + 1, 3 * n_out, 64, 1024)]
    del junk


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same_bits(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def _case(name):
    return hr.load(name)


@functools.lru_cache(maxsize=None)
def _restated_hybrid(name):
    g = _case(name)
    return hr.hybrid(g["x"], g["rect"].tolist())


def _hybrid(x_dev, rect, n_out):
    import ncde_amd
    _poison(n_out)
    out, lengths = ncde_amd.linear_rectilinear_hybrid_coeffs(x_dev, [int(r) for r in rect], return_lengths=True)
    torch.cuda.synchronize()
    return out, lengths


def _copied_mask(x, rect, out_shape):
    """[B, 1, C] -> broadcast over the rows: True where the table holds copies of input values."""
    B, _, C = x.shape
    m = np.zeros((B, 1, C), bool)
    m[:, :, [0] + list(rect)] = True
    m[:, 0, :] |= ~np.isnan(x).any(axis=1)
    return np.broadcast_to(m, out_shape)


def _check_hybrid(got, lengths, name):
    g = _case(name)
    want, (mine, _) = g["out"], _restated_hybrid(name)
    assert tuple(got.shape) == want.shape and got.dtype == torch.float32
    assert lengths.dtype == torch.int32 and lengths.cpu().numpy().tolist() == g["lengths"].tolist()
    got = got.cpu().numpy()
    assert np.isfinite(got).all(), (name, "unwritten or non-finite elements", int((~np.isfinite(got)).sum()))
    copied = _copied_mask(g["x"], g["rect"].tolist(), want.shape)
    bad = np.argwhere(copied & (_bits(got) != _bits(want)))
    assert bad.size == 0, (name, "a copied value differs from the golden", len(bad), bad[:4].tolist())
    err = gu.relerr(got, mine)
    print("%-28s T %4d lengths %s relerr vs restatement %.2e, bit-identical %s" % (name, want.shape[1], g["lengths"].tolist(), err, _same_bits(got, want)))
    assert err <= 1e-6, (name, err)
    if not g["meta"]["nan_linear"]:
        assert _same_bits(got, want), name


@pytest.mark.parametrize("name", hr.cases("hybrid"))
def test_hybrid_goldens(name, gpu_lib):
    g = _case(name)
    x = torch.from_numpy(g["x"]).cuda()
    keep = x.clone()
    got, lengths = _hybrid(x, g["rect"], g["out"].size)
    _check_hybrid(got, lengths, name)
    again, lengths2 = _hybrid(x, g["rect"], g["out"].size)
    assert _same_bits(again, got) and torch.equal(lengths, lengths2), (name, "two calls, different bits")
    assert _same_bits(x, keep), (name, "the input was modified")
    import ncde_amd
    assert _same_bits(ncde_amd.linear_rectilinear_hybrid_coeffs(x, g["rect"].tolist()), got)          # return_lengths=False: the table alone


def test_hybrid_with_an_empty_list_is_the_linear_builder(gpu_lib):
    import ncde_amd
    g = _case("g18_hybrid_no_rect")
    x = torch.from_numpy(g["x"]).cuda()
    got, lengths = _hybrid(x, [], g["out"].size)
    assert _same_bits(got, ncde_amd.linear_interpolation_coeffs(x, initial_value_if_nan=0.0))
    assert lengths.tolist() == [g["x"].shape[1]] * g["x"].shape[0]


def test_hybrid_flattens_batch_dimensions(gpu_lib):
    g = _case("g18_hybrid_dense_linear")                                                  # B = 4 -> [2, 2, L, C]
    B, L, C = g["x"].shape
    x = torch.from_numpy(g["x"]).cuda().reshape(2, 2, L, C)
    got, lengths = _hybrid(x, g["rect"], g["out"].size)
    assert got.shape == (2, 2) + g["out"].shape[1:] and lengths.shape == (2, 2)
    assert _same_bits(got.reshape(B, -1, C), g["out"]) and lengths.reshape(-1).tolist() == g["lengths"].tolist()


def _carve(x_np, layout, device="cuda"):
    """strided_views.carve for an input that holds NaNs itself (carve checks its view with a comparison that NaN fails): the same
    geometry, for the layouts whose samples do not share storage."""
    sb, st, off, n = sv.geometry(x_np.shape, layout)
    base = torch.full((n,), NAN, dtype=torch.float32, device=device)
    view = base.as_strided(x_np.shape, (sb, st, 1), off)
    view.copy_(torch.from_numpy(x_np))
    assert view.stride() == (sb, st, 1) and np.array_equal(view.cpu().numpy(), x_np, equal_nan=True)
    return view, base


@pytest.mark.parametrize("layout", ["row_padded", "batch_slice", "time_major", "time_prefix"])
def test_hybrid_on_a_strided_view(layout, gpu_lib):
    """x carved out of a buffer that is NaN wherever the view does not point (the layouts of tests/strided_views.py)."""
    name = "g18_hybrid_b3_l9_c6"
    g = _case(name)
    view, base = _carve(g["x"], layout)
    assert layout == "contiguous" or not view.is_contiguous()
    keep = base.clone()
    got, lengths = _hybrid(view, g["rect"], g["out"].size)
    _check_hybrid(got, lengths, name)
    assert _same_bits(base, keep), "the buffer behind the view was written"
    import ncde_amd
    m = hr.load("g18_fill_plain_init0_ff1")
    view, base = _carve(m["x"], layout)
    assert _same_bits(ncde_amd.linear_interpolation_coeffs(view, initial_value_if_nan=0.0, forward_fill=True), m["out"])


def _fill_call(g, x):
    import ncde_amd
    m = g["meta"]
    _poison(g["out"].size)
    out = ncde_amd.linear_interpolation_coeffs(x, rectilinear=m["rectilinear"], initial_value_if_nan=m["initial_value_if_nan"], forward_fill=m["forward_fill"])
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", hr.cases("fill"))
def test_fill_option_goldens(name, gpu_lib):
    g = _case(name)
    m = g["meta"]
    x = torch.from_numpy(g["x"]).cuda()
    keep = x.clone()
    got = _fill_call(g, x)
    want = g["out"]
    mine = hr.linear_coeffs(g["x"], m["rectilinear"], m["initial_value_if_nan"], m["forward_fill"])
    assert tuple(got.shape) == want.shape and torch.isfinite(got).all()
    assert _same_bits(_fill_call(g, x), got), (name, "two calls, different bits")
    assert _same_bits(x, keep), (name, "the input was modified")
    g_np = got.cpu().numpy()
    # copies: every series without a NaN, and everything once a forward fill or the rectilinear preparation has run (no interior gap is
    # left to interpolate: leading gaps take the first observation, series without one are zero)
    copied = np.broadcast_to(~np.isnan(g["x"]).any(axis=1, keepdims=True), (g["x"].shape[0], want.shape[1], want.shape[2]))
    if m["forward_fill"] or m["rectilinear"] is not None:
        copied = np.ones(want.shape, bool)
    assert not (copied & (_bits(g_np) != _bits(want))).any(), (name, "a copied value differs from the golden")
    err = gu.relerr(g_np, mine)
    print("%-34s relerr vs restatement %.2e, bit-identical %s" % (name, err, _same_bits(g_np, want)))
    assert err <= 1e-6, (name, err)


@pytest.mark.parametrize("rectilinear", [None, 0])
def test_fill_defaults_are_the_existing_call(rectilinear, gpu_lib):
    """Both new arguments at their defaults: the same kernel on the same input, bit for bit -- against the plain call and against the
    C entry point the plain call has always made."""
    import ncde_amd
    g = _case("g18_fill_plain_initnone_ff0")
    x = torch.from_numpy(g["x"]).cuda()
    B, L, C = x.shape
    T = L if rectilinear is None else 2 * L - 1
    plain = ncde_amd.linear_interpolation_coeffs(x, rectilinear=rectilinear)
    explicit = ncde_amd.linear_interpolation_coeffs(x, rectilinear=rectilinear, initial_value_if_nan=None, forward_fill=False)
    direct = torch.full((B, T, C), NAN, device="cuda")
    assert gpu_lib.ncde_prepare_linear(x.data_ptr(), B, L, C, -1 if rectilinear is None else rectilinear, direct.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert _same_bits(plain, explicit) and _same_bits(plain, direct)


def test_forward_fill_golden(gpu_lib):
    import ncde_amd
    g = _case("g18_forward_fill")
    x = torch.from_numpy(g["x"]).cuda()
    keep = x.clone()
    _poison(g["out"].size)
    got = ncde_amd.forward_fill(x)
    torch.cuda.synchronize()
    assert got.shape == x.shape and np.array_equal(got.cpu().numpy(), g["out"], equal_nan=True)
    assert np.array_equal(np.isnan(got.cpu().numpy()), np.isnan(g["out"])) and np.isnan(g["out"]).any()
    assert _same_bits(ncde_amd.forward_fill(x), got) and _same_bits(x, keep)
    B, L, C = x.shape
    assert _same_bits(ncde_amd.forward_fill(x.reshape(B, 1, L, C)).reshape(B, L, C), got)
    assert _same_bits(ncde_amd.forward_fill(x[0]), got[0])


@pytest.mark.parametrize("B,L,C", [(2, 700, 3), (2, 5, 300), (3, 300, 64), (1, 1, 4)])
def test_forward_fill_across_time_chunks_and_wide_rows(B, L, C, gpu_lib):
    """The kernel splits time into 256 / C chunks and carries the last value from chunk to chunk (C <= 256), or loops over the channels
    (C > 256): long gaps that span several chunks, gaps at chunk borders, series without observation."""
    import ncde_amd
    rng = np.random.default_rng(B * 1000 + L + C)
    x = rng.standard_normal((B, L, C)).astype(np.float32)
    x[rng.random(x.shape) < 0.9] = NAN
    x[:, :, 0] = NAN
    if L > 1:
        x[:, 1, 0] = 1.0                                                                  # one observation, carried to the end
    xd = torch.from_numpy(x).cuda()
    _poison(x.size)
    got = ncde_amd.forward_fill(xd).cpu().numpy()
    want = hr.forward_fill(x)
    assert np.array_equal(got, want, equal_nan=True)
    got = ncde_amd.linear_interpolation_coeffs(xd, initial_value_if_nan=0.5, forward_fill=True).cpu().numpy() if L > 1 else None
    assert L == 1 or np.array_equal(got, hr.linear_coeffs(x, None, 0.5, True))


def test_filled_knots_are_causal(gpu_lib):
    """forward_fill=True, initial_value_if_nan=0.0: whatever comes after index k leaves the knots 0 .. k bitwise unchanged.  Every k at L = 9."""
    import ncde_amd
    g = _case("g18_fill_plain_init0_ff1")
    x = g["x"]
    B, L, C = x.shape
    rng = np.random.default_rng(7)
    for rectilinear in (None, 0):
        base = ncde_amd.linear_interpolation_coeffs(torch.from_numpy(x).cuda(), rectilinear=rectilinear, initial_value_if_nan=0.0, forward_fill=True)
        for k in range(L):
            y = x.copy()
            tail = rng.standard_normal((B, L - k - 1, C)).astype(np.float32) * 10
            tail[rng.random(tail.shape) < 0.3] = NAN
            tail[..., 0] = y[:, k + 1:, 0] + 0.25                                         # the time channel stays observed
            y[:, k + 1:] = tail
            out = ncde_amd.linear_interpolation_coeffs(torch.from_numpy(y).cuda(), rectilinear=rectilinear, initial_value_if_nan=0.0, forward_fill=True)
            n = k + 1 if rectilinear is None else 2 * k + 1                               # rows 2k+1 .. hold t_{k+1}
            assert _same_bits(out[:, :n], base[:, :n]), (rectilinear, k)
            assert k == L - 1 or not _same_bits(out, base)


def test_hybrid_rows_are_causal(gpu_lib):
    """No NaN in the linear channels: the rows a sample keeps from raw indices 0 .. k -- (k + 1) + the number of rectilinear changes up to
    k of them -- do not depend on what comes after k."""
    g = _case("g18_hybrid_dense_linear")
    x, rect = g["x"], g["rect"].tolist()
    B, L, C = x.shape
    rv = hr.forward_fill(hr._set_initial(x[..., rect], 0.0))                              # the rectilinear channels as the table holds them
    changes = np.concatenate([np.zeros((B, 1), int), np.cumsum((rv[:, 1:] != rv[:, :-1]).any(axis=-1), axis=1)], axis=1)      # [B, L]: up to k
    base, base_len = _hybrid(torch.from_numpy(x).cuda(), rect, g["out"].size)
    rng = np.random.default_rng(11)
    for k in range(L):
        y = x.copy()
        tail = rng.integers(0, 4, (B, L - k - 1, C)).astype(np.float32) + 0.125
        tail[..., rect] = np.where(rng.random((B, L - k - 1, len(rect))) < 0.4, NAN, tail[..., rect])
        tail[..., 0] = y[:, k + 1:, 0] + 0.25
        y[:, k + 1:] = tail
        out, _ = _hybrid(torch.from_numpy(y).cuda(), rect, g["out"].size)
        for b in range(B):
            n = (k + 1) + int(changes[b, k])
            assert n <= base_len[b].item() and n <= out.shape[1]
            assert _same_bits(out[b, :n], base[b, :n]), (k, b, n)
    assert (changes[:, -1] + L == g["lengths"]).all()                                    # k = L - 1: the whole sample


def test_hybrid_coefficients_drive_the_model_like_the_references(gpu_lib):
    """End to end on a case whose table only copies values (bit-equal with the reference's): NeuralCDE on the coefficients built on the
    GPU and on the uploaded golden coefficients gives the same bits."""
    import ncde_amd
    g = _case("g18_hybrid_dense_linear")
    assert not g["meta"]["nan_linear"]
    x = torch.from_numpy(g["x"]).cuda()
    built = ncde_amd.linear_rectilinear_hybrid_coeffs(x, g["rect"].tolist())
    golden = torch.from_numpy(g["out"]).cuda()
    assert _same_bits(built, golden)
    torch.manual_seed(5)
    model = ncde_amd.NeuralCDE(x.shape[-1], 8, 3, hidden_hidden_dim=8, num_layers=2, interpolation="linear", return_sequences=True).cuda()
    with torch.no_grad():
        y_built, y_golden = model(built), model(golden)
    torch.cuda.synchronize()
    assert y_built.shape[:2] == (x.shape[0], g["out"].shape[1]) and torch.isfinite(y_built).all()
    assert torch.equal(y_built, y_golden)
