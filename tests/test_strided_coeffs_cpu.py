"""The layout helper of the strided-coefficient tests (tests/strided_views.py) on the CPU, and the C-ABI's stride contract on the C++
restatement (oracle/ncde_cpu.cpp behind the same NcdeProblem): a view of every layout holds exactly the values it was made from, the
buffer around it is NaN, and forward, continuous adjoint and exact discrete backward read through the view give the bits of the
contiguous call.  This pins the fixture: when tests/test_strided_coeffs_gpu.py fails, the kernel is wrong and not the view.
(`far` is left to the GPU file: an 8 GiB host buffer is not a unit-test fixture.)"""
import numpy as np
import pytest
import torch

import golden_util as gu
import strided_views as sv

B, C, H, HH, NL = 5, 3, 7, 15, 2
LAYOUTS = [l for l in sv.layouts() if l != "far"]
CASES = [("linear", "rk4", False), ("cubic", "midpoint", True), ("linear", "euler", True)]


def _inputs(interp, layout):
    """Raw length 3 (5 rectilinear knots) / a 4-knot cubic; the values the layout can hold; z0 differs per sample in every layout."""
    if interp == "cubic":
        coeffs = gu.data.make_cubic_coeffs(B, 4, C - 1, seed=71)
    else:
        coeffs = gu.data.make_rectilinear_coeffs(B, 3, C - 1, missing=0.3, seed=71)
        assert coeffs.shape[1] == 5
    z0 = (gu.data.normal(73, B * H, stream=2).reshape(B, H) * 0.5).astype(np.float32)
    p = dict(gu.data.make_field_weights(H, HH, C, seed=72))
    return sv.logical(coeffs, layout), z0, p


@pytest.mark.parametrize("interp", ["linear", "cubic"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_view_holds_the_values_and_the_rest_of_the_buffer_is_nan(layout, interp):
    coeffs, _, _ = _inputs(interp, layout)
    view, base = sv.carve(coeffs, layout, "cpu")
    Bv, R, K = coeffs.shape
    assert tuple(view.shape) == coeffs.shape and view.stride(2) == 1
    assert np.array_equal(view.contiguous().numpy(), coeffs) and np.isfinite(coeffs).all()
    assert np.array_equal(sv.make_view(coeffs, layout, "cpu").numpy(), coeffs)
    inside = sv.inside_mask(view, base)
    assert torch.isnan(base[~inside]).all() and torch.isfinite(base[inside]).all()
    sb, st = view.stride(0), view.stride(1)
    want = {"contiguous": sb == R * K and st == K and view.is_contiguous(),
            "time_prefix": sb == (R + 3) * K and st == K,
            "row_padded": st == K + 3 and st % 2 == (K + 3) % 2 and sb == R * st + 5,
            "batch_slice": sb == 2 * R * K and st == K and view.storage_offset() % 2 == (1 + 3 * R * K) % 2,
            "time_major": sb == K and st == Bv * K,
            "broadcast": sb == 0 and st == K,
            "overlap": sb == K and st == K}[layout]
    assert want, (layout, view.stride(), view.storage_offset())
    if layout != "contiguous":
        assert int((~inside).sum()) >= 2 * sv.PAD and not view.is_contiguous()
    if layout == "time_prefix":      # the row behind every sample's prefix exists and is NaN
        assert all(torch.isnan(base[view.storage_offset() + b * sb + R * st:][:K]).all() for b in range(Bv))
    if layout == "batch_slice":      # what the name says: every second sample of a larger batch, from the fourth on
        big = base[sv.PAD + 1:][:(2 * Bv + 3) * R * K].view(2 * Bv + 3, R, K)
        assert big[3::2].data_ptr() == view.data_ptr() and big[3::2].stride() == view.stride()
        assert (view.data_ptr() - base.data_ptr()) // 4 % 2 == (sv.PAD + 1 + 3 * R * K) % 2


def test_layouts_that_share_storage_refuse_values_they_cannot_hold():
    coeffs = gu.data.make_rectilinear_coeffs(B, 3, C - 1, missing=0.3, seed=71)
    for layout in ("broadcast", "overlap"):
        with pytest.raises(ValueError):
            sv.make_view(coeffs, layout, "cpu")
        held = sv.logical(coeffs, layout)
        assert held.shape == coeffs.shape and np.array_equal(held[0], coeffs[0]) and not np.array_equal(held, coeffs)
    assert np.array_equal(sv.logical(coeffs, "overlap")[2, 1], sv.logical(coeffs, "overlap")[1, 2])


def test_far_geometry_puts_the_last_sample_beyond_two_to_the_31_elements():
    for Bf, R, K in ((17, 5, 20), (37, 3, 32), (2, 5, 4)):
        sb, st, off, n = sv.geometry((Bf, R, K), "far")
        assert sb % 2 == 1 and st == K and (Bf - 1) * sb >= 2 ** 31 and (Bf - 1) * (sb - 2) < 2 ** 31
        assert n * 4 <= (sv.FAR_BUFFER_GIB + 1) * 2 ** 30 and n >= off + (Bf - 1) * sb + R * K


@pytest.mark.parametrize("interp,method,seq", CASES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_cpu_restatement_reads_through_the_strides(layout, interp, method, seq):
    """libncde_cpu.so on the view against itself on the contiguous copy: forward, continuous adjoint and exact discrete backward, bit
    for bit and finite (one read outside the view would make them NaN).  On one thread: the restatement adds its per-thread gradient
    partials in the order the threads arrive, which no two runs share."""
    import cpu_lib_util as cu
    threads = cu.cpu_lib().ncde_cpu_set_threads(1)
    try:
        _compare_on_the_cpu_library(cu, layout, interp, method, seq)
    finally:
        cu.cpu_lib().ncde_cpu_set_threads(threads)


def _compare_on_the_cpu_library(cu, layout, interp, method, seq):
    coeffs, z0, p = _inputs(interp, layout)
    layers = [("W0", "b0")] + [("W1", "b1")] * (NL - 1)
    view = sv.make_view(coeffs, layout, "cpu").numpy()
    assert view.strides[2] == 4 and np.array_equal(view, coeffs)
    ref = cu.CpuCase(coeffs, interp, z0, p, layers, method, seq)
    got = cu.CpuCase(coeffs, interp, z0, p, layers, method, seq).point_at(view)
    if layout != "contiguous":
        assert (got.p.coeffs, got.p.coeffs_stride_b, got.p.coeffs_stride_t) != (ref.p.coeffs, ref.p.coeffs_stride_b, ref.p.coeffs_stride_t)
        assert (got.p.coeffs_stride_b, got.p.coeffs_stride_t) == (view.strides[0] // 4, view.strides[1] // 4)
    z, rec = ref.forward(record=True)
    zv, recv = got.forward(record=True)
    assert np.isfinite(zv).all() and np.array_equal(zv, z) and np.array_equal(recv, rec)
    assert np.array_equal(got.forward(), ref.forward())
    gout = (gu.data.normal(75, z.size, stream=1).reshape(z.shape) / np.sqrt(z.shape[1])).astype(np.float32)
    for src, srcv, disc in ((z, zv, False), (rec, recv, True)):
        dz0, g = ref.backward(src, gout, discrete=disc)
        dz0v, gv = got.backward(srcv, gout, discrete=disc)
        assert np.isfinite(dz0v).all() and np.array_equal(dz0v, dz0), disc
        for k in g:
            assert np.isfinite(gv[k]).all() and np.array_equal(gv[k], g[k]), (disc, k)
        assert np.any(dz0) and np.any(g["Wo"])
