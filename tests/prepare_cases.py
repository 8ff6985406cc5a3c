"""The case table of the coefficient-builder tests (csrc/ncde_prepare.hip), its inputs, its fp32 mirrors and its error metric.

One table, two readers: tests/test_prepare_gpu.py runs every case on the GPU, tests/test_prepare_cpu.py walks the same table
without one (expected launch paths through ``ncde_prepare_kernel_name``, mirrors against the float64 reference).

A case: (id, builder, B, L, C, user grid?, rectilinear time channel / None, gap pattern, expected launch path[, eps, order]).
The shapes sit on the gates of the dispatch (``prepare_plan`` in ncde_prepare.hip):
  linear   LDS variant iff  4 * (L*C*(3, rectilinear: 2) + 64*C) <= 64 KB and C <= 256; inside it nch = min(64, 256 / C) time
           chunks of cl = ceil(L / nch) steps per channel; 16-byte staging iff L*C % 4 == 0 (and the sample offset too)
  cubic    LDS variant iff C <= 64, default grid and one sample fits 150 KB; nsmp = 64 / C samples per workgroup, fewer while
           they exceed 28 KB (nsmp = 1 may); forward / backward chains in blocks of 8 steps
  smooth   one kernel, grid-stride above 4096 x 256 elements
"""
import numpy as np

import coeff_oracle as data
import coeff_ref64 as ref64

LDS, V1 = "ncde_linear_coeffs_lds", "ncde_linear_coeffs"
CUB, SMOOTH = "ncde_cubic_coeffs", "ncde_smooth_coeffs"


def _cl(n):
    return "ncde_cubic_coeffs_lds<nsmp=%d>" % n


def _both_grids(rows):
    return [(name + ("_tgrid" if g else ""), bld, B, L, C, g, r, gaps, path) for (name, bld, B, L, C, _, r, gaps, path) in rows for g in (False, True)]


CASES = _both_grids([
    # ---- linear NaN fill ---------------------------------------------------------------------------------------------------------
    ("lin_lds_cl9", "linear", 5, 300, 7, None, None, "edges", LDS),          # nch = 36, cl = 9: serial scans, carries over empty chunks
    ("lin_lds_nch1", "linear", 3, 5, 200, None, None, "edges", LDS),         # C in 129..234: one chunk per channel
    ("lin_lds_scalar_a", "linear", 4, 33, 5, None, None, "edges", LDS),      # L*C % 4 != 0: scalar staging
    ("lin_lds_scalar_b", "linear", 3, 7, 3, None, None, "edges", LDS),       # odd sample offsets
    ("lin_v1_long", "linear", 3, 700, 9, None, None, "edges", V1),           # beyond the LDS gate; B*C % 256 tail
    ("lin_v1_wide", "linear", 2, 6, 300, None, None, "edges", V1),           # C > 256
]) + [
    # ---- rectilinear ---------------------------------------------------------------------------------------------------------------
    ("rect_quad_t0", "rect", 9, 150, 20, False, 0, "edges", LDS),            # C % 4 == 0: 16-byte stores
    ("rect_quad_t5", "rect", 9, 150, 20, False, 5, "edges", LDS),            # time channel inside a quad
    ("rect_quad_t19", "rect", 9, 150, 20, False, 19, "edges", LDS),          # time channel last
    ("rect_scalar_t7", "rect", 9, 150, 19, False, 7, "edges", LDS),          # scalar stores
    ("rect_scalar_t18", "rect", 9, 150, 19, False, 18, "edges", LDS),
    ("rect_v1_t4", "rect", 2, 1000, 9, False, 4, "edges", V1),
    # ---- cubic, LDS variant, complete series: L - 1 around the blocks of 8, every C class, B < nsmp and ragged last workgroups -----
    ("cub_lds_L2_C1", "cubic", 1, 2, 1, False, None, "none", _cl(64)),
    ("cub_lds_L3_C3", "cubic", 7, 3, 3, False, None, "none", _cl(21)),
    ("cub_lds_L4_C4", "cubic", 50, 4, 4, False, None, "none", _cl(16)),
    ("cub_lds_L5_C5", "cubic", 7, 5, 5, False, None, "none", _cl(12)),
    ("cub_lds_L9_C8", "cubic", 50, 9, 8, False, None, "none", _cl(8)),
    ("cub_lds_L10_C33", "cubic", 7, 10, 33, False, None, "none", _cl(1)),
    ("cub_lds_L11_C64", "cubic", 1, 11, 64, False, None, "none", _cl(1)),
    ("cub_lds_L17_C3", "cubic", 50, 17, 3, False, None, "none", _cl(21)),
    ("cub_lds_L18_C5", "cubic", 7, 18, 5, False, None, "none", _cl(12)),
    ("cub_lds_L10_C64", "cubic", 50, 10, 64, False, None, "none", _cl(1)),
    ("cub_lds_L182_C4", "cubic", 7, 182, 4, False, None, "none", _cl(4)),
    ("cub_lds_L182_C1", "cubic", 50, 182, 1, False, None, "none", _cl(17)),
    ("cub_lds_over_budget", "cubic", 4, 500, 8, False, None, "none", _cl(1)),      # one sample above the 28 KB budget
    # ---- cubic, LDS variant, workgroups with and without a NaN in one launch; all workgroups on the per-series routine -----------
    ("cub_lds_mixed", "cubic", 50, 40, 4, False, None, "samples_3_41", _cl(16)),
    ("cub_lds_gaps", "cubic", 7, 18, 5, False, None, "edges", _cl(12)),
    ("cub_lds_gaps_L2", "cubic", 6, 2, 3, False, None, "edges", _cl(21)),
    ("cub_lds_gaps_L3", "cubic", 6, 3, 3, False, None, "edges", _cl(21)),
    # ---- cubic, global-memory kernel on the default grid: uniform sweep on the swept-diagonal table ------------------------------
    ("cub_glob_wide", "cubic", 3, 30, 80, False, None, "none", CUB),
    ("cub_glob_wide_gaps", "cubic", 3, 30, 80, False, None, "edges", CUB),
    ("cub_glob_long", "cubic", 2, 2500, 8, False, None, "none", CUB),
    ("cub_glob_long_gaps", "cubic", 2, 2500, 8, False, None, "edges", CUB),
    ("cub_glob_L3", "cubic", 2, 3, 80, False, None, "none", CUB),
    ("cub_glob_L4", "cubic", 2, 4, 80, False, None, "none", CUB),
    ("cub_glob_L5", "cubic", 2, 5, 80, False, None, "none", CUB),
    # ---- cubic on a user grid ------------------------------------------------------------------------------------------------------
    ("cub_tgrid", "cubic", 37, 50, 5, True, None, "none", CUB),
    ("cub_tgrid_gaps", "cubic", 37, 50, 5, True, None, "edges", CUB),               # B*C % 64 != 0
    ("cub_tgrid_gaps_L2", "cubic", 6, 2, 3, True, None, "edges", CUB),
    ("cub_tgrid_gaps_L3", "cubic", 6, 3, 3, True, None, "edges", CUB),
    # ---- smoothed-linear: B*P*C above one 4096 x 256 grid; the shortest paths ----------------------------------------------------
    ("smooth3_eps05_big", "smooth", 128, 300, 32, False, None, "none", SMOOTH, 0.5, 3),
    ("smooth3_eps1_big", "smooth", 128, 300, 32, False, None, "none", SMOOTH, 1.0, 3),
    ("smooth5_eps05_big", "smooth", 128, 300, 32, False, None, "none", SMOOTH, 0.5, 5),
    ("smooth5_eps1_big", "smooth", 128, 300, 32, False, None, "none", SMOOTH, 1.0, 5),
    ("smooth3_T2", "smooth", 5, 2, 3, False, None, "none", SMOOTH, 0.3, 3),
    ("smooth5_T2", "smooth", 5, 2, 3, False, None, "none", SMOOTH, 0.3, 5),
    ("smooth3_T3", "smooth", 5, 3, 3, False, None, "none", SMOOTH, 0.3, 3),
    ("smooth5_T3", "smooth", 5, 3, 3, False, None, "none", SMOOTH, 0.3, 5),
]
IDS = [c[0] for c in CASES]
SMOOTH_GRID_ELEMS = 4096 * 256

# the hand-made gap patterns, one series each (the remaining series keep their random gaps)
PATTERNS = ("leading", "trailing", "all_nan", "one_first", "one_middle", "one_last", "ends_only", "long_gap")


def _apply(col, pattern):
    L = col.shape[0]
    keep = np.zeros(L, dtype=bool)
    if pattern == "leading":
        keep[max(1, L // 3):] = True
    elif pattern == "trailing":
        keep[:L - max(1, L // 3)] = True
    elif pattern == "one_first":
        keep[0] = True
    elif pattern == "one_middle":
        keep[L // 2] = True
    elif pattern == "one_last":
        keep[L - 1] = True
    elif pattern == "ends_only":
        keep[0] = keep[L - 1] = True
    elif pattern == "long_gap":          # an interior gap of half the series: longer than two time chunks of the LDS linear kernel
        keep[:] = True
        keep[max(1, L // 4):max(1, L // 4) + L // 2] = False
        keep[L - 1] = True
    # a value for every kept entry (the random gaps may have taken it), NaN elsewhere
    col[:] = np.where(keep, np.where(np.isnan(col), np.float32(0.25), col), np.float32(np.nan))


def pattern_series(case):
    """{pattern: (sample, channel)} of the hand-made series of an 'edges' case."""
    _, _, B, L, C, _, rect = case[:7]
    series = [(b, c) for b in range(B) for c in range(C) if c != rect]
    assert len(series) >= len(PATTERNS), "too few series for the gap patterns"
    stride = len(series) // len(PATTERNS)
    return {p: series[j * stride] for j, p in enumerate(PATTERNS)}


def make_input(case):
    """-> (x[B, L, C] fp32, t[L] fp32 or None).  Seeds are fixed per case (its position in the table)."""
    name, builder, B, L, C, grid, rect, gaps = case[:8]
    seed = 1500 + IDS.index(name)
    if builder == "smooth":
        x = (data.normal(seed, B * L * C, stream=3).reshape(B, L, C) * 0.5).astype(np.float32)
        return x, None
    missing = 0.4 if gaps == "edges" else 0.0
    if C >= 2:
        x = data.synthetic_series(B, L, C - 1, missing=missing, seed=seed)      # channel 0: time i / L, never missing
    else:
        x = (np.cumsum(data.normal(seed, B * L, stream=5).reshape(B, L, 1), axis=1) / np.sqrt(L)).astype(np.float32)
    if rect:
        x[..., [0, rect]] = x[..., [rect, 0]]
    if gaps == "edges":
        for pattern, (b, c) in pattern_series(case).items():
            _apply(x[b, :, c], pattern)
    elif gaps == "samples_3_41":
        x[3, 5:9, 1] = np.nan
        x[3, 0, 2] = np.nan
        x[41, 1:-1, 3] = np.nan
        x[41, -4:, 0] = np.nan
    else:
        assert gaps == "none" and not np.isnan(x).any()
    t = np.cumsum(0.3 + 1.4 * data.uniform01(seed, L, stream=3)).astype(np.float32) if grid else None
    return x, t


def sections(case):
    builder = case[1]
    return {"linear": 1, "rect": 1, "cubic": 4}[builder] if builder != "smooth" else case[10] + 1


def smooth_mirror(x, eps, order):
    """fp32 rows of the smoothed path from the class's torch restatement of the reference's formulas, on CPU tensors."""
    import torch
    from ncde_amd.interpolation import _matching_coefficients
    B, T, C = x.shape
    W, P = order + 1, ref64.smooth_pieces(T, eps)
    out = np.zeros((B, P, W, C), dtype=np.float32)
    out[:, 0, 0], out[:, 0, 1] = x[:, 0], x[:, 1] - x[:, 0]
    if T > 2:
        mc = _matching_coefficients(torch.from_numpy(x), eps, order).numpy()        # [B, T-2, C, order+1], highest power first
        m = np.stack([mc[..., order - q] * np.float32(max(q, 1)) for q in range(W)], axis=2)
        if eps < 1:
            out[:, 1::2] = m
            out[:, 2::2, 0] = (torch.from_numpy(x[:, 1:-1]) + eps * torch.from_numpy(x[:, 2:] - x[:, 1:-1])).numpy()
            out[:, 2::2, 1] = x[:, 2:] - x[:, 1:-1]
        else:
            out[:, 1:] = m
    return out.reshape(B, P, W * C)


def mirror(case, x, t):
    """The fp32 host mirror (oracle/coeff_oracle.py, pinned to the reference) of the case."""
    builder, rect = case[1], case[6]
    if builder == "linear":
        return data.linear_interpolation_coeffs(x, t=t)
    if builder == "rect":
        return data.linear_interpolation_coeffs(x, rectilinear=rect)
    if builder == "cubic":
        return data.natural_cubic_coeffs(x, t=t)
    return smooth_mirror(x, case[9], case[10])


def reference64(case, x, t):
    builder, rect = case[1], case[6]
    if builder == "linear":
        return ref64.linear(x, t=t)
    if builder == "rect":
        return ref64.linear(x, rectilinear=rect)
    if builder == "cubic":
        return ref64.natural_cubic(x, t=t)
    return ref64.smooth(x, case[9], case[10])


def kernel_name(lib, case):
    """What ``ncde_prepare_kernel_name`` answers for the case (smooth: its single kernel)."""
    _, builder, B, L, C, grid, rect = case[:7]
    if builder == "smooth":
        return SMOOTH
    kind = 1 if builder == "cubic" else 0
    got = lib.ncde_prepare_kernel_name(kind, B, L, C, int(bool(grid)), -1 if rect is None else rect)
    return None if got is None else got.decode()


def section_errors(got, want64, n_sections, floor=2.0 ** -24):
    """Per series and section: E[N, S, C] = max_t |got - want| / max(max_t |want|, tiny), and the sizes max_t |want|.

    got / want64: [N, T, S*C].  ``tiny`` keeps a section that is (nearly) zero in exact arithmetic -- a straight series' 2c / 3d --
    measurable: ``floor`` x the size of the series' own values (section a), never below 1e-30.  The default floor is fp32
    resolution; the float64 pins of coeff_ref64 use 1 (a section that small is the residue of a cancellation in BOTH float64
    algorithms, so it is measured against the values that cancelled)."""
    N, T, SC = want64.shape
    C = SC // n_sections
    g = np.asarray(got, dtype=np.float64).reshape(N, T, n_sections, C)
    w = want64.reshape(N, T, n_sections, C)
    diff = np.abs(g - w).max(axis=1)
    size = np.abs(w).max(axis=1)
    tiny = np.maximum(floor * size[:, :1, :], 1e-30)
    return diff / np.maximum(size, tiny), size


def case_errors(got, want64, n_sections, floor=2.0 ** -24):
    """E per section, the worst series of the case: [S]."""
    return section_errors(got, want64, n_sections, floor)[0].max(axis=(0, 2))
