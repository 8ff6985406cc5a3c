"""The causal control-path builders without a GPU: the host restatement (tests/hybrid_ref.py) against the goldens g18_* of the
imported reference, the argument checks of the Python entries, and the C entry points' refusal of bad arguments (they return before
anything is launched, in the style of tests/test_host_cpu.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import hybrid_ref as hr
import ncde_amd
from ncde_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
INVALID, WORKSPACE = -1, -3
NEW_ENTRIES = ("ncde_prepare_fill", "ncde_prepare_hybrid_workspace_bytes", "ncde_prepare_hybrid_count", "ncde_prepare_hybrid_write")


def _equal_with_nan(a, b):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


def test_the_manifest_lists_every_case_the_issue_names():
    names = set(hr.cases("hybrid"))
    for tag in ("known_answer", "b3_l9_c6", "l2", "no_rect", "every_row", "ragged", "c2", "l33", "l65", "l130", "l257", "l1025"):
        assert "g18_hybrid_" + tag in names
    fills = [hr.load(n)["meta"] for n in hr.cases("fill")]
    for rect in (None, 0):
        for initial in (None, 0.0):
            for ff in (False, True):
                assert any(m["rectilinear"] == rect and m["initial_value_if_nan"] == initial and m["forward_fill"] == ff for m in fills)
    g = hr.load("g18_hybrid_b3_l9_c6")
    assert g["x"].shape == (3, 9, 6) and len(set(g["lengths"].tolist())) == 3          # the padding is exercised
    g = hr.load("g18_hybrid_every_row")
    assert g["out"].shape[1] == 2 * g["x"].shape[1] - 1 and (g["lengths"] == g["out"].shape[1]).all()
    g = hr.load("g18_hybrid_ragged")
    assert g["lengths"].min() < g["lengths"].max() and (g["x"][2, 3:, 0] == g["x"][2, 2, 0]).all()
    x = hr.load(hr.cases("fill")[0])["x"]                                                # leading, interior, trailing gaps, one empty channel
    assert np.isnan(x[:, 0, 1]).all() and np.isnan(x[:, 3, 2]).all() and np.isnan(x[:, -1, 3]).all() and np.isnan(x[:, :, 4]).all()
    assert not np.isnan(x[:, 0, 2]).all() and not np.isnan(x[..., 0]).any()


@pytest.mark.parametrize("name", hr.cases("hybrid"))
def test_restatement_reproduces_the_hybrid_goldens(name):
    g = hr.load(name)
    x0 = g["x"].copy()
    out, lengths = hr.hybrid(g["x"], g["rect"].tolist())
    assert out.shape == g["out"].shape and out.dtype == np.float32
    assert torch.equal(torch.from_numpy(out), torch.from_numpy(g["out"]))
    assert torch.equal(torch.from_numpy(lengths), torch.from_numpy(g["lengths"])) and lengths.dtype == np.int32
    assert lengths.max() == out.shape[1] and np.array_equal(hr.lengths_of(g["out"], g["rect"].tolist()), lengths)
    assert np.isfinite(out).all()
    assert _equal_with_nan(g["x"], x0)                                                   # the input is unmodified


def test_known_answer_of_the_reference_written_out():
    """src/tests/test_interpolation.py: changes register at times 1 and 4 only."""
    x = torch.tensor([[0.0, 1.0, 2.0, 3.0, 4.0], [3.0, 1.4, NAN, 3.4, NAN], [NAN, 1.5, NAN, NAN, NAN], [NAN, NAN, NAN, NAN, 1.2], [NAN] * 5]).T.unsqueeze(0)
    want = torch.tensor([[[0.0, 3.0, 0.0, 0.0, 0.0], [1.0, 1.4, 0.0, 0.0, 0.0], [1.0, 1.4, 1.5, 0.0, 0.0], [2.0, 2.4, 1.5, 0.0, 0.0],
                          [3.0, 3.4, 1.5, 0.0, 0.0], [4.0, 3.4, 1.5, 0.0, 0.0], [4.0, 3.4, 1.5, 1.2, 0.0]]])
    g = hr.load("g18_hybrid_known_answer")
    assert _equal_with_nan(g["x"], x) and g["rect"].tolist() == [2, 3, 4]
    assert torch.equal(torch.from_numpy(g["out"]), want)
    out, lengths = hr.hybrid(x.numpy(), [2, 3, 4])
    assert torch.equal(torch.from_numpy(out), want) and lengths.tolist() == [7]


@pytest.mark.parametrize("name", hr.cases("fill"))
def test_restatement_reproduces_the_fill_goldens(name):
    g = hr.load(name)
    m, x0 = g["meta"], g["x"].copy()
    out = hr.linear_coeffs(g["x"], m["rectilinear"], m["initial_value_if_nan"], m["forward_fill"])
    assert out.shape == g["out"].shape and torch.equal(torch.from_numpy(out), torch.from_numpy(g["out"]))
    assert np.isfinite(out).all() and _equal_with_nan(g["x"], x0)


def test_restatement_reproduces_forward_fill():
    g = hr.load("g18_forward_fill")
    assert np.isnan(g["out"]).any()                                                      # leading gaps stay
    assert _equal_with_nan(hr.forward_fill(g["x"]), g["out"])


def test_empty_rectilinear_list_is_the_linear_builder_with_initial_value_zero():
    g = hr.load("g18_hybrid_no_rect")
    assert g["rect"].size == 0
    assert torch.equal(torch.from_numpy(g["out"]), torch.from_numpy(hr.linear_coeffs(g["x"], initial_value_if_nan=0.0)))


def test_python_entries_check_their_arguments_before_anything_runs():
    x = torch.zeros(2, 5, 4)
    x[0, 0, 2] = NAN
    x0 = x.clone()
    hy = ncde_amd.linear_rectilinear_hybrid_coeffs
    with pytest.raises(NotImplementedError, match="lags channel 0"):
        hy(x, [2], time_index=1)
    for bad in ((2, 3), 2, None, torch.tensor([2])):
        with pytest.raises(TypeError):
            hy(x, bad)
    with pytest.raises(TypeError):
        hy(x, [2.0])
    with pytest.raises(TypeError):
        hy(x, [True])
    with pytest.raises(TypeError):
        hy(x, [2], time_index="0")
    for bad in ([4], [-1], [0], [0, 2], [2, 2], [1, 2, 3, 1]):
        with pytest.raises(ValueError):
            hy(x, bad)
    with pytest.raises(ValueError):
        hy(torch.zeros(5), [])
    with pytest.raises(NotImplementedError, match="no CPU fallback"):                     # well-formed: only the device is missing
        hy(x, [2, 3])
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        hy(x, [])
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        ncde_amd.forward_fill(x)
    with pytest.raises(NotImplementedError):
        ncde_amd.forward_fill(x.double())
    lin = ncde_amd.linear_interpolation_coeffs
    for bad in ("0", [0.0], torch.tensor(0.0), True):
        with pytest.raises(TypeError):
            lin(x, initial_value_if_nan=bad)
    for bad in (1, "yes", None):
        with pytest.raises(TypeError):
            lin(x, forward_fill=bad)
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        lin(x, initial_value_if_nan=0.0, forward_fill=True)
    assert _equal_with_nan(x, x0)


def test_docstrings_state_the_deliberate_differences():
    assert "never modifies" in ncde_amd.linear_interpolation_coeffs.__doc__
    doc = ncde_amd.linear_rectilinear_hybrid_coeffs.__doc__
    assert "never modified" in doc and "only synchronisation" in doc


def test_new_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ncde_hip.h")).read()
    lib = ncde_amd.lib()
    for name in NEW_ENTRIES:
        assert name in _lib.EXPORTS and re.search(r"\b%s\(" % name, hdr) and hasattr(lib, name)
    assert lib.ncde_version() == _lib.NCDE_ABI_VERSION == 4                               # new entry points only: the ABI version stays


def test_c_entries_refuse_bad_arguments_without_launching():
    lib = ncde_amd.lib()
    X, O, W, N, M, R = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000                     # dummy device pointers, never dereferenced
    fill = lib.ncde_prepare_fill
    assert fill(None, 2, 5, 3, 1, 0.0, 1, O, None) == INVALID
    assert fill(X, 2, 5, 3, 1, 0.0, 1, None, None) == INVALID
    assert fill(X, 2, 5, 3, 1, 0.0, 1, X, None) == INVALID                                # in place
    for B, L, C in ((0, 5, 3), (2, 0, 3), (2, 5, 0), (2, 1 << 29, 4)):
        assert fill(X, B, L, C, 1, 0.0, 1, O, None) == INVALID
    wsb = lib.ncde_prepare_hybrid_workspace_bytes
    assert wsb(2, 1, 3) == INVALID and wsb(2, 5, 1) == INVALID and wsb(0, 5, 3) == INVALID and wsb(2, 1 << 29, 4) == INVALID
    need = wsb(3, 9, 6)
    assert need >= 4 * (3 * 17 + 3 + 6)
    count, write = lib.ncde_prepare_hybrid_count, lib.ncde_prepare_hybrid_write
    assert count(None, 3, 9, 6, R, 2, W, need, N, M, None) == INVALID
    assert count(X, 3, 9, 6, None, 2, W, need, N, M, None) == INVALID                     # indices announced, none passed
    assert count(X, 3, 9, 6, R, 6, W, need, N, M, None) == INVALID                        # more rectilinear channels than C - 1
    assert count(X, 3, 9, 6, R, -1, W, need, N, M, None) == INVALID
    assert count(X, 3, 9, 6, R, 2, None, need, N, M, None) == INVALID
    assert count(X, 3, 9, 6, R, 2, W, need, None, M, None) == INVALID
    assert count(X, 3, 9, 6, R, 2, W, need, N, None, None) == INVALID
    assert count(X, 3, 1, 6, R, 2, W, need, N, M, None) == INVALID
    assert count(X, 3, 9, 6, R, 2, W, need - 1, N, M, None) == WORKSPACE
    assert write(None, X, 3, 9, 6, 2, W, need, N, 11, O, None) == INVALID
    assert write(X, None, 3, 9, 6, 2, W, need, N, 11, O, None) == INVALID                 # three linear channels, no table
    assert write(X, X, 3, 9, 6, 2, W, need, N, 0, O, None) == INVALID
    assert write(X, X, 3, 9, 6, 2, W, need, N, 18, O, None) == INVALID                    # T > 2L - 1
    assert write(X, X, 3, 9, 6, 2, W, need, N, 11, None, None) == INVALID
    assert write(X, X, 3, 9, 6, 2, W, need, None, 11, O, None) == INVALID
    assert write(X, X, 3, 9, 6, 2, None, need, N, 11, O, None) == INVALID
    assert write(X, X, 3, 9, 6, 2, W, need - 1, N, 11, O, None) == WORKSPACE
    assert isinstance(need, int) and ctypes.sizeof(ctypes.c_int) == 4
