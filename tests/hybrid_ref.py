"""Host restatement (numpy, fp32) of the causal control-path builders, written from their stated semantics and not from the
reference's code: the fill options of ``linear_interpolation_coeffs``, ``forward_fill`` and the linear / rectilinear hybrid scheme.
tests/test_hybrid_cpu.py pins it to the goldens g18_* (outputs of the imported reference, tools/gen_golden_hybrid.py) with
``torch.equal``; the GPU tests compare the kernels with it.  No function here writes its argument.

    forward_fill(x)                                         [..., L, C] -> same shape, leading NaNs stay
    linear_coeffs(x, rectilinear, initial_value_if_nan, forward_fill)
    hybrid(x, rectilinear_indices) -> (out [B, T, C], lengths [B] int32)
    load(name) / cases(kind)                                the goldens and their manifest
"""
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = "MANIFEST_hybrid.json"


def forward_fill(x):
    """Every NaN takes the last observation before it along axis -2; NaNs before the first observation of a channel stay."""
    x = np.asarray(x, np.float32)
    L = x.shape[-2]
    idx = np.where(np.isnan(x), -1, np.arange(L).reshape(L, 1))
    idx = np.maximum.accumulate(idx, axis=-2)                       # index of the last observation at or before i (-1: none)
    out = np.take_along_axis(x, np.maximum(idx, 0), axis=-2)
    return np.where(idx < 0, np.float32("nan"), out).astype(np.float32)


def _set_initial(x, value):
    x = np.array(x, np.float32, copy=True)
    first = x[..., 0, :]
    first[np.isnan(first)] = np.float32(value)
    return x


def _nan_fill(x):
    """The linear NaN handling on the integer grid: interior gaps interpolated as prev + ratio * (next - prev) with
    ratio = (i - i_prev) / (i_next - i_prev), every operation in fp32; leading / trailing gaps take the first / last observation;
    a series without observation is zero."""
    x = np.asarray(x, np.float32)
    L = x.shape[-2]
    ar = np.arange(L).reshape(L, 1)
    nan = np.isnan(x)
    prv = np.maximum.accumulate(np.where(nan, -1, ar), axis=-2)
    nxt = np.flip(np.minimum.accumulate(np.flip(np.where(nan, L, ar), axis=-2), axis=-2), axis=-2)
    pv = np.take_along_axis(x, np.maximum(prv, 0), axis=-2)
    qv = np.take_along_axis(x, np.minimum(nxt, L - 1), axis=-2)
    i32 = np.broadcast_to(ar, x.shape).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = (i32 - prv.astype(np.float32)) / (nxt.astype(np.float32) - prv.astype(np.float32))
        mid = pv + ratio * (qv - pv)
    out = np.where(~nan, x, np.where((prv < 0) & (nxt >= L), np.float32(0.0), np.where(prv < 0, qv, np.where(nxt >= L, pv, mid))))
    return out.astype(np.float32)


def _rectilinear(x, time_index):
    """Forward fill, every row twice, the time channel advanced by one slot: 2L-1 rows."""
    f = np.repeat(forward_fill(x), 2, axis=-2)
    f[..., :-1, time_index] = f[..., 1:, time_index].copy()
    return f[..., :-1, :]


def linear_coeffs(x, rectilinear=None, initial_value_if_nan=None, forward_fill_=False):
    x = np.asarray(x, np.float32)
    if initial_value_if_nan is not None:
        x = _set_initial(x, initial_value_if_nan)
    if rectilinear is not None:
        x = _rectilinear(x, rectilinear)
    if forward_fill_:
        x = forward_fill(x)
    return _nan_fill(x)


def hybrid(x, rectilinear_indices):
    """-> (out [B, T, C], lengths [B]); time is channel 0."""
    x = np.asarray(x, np.float32)
    B, L, C = x.shape
    rect = list(rectilinear_indices)
    lin = [c for c in range(C) if c != 0 and c not in rect]
    lin_v = linear_coeffs(x[..., lin], initial_value_if_nan=0.0) if lin else None
    rect_v = forward_fill(_set_initial(x[..., rect], 0.0)) if rect else None
    full = np.empty((B, 2 * L - 1, C), np.float32)
    full[:, 0::2, 0] = x[:, :, 0]
    full[:, 1::2, 0] = x[:, 1:, 0]
    if lin:
        full[:, 0::2, lin] = lin_v
        full[:, 1::2, lin] = lin_v[:, 1:]
    if rect:
        full[:, 0::2, rect] = rect_v
        full[:, 1::2, rect] = rect_v[:, :-1]
    key = full[:, :, [0] + rect]
    keep = np.concatenate([np.ones((B, 1), bool), (key[:, 1:] != key[:, :-1]).any(axis=-1)], axis=1)
    lengths = keep.sum(axis=1).astype(np.int32)
    T = int(lengths.max())
    out = np.empty((B, T, C), np.float32)
    for b in range(B):
        rows = full[b, keep[b]]
        out[b, :len(rows)] = rows
        out[b, len(rows):] = rows[-1]
    return out, lengths


def load(name):
    f = np.load(os.path.join(GOLD, name + ".npz"))
    d = {k: f[k] for k in f.files if k != "meta"}
    d["meta"] = json.loads(str(f["meta"]))
    return d


def cases(kind):
    """Names of the goldens of one kind: "hybrid", "fill" or "forward_fill"."""
    with open(os.path.join(GOLD, MANIFEST)) as fh:
        return [m["name"] for m in json.load(fh) if m["kind"] == kind]


def lengths_of(out, rectilinear_indices):
    """Kept rows per sample, read off a padded hybrid table: a kept row differs from the kept row before it in time or in a
    rectilinear channel (the rows dropped in between equal their predecessors there), and the padding repeats the last row."""
    key = np.asarray(out)[:, :, [0] + list(rectilinear_indices)]
    return (1 + (key[:, 1:] != key[:, :-1]).any(axis=-1).sum(axis=1)).astype(np.int32)
