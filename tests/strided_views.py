"""Non-contiguous layouts of a control-path coefficient tensor [B, R, K] (K = C, 4C or 6C; R rows), for the tests that hand the
kernels `coeffs_stride_b` / `coeffs_stride_t` other than R K / K (include/ncde_hip.h: element strides, any batch stride >= 0, a
time stride of at least one row, a base pointer aligned to 4 bytes only).

Every view is carved with `as_strided` out of a larger buffer that is NaN wherever the view does not point, so an element read outside
the logical tensor poisons the result instead of silently matching.  A plain module (no fixtures): `layouts`, `logical`, `make_view`,
`carve`.

    contiguous    the control
    time_prefix   the first R rows of a buffer with R + 3 rows per sample (online prediction): stride_b != R stride_t, row R is NaN
    row_padded    stride_t = K + 3 (odd: rows not 16-byte aligned), stride_b = R stride_t + 5
    batch_slice   big[3::2] of a buffer that starts at an odd element: pointer 4-byte aligned only, stride_b = 2 R K
    time_major    [R, B, K] storage transposed: stride_b = K < stride_t = B K
    broadcast     one sample expanded over the batch: stride_b = 0
    overlap       stride_b = stride_t = K: sample b, row r is storage row b + r
    far           stride_t = K, stride_b = ceil(2^31 / (B - 1)) rounded up to odd: the last sample starts beyond 2^31 elements

`broadcast` and `overlap` constrain the VALUES (samples share storage): `logical(coeffs, layout)` returns the tensor such a view can
hold, made from the given one; a case for these layouts is built from that.
"""
import numpy as np
import torch

LAYOUTS = ("contiguous", "time_prefix", "row_padded", "batch_slice", "time_major", "broadcast", "overlap", "far")
PAD = 64            # NaN elements in front of and behind the storage of every layout but `contiguous`
FAR_HALO = 1024     # `far`: elements set to NaN on either side of each sample (the 8 GiB in between are never touched)
FAR_BUFFER_GIB = 8
FAR_MIN_FREE_GIB = 16


class FarLayoutNeedsMemory(RuntimeError):
    """The device has less than FAR_MIN_FREE_GIB free: the caller skips (the only skip these layouts know)."""


def layouts(interp=None):
    """Names of the layouts, `contiguous` first.  `interp` ("linear", "cubic", "quintic") is accepted for the call sites' sake: the row
    width K differs between the kinds, the set of layouts does not."""
    return list(LAYOUTS)


def logical(coeffs_np, layout):
    """The values a view of this layout holds when it is made from `coeffs_np`: the tensor itself, except where the layout shares
    storage between samples."""
    B, R, K = coeffs_np.shape
    if layout == "broadcast":
        return np.ascontiguousarray(np.broadcast_to(coeffs_np[:1], (B, R, K)))
    if layout == "overlap":
        rows = coeffs_np.reshape(B * R, K)[:B + R - 1]
        return np.ascontiguousarray(rows[np.arange(B)[:, None] + np.arange(R)[None, :]])
    return coeffs_np


def geometry(shape, layout):
    """-> (stride_b, stride_t, storage offset, buffer length), all in elements."""
    B, R, K = shape
    if layout == "contiguous":
        return R * K, K, 0, B * R * K
    if layout == "time_prefix":
        sb, st, off = (R + 3) * K, K, PAD
    elif layout == "row_padded":
        st = K + 3
        sb, off = R * st + 5, PAD
    elif layout == "batch_slice":      # big = buffer[PAD + 1:].view(2 B + 3, R, K); view = big[3::2]
        sb, st, off = 2 * R * K, K, PAD + 1 + 3 * R * K
    elif layout == "time_major":
        sb, st, off = K, B * K, PAD
    elif layout == "broadcast":
        sb, st, off = 0, K, PAD
    elif layout == "overlap":
        sb, st, off = K, K, PAD
    elif layout == "far":
        assert B >= 2, "the far layout needs two samples"
        sb = -(-2 ** 31 // (B - 1)) | 1
        st, off = K, PAD
        assert (B - 1) * sb >= 2 ** 31
    else:
        raise ValueError("unknown layout %r" % (layout,))
    last = off + (B - 1) * sb + (R - 1) * st + K
    if layout == "time_prefix":
        last = off + B * sb                       # the three rows behind the last sample's prefix belong to the buffer
    if layout == "batch_slice":
        last = PAD + 1 + (2 * B + 3) * R * K
    return sb, st, off, last + PAD


def carve(coeffs_np, layout, device):
    """-> (view [B, R, K] with the values of `coeffs_np`, the flat buffer it points into).  Raises ValueError if the layout cannot
    hold these values (`broadcast`, `overlap`: see `logical`)."""
    coeffs_np = np.ascontiguousarray(coeffs_np, np.float32)
    B, R, K = coeffs_np.shape
    sb, st, off, n = geometry(coeffs_np.shape, layout)
    device = torch.device(device)
    if layout == "far":
        if device.type == "cuda":
            free = torch.cuda.mem_get_info(device)[0]
            if free < FAR_MIN_FREE_GIB * 2 ** 30:
                raise FarLayoutNeedsMemory("the far layout allocates a %d GiB buffer and wants %d GiB free; torch.cuda.mem_get_info() "
                                           "reports %.1f GiB" % (FAR_BUFFER_GIB, FAR_MIN_FREE_GIB, free / 2 ** 30))
        base = torch.empty(n, dtype=torch.float32, device=device)
        assert n * 4 <= (FAR_BUFFER_GIB + 1) * 2 ** 30
        for b in range(B):
            lo = off + b * sb
            base[max(lo - FAR_HALO, 0):min(lo + R * K + FAR_HALO, n)] = float("nan")
    else:
        base = torch.full((n,), float("nan"), dtype=torch.float32, device=device)
    idx = off + sb * np.arange(B, dtype=np.int64)[:, None, None] + st * np.arange(R, dtype=np.int64)[None, :, None] + np.arange(K, dtype=np.int64)
    uniq, first = np.unique(idx.ravel(), return_index=True)      # (shared storage: one write per element)
    base[torch.from_numpy(uniq).to(device)] = torch.from_numpy(coeffs_np.ravel()[first]).to(device)
    view = base.as_strided((B, R, K), (sb, st, 1), off)
    assert view.stride() == (sb, st, 1) or 1 in (B, R, K)
    if not np.array_equal(view.cpu().numpy(), coeffs_np):
        raise ValueError("a %s view cannot hold these values: build the case from logical(coeffs, %r)" % (layout, layout))
    return view, base


def make_view(coeffs_np, layout, device):
    """A device tensor [B, R, K] of this layout whose logical values equal `coeffs_np`."""
    return carve(coeffs_np, layout, device)[0]


def inside_mask(view, base):
    """Boolean mask over `base` (host tensors): the elements `view` points at."""
    B, R, K = view.shape
    sb, st, sk = view.stride()
    idx = view.storage_offset() + sb * torch.arange(B)[:, None, None] + st * torch.arange(R)[None, :, None] + sk * torch.arange(K)
    m = torch.zeros(base.numel(), dtype=torch.bool)
    m[idx.reshape(-1)] = True
    return m
