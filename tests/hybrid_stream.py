"""Rows, conditions on them and the fp64 reference of the online HYBRID step (``NeuralCDE.online(..., rectilinear_indices=R)``,
DESIGN.md 5.14 "Hybrid step"), shared by tests/test_online_hybrid_cpu.py (the torch-op step) and tests/test_online_hybrid_gpu.py
(the fused kernels).  Helper only: no test functions, and nothing here imports or calls ``online.py``.

Reference, per stream and prefix x_0..x_k: fill the prefix causally (NaN -> ``initial_value_if_nan`` on the first row, the last
filled value afterwards, every channel), build ``hybrid_ref.hybrid`` on the filled prefix (the host restatement of
``linear_rectilinear_hybrid_coeffs`` that tests/test_hybrid_cpu.py pins to the reference's outputs), run the fp64 twin of the model
(``stream_ref._twin``, interpolation "linear") on those coefficients and read the row ``lengths - 1``, the stream's last kept knot.
The streams of a prefix are solved as one batch: a stream with fewer kept knots is padded by repeating its last row, which a causal
solve does not see at the knot that is read.  A prefix of one row is padded with a second row (the builder wants two) and read at
knot 0.  Computed once per key (stream_edges.reference), shared, never modified.

Bounds are those of the sibling files: stream_edges.tol (su.TIGHT_Z = 2e-5 of max |ref| on the GPU, a quarter of it for the fp32
torch-op step on the CPU, 1e-10 in fp64)."""
import warnings

import numpy as np
import torch

import hybrid_ref
import stream_edges as se
import stream_ref as sr

NAN = float("nan")
# the main case: two tiles, the second partial; R = the sparse channels.  busy: a stream whose sparse channel 2 changes at every row
# (in the partial tile, so that the full tile can have a row without any piece B); quiet: (row, tile) at which no stream of the
# tile observes a sparse channel
BASE = dict(C=5, R=(2, 4), H=12, HH=10, nl=2, n_out=3, B=19, rows=6, init=-0.5, seed=9101, busy=17, quiet=(3, 0))


def make_rows(seed, n, B, C, R, busy=None, quiet=None, missing=0.3, sparse_missing=0.8, repeat=0.35):
    """[n, B, C] fp32.  Channel 0: strictly increasing irregular times.  Linear channels: random walks with a share `missing` of
    NaNs.  Sparse channels R: observed rarely (NaN share `sparse_missing`), and an observation repeats the channel's previous
    observed value with probability `repeat` (a re-observation that must not add a piece)."""
    rng = np.random.default_rng(seed)
    x = np.empty((n, B, C), np.float64)
    x[:, :, 0] = np.cumsum(rng.uniform(0.5, 1.5, (n, B)), axis=0)
    for c in range(1, C):
        if c in R:
            v = np.full((n, B), NAN)
            held = np.full(B, NAN)
            for r in range(n):
                seen = rng.random(B) >= sparse_missing
                same = (rng.random(B) < repeat) & ~np.isnan(held)
                new = np.where(same, held, np.round(rng.standard_normal(B) * 2.0, 2))
                v[r] = np.where(seen, new, NAN)
                held = np.where(seen, new, held)
            x[:, :, c] = v
        else:
            v = np.cumsum(rng.standard_normal((n, B)), axis=0)
            v[rng.random(v.shape) < missing] = NAN
            x[:, :, c] = v
    if busy is not None and R:
        x[:, busy, R[0]] = 0.25 * np.arange(1, n + 1) * (1 + busy % 3)
    if quiet is not None and R:
        r, tile = quiet
        x[r, 16 * tile:16 * tile + 16][:, list(R)] = NAN
    return np.ascontiguousarray(x, dtype=np.float32)


def causal_fill(rows, init):
    """rows [n, B, C] -> the rows as the handle fills them: NaN -> init on row 0, the last filled value afterwards."""
    f = np.array(rows, np.float32, copy=True)
    f[0][np.isnan(f[0])] = np.float32(init)
    for r in range(1, f.shape[0]):
        f[r] = np.where(np.isnan(f[r]), f[r - 1], f[r])
    return f


def piece_b(rows, R, init):
    """[n, B] bool: the stream takes the second piece at that row (row 0 takes none)."""
    f = causal_fill(rows, init)
    has = np.zeros(f.shape[:2], bool)
    if R:
        has[1:] = (f[1:][:, :, list(R)] != f[:-1][:, :, list(R)]).any(axis=-1)
    return has


def assert_rows(rows, R, init):
    """The rows hold what the hybrid case is about (conditions on the inputs only)."""
    n, B, C = rows.shape
    R = list(R)
    f, has = causal_fill(rows, init), piece_b(rows, R, init)
    tiles = [slice(b, min(b + 16, B)) for b in range(0, B, 16)]
    assert (np.diff(rows[:, :, 0], axis=0) > 0).all() and not np.isnan(rows[:, :, 0]).any()      # the precondition
    assert (~has[1:]).any(), "(a) a stream-row without piece B"
    assert any(not has[r, t].any() for r in range(1, n) for t in tiles if t.stop - t.start == 16), "(b) a row at which a whole 16-stream tile has no piece B"
    assert any(has[r, t].any() and not has[r, t].all() for r in range(1, n) for t in tiles), "(c) a tile-row with both kinds of stream"
    assert has[1:].all(axis=0).any(), "(d) a stream with piece B at every row"
    seen_same = ~np.isnan(rows[1:][:, :, R]) & (f[1:][:, :, R] == f[:-1][:, :, R])
    assert (seen_same.any(axis=-1) & ~has[1:]).any(), "(e) a re-observed unchanged sparse value on a stream-row without piece B"
    assert np.isnan(rows[0][:, R]).any(), "(f) a first row with a NaN in a sparse channel"
    assert np.isnan(rows[:, :, [c for c in range(1, C) if c not in R]]).any()      # ... and NaNs in the linear channels


def base_rows(seed=None):
    s = BASE
    return make_rows(s["seed"] if seed is None else seed, s["rows"], s["B"], s["C"], s["R"], busy=s["busy"], quiet=s["quiet"])


def prefix_reference(model, rows, R, init):
    """model: the (fp32, CPU) linear model whose hybrid handle is under test.  -> (z [n, B, H], out [n, B, n_out]) in fp64."""
    from ncde_amd import unfused
    assert model.interpolation == "linear"
    n, B, C = rows.shape
    f = causal_fill(rows, init)
    hid, full = sr._twin(model, False), sr._twin(model, model.apply_final_linear)
    zs, outs = [], []
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for k in range(n):
            xs = np.ascontiguousarray(np.swapaxes(f[:k + 1], 0, 1))      # [B, k + 1, C]
            if k == 0:      # the builder wants two rows; the path is causal, so knot 0 does not see the row appended here
                pad = xs.copy()
                pad[..., 0] += 1.0
                xs = np.concatenate([xs, pad], axis=1)
            coeffs, lengths = hybrid_ref.hybrid(xs, list(R))
            assert not np.isnan(coeffs).any()
            at = torch.from_numpy(np.zeros(B, np.int64) if k == 0 else lengths.astype(np.int64) - 1)
            X, z0 = hid._control_and_start(torch.from_numpy(coeffs.astype(np.float64)))
            sol = unfused.cdeint_unfused(X, hid.func, z0, X.grid_points, False, hid.vector_field_type, hid.solver, 1.0)
            pick = torch.arange(B)
            zs.append(hid._readout(sol)[pick, at].numpy())
            outs.append(full._readout(sol)[pick, at].numpy())
    return np.stack(zs), np.stack(outs)


def reference(key, build_model, rows, R, init):
    """(z, out) of prefix_reference, once per key."""
    return se.reference(("hybrid",) + tuple(key), lambda: prefix_reference(build_model(), rows, R, init))


def model(kind, mode, device, dtype=torch.float32, seed=91, C=5, H=12, HH=10, nl=2, n_out=3, path="linear", **kw):
    """Built on the CPU under the seed, then moved.  kind "low-rank": sparsity 0.5, rank = ceil(C / 2) < C."""
    if kind == "low-rank":
        kw.setdefault("sparsity", 0.5)
    return se.make_model(seed, C, H, n_out, HH, nl, path, device, dtype, vector_field=kind, vector_field_type=mode, **kw)


def step_through(h, x):
    """One call per row -> (outs [n, B, n_out], zs [n, B, H]) as numpy."""
    outs, zs = [], []
    for k in range(x.size(0)):
        outs.append(h.step(x[k]).cpu().numpy())
        zs.append(h.z.cpu().numpy().copy())
    return np.stack(outs), np.stack(zs)


def worst(outs, zs, z_ref, o_ref, bound, what):
    """Every step within `bound` of max |ref| -> the largest error; the figures are printed before they are asserted."""
    w = 0.0
    for k in range(outs.shape[0]):
        e_out, e_z = se.err(outs[k], o_ref[k]), se.err(zs[k], z_ref[k])
        print("%s step %d: out %.3e z %.3e" % (what, k, e_out, e_z))
        assert e_out <= bound and e_z <= bound, (what, k, e_out, e_z)
        w = max(w, e_out, e_z)
    assert np.abs(z_ref[-1] - z_ref[0]).max() > 1e-3      # the state moved: not a vacuous pass
    print("%s: worst %.3e" % (what, w))
    return w
