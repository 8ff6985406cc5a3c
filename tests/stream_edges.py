"""Seeded cases and device-agnostic checks of the online step at its edges (staggered streams, masks, reset, time channel, strides,
missing data, wide shapes), shared by tests/test_online_edges_cpu.py (the torch-op step, fp32 and fp64) and
tests/test_online_edges_gpu.py (the fused kernel).  Helper only: no test functions.

Every model is built on the CPU under its seed and then moved, so both files step the same weights on the same rows; the fp64
reference of a case (stream_ref.prefix_reference) is computed once per session and never modified.

Bounds: against the fp64 reference 2e-5 of max |ref| on the GPU (su.TIGHT_Z); a quarter of that for the fp32 torch-op step on the
CPU -- the drift rule of tools/gen_golden_stream.py, which is what admits a seed -- and 1e-10 in fp64 (tests/test_online_cpu.py)."""
import functools
import warnings

import numpy as np
import torch

import golden_util as gu
import stream_ref as sr
import stream_util as su

NAN = float("nan")
GARBAGE = np.float32(1.0e6)      # what a stream that does NOT receive a call's row is offered: never to be read


def tol(device, dtype):
    if torch.device(device).type == "cuda":
        return su.TIGHT_Z
    return su.TIGHT_Z / 4 if dtype == torch.float32 else 1e-10


class stepping:
    """Context of the handle calls of a check: on the GPU every warning is an error and the fused route must have emitted none; on
    the CPU the once-only 'unfused' warning of the torch-op step is expected and ignored."""

    def __init__(self, device):
        self.cuda = torch.device(device).type == "cuda"

    def __enter__(self):
        from ncde_amd import unfused
        unfused._WARNED.clear()
        self.cm = warnings.catch_warnings()
        self.cm.__enter__()
        warnings.simplefilter("error" if self.cuda else "ignore")
        return self

    def __exit__(self, *exc):
        from ncde_amd import unfused
        self.cm.__exit__(*exc)
        if self.cuda and exc[0] is None:
            assert not unfused._WARNED, unfused._WARNED
        return False


def make_model(seed, C, H, n_out, HH, nl, path, device="cpu", dtype=torch.float32, **kw):
    import ncde_amd
    torch.manual_seed(seed)
    model = ncde_amd.NeuralCDE(C, H, n_out, hidden_hidden_dim=HH, num_layers=nl, interpolation=path, return_sequences=True, **dict({"solver": "rk4"}, **kw))
    return model.to(device=device, dtype=dtype)


def make_rows(seed, n, B, C, time_index=0, missing=0.3):
    """[n, B, C] fp32: increasing irregular times in channel `time_index`, random walks with a share `missing` of NaNs elsewhere."""
    rng = np.random.default_rng(seed)
    t = np.cumsum(rng.uniform(0.5, 1.5, (n, B, 1)), axis=0)
    v = np.cumsum(rng.standard_normal((n, B, C - 1)), axis=0)
    v[rng.random(v.shape) < missing] = NAN
    order = list(range(1, C))
    order.insert(time_index, 0)
    return np.ascontiguousarray(np.concatenate([t, v], axis=2)[:, :, order], dtype=np.float32)


def dev(a, device, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=device) if dtype is None else t.to(device=device, dtype=dtype)


def err(got, ref):
    return gu.relerr(got.detach().cpu().numpy() if torch.is_tensor(got) else got, ref)


@functools.lru_cache(maxsize=None)
def _reference(key):
    """key -> (z, out) of prefix_reference; the arguments behind a key are fixed by the functions below."""
    return _REF_ARGS[key]()


_REF_ARGS = {}


def reference(key, build):
    _REF_ARGS.setdefault(key, build)
    return _reference(key)


# ---- (a) staggered streams ---------------------------------------------------------------------------------------------------------
# one string per stream, one character per call: '1' = the stream receives that call's row.  Tiles: streams 0-15 and 16-18.
SCHEDULE = ["111111",      # 0 receives every row
            "000111",      # 1 joins at call 3 (its first row holds NaNs)
            "010000",      # 2 receives exactly one row and never steps
            "000000",      # 3 never receives anything
            "110011",      # 4 pauses for two calls
            "001111",      # 5 has received one row when call 3 comes
            "101010", "011011", "100001", "000010", "111000", "010101", "001100", "110110", "000011", "111101",
            "111111", "000011", "100011"]
STAG = dict(B=19, C=5, H=12, HH=10, nl=2, n_out=3, init=-0.5, calls=6)


def schedule():
    A = np.array([[ch == "1" for ch in s] for s in SCHEDULE]).T
    assert A.shape == (STAG["calls"], STAG["B"])
    return np.ascontiguousarray(A)


def assert_schedule(A):
    """The schedule holds what the staggered case is about."""
    before = np.cumsum(A, axis=0) - A      # rows received before each call
    assert A[:, 0].all() and not A[:3, 1].any() and A[3:, 1].all() and A[:, 2].sum() == 1 and not A[:, 3].any()
    assert A[:2, 4].all() and not A[2:4, 4].any() and A[4:, 4].all()
    for tile in (slice(0, 16), slice(16, 19)):      # at one call, one tile steps streams with 0, 1 and >= 2 rows behind them
        assert any(set(np.minimum(before[j, tile][A[j, tile]], 2)) == {0, 1, 2} for j in range(A.shape[0])), tile
    j = 3
    assert set(np.minimum(before[j, :16][A[j, :16]], 2)) == {0, 1, 2} and before[j, 1] == 0 and before[j, 5] == 1
    assert (~A[j, :16]).any()      # ... next to streams that receive nothing


def staggered_rows(first_all=False):
    """Rows of the staggered case; a stream that does not receive a call's row is offered GARBAGE there.  first_all: call 0 is an
    unmasked call (every stream receives its row)."""
    A = schedule()
    if first_all:
        A[0] = True
    x = make_rows(4101, STAG["calls"], STAG["B"], STAG["C"])
    x[3, 1, 1] = x[3, 1, 3] = NAN      # NaNs in a joining stream's first row
    x[~A] = GARBAGE
    return x, A


def staggered_model(path, device, dtype):
    s = STAG
    return make_model(41, s["C"], s["H"], s["n_out"], s["HH"], s["nl"], path, device, dtype)


def staggered_reference(path, first_all=False):
    def build():
        x, A = staggered_rows(first_all)
        return sr.prefix_reference(staggered_model(path, "cpu", torch.float32), x, A, None, STAG["init"], 0)
    return reference(("staggered", path, first_all), build)


def check_staggered(device, dtype, path):
    x_np, A = staggered_rows()
    assert_schedule(A)
    model = staggered_model(path, device, dtype)
    z_ref, o_ref = staggered_reference(path)
    x, act = dev(x_np, device, dtype), dev(A, device)
    bound, worst = tol(device, dtype), 0.0
    with stepping(device):
        h = model.online(STAG["B"], initial_value_if_nan=STAG["init"])
        # on the GPU a handle of batch 1; on the CPU a handle of the same batch in which no other stream ever receives a row (the
        # host BLAS takes another routine for a single row, which rounds differently: tools/gen_golden_stream.py notes the same)
        nb = 1 if h.z.is_cuda else STAG["B"]
        alone = [model.online(nb, initial_value_if_nan=STAG["init"]) for _ in range(STAG["B"])]
        for j in range(STAG["calls"]):
            before = h.state_dict()
            out = h.step(x[j], active=act[j])
            after = h.state_dict()
            for key in before:      # a stream without a row: its state untouched
                assert torch.equal(before[key][~act[j]], after[key][~act[j]]), (j, key)
            e_out, e_z = err(out, o_ref[j]), err(h.z, z_ref[j])
            print("staggered %s %s call %d: out %.3e z %.3e" % (path, dtype, j, e_out, e_z))
            assert e_out <= bound and e_z <= bound, (j, e_out, e_z)
            worst = max(worst, e_out, e_z)
            for b in np.nonzero(A[j])[0]:      # ... and every stream answers what it answers alone in a handle of its own
                if nb == 1:
                    ob, i = alone[b].step(x[j, b:b + 1]), 0
                else:
                    only = torch.zeros(nb, dtype=torch.bool, device=x.device)
                    only[b] = True
                    ob, i = alone[b].step(torch.where(only[:, None], x[j], x.new_full((), float(GARBAGE))), active=only), b
                assert torch.equal(ob[i], out[b]) and torch.equal(alone[b].z[i], h.z[b]), (j, b)
                assert torch.equal(alone[b].last_row[i], h.last_row[b]) and torch.equal(alone[b].prev_dx[i], h.prev_dx[b]), (j, b)
        assert h.count.cpu().tolist() == A.sum(axis=0).tolist()
    assert np.abs(z_ref[-1] - z_ref[0]).max() > 1e-3
    return worst


# ---- (b) a per-row mask in one call --------------------------------------------------------------------------------------------------
def check_row_mask(device, dtype, path):
    """After an unmasked first call nothing waits for a first row any more: step(x[1:], active=A[1:]) is ONE advance (on the GPU one
    launch with m = 5 rows and a [5, B] mask), bit-identical to five masked single calls."""
    x_np, A = staggered_rows(first_all=True)
    model = staggered_model(path, device, dtype)
    z_ref, o_ref = staggered_reference(path, True)
    x, act = dev(x_np, device, dtype), dev(A, device)
    with stepping(device):
        h1 = model.online(STAG["B"], initial_value_if_nan=STAG["init"])
        first = h1.step(x[0])
        assert h1._may_init is False      # so the next call is not split into rows
        many = h1.step(x[1:], active=act[1:])
        h2 = model.online(STAG["B"], initial_value_if_nan=STAG["init"])
        singles = [h2.step(x[0])] + [h2.step(x[j], active=act[j]) for j in range(1, STAG["calls"])]
    got = torch.cat([first[None], many])
    assert torch.equal(got, torch.stack(singles))
    for k in h1.state_dict():
        assert torch.equal(h1.state_dict()[k], h2.state_dict()[k]), k
    assert h1.count.cpu().tolist() == A.sum(axis=0).tolist()
    e_out, e_z = err(got, o_ref), err(h1.z, z_ref[-1])
    print("row mask %s %s: out %.3e z %.3e" % (path, dtype, e_out, e_z))
    assert e_out <= tol(device, dtype) and e_z <= tol(device, dtype), (e_out, e_z)
    return max(e_out, e_z)


# ---- (c) reset(mask) and the state dict ----------------------------------------------------------------------------------------------
RESET = dict(B=19, C=5, H=12, HH=10, nl=2, n_out=3, init=-0.5, rows=7, at=3)


def reset_rows():
    x = make_rows(4301, RESET["rows"], RESET["B"], RESET["C"])
    x[RESET["at"], 0, 1] = NAN      # a NaN directly after the reset: the initial value, not the stale row
    return x, np.arange(RESET["B"]) % 3 == 0


def reset_model(path, device, dtype):
    s = RESET
    return make_model(43, s["C"], s["H"], s["n_out"], s["HH"], s["nl"], path, device, dtype)


def check_reset(device, dtype, path):
    s = RESET
    x_np, mask = reset_rows()
    model = reset_model(path, device, dtype)
    whole = reference(("reset", path, 0), lambda: sr.prefix_reference(reset_model(path, "cpu", torch.float32), x_np, None, None, s["init"], 0))
    tail = reference(("reset", path, 1), lambda: sr.prefix_reference(reset_model(path, "cpu", torch.float32), x_np[s["at"]:], None, None, s["init"], 0))
    x, bound, worst = dev(x_np, device, dtype), tol(device, dtype), 0.0
    with stepping(device):
        h = model.online(s["B"], initial_value_if_nan=s["init"])
        h.step(x[:s["at"]])
        saved = h.state_dict()
        h.reset(dev(mask, device))
        assert not h.count[dev(mask, device)].any() and bool((h.count[dev(~mask, device)] == s["at"]).all())
        for j in range(s["at"], s["rows"]):
            out = h.step(x[j])
            for grp, (z_ref, o_ref), k in ((mask, tail, j - s["at"]), (~mask, whole, j)):
                e_out, e_z = err(out[dev(grp, device)], o_ref[k][grp]), err(h.z[dev(grp, device)], z_ref[k][grp])
                print("reset %s %s row %d %s: out %.3e z %.3e" % (path, dtype, j, "restarted" if grp is mask else "running", e_out, e_z))
                assert e_out <= bound and e_z <= bound, (j, e_out, e_z)
                worst = max(worst, e_out, e_z)
            if j == s["at"]:
                assert float(h.last_row[0, 1]) == s["init"]
        assert h.count.cpu().tolist() == [s["rows"] - s["at"] if m_ else s["rows"] for m_ in mask]
        # state_dict -> a new handle -> load_state_dict: bit-equal to not interrupting
        ha, hb = model.online(s["B"], initial_value_if_nan=s["init"]), model.online(s["B"], initial_value_if_nan=s["init"])
        ha.step(x[:s["at"]])
        for k in saved:
            assert torch.equal(saved[k], ha.state_dict()[k]) and saved[k].device == x.device, k
        hb.load_state_dict(saved)
        assert torch.equal(ha.step(x[s["at"]:]), hb.step(x[s["at"]:]))
        for k in saved:
            assert torch.equal(ha.state_dict()[k], hb.state_dict()[k]), k
    return worst


# ---- (d) the time channel ------------------------------------------------------------------------------------------------------------
TIME = dict(B=17, C=5, H=12, HH=10, nl=2, n_out=2, init=0.25, rows=5)


def time_model(path, device, dtype):
    s = TIME
    return make_model(45, s["C"], s["H"], s["n_out"], s["HH"], s["nl"], path, device, dtype)


def check_time_index(device, dtype):
    """Rectilinear with time in the LAST channel against the fp64 reference; on a linear path time_index changes nothing."""
    s = TIME
    ti = s["C"] - 1
    x_np = make_rows(4501, s["rows"], s["B"], s["C"], time_index=ti)
    x_np[0, 2, 0] = NAN
    assert not np.isnan(x_np[:, :, ti]).any() and np.isnan(x_np[:, :, 0]).any()
    x = dev(x_np, device, dtype)
    model = time_model("rectilinear", device, dtype)
    z_ref, o_ref = reference(("time", ti), lambda: sr.prefix_reference(time_model("rectilinear", "cpu", torch.float32), x_np, None, None, s["init"], ti))
    with stepping(device):
        outs, zs, lasts = su.step_through(model.online(s["B"], initial_value_if_nan=s["init"], time_index=ti), x, None, quiet=False)
        wrong, _, _ = su.step_through(model.online(s["B"], initial_value_if_nan=s["init"], time_index=0), x, None, quiet=False)
        lin = time_model("linear", device, dtype)
        same = [su.step_through(lin.online(s["B"], initial_value_if_nan=s["init"], time_index=t), x, None, quiet=False) for t in (0, 2, ti)]
    e_out, e_z = err(outs, o_ref), err(zs, z_ref)
    print("time_index %d %s: out %.3e z %.3e; with time_index 0 instead %.3e" % (ti, dtype, e_out, e_z, err(wrong, o_ref)))
    assert e_out <= tol(device, dtype) and e_z <= tol(device, dtype), (e_out, e_z)
    assert err(wrong, o_ref) > 100 * su.TIGHT_Z      # the case tells the channels apart
    for other in same[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(same[0], other))
    return max(e_out, e_z)


# ---- (e) strides ---------------------------------------------------------------------------------------------------------------------
def strided_inputs(x):
    """x [m, B, C] contiguous -> {name: a view (or expansion) with the same values and other strides}."""
    m, B, C = x.shape
    wide = torch.full((m, B, C + 3), 9.0e5, dtype=x.dtype, device=x.device)
    wide[..., :C] = x
    bf = x.transpose(0, 1).contiguous()
    gap = torch.full((m, B, 2 * C), 9.0e5, dtype=x.dtype, device=x.device)
    gap[..., ::2] = x
    views = {"wide": wide[..., :C], "batch_first": bf.transpose(0, 1), "channel_stride_2": gap[..., ::2]}
    assert views["wide"].stride() == (B * (C + 3), C + 3, 1) and views["channel_stride_2"].stride(2) == 2
    assert m == 1 or views["batch_first"].stride() == (C, m * C, 1)
    return views


def check_strides(device, dtype, path):
    """Every view gives the bits of its contiguous copy, expanded (stride 0) rows included."""
    B, C, m = 17, 5, 4
    model = make_model(47, C, 12, 3, 10, 2, path, device, dtype)
    x = dev(make_rows(4701, m + 1, B, C), device, dtype)

    def run(first, rest):
        h = model.online(B, initial_value_if_nan=0.5)
        a = h.step(first)
        b = h.step(rest)
        return [a, b] + [h.state_dict()[k] for k in sorted(h.state_dict())]

    def same(p, q):
        return all(torch.equal(u, v) for u, v in zip(p, q))

    with stepping(device):
        base = run(x[0], x[1:])
        for name, v in strided_inputs(x[1:]).items():
            assert torch.equal(v.nan_to_num(nan=-7.0), x[1:].nan_to_num(nan=-7.0)) and not v.is_contiguous()
            assert same(run(x[0], v), base), name
        assert same(run(strided_inputs(x[:1])["wide"][0], x[1:]), base), "wide first row"
        row = x[1, 0]      # one row for every stream: stride 0 over the batch
        assert row.expand(B, C).stride() == (0, 1)
        assert same(run(x[0], row.expand(B, C)), run(x[0], row.repeat(B, 1))), "expand over the batch"
        assert same(run(row.expand(B, C), x[2:]), run(row.repeat(B, 1), x[2:])), "expand over the batch, first row"
        x1 = x[1]          # one [B, C] row m times: stride 0 over the rows
        assert x1.expand(m, B, C).stride() == (0, C, 1)
        assert same(run(x[0], x1.expand(m, B, C)), run(x[0], x1.expand(m, B, C).contiguous())), "expand over the rows"
        assert same(run(x[0], row.expand(m, B, C)), run(x[0], row.expand(m, B, C).contiguous())), "expand over rows and batch"
    assert (base[1][-1] - base[0]).abs().max() > 1e-3


# ---- (j) missing data ----------------------------------------------------------------------------------------------------------------
def check_missing(device, dtype, path):
    B, C, n, init = 6, 5, 6, -0.5
    dead, blank, at = 3, 2, 4      # channel never observed; row with every value channel NaN; reset before this row
    x_np = make_rows(4901, n, B, C)
    x_np[:, :, dead] = NAN
    x_np[blank, :, 1:] = NAN
    x_np[blank - 1, :, 1] = np.float32(0.75)      # something to carry over the blank row
    x_np[at, 0, 1] = NAN
    x_np[at - 1, 0, 1] = np.float32(1.5)          # the stale value a reset stream must NOT take
    mask = np.arange(B) == 0

    def mk(dv="cpu", dt=torch.float32):
        return make_model(49, C, 12, 3, 10, 2, path, dv, dt)
    whole = reference(("missing", path, 0), lambda: sr.prefix_reference(mk(), x_np, None, None, init, 0))
    tail = reference(("missing", path, 1), lambda: sr.prefix_reference(mk(), x_np[at:], None, None, init, 0))
    model, x, bound, worst = mk(device, dtype), dev(x_np, device, dtype), tol(device, dtype), 0.0
    rect = path == "rectilinear"
    with stepping(device):
        h = model.online(B, initial_value_if_nan=init)
        for j in range(n):
            if j == at:
                h.reset(dev(mask, device))
            prev = h.last_row.clone()
            out = h.step(x[j])
            assert bool((h.last_row[:, dead] == init).all()), j      # never observed: the initial value for ever
            if j == blank:      # only time moves
                assert torch.equal(h.last_row[:, 1:], prev[:, 1:]) and bool((h.last_row[:, 0] > prev[:, 0]).all())
                assert bool((h.last_row[:, 1] == 0.75).all())
                if rect:        # the second piece's own dX/dt is zero (its first stage still reads the time piece to its left)
                    assert not h.prev_dx.any()
                else:
                    assert not h.prev_dx[:, 1:].any() and torch.equal(h.prev_dx[:, 0], h.last_row[:, 0] - prev[:, 0])
            if j == at:
                assert float(h.last_row[0, 1]) == init and float(prev[0, 1]) == 0.0
            for grp, (z_ref, o_ref), k in ((mask, tail, j - at), (~mask, whole, j)):
                if k < 0:
                    z_ref, o_ref, k = whole[0], whole[1], j
                g = dev(grp, device)
                e_out, e_z = err(out[g], o_ref[k][grp]), err(h.z[g], z_ref[k][grp])
                print("missing %s %s row %d: out %.3e z %.3e" % (path, dtype, j, e_out, e_z))
                assert e_out <= bound and e_z <= bound, (j, e_out, e_z)
                worst = max(worst, e_out, e_z)
    assert np.abs(whole[0][blank] - whole[0][blank - 1]).max() > 1e-3      # the blank row moved the state (time did)
    return worst


# ---- (g) wide shapes -----------------------------------------------------------------------------------------------------------------
# name -> (C, H, HH, nl, B, rows); H352 / H368: the last shape the LDS plan of the step holds and the first it does not
WIDE = {"H192": (6, 192, 192, 2, 17, 4), "H352": (4, 352, 352, 2, 17, 3), "H368": (4, 368, 368, 2, 5, 3)}


def wide_model(name, path, device="cpu", dtype=torch.float32, **kw):
    C, H, HH, nl, B, n = WIDE[name]
    return make_model(51, C, H, 2, HH, nl, path, device, dtype, apply_final_linear=False, **kw)


def wide_rows(name):
    C, H, HH, nl, B, n = WIDE[name]
    return make_rows(5101, n, B, C)


def wide_reference(name, path):
    """-> z [rows, B, H] in fp64"""
    return reference(("wide", name, path), lambda: sr.prefix_reference(wide_model(name, path), wide_rows(name), None, None, 0.0, 0))[0]


# ---- (f) layer stacks ----------------------------------------------------------------------------------------------------------------
# (a stack of tests/layer_topologies.py or a tuple of widths, H, HH)
STACKS = [("distinct3", 20, 20), ("tied_all3", 20, 20), ("w_tied_b_own", 20, 20), ("deep8_distinct", 20, 20),
          ((93, 15, 47), 47, None), ((128, 16), 16, None)]
STACK_DIMS = dict(B=17, C=7, rows=4)


def stack_id(s):
    import layer_topologies as lt
    return s[0] if isinstance(s[0], str) else lt.widths_id((s[1], s[0]))


def stack_case(spec, H, HH, method, path):
    """The case dict of tests/layer_topologies.py for a stack, with coefficients built on the host from seeded ROWS (case["rows"],
    [rows, B, C]) the way the causal builders do; z0 is the case's own."""
    import hybrid_ref
    import layer_topologies as lt
    d = STACK_DIMS
    case = lt.bare_case(spec if isinstance(spec, str) else list(spec), d["C"], H, HH, "linear", method, True, d["B"], 2, 5300 + H)
    rows = make_rows(5301, d["rows"], d["B"], d["C"])
    rect = path == "rectilinear"
    case["rows"] = rows
    case["coeffs"] = hybrid_ref.linear_coeffs(np.swapaxes(rows, 0, 1), rectilinear=0 if rect else None, initial_value_if_nan=0.0, forward_fill_=not rect)
    return case


def stack_oracle(case, dtype=np.float64):
    """The oracle's fixed-step solve of a stack case in `dtype` -> z at every knot, [B, T, H]."""
    import ncde_oracle as orc
    m = case["meta"]
    t = {k: torch.from_numpy(np.asarray(v, dtype)) for k, v in case["params"].items()}
    field = orc.Field([(t[w], t[b]) for w, b in case["layers"]], t["Wo"], t["bo"], case["H"], case["C"], "original", "matmul", None, None, None, None)
    with torch.no_grad():
        z = orc.solve_forward(orc.Control(case["coeffs"].astype(dtype), "linear"), field, torch.from_numpy(case["z0"].astype(dtype)), m["method"], True)
    assert z.numpy().dtype == dtype
    return z.numpy()
