"""Online inference of StackedNeuralCDE on the GPU: the one-launch step (ncde_stream_stack_step, csrc/ncde_stream.hip) against the
reference-recorded stack (tests/golden/g16_f_stacked.npz), against the stack's own batch forward in fp64, and against the chain of
per-layer handles, each on ncde_stream_step.

Bounds: forward <= 2e-5 of max |ref| (stream_util.TIGHT_Z).  Against the chain the stage code and its order are shared, so the
outputs and every layer's state are compared bit for bit; so are the launch-shape properties (rows per call, masks, n_stack = 1)."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import golden_util as gu
import stack_util as sk
import stream_util as su

pytestmark = pytest.mark.gpu

SHAPES = {"wide-narrow-wide": [20, 7, 33], "widest-first": [33, 7, 20]}      # no multiple of 4 or 16; B 19: a partial last tile
C_IN, B, L = 5, 19, 6
_REF = {}


def _case(tag):
    """(model on the GPU, rows [L, B, C], fp64 reference [L, B, out]) of one of SHAPES: built once, shared, never modified."""
    if tag not in _REF:
        model = sk.stack(C_IN, SHAPES[tag], 3, seed=21, device="cuda")
        x = sk.observations(L, B, C_IN, seed=17, device="cuda")
        _REF[tag] = (model, x, sk.prefix_reference(sk.as_fp64(model), x, 0.5).numpy())
    return _REF[tag]


def _fused(model, batch=B, v=0.5):
    h = model.online(batch, initial_value_if_nan=v, one_launch=True)
    assert h._use_kernel(torch.empty(1, batch, model.input_dim, device="cuda")), "the query refused the stack"
    return h


def _stack_abi(gpu_lib, layers, x, act, n=None, rectilinear=0, problems=None):
    """ncde_stream_stack_step on the handles' own problems and state, no first-row handling -> (rc, output of the last layer)."""
    from ncde_amd import _lib
    n = len(layers) if n is None else n
    ps = problems or [lay._problem() for lay in layers]
    args = [lay._stream_args(x if i == 0 else None, act, x.size(0), readout=i == len(layers) - 1) for i, lay in enumerate(layers)]
    args[0][0].rectilinear = rectilinear
    parr = (ctypes.POINTER(_lib.NcdeProblem) * max(n, len(ps)))(*[ctypes.pointer(p) for p in ps])
    sarr = (ctypes.POINTER(_lib.NcdeStream) * max(n, len(ps)))(*[ctypes.pointer(a[0]) for a in args])
    rc = gpu_lib.ncde_stream_stack_step(parr, sarr, n, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, args[-1][1]


def _chain_abi(layers, x, act):
    """The same rows through ncde_stream_step layer after layer, no first-row handling -> output of the last layer."""
    h = x
    for lay in layers:
        h = lay._advance_kernel(h, act)
    return h


def _preset(layers, seed, count):
    """Gives every layer a state the caller chose (z random, the rest as after `count` rows)."""
    g = torch.Generator().manual_seed(seed)
    for lay in layers:
        lay.z.copy_(torch.randn(lay.z.shape, generator=g).cuda())
        lay.last_row.copy_(torch.randn(lay.last_row.shape, generator=g).cuda() if count else torch.zeros_like(lay.last_row))
        lay.prev_dx.copy_(torch.randn(lay.prev_dx.shape, generator=g).cuda() if count > 1 else torch.zeros_like(lay.prev_dx))
        lay.count.fill_(count)


def test_golden_stack_on_the_fused_route(gpu_lib):
    from ncde_amd import unfused
    model = sk.golden_model("cuda")
    x, ref = sk.golden_rows("cuda")
    h = model.online(x.size(1), one_launch=True)
    ps, arr = h._problems()
    assert gpu_lib.ncde_stream_stack_kernel_name(arr, len(ps)) == b"ncde_stream_stack_step"
    assert gpu_lib.ncde_stream_stack_workspace_bytes(arr, len(ps)) == 0
    unfused._WARNED.clear()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        outs = torch.stack([h.step(x[k]) for k in range(x.size(0))]).cpu().numpy()
    assert h.fused is True and not unfused._WARNED, unfused._WARNED
    for k in range(x.size(0)):
        e = gu.relerr(outs[k], ref[k])
        print("g16_f_stacked fused step %d: %.3e" % (k, e))
        assert e <= su.TIGHT_Z, (k, e)
    assert [lay.count.cpu().tolist() for lay in h.layers] == [[x.size(0)] * x.size(1)] * 2
    # the default is the chain of the layers' own kernels (measured faster per call): the same bits
    d = model.online(x.size(1))
    assert np.array_equal(torch.stack([d.step(x[k]) for k in range(x.size(0))]).cpu().numpy(), outs) and d.fused is False


@pytest.mark.parametrize("tag", list(SHAPES))
def test_one_launch_equals_the_chain_bit_for_bit_and_meets_fp64(gpu_lib, tag):
    model, x, ref = _case(tag)
    h, chain = _fused(model), sk.chain_handles(model, B, 0.5)
    for k in range(L):
        out = h.step(x[k])
        want = sk.chain_step(chain, model, x[k])
        assert h.fused is True
        d = float((out.double() - want.double()).abs().max())
        e = gu.relerr(out.cpu().numpy(), ref[k])
        print("%s call %d: |fused - chain| %.3e, fused vs fp64 %.3e, chain vs fp64 %.3e" % (tag, k, d, e, gu.relerr(want.cpu().numpy(), ref[k])))
        assert torch.equal(out, want), (k, d)
        sk.assert_states_equal(sk.states(h.layers), sk.states(chain), (tag, k))
        assert e <= su.TIGHT_Z, (k, e)
    assert np.abs(ref[-1] - ref[0]).max() > 1e-3


@pytest.mark.parametrize("tag", list(SHAPES))
def test_rows_in_one_launch_equal_single_calls(gpu_lib, tag):
    model, x, _ = _case(tag)
    h1, hm = _fused(model), _fused(model)
    singles = torch.stack([h1.step(x[k]) for k in range(L)])
    first = hm.step(x[0])
    many = hm.step(x[1:])      # L - 1 rows, one launch
    assert torch.equal(torch.cat([first[None], many]), singles)
    sk.assert_states_equal(sk.states(h1.layers), sk.states(hm.layers), tag)


def test_mask_in_one_launch_equals_masked_single_calls(gpu_lib):
    model, x, _ = _case("wide-narrow-wide")
    g = torch.Generator().manual_seed(4)
    act = (torch.rand(L, B, generator=g) < 0.6).cuda()
    act[0] = True      # every stream has started: the rows below go in one launch
    act[1:, 3] = False      # one stream never receives another row
    h1, hm = _fused(model), _fused(model)
    outs = []
    for k in range(L):
        before = sk.states(h1.layers)
        outs.append(h1.step(x[k], active=act[k]))
        after = sk.states(h1.layers)
        for key in before:      # non-receivers: untouched at every layer
            assert torch.equal(before[key][~act[k]], after[key][~act[k]]), (k, key)
        if k > 0:
            assert torch.equal(outs[k][~act[k]], outs[k - 1][~act[k]])
    hm.step(x[0], active=act[0])
    for lay in hm.layers:      # (known to the caller, not to the handle: with a mask it keeps checking for first rows, row by row)
        lay._may_init = False
    before = sk.states(hm.layers)
    many = hm.step(x[1:], active=act[1:])
    assert torch.equal(many, torch.stack(outs[1:]))
    sk.assert_states_equal(sk.states(h1.layers), sk.states(hm.layers), "masked")
    for key, v in sk.states(hm.layers).items():
        assert torch.equal(v[3], before[key][3]), key
    assert hm.layers[2].count.cpu().tolist() == act.sum(0).cpu().tolist()


def test_first_rows_in_mid_launch_through_the_abi(gpu_lib):
    """Streams whose first row arrives at row 2 of a 4-row launch (count 0, z of every layer as the caller set it): no step at any
    layer at that row, the row kept, steps from the next row on -- as the chain of single steps does it."""
    model, x, _ = _case("widest-first")
    act = torch.ones(4, B, dtype=torch.uint8, device="cuda")
    act[:2, ::3] = 0
    act[3, 1] = 0
    a, b = model.online(B, initial_value_if_nan=0.5, one_launch=True).layers, sk.chain_handles(model, B, 0.5)
    _preset(a, 5, 0)
    _preset(b, 5, 0)
    z_set = [lay.z.clone() for lay in a]
    rc, out = _stack_abi(gpu_lib, a, x[:4], act)
    assert rc == 0
    want = _chain_abi(b, x[:4], act)
    assert torch.equal(out, want)
    sk.assert_states_equal(sk.states(a), sk.states(b), "first rows in mid-launch")
    assert a[2].count.cpu().tolist() == act.sum(0).cpu().tolist()
    late = torch.zeros(B, dtype=torch.bool)
    late[::3] = True
    late = late.cuda()
    # rows 0 and 1 answer the readout of z as set; the first row (row 2) takes no step at any layer: the same answer; row 3 steps
    assert torch.equal(out[1][late], out[0][late]) and torch.equal(out[2][late], out[1][late])
    with torch.no_grad():      # (the kernel's readout sums 20 products in its own order: round-off of O(1) numbers, not bits)
        assert float((out[0][late] - model.ncdes[2].final_linear(z_set[2])[late]).abs().max()) <= 1e-5
    assert not torch.equal(out[3][late], out[2][late])


def test_a_stack_of_one_is_the_single_step(gpu_lib):
    model, x, _ = _case("wide-narrow-wide")
    a, b = [model.ncdes[0].online(B, initial_value_if_nan=0.5)], [model.ncdes[0].online(B, initial_value_if_nan=0.5)]
    _preset(a, 6, 0)
    _preset(b, 6, 0)
    rc, out = _stack_abi(gpu_lib, a, x, None)
    assert rc == 0 and torch.equal(out, _chain_abi(b, x, None))
    sk.assert_states_equal(sk.states(a), sk.states(b), "n_stack 1")
    assert a[0].count.cpu().tolist() == [L] * B


def test_a_stack_of_four(gpu_lib):
    model = sk.stack(C_IN, [12, 21, 6, 17], 2, seed=2, device="cuda")
    x = sk.observations(L, B, C_IN, seed=3, device="cuda")
    ref = sk.prefix_reference(sk.as_fp64(model), x, 0.0).numpy()
    h, chain = _fused(model, v=0.0), sk.chain_handles(model, B)
    for k in range(L):
        out, want = h.step(x[k]), sk.chain_step(chain, model, x[k])
        assert torch.equal(out, want), k
        assert gu.relerr(out.cpu().numpy(), ref[k]) <= su.TIGHT_Z, k
    sk.assert_states_equal(sk.states(h.layers), sk.states(chain), "n_stack 4")


def test_a_method_per_layer_through_the_abi(gpu_lib):
    """midpoint, euler and rk4 in one stack: every layer's problem carries its own method."""
    from ncde_amd import _lib
    model = sk.stack(C_IN, [20, 7, 33], 3, seed=21, device="cuda")
    x = sk.observations(L, B, C_IN, seed=17, device="cuda")
    for ncde, method in zip(model.ncdes, ("midpoint", "euler", "rk4")):
        ncde.solver = method
    a, b = model.online(B).layers, sk.chain_handles(model, B)
    assert [lay._problem().method for lay in a] == [_lib.METHOD[m] for m in ("midpoint", "euler", "rk4")]
    _preset(a, 8, 0)
    _preset(b, 8, 0)
    rc, out = _stack_abi(gpu_lib, a, x, None)
    assert rc == 0 and torch.equal(out, _chain_abi(b, x, None))
    sk.assert_states_equal(sk.states(a), sk.states(b), "methods")
    rk4 = sk.chain_handles(sk.stack(C_IN, [20, 7, 33], 3, seed=21, device="cuda"), B)
    _preset(rk4, 8, 0)
    assert not torch.equal(_chain_abi(rk4, x, None), out)      # the methods matter


def test_lds_boundary(gpu_lib):
    """The first two-layer stack (C = 4) the query refuses takes the chain and meets the bound; the largest accepted one runs on the
    one launch, equals the chain and meets the bound."""
    H, rc, msg = sk.first_refused_width()
    assert rc == -2
    rows = 3
    x = sk.observations(rows, 3, 4, seed=12, device="cuda")
    for width, fused in ((H, False), (H - 1, True)):
        model = sk.stack(4, [width, width], 2, seed=13, device="cuda")
        ref = sk.prefix_reference(sk.as_fp64(model), x, 0.0).numpy()
        h, chain = model.online(3, one_launch=True), sk.chain_handles(model, 3)
        with warnings.catch_warnings():
            warnings.simplefilter("error")      # the chain warns of nothing either: every layer alone is on its kernel
            outs = torch.stack([h.step(x[k]) for k in range(rows)])
        assert h.fused is fused, (width, msg)
        want = torch.stack([sk.chain_step(chain, model, x[k]) for k in range(rows)])
        e = gu.relerr(outs.cpu().numpy(), ref)
        print("width %d (%s): vs fp64 %.3e" % (width, "one launch" if fused else "chain", e))
        assert e <= su.TIGHT_Z, (width, e)
        assert torch.equal(outs, want), width
        sk.assert_states_equal(sk.states(h.layers), sk.states(chain), width)


def test_refusals_leave_the_state_untouched(gpu_lib):
    model, x, _ = _case("wide-narrow-wide")
    layers = model.online(B).layers
    _preset(layers, 9, 2)
    before = sk.states(layers)
    ps = [lay._problem() for lay in layers]
    INVALID, UNSUPPORTED = -1, -2
    assert _stack_abi(gpu_lib, layers, x, None, rectilinear=1)[0] == INVALID
    assert _stack_abi(gpu_lib, layers, x, None, n=0)[0] == INVALID
    assert _stack_abi(gpu_lib, layers, x, None, problems=ps + ps[:2], n=5)[0] == INVALID
    assert _stack_abi(gpu_lib, layers, x, None, problems=[ps[0], ps[2], ps[1]])[0] == INVALID      # channels do not chain
    bad = layers[1]._problem()
    bad.interp = 1
    assert _stack_abi(gpu_lib, layers, x, None, problems=[ps[0], bad, ps[2]])[0] == INVALID
    bad = layers[2]._problem()
    bad.batch = B + 1
    assert _stack_abi(gpu_lib, layers, x, None, problems=[ps[0], ps[1], bad])[0] == INVALID
    bad = layers[1]._problem()
    bad.field_input = 2
    assert _stack_abi(gpu_lib, layers, x, None, problems=[ps[0], bad, ps[2]])[0] == UNSUPPORTED
    sk.assert_states_equal(before, sk.states(layers), "refusals")
    # a stack refused for its LDS plan
    H, _, _ = sk.first_refused_width()
    wide = sk.stack(4, [H, H], 2, seed=13, device="cuda").online(3).layers
    _preset(wide, 10, 2)
    before = sk.states(wide)
    rc, _ = _stack_abi(gpu_lib, wide, sk.observations(2, 3, 4, seed=12, device="cuda"), None)
    assert rc == UNSUPPORTED and b"B of LDS" in gpu_lib.ncde_last_error_string()
    sk.assert_states_equal(before, sk.states(wide), "LDS refusal")
    # and the same buffers then step
    rc, _ = _stack_abi(gpu_lib, layers, x, None)
    assert rc == 0 and layers[0].count.cpu().tolist() == [2 + L] * B
