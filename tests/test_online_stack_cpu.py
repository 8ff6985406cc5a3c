"""Online inference of StackedNeuralCDE on the CPU: ``StackedNeuralCDE.online`` (here the chain of the layer handles' torch-op steps,
the semantics the one-launch kernel implements) against the reference-recorded stack (tests/golden/g16_f_stacked.npz) at every knot
and against the stack's own batch forward in fp64; static features, masks, the state handling, the argument errors, and the answers
of the stacked step's C-ABI queries, which need no device.

Bounds: forward <= 2e-5 of max |ref| in fp32 (stream_util.TIGHT_Z); fp64 <= 1e-10, as for the g19 goldens."""
import warnings

import numpy as np
import pytest
import torch

import golden_util as gu
import stack_util as sk
import stream_util as su


def _quiet_steps(h, x, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return torch.stack([h.step(x[k], **kw) for k in range(x.size(0))])


def test_golden_stack_step_by_step_and_all_rows_at_once():
    model = sk.golden_model("cpu")
    x, ref = sk.golden_rows("cpu")
    h = model.online(x.size(1))
    assert len(h.layers) == 2 and h.fused is None
    outs = _quiet_steps(h, x).numpy()
    assert h.fused is False      # CPU tensors: the chain of the layer handles
    for k in range(x.size(0)):
        e = gu.relerr(outs[k], ref[k])
        print("g16_f_stacked step %d: %.3e" % (k, e))
        assert e <= su.TIGHT_Z, (k, e)
    h2 = model.online(x.size(1))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        many = h2.step(x).numpy()
    assert many.shape == ref.shape and gu.relerr(many, ref) <= su.TIGHT_Z
    assert np.array_equal(many, outs)
    assert [int(lay.count.min()) for lay in h2.layers] == [x.size(0)] * 2


@pytest.mark.parametrize("dims", [[9, 5, 7], [6, 11]])
def test_fp64_handle_against_the_batch_forward_of_every_prefix(dims):
    L, B, C, v = 6, 5, 4, 0.25
    model = sk.stack(C, dims, 3, seed=5, dtype=torch.float64)
    x = sk.observations(L, B, C, seed=9, dtype=torch.float64)
    assert torch.isnan(x[0]).any() and torch.isnan(x[1:]).any()
    ref = sk.prefix_reference(model, x, v)
    outs = _quiet_steps(model.online(B, initial_value_if_nan=v), x)
    e = gu.relerr(outs.numpy(), ref.numpy())
    print("fp64 stack %s: %.3e" % (dims, e))
    assert e <= 1e-10, e
    assert (ref[-1] - ref[0]).abs().max() > 1e-3


@pytest.mark.parametrize("everywhere", [False, True])
def test_static_features(everywhere):
    L, B, C, S = 5, 4, 3, 2
    model = sk.stack(C, [7, 5], 2, seed=3, dtype=torch.float64, static_dim=S, static_in_all_layers=everywhere)
    assert (model.ncdes[1].static_dim == S) == everywhere
    x = sk.observations(L, B, C, seed=4, dtype=torch.float64)
    static = torch.randn(B, S, dtype=torch.float64)
    ref = sk.prefix_reference(model, x, 0.0, static)
    h = model.online(B)
    with pytest.raises(ValueError, match="static"):
        h.step(x[0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        first = h.step(x[0], static=static)
        rest = h.step(x[1:])      # every stream has started: static is no longer read
    e = gu.relerr(torch.cat([first[None], rest]).numpy(), ref.numpy())
    print("static_in_all_layers=%s: %.3e" % (everywhere, e))
    assert e <= 1e-10, e
    other = sk.prefix_reference(model, x, 0.0, static + 1.0)
    assert (other - ref).abs().max() > 1e-3      # the static features matter


def test_masked_streams_equal_themselves_alone():
    """Stream 1 joins at call 2, stream 2 pauses at calls 2 and 3: each stream's outputs at the calls it received a row equal those of
    a batch-1 handle fed that stream's rows alone, and a stream without a row keeps every layer's state, bit for bit.
    In fp64, to 1e-12 of the largest output: the host's matrix products may sum in another order at batch 1 than at batch 3, which
    moves the last bits of an fp64 number (1e-16) and is carried through at most 5 steps x 4 stages x 2 layers; a stream that read
    another stream's row or state would differ at the 1e-1 level."""
    L, B, C = 6, 3, 4
    model = sk.stack(C, [6, 9], 2, seed=8, dtype=torch.float64)
    x = sk.observations(L, B, C, seed=2, dtype=torch.float64)
    act = torch.ones(L, B, dtype=torch.bool)
    act[:2, 1] = False
    act[2:4, 2] = False
    h = model.online(B, initial_value_if_nan=0.5)
    outs = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for k in range(L):
            before = h.state_dict()
            outs.append(h.step(x[k], active=act[k]))
            after = h.state_dict()
            assert sorted(before) == ["layers.%d.%s" % (i, key) for i in range(2) for key in sorted(("z", "last_row", "prev_dx", "count"))]
            for key in before:
                assert torch.equal(before[key][~act[k]], after[key][~act[k]]), (k, key)
        for b in range(B):
            alone = model.online(1, initial_value_if_nan=0.5)
            for k in range(L):
                if act[k, b]:
                    e = gu.relerr(alone.step(x[k, b:b + 1]).numpy(), outs[k][b:b + 1].numpy())
                    assert e <= 1e-12, (b, k, e)
        # the same rows and mask in one call
        h2 = model.online(B, initial_value_if_nan=0.5)
        assert torch.equal(h2.step(x, active=act), torch.stack(outs))
    assert h.layers[1].count.tolist() == [6, 4, 4]


def test_reset_state_dict_round_trip_and_argument_errors():
    import ncde_amd
    L, B, C = 6, 4, 3
    model = sk.stack(C, [5, 6], 2, seed=1)
    x = sk.observations(L, B, C, seed=6)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        h = model.online(B)
        h.step(x[:3])
        saved = h.state_dict()
        assert len(saved) == 8 and int(saved["layers.1.count"].min()) == 3 and tuple(saved["layers.1.last_row"].shape) == (B, 5)
        tail = h.step(x[3:])
        h2 = model.online(B)
        h2.load_state_dict(saved)
        assert torch.equal(h2.step(x[3:]), tail)
        sk.assert_states_equal(h.state_dict(), h2.state_dict(), "round trip")
        assert not torch.equal(saved["layers.0.z"], h.layers[0].z)      # state_dict() hands out copies
        with pytest.raises(ValueError, match="layers.1.prev_dx"):
            h2.load_state_dict({k: v for k, v in saved.items() if k != "layers.1.prev_dx"})
        with pytest.raises(ValueError, match="layers.1.z"):
            h2.load_state_dict(dict(saved, **{"layers.1.z": torch.zeros(B, 5)}))
        sk.assert_states_equal(h.state_dict(), h2.state_dict(), "a refused load")
        mask = torch.tensor([True, False, True, False])
        h2.load_state_dict(saved)
        h2.reset(mask)
        for lay in h2.layers:
            assert not lay.count[mask].any() and bool((lay.count[~mask] == 3).all()) and not lay.z[mask].any()
        again, fresh = h2.step(x[0]), model.online(B).step(x[0])
        assert torch.equal(again[mask], fresh[mask])
        h2.reset()
        assert not any(lay.count.any() or lay.z.any() for lay in h2.layers)
    # the ValueErrors of the single handle
    with pytest.raises(ValueError, match="initial_value_if_nan"):
        model.online(B, initial_value_if_nan=None)
    with pytest.raises(ValueError, match="batch_size"):
        model.online(0)
    h = model.online(B)
    good = torch.zeros(B, C)
    for bad in (torch.zeros(B, C + 1), torch.zeros(B - 1, C), torch.zeros(2, B, C, 1), torch.zeros(C)):
        with pytest.raises(ValueError, match="x_new"):
            h.step(bad)
    with pytest.raises(ValueError, match="x_new"):
        h.step(good.double())
    with pytest.raises(ValueError, match="active"):
        h.step(good, active=torch.ones(B - 1, dtype=torch.bool))
    with pytest.raises(ValueError, match="grad"):
        h.step(good.clone().requires_grad_(True))
    assert not any(lay.count.any() for lay in h.layers)      # nothing above advanced a stream
    assert isinstance(h, ncde_amd.OnlineStackedNeuralCDE) and h.layers[0].model is model.ncdes[0]


# ---- the C-ABI queries (no device needed: they read the problems only) -----------------------------------------------------------
def test_stack_queries_accept_and_refuse():
    from ncde_amd import _lib
    assert _lib.NCDE_STREAM_MAX_STACK == 4
    widths = [5, 20, 7, 33, 12]
    chain = [sk.dummy_problem(C=widths[i], H=widths[i + 1]) for i in range(4)]
    for n in (1, 2, 3, 4):
        assert sk.query(chain[:n])[0] == 0, n
    INVALID, UNSUPPORTED = -1, -2
    assert sk.query(chain, 0)[0] == INVALID and sk.query(chain + [sk.dummy_problem(C=12, H=4)])[0] == INVALID
    assert sk.query([chain[0], None, chain[2]])[0] == INVALID
    rc, msg = sk.query([chain[0], chain[2]])
    assert rc == INVALID and "channels" in msg
    assert sk.query([chain[0], sk.dummy_problem(B=20, C=20, H=7)])[0] == INVALID
    assert sk.query([chain[0], sk.dummy_problem(C=20, H=7, interp=1)])[0] == INVALID
    for field, value in (("field_kind", _lib.FIELD_KIND["gru"]), ("field_kind", _lib.FIELD_KIND["lowrank"]),
                         ("field_input", _lib.FIELD_INPUT["evaluate"]), ("field_input", _lib.FIELD_INPUT["derivative"])):
        for where in (0, 1):
            ps = [sk.dummy_problem(C=5, H=20), sk.dummy_problem(C=20, H=7)]
            setattr(ps[where], field, value)
            assert sk.query(ps)[0] == UNSUPPORTED, (field, value, where)


def test_stack_lds_boundary_by_the_query():
    H, rc, msg = sk.first_refused_width(HH=8, nl=1)
    print("first refused width of a two-layer stack: %d (%s)" % (H, msg))
    assert rc == -2 and "B of LDS" in msg
    # the bytes the message names are the plan: scratch of the widest layer + the state of every layer
    HS, CS = (H + 15) // 16 * 256, (H + 3) // 4 * 64      # floats of an [h][s] image (= the layer images: HH 8 <= H) and of a [c][s] image
    need = 4 * ((4 * HS + 2 * HS + 3 * CS + 32) + (HS + 2 * 4 * 16 + 16) + (HS + 2 * CS + 16))
    assert str(need) in msg and need > 160 * 1024
    assert sk.query([sk.dummy_problem(B=3, C=4 if i == 0 else H - 1, H=H - 1, HH=8, nl=1) for i in range(2)])[0] == 0
