"""Helpers of the stacked online-inference tests: the reference-recorded stack (tests/golden/g16_f_stacked.npz), random stacks and
their observations, the stack's own batch forward chained over the unfused solver, and the chain of per-layer online handles."""
import ctypes
import json
import os
import warnings

import numpy as np
import torch

import golden_util as gu

_CACHE = {}


def golden():
    """-> (arrays, meta) of g16_f_stacked: read once, shared, never modified."""
    if "g" not in _CACHE:
        f = dict(np.load(os.path.join(gu.GOLD, "g16_f_stacked.npz")))
        _CACHE["g"] = (f, json.loads(str(f["meta"])))
    return _CACHE["g"]


def golden_model(device, dtype=torch.float32):
    import ncde_amd
    f, m = golden()
    model = ncde_amd.StackedNeuralCDE(adjoint=False, return_sequences=True, **m["ctor"])
    model.load_state_dict({k[3:]: torch.from_numpy(f[k]) for k in f if k.startswith("sd_")})
    return model.to(device=device, dtype=dtype)


def golden_rows(device, dtype=torch.float32):
    """The golden's coefficient rows as observations [L, B, C] (already filled: no NaN) and the expected outputs [L, B, out]."""
    f, _ = golden()
    x = torch.from_numpy(f["coeffs"]).to(device=device, dtype=dtype).transpose(0, 1).contiguous()
    return x, np.swapaxes(f["out_seq"], 0, 1)


def observations(L, B, C, seed, device="cpu", dtype=torch.float32, missing=0.3):
    """[L, B, C]: channel 0 is an increasing time, the others a random walk with `missing` of their entries NaN (first row included).
    Every value is an fp32 number, whatever `dtype`: the fp32 restatement of the fill (prefix_reference) then copies it exactly."""
    g = torch.Generator().manual_seed(seed)
    x = torch.cumsum(torch.rand(L, B, C, generator=g, dtype=torch.float64) * 0.5 + 0.1, dim=0)
    x[:, :, 1:] = torch.cumsum(torch.randn(L, B, C - 1, generator=g, dtype=torch.float64) * 0.4, dim=0)
    x[:, :, 1:][torch.rand(L, B, C - 1, generator=g) < missing] = float("nan")
    return x.float().to(device=device, dtype=dtype)


def stack(input_dim, hidden_dims, output_dim, seed, device="cpu", dtype=torch.float32, **kw):
    import ncde_amd
    torch.manual_seed(seed)
    return ncde_amd.StackedNeuralCDE(input_dim, list(hidden_dims), output_dim, adjoint=False, return_sequences=True, **kw).to(device=device, dtype=dtype)


def batch_forward(model, coeffs, static=None):
    """StackedNeuralCDE.forward with every layer's solve on the unfused torch-op solver (any device, any dtype), as
    tests/test_control_grad_cpu.py chains it -> [B, L, output_dim]."""
    from ncde_amd import unfused
    h = coeffs
    with torch.no_grad():
        for layer in model.ncdes:
            X, z0 = layer._control_and_start((static, h) if layer.static_dim else h)
            h = layer._readout(unfused.cdeint_unfused(X, layer.func, z0, X.grid_points, False, "matmul", layer.solver, 1))
    return h


def prefix_reference(model, x, v, static=None):
    """What the stack answers after each observation: for every prefix x[:k + 1] the path of layer 0 is built by
    linear_interpolation_coeffs(initial_value_if_nan=v, forward_fill=True) -- its numpy restatement tests/hybrid_ref.py, since the
    package's builder runs on the GPU in fp32 only; the fill copies values, so on fp32-valued rows and an fp32-valued v it is exact --
    and the output at the prefix's LAST knot is kept (observation 0, which alone
    is no path: knot 0 of the two-row prefix) -> [L, B, output_dim] in fp64.  `model` is fp64."""
    import hybrid_ref
    xb = x.to(device="cpu", dtype=torch.float64).transpose(0, 1).contiguous().numpy()
    st = None if static is None else static.to(device="cpu", dtype=torch.float64)
    rows = []
    for k in range(x.size(0)):
        coeffs = torch.from_numpy(hybrid_ref.linear_coeffs(xb[:, :max(k, 1) + 1], initial_value_if_nan=v, forward_fill_=True)).to(torch.float64)
        rows.append(batch_forward(model, coeffs, st)[:, k])
    return torch.stack(rows)


def as_fp64(model):
    import copy
    return copy.deepcopy(model).to(device="cpu", dtype=torch.float64)


def chain_handles(model, B, v=0.0):
    """One OnlineNeuralCDE per layer: the chain a user writes by hand, every layer on its own single-layer step."""
    return [ncde.online(B, initial_value_if_nan=v) for ncde in model.ncdes]


def chain_step(handles, model, x_new, static=None, active=None):
    h = x_new
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for lay in handles:
            h = lay.step(h, static=static if lay.model.static_dim else None, active=active)
    return h


def states(layers):
    from ncde_amd.online import STATE_KEYS
    return {"layers.%d.%s" % (i, k): getattr(lay, k).clone() for i, lay in enumerate(layers) for k in STATE_KEYS}


def assert_states_equal(a, b, where):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), (where, k, float((a[k].double() - b[k].double()).abs().max()))


# ---- the C-ABI queries (no device needed: they read the problems only) -----------------------------------------------------------
def dummy_problem(B=19, C=5, H=20, HH=15, nl=3, interp=0, method=2):
    """A structurally valid problem with dummy (never dereferenced) device pointers."""
    from ncde_amd import _lib
    p = _lib.NcdeProblem()
    p.abi_version = _lib.NCDE_ABI_VERSION
    p.batch, p.n_knots, p.channels, p.hidden = B, 2, C, H
    p.interp, p.method, p.output, p.flags = interp, method, _lib.OUT_KNOTS, 0
    p.n_layers = nl
    for l in range(nl):
        p.layer_in[l], p.layer_out[l] = (H if l == 0 else HH), HH
        p.layer_W[l], p.layer_b[l] = 0x1000, 0x1100
    p.Wo, p.bo = 0x3000, 0x3100
    return p


def query(problems, n=None):
    from ncde_amd import _lib
    lib = _lib.lib()
    arr = (ctypes.POINTER(_lib.NcdeProblem) * max(len(problems), 1))(*[ctypes.pointer(p) if p is not None else None for p in problems])
    n = len(problems) if n is None else n
    rc = lib.ncde_stream_stack_workspace_bytes(arr, n)
    name = lib.ncde_stream_stack_kernel_name(arr, n)
    assert (name == b"ncde_stream_stack_step") == (rc == 0) and (name is None) == (rc != 0)
    return rc, (lib.ncde_last_error_string() or b"").decode()


def first_refused_width(n_stack=2, HH=15, nl=3):
    """The smallest hidden width H at which a stack of n_stack layers (C = 4, then H -> H -> ..) is refused for its LDS plan, found by
    the query: every layer alone is still accepted there (the single step carries one state, the stack n_stack of them)."""
    from ncde_amd import _lib
    lib = _lib.lib()
    for H in range(1, 4096):
        ps = [dummy_problem(B=3, C=4 if i == 0 else H, H=H, HH=HH, nl=nl) for i in range(n_stack)]
        rc, msg = query(ps)
        if rc != 0:
            assert all(lib.ncde_stream_workspace_bytes(ctypes.byref(p)) == 0 for p in ps), H
            return H, rc, msg
    raise AssertionError("no width refused")
