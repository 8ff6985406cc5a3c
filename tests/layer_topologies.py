"""Layer stacks beyond the reference's three ([W0], [W0, W1], [W0, W1, W1, ...]): un-shared, tied and uneven-width inner nets.

The C ABI takes up to NCDE_MAX_LAYERS = 8 independent (layer_W[l], layer_b[l], layer_in[l], layer_out[l]) entries, and FieldSpec lets
entries repeat the same Parameters.  Every dispatcher has its own rule about which of those pointers may alias, and every alias
changes where gradient partials land; this module names the stacks that flip those rules and builds seeded cases for them in the
case-dict layout of tests/test_gpu_parity.py::_seeded_case, so that gpu_util.run_case / run_adjoint_direct / kernel_names and
_grad_errors take them as they are.  Helper only: no test functions."""
import functools

import numpy as np

import golden_util as gu

# name -> [(Wname, bname) per layer]; a repeated name is ONE shared tensor.  Layer 0 maps H -> HH, every further layer HH -> HH.
TOPOLOGIES = {
    "ref_shared3": [("W0", "b0"), ("W1", "b1"), ("W1", "b1")],              # control: the reference's stack
    "distinct3": [("W0", "b0"), ("W1", "b1"), ("W2", "b2")],
    "distinct4": [("W0", "b0"), ("W1", "b1"), ("W2", "b2"), ("W3", "b3")],
    "tied_all2": [("W0", "b0")] * 2,
    "tied_all3": [("W0", "b0")] * 3,
    "tied_first_last": [("W0", "b0"), ("W1", "b1"), ("W0", "b0")],
    "alternating4": [("W0", "b0"), ("W1", "b1"), ("W0", "b0"), ("W1", "b1")],
    "late_share": [("W0", "b0"), ("W1", "b1"), ("W2", "b2"), ("W2", "b2")],
    "early_share": [("W0", "b0"), ("W1", "b1"), ("W1", "b1"), ("W2", "b2")],
    "w_tied_b_own": [("W0", "b0"), ("W0", "b1")],
    "w_shared_b_own": [("W0", "b0"), ("W1", "b1"), ("W1", "b2")],
    "b_shared_w_own": [("W0", "b0"), ("W1", "b1"), ("W2", "b1")],
    "deep6_shared": [("W0", "b0")] + [("W1", "b1")] * 5,
    "deep8_distinct": [("W%d" % i, "b%d" % i) for i in range(8)],        # the ABI maximum
}
# stacks that apply layer 0's matrix again further up: only possible when layer 0 is square (H = HH)
NEEDS_SQUARE = ("tied_all2", "tied_all3", "tied_first_last", "alternating4", "w_tied_b_own")
# a tensor used by more than one layer
TIED = tuple(k for k, v in TOPOLOGIES.items() if len(set(w for w, _ in v)) < len(v) or len(set(b for _, b in v)) < len(v))
DEEP = ("deep6_shared", "deep8_distinct")

# (H, widths): a different width per layer, all layers distinct
WIDTHS = [(48, [64, 32]), (32, [16, 32, 16]), (47, [93, 15, 47]), (16, [128, 16])]


def widths_id(w):
    return "H%d_%s" % (w[0], "x".join(str(n) for n in w[1]))


def stack_of(spec, H, HH):
    """spec: a TOPOLOGIES name, or a list of widths (all layers distinct) -> ([(Wname, bname)], [(out, in) per layer])."""
    if isinstance(spec, str):
        layers = list(TOPOLOGIES[spec])
        assert H == HH or spec not in NEEDS_SQUARE, "%s applies layer 0's matrix twice: H must equal HH" % spec
        dims = [(HH, H)] + [(HH, HH)] * (len(layers) - 1)
    else:
        w = [H] + list(spec)
        layers = [("W%d" % i, "b%d" % i) for i in range(len(spec))]
        dims = [(w[i + 1], w[i]) for i in range(len(spec))]
    return layers, dims


def _draw(seed, stream, shape, fan_in):
    """The project's deterministic generator (data.normal) at the variance of make_field_weights' U(-1/sqrt(fan_in), 1/sqrt(fan_in))."""
    n = int(np.prod(shape))
    return (gu.data.normal(seed, n, stream=stream).reshape(shape) / np.sqrt(3.0 * fan_in)).astype(np.float32)


def make_weights(layers, dims, C, H, seed, kind="original"):
    """One array per distinct name, shaped by the first layer that uses it (a later use with another shape is a mistake in the stack)."""
    p = {}
    for (wn, bn), (dout, din) in zip(layers, dims):
        if wn not in p:
            p[wn] = _draw(seed, 20 + 2 * int(wn[1:]), (dout, din), din)
        if bn not in p:
            p[bn] = _draw(seed, 21 + 2 * int(bn[1:]), (dout,), din)
        assert p[wn].shape == (dout, din) and p[bn].shape == (dout,), (wn, bn, dout, din)
    dl = dims[-1][0]
    p["Wo"], p["bo"] = _draw(seed, 3, (H * C, dl), dl), _draw(seed, 4, (H * C,), dl)
    if kind in ("minimal", "gru"):
        p["Wg"], p["bg"] = _draw(seed, 6, (H * C, dl), dl), _draw(seed, 7, (H * C,), dl)
    if kind == "gru":
        p["Wr"], p["br"] = _draw(seed, 8, (H, H), H), _draw(seed, 9, (H,), H)
    return p


def param_names(layers, kind="original"):
    """Field.unique_params() / FieldSpec.unique_params() order: the inner net layer by layer (W, then b, first use), reset net,
    sigmoid head, tanh head."""
    out = []
    for w, b in layers:
        for n in (w, b):
            if n not in out:
                out.append(n)
    return out + (["Wr", "br"] if kind == "gru" else []) + (["Wg", "bg"] if kind != "original" else []) + ["Wo", "bo"]


def make_inputs(interp, B, L, C, H, seed):
    """(coeffs, z0) of a seeded case, as _seeded_case builds them."""
    if interp == "cubic":
        coeffs = gu.data.make_cubic_coeffs(B, L, C - 1, seed=seed)
        x0 = coeffs[:, 0, :C]
    else:
        coeffs = gu.data.make_rectilinear_coeffs(B, L, C - 1, missing=0.3, seed=seed)
        x0 = coeffs[:, 0]
    rw = gu.data.make_readin_weights(H, C, 1, seed=seed + 1)
    return coeffs, (x0 @ rw["Wi"].T + rw["bi"]).astype(np.float32)


def bare_case(spec, C, H, HH, interp, method, seq, B, L, seed, kind="original"):
    """The case without its expectations (inputs, weights, names)."""
    layers, dims = stack_of(spec, H, HH)
    coeffs, z0 = make_inputs(interp, B, L, C, H, seed)
    p = make_weights(layers, dims, C, H, seed + 1, kind)
    meta = {"kind": interp, "method": method, "sequence": seq, "param_names": param_names(layers, kind), "field_kind": kind,
            "field_mode": "matmul", "dims": {"C": C, "H": H, "HH": dims[0][0], "nl": len(layers)}, "field": "original",
            "topology": spec if isinstance(spec, str) else widths_id((H, spec))}
    return {"meta": meta, "coeffs": coeffs, "z0": z0, "params": p, "layers": layers, "H": H, "C": C}


class ReluMargin:
    """Context: while active, every evaluation of `field`'s inner net (the oracle's `Field.on_pre` observer) records how close its
    ReLU pre-activations come to zero, relative to what fp32 can decide.  A pre-activation is a K-term fp32 dot product whose partial
    sums reach the magnitude of the layer's largest outputs; each of its K additions rounds by up to half an ulp at that magnitude,
    and K such roundings (uniform, independent) add up to a standard deviation of sqrt(K / 12) * eps * max|pre|.  Two correct fp32
    evaluations that sum in different orders differ by that much.  `worst` is the smallest |pre| / (sqrt(K / 12) * eps * max|pre|)
    seen: below 1, the sign of that pre-activation -- one sample's ReLU mask, and with it that sample's gradient, which is
    discontinuous there -- is not determined in fp32, and an expectation computed through it checks nothing at any tolerance."""
    EPS = float(np.finfo(np.float32).eps)

    def __init__(self, field):
        self.field, self.worst = field, float("inf")

    def _see(self, li, pre):
        a = pre.detach().abs()
        k = self.field.layers[li][0].shape[1]
        self.worst = min(self.worst, float(a.min() / (a.max() * np.sqrt(k / 12.0) * self.EPS)))

    def __enter__(self):
        self.field.on_pre = self._see
        return self

    def __exit__(self, *exc):
        self.field.on_pre = None
        return False


MAX_RESEEDS = 32


def well_posed(build, seed):
    """build(seed) -> (result, worst ReluMargin ratio of the oracle runs behind it).  Returns the result of the first seed of seed,
    seed + 1000, ... whose expectation is decided in fp32 (ratio >= 1).  The choice reads the oracle alone, never a kernel's output."""
    for k in range(MAX_RESEEDS):
        out, worst = build(seed + 1000 * k)
        if worst >= 1.0:
            return out
    raise AssertionError("no well-posed seed among %d" % MAX_RESEEDS)


def add_expectations(case, seed):
    """Forward, continuous adjoint, exact discrete backward and stage record of the oracle, in _seeded_case's keys."""
    import ncde_oracle as orc
    m = case["meta"]
    field = gu.oracle_field(case)
    ctl = orc.Control(case["coeffs"], m["kind"])
    with ReluMargin(field) as rm:
        z = orc.solve_forward(ctl, field, case["z0"], m["method"], m["sequence"])
        gout = (gu.data.normal(seed + 2, z.numel(), stream=1).reshape(z.shape) / np.sqrt(z.shape[1])).astype(np.float32)
        dz0, gp = orc.solve_adjoint(ctl, field, z, gout, m["method"], m["sequence"])
        bdz0, bgp = orc.solve_discrete_backward(ctl, field, case["z0"], gout, m["method"], m["sequence"])
        case["stage_record"] = orc.stage_record(ctl, field, case["z0"], m["method"]).numpy()
    case["relu_margin"] = rm.worst
    ex = case["expect"] = {"z_out": z.numpy(), "grad_out": gout, "dz0": dz0.numpy()}
    assert len(gp) == len(m["param_names"])
    for n_, g_ in zip(m["param_names"], gp):
        ex["d" + n_] = g_.numpy()
    ex["bp_dz0"] = bdz0.numpy()
    for n_, g_ in zip(m["param_names"], bgp):
        ex["bp_d" + n_] = g_.numpy()
    return case


def make_case(spec, C, H, HH, interp, method, seq, B, L, seed, kind="original"):
    """spec: a TOPOLOGIES name or a list of widths (then HH is not used).  -> the case-dict of _seeded_case, on the first seed of
    seed, seed + 1000, ... whose expectations are decided in fp32 (ReluMargin; meta["seed"] is the one used)."""
    def build(sd):
        case = add_expectations(bare_case(spec, C, H, HH, interp, method, seq, B, L, sd, kind), sd)
        case["meta"]["seed"] = sd
        return case, case["relu_margin"]
    return well_posed(build, seed)


@functools.lru_cache(maxsize=None)
def cached_case(spec, C, H, HH, interp, method, seq, B, L, seed, kind="original"):
    """make_case computed once per session (spec hashable: a name or a tuple of widths); callers do not modify it."""
    return make_case(spec if isinstance(spec, str) else list(spec), C, H, HH, interp, method, seq, B, L, seed, kind)


def untied(case):
    """The same stack with every layer given its OWN, equal-valued tensors -> (case without expectations, {new name: original
    name}).  dL/d(tied tensor) = the sum of dL/d(its copies): exact algebra, whatever the stack."""
    p = {k: v for k, v in case["params"].items() if k in ("Wo", "bo", "Wg", "bg", "Wr", "br")}
    layers, origin = [], {}
    for l, (w, b) in enumerate(case["layers"]):
        wn, bn = "W%d" % l, "b%d" % l
        p[wn], p[bn] = case["params"][w].copy(), case["params"][b].copy()
        origin[wn], origin[bn] = w, b
        layers.append((wn, bn))
    kind = case["meta"].get("field_kind", "original")
    meta = dict(case["meta"], param_names=param_names(layers, kind))
    out = {k: v for k, v in case.items() if k not in ("expect", "stage_record")}
    out.update(meta=meta, params=p, layers=layers)
    return out, origin


def sum_over_copies(grads, origin, names):
    """{copy name: gradient} -> {original name: sum over its copies} for the original names in `names`."""
    out = {}
    for n in names:
        parts = [np.asarray(grads[c], np.float64) for c, o in origin.items() if o == n] if n in origin.values() else [np.asarray(grads[n], np.float64)]
        out[n] = sum(parts)
    return out


def autograd64(case, grad_out):
    """torch autograd in fp64 through the oracle's own fixed-step solve (orc.Control / orc._step run in the dtype of their inputs):
    -> (z, dL/dz0, {name: dL/dparam}) for L = sum(z * grad_out), as float64 numpy arrays."""
    import torch
    import ncde_oracle as orc
    m = case["meta"]
    t = {k: torch.from_numpy(np.asarray(v, np.float64)).requires_grad_(True) for k, v in case["params"].items()}
    field = orc.Field([(t[w], t[b]) for w, b in case["layers"]], t["Wo"], t["bo"], case["H"], case["C"], m.get("field_kind", "original"),
                      m.get("field_mode", "matmul"), t.get("Wg"), t.get("bg"), t.get("Wr"), t.get("br"))
    z0 = torch.from_numpy(case["z0"].astype(np.float64)).requires_grad_(True)
    z = orc.solve_forward(orc.Control(case["coeffs"].astype(np.float64), m["kind"]), field, z0, m["method"], m["sequence"])
    assert z.dtype == torch.float64
    (z * torch.from_numpy(np.asarray(grad_out, np.float64))).sum().backward()
    return z.detach().numpy(), z0.grad.numpy(), {k: v.grad.numpy() for k, v in t.items() if v.grad is not None}


def torch_field(case, device, dtype):
    """The case's stack as a plain torch module (repeated names share one Parameter), evaluated by torch ops: what the unfused solver
    integrates -- in fp64 on the GPU it is the reference of tests/test_control_grad_gpu.py for cases without a golden; it also
    exposes fused_spec(), so in fp32 cdeint may take either route with it.
    -> (module, {name: Parameter})"""
    import torch

    class TorchField(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.ParameterDict({k: torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(v)).to(device=device, dtype=dtype))
                                             for k, v in case["params"].items()})
            self.nfe = 0

        def fused_spec(self):
            from ncde_amd import solver
            return solver.FieldSpec([(self.p[w], self.p[b]) for w, b in case["layers"]], self.p["Wo"], self.p["bo"])

        def forward(self, t, h):
            for w, b in case["layers"]:
                h = torch.relu(torch.nn.functional.linear(h, self.p[w], self.p[b]))
            self.nfe += 1
            return torch.tanh(torch.nn.functional.linear(h, self.p["Wo"], self.p["bo"])).view(-1, case["H"], case["C"])
    f = TorchField()
    return f, dict(f.p.items())


def mlp_field(case, device):
    """ncde_amd.MLPField with the case's weights loaded (every layer its own tensors: the distinct* and WIDTHS stacks)."""
    import torch
    import ncde_amd
    names = [n for wb in case["layers"] for n in wb]
    assert len(set(names)) == len(names), "MLPField is an un-shared stack"
    f = ncde_amd.MLPField(case["C"], case["H"], [case["params"][w].shape[0] for w, _ in case["layers"]]).to(device)
    with torch.no_grad():
        for lin, (w, b) in zip(f.hidden_layers, case["layers"]):
            lin.weight.copy_(torch.from_numpy(case["params"][w]))
            lin.bias.copy_(torch.from_numpy(case["params"][b]))
        f.out_layer.weight.copy_(torch.from_numpy(case["params"]["Wo"]))
        f.out_layer.bias.copy_(torch.from_numpy(case["params"]["bo"]))
    return f


def mlp_grads(f, case):
    """{case parameter name: .grad of the MLPField's tensor} as numpy arrays."""
    out = {}
    for lin, (w, b) in zip(f.hidden_layers, case["layers"]):
        out[w], out[b] = lin.weight.grad.cpu().numpy(), lin.bias.grad.cpu().numpy()
    out["Wo"], out["bo"] = f.out_layer.weight.grad.cpu().numpy(), f.out_layer.bias.grad.cpu().numpy()
    return out
