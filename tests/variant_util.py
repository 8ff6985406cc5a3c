"""Helpers shared by the tests of the variant kernels (ncde_fwd_variant / ncde_adj_variant: gated fields, evaluate / derivative
inputs): the kernels' LDS plan restated in Python from DESIGN.md section 5.4 (never asking the library), a plain torch field for any
(kind, mode) on any layer list, and deterministic weights for every input mode.  Helper only: no test functions."""
import collections

import numpy as np
import torch

import layer_topologies as lt

LDS_LIMIT_FLOATS = 160 * 1024 // 4
MAX_DLAST = 128            # VR_MAXJT = 8 column tiles of the last hidden width
DW_REG_TILES = 16          # 4 waves x VR_DWT = 4 register tiles of 16 x 16 per matrix
SCRATCH = 4 * 16 * 17      # the adjoint's per-wave transpose scratch

Plan = collections.namedtuple("Plan", "ok_fwd ok_adj gacc_in_lds res_fwd res_adj dw_reg dw_why floats_fwd floats_adj theta")


def _ru(x, m):
    return (x + m - 1) // m * m


def field_dims(mode, C, H):
    """-> (d0, rows): width of the field input and rows of the heads."""
    return (H, H * C) if mode == "matmul" else (H + C, H)


def ref_stack(mode, C, H, HH, nl):
    """The reference's stack: layer 0 (d0 -> HH), then ONE shared layer (HH -> HH) at every further position."""
    d0 = field_dims(mode, C, H)[0]
    return [("W0", "b0")] + [("W1", "b1")] * (nl - 1), [(HH, d0)] + [(HH, HH)] * (nl - 1)


def theta_size(kind, mode, C, H, dims, layers):
    """Floats of one workgroup's gradient partial: every distinct layer tensor once, tanh head, sigmoid head, reset gate."""
    d0, rows = field_dims(mode, C, H)
    seen, n = set(), 0
    for (w, b), (dout, din) in zip(layers, dims):
        if w not in seen:
            n += dout * din
        if b not in seen:
            n += dout
        seen.update((w, b))
    head = rows * (dims[-1][0] + 1)
    return n + head * (2 if kind != "original" else 1) + (d0 * (d0 + 1) if kind == "gru" else 0)


def _residency(kind, mode, C, H, dims, layers, used):
    """Which matrices get an LDS image [ru16(N)][ru16(K) + 1] behind `used` floats, in the host's order: reset gate, the layers (a
    layer sharing BOTH tensors of an earlier one takes that one's answer), tanh head, sigmoid head.
    -> {"r": bool | None, "layers": [bool], "o": bool, "g": bool | None}"""
    d0, rows = field_dims(mode, C, H)
    off = [used]

    def take(N, K):
        need = _ru(N, 16) * (_ru(K, 16) + 1)
        if off[0] + need > LDS_LIMIT_FLOATS:
            return False
        off[0] += need
        return True
    res = {"r": take(d0, d0) if kind == "gru" else None, "layers": []}
    for l, (wb, (dout, din)) in enumerate(zip(layers, dims)):
        first = [q for q in range(l) if layers[q] == wb]
        res["layers"].append(res["layers"][first[-1]] if first else take(dout, din))
    res["o"] = take(rows, dims[-1][0])
    res["g"] = take(rows, dims[-1][0]) if kind != "original" else None
    return res


def _dw_reg(kind, mode, C, H, dims, layers):
    """The adjoint kernel's own rule: hidden and reset weight gradients stay in registers iff there are at most two distinct hidden
    MATRICES (layer 0's and one other, each always at one shape) of at most 16 tiles of 16 x 16, and -- gru -- the d0 x d0 reset
    matrix has at most 16 tiles as well.  -> "registers", or why not: "topology" (asked first), else "size"."""
    tiles = lambda n, k: (_ru(n, 16) // 16) * (_ru(k, 16) // 16)      # noqa: E731
    other, ok = None, True
    for l, (w, _) in enumerate(layers):
        if w == layers[0][0]:
            ok = ok and dims[l] == dims[0]
            continue
        if other is None:
            other = l
        ok = ok and w == layers[other][0] and dims[l] == dims[other]
    if not ok:
        return "topology"
    d0 = field_dims(mode, C, H)[0]
    fits = tiles(*dims[0]) <= DW_REG_TILES and (other is None or tiles(*dims[other]) <= DW_REG_TILES)
    return "registers" if fits and (kind != "gru" or tiles(d0, d0) <= DW_REG_TILES) else "size"


def vr_plan(kind, mode, C, H, dims, layers=None):
    """The variant kernels' plan for a field of `kind` ("original", "minimal", "gru") with input `mode` ("matmul", "evaluate",
    "derivative"): dims = [(out, in)] per layer (in of layer 0 = d0), layers = their (Wname, bname) (None: all distinct).
    -> Plan(ok_fwd, ok_adj, gacc_in_lds, res_fwd, res_adj, dw_reg, dw_why, floats_fwd, floats_adj, theta): each pass fits 160 KB with a last
    width <= 128; the gradient partial lives in LDS; the residency of r / every layer / o / g per pass (None for a refused pass);
    the register weight gradients (dw_why: "registers", "size" or "topology"); the floats of each pass before the resident images; the floats of the partial."""
    layers = layers or [("W%d" % i, "b%d" % i) for i in range(len(dims))]
    L = len(dims)
    d0 = field_dims(mode, C, H)[0]
    assert dims[0][1] == d0 and all(dims[l][1] == dims[l - 1][0] for l in range(1, L))
    Hp, Cp = _ru(H, 16), _ru(C, 4)
    Dp = max([Hp, _ru(d0, 16)] + [_ru(d[0], 16) for d in dims])
    HS, DS = 16 * Hp, 16 * Dp
    theta = theta_size(kind, mode, C, H, dims, layers)
    fwd = 7 * DS + 4 * HS + 16 * Cp
    adj = (15 + 2 * L) * DS + 9 * HS + 16 * Cp + SCRATCH
    gacc = adj + theta <= LDS_LIMIT_FLOATS
    if gacc:
        adj += theta
    why = _dw_reg(kind, mode, C, H, dims, layers)
    shape_ok = L >= 1 and dims[-1][0] <= MAX_DLAST
    ok_fwd, ok_adj = shape_ok and fwd <= LDS_LIMIT_FLOATS, shape_ok and adj <= LDS_LIMIT_FLOATS
    return Plan(ok_fwd, ok_adj, gacc, _residency(kind, mode, C, H, dims, layers, fwd) if ok_fwd else None,
                _residency(kind, mode, C, H, dims, layers, adj) if ok_adj else None, why == "registers", why, fwd, adj, theta)


def pattern(res):
    """Residency as one word: "all", "none" or "mixed" over the matrices the field has."""
    flags = [v for v in [res["r"], res["o"], res["g"]] + list(res["layers"]) if v is not None]
    return "all" if all(flags) else ("none" if not any(flags) else "mixed")


def param_names(layers, kind):
    """Every distinct tensor: the inner net (first use), reset gate, sigmoid head, tanh head."""
    return lt.param_names(layers, kind)


def make_weights(layers, dims, kind, mode, C, H, seed, gain=1.0, scale=1.0, reset_scale=1.0):
    """One fp32 array per distinct name at torch's Linear scale (layer_topologies._draw): the inner net shaped by `dims` (layer 0
    takes d0 inputs), heads of `rows` rows, the reset gate d0 x d0.  gain multiplies the inner matrices, scale the heads and their
    biases, reset_scale the reset gate and its bias."""
    d0, rows = field_dims(mode, C, H)
    p = {}
    for (wn, bn), (dout, din) in zip(layers, dims):
        if wn not in p:
            p[wn] = lt._draw(seed, 20 + 2 * int(wn[1:]), (dout, din), din) * np.float32(gain)
        if bn not in p:
            p[bn] = lt._draw(seed, 21 + 2 * int(bn[1:]), (dout,), din)
        assert p[wn].shape == (dout, din) and p[bn].shape == (dout,), (wn, bn, dout, din)
    dl = dims[-1][0]
    p["Wo"], p["bo"] = lt._draw(seed, 3, (rows, dl), dl) * np.float32(scale), lt._draw(seed, 4, (rows,), dl) * np.float32(scale)
    if kind != "original":
        p["Wg"], p["bg"] = lt._draw(seed, 6, (rows, dl), dl) * np.float32(scale), lt._draw(seed, 7, (rows,), dl) * np.float32(scale)
    if kind == "gru":
        p["Wr"], p["br"] = lt._draw(seed, 8, (d0, d0), d0) * np.float32(reset_scale), lt._draw(seed, 9, (d0,), d0) * np.float32(reset_scale)
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in p.items()}


class StackField(torch.nn.Module):
    """A field of any (kind, mode) on ANY layer stack as a plain torch module: `layers` = [(Wname, bname)] into the parameter dict
    `p` (arrays; a repeated name is ONE Parameter, so a tied tensor collects the gradient of every use).  forward(t, u) is torch ops
    only -- what the unfused solver integrates (u = z, or [z, X(t)] / [z, dX/dt(t)] as its ControlledField hands it); fused_spec()
    hands the same Parameters to the fused kernels.  ncde_amd's gated modules build the reference's stack only.
    `layers` (the tensors per layer) and `on_pre` make it observable by layer_topologies.ReluMargin like the oracle's Field."""
    on_pre = None

    def __init__(self, p, layers, H, C, kind, mode, device="cpu", dtype=torch.float32):
        super().__init__()
        self.layer_names, self.H, self.C, self.kind, self.mode = list(layers), H, C, kind, mode
        self.p = torch.nn.ParameterDict({k: torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(v)).to(device=device, dtype=dtype))
                                         for k, v in p.items()})
        self.nfe = 0

    @property
    def layers(self):
        return [(self.p[w], self.p[b]) for w, b in self.layer_names]

    def fused_spec(self):
        from ncde_amd import solver
        g = lambda k: self.p[k] if k in self.p else None      # noqa: E731
        return solver.FieldSpec(self.layers, self.p["Wo"], self.p["bo"], self.kind, self.mode, g("Wg"), g("bg"), g("Wr"), g("br"))

    def _net(self, x):
        for li, (w, b) in enumerate(self.layers):
            pre = torch.nn.functional.linear(x, w, b)
            if self.on_pre is not None:
                self.on_pre(li, pre)
            x = torch.relu(pre)
        return x

    def forward(self, t, u):
        q = self.p
        inner = self._net(u)
        self.nfe += 1
        if self.kind == "gru":
            reset = self._net(torch.sigmoid(torch.nn.functional.linear(u, q["Wr"], q["br"])) * u)
        else:
            reset = inner
        m = torch.tanh(torch.nn.functional.linear(reset, q["Wo"], q["bo"]))
        if self.kind != "original":
            m = torch.sigmoid(torch.nn.functional.linear(inner, q["Wg"], q["bg"])) * m
        return m.view(*u.shape[:-1], self.H, self.C) if self.mode == "matmul" else m
