"""Helpers shared by the low-rank vector-field tests and tools/gen_golden_lowrank.py: the field's forward restated in fp64 torch
(the reference's module cannot be imported where its third-party ``sparselinear`` is absent, so the formula of
src/ncde/vector_fields/sparsity.py:33-55 is pinned here, independently of ncde_amd.LowRankVectorField), deterministic weights, and
the loading of a parameter dict into the package's field."""
import numpy as np
import torch

PARAM_KEYS = {"W0": "net_to_hh.0.weight", "b0": "net_to_hh.0.bias", "W1": "net_to_hh.2.weight", "b1": "net_to_hh.2.bias",
              "Wh": "M_h.weight", "bh": "M_h.bias", "Wq": "M_o.weight", "bq": "M_o.bias"}


def rank_of(C, sparsity):
    return int(np.ceil(C * (1 - sparsity)))


def restated_forward(p, z, H, C, R, nl, layers=None):
    """dz/dt matrix [B, H, C] in fp64 from a parameter dict of arrays: hh = the Linear+ReLU stack, P = M_h(hh) viewed [H, R]
    (row index h R + r), Q = M_o(hh) viewed [R, C] (row index r C + c), M = tanh(P @ Q).  `layers`: [(Wname, bname)] per layer (a
    repeated name is one shared tensor); None = the reference's stack of nl layers (W0, then the shared W1)."""
    if layers is None:
        layers = [("W0", "b0")] + [("W1", "b1")] * (nl - 1)
    t = {k: torch.as_tensor(np.asarray(v)).double() for k, v in p.items()}
    hh = torch.as_tensor(z).double()
    for w, b in layers:
        hh = torch.relu(hh @ t[w].T + t[b])
    P = (hh @ t["Wh"].T + t["bh"]).reshape(-1, H, R)
    Q = (hh @ t["Wq"].T + t["bq"]).reshape(-1, R, C)
    M = torch.zeros(hh.shape[0], H, C, dtype=torch.float64)
    for r in range(R):
        M = M + P[:, :, r:r + 1] * Q[:, r:r + 1, :]
    return torch.tanh(M)


def make_weights(data, H, HH, C, R, nl, seed, scale=1.0):
    """Parameter dict (fp32 arrays) at torch's Linear scale; `scale` multiplies the two head matrices."""
    p = {}
    p["W0"], p["b0"] = data.linear_weights(seed, 1, HH, H)
    if nl > 1:
        p["W1"], p["b1"] = data.linear_weights(seed, 2, HH, HH)
    p["Wh"], p["bh"] = data.linear_weights(seed, 6, H * R, HH)
    p["Wq"], p["bq"] = data.linear_weights(seed, 7, R * C, HH)
    for k in ("Wh", "bh", "Wq", "bq"):
        p[k] = (p[k] * np.float32(scale)).astype(np.float32)
    return p


def param_names(nl):
    return ["W0", "b0"] + (["W1", "b1"] if nl > 1 else []) + ["Wh", "bh", "Wq", "bq"]


def make_field(ncde_amd, p, C, H, HH, nl, sparsity, device="cpu", dtype=torch.float32):
    """ncde_amd.LowRankVectorField holding the dict's parameters -> (field, {name: Parameter})."""
    f = ncde_amd.LowRankVectorField(C, H, HH, nl, sparsity=sparsity)
    sd = {PARAM_KEYS[k]: torch.from_numpy(np.ascontiguousarray(p[k])) for k in param_names(nl)}
    for i in range(2, nl):      # the shared inner Linear appears once per use in the state_dict (net_to_hh.2, .4, ...)
        sd["net_to_hh.%d.weight" % (2 * i)], sd["net_to_hh.%d.bias" % (2 * i)] = sd["net_to_hh.2.weight"], sd["net_to_hh.2.bias"]
    f.load_state_dict(sd)
    f = f.to(device=device, dtype=dtype)
    named = dict(f.named_parameters())
    return f, {k: named[PARAM_KEYS[k]] for k in param_names(nl)}


def head_weights(data, H, C, R, dlast, seed, scale=1.0):
    """M_h [H R, dlast] and M_o [R C, dlast] with their biases at torch's Linear scale, `scale` times as large."""
    p = {}
    p["Wh"], p["bh"] = data.linear_weights(seed, 6, H * R, dlast)
    p["Wq"], p["bq"] = data.linear_weights(seed, 7, R * C, dlast)
    return {k: (v * np.float32(scale)).astype(np.float32) for k, v in p.items()}


class StackField(torch.nn.Module):
    """The low-rank field on ANY layer stack, as a plain torch module: `layers` = [(Wname, bname)] per layer into the parameter dict
    `p` (arrays; a repeated name is ONE Parameter, so a tied tensor collects the gradient of every use), heads Wh, bh, Wq, bq.
    forward() is torch ops only -- what the unfused solver integrates; fused_spec() hands the same Parameters to the fused kernels.
    ncde_amd.LowRankVectorField builds the reference's stack only."""

    def __init__(self, p, layers, H, C, R, device="cpu", dtype=torch.float32):
        super().__init__()
        self.layers, self.H, self.C, self.R = list(layers), H, C, R
        self.p = torch.nn.ParameterDict({k: torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(v)).to(device=device, dtype=dtype))
                                         for k, v in p.items()})
        self.nfe = 0

    def fused_spec(self):
        from ncde_amd import solver
        q = self.p
        return solver.FieldSpec([(q[w], q[b]) for w, b in self.layers], q["Wh"], q["bh"], "lowrank", "matmul", q["Wq"], q["bq"], rank=self.R)

    def forward(self, t, z):
        hh = z
        for w, b in self.layers:
            hh = torch.relu(torch.nn.functional.linear(hh, self.p[w], self.p[b]))
        self.nfe += 1
        P = torch.nn.functional.linear(hh, self.p["Wh"], self.p["bh"]).view(*z.shape[:-1], self.H, self.R)
        Q = torch.nn.functional.linear(hh, self.p["Wq"], self.p["bq"]).view(*z.shape[:-1], self.R, self.C)
        return torch.tanh(P @ Q)


LDS_LIMIT_FLOATS = 160 * 1024 // 4


def _ru(x, m):
    return (x + m - 1) // m * m


def theta_size(H, C, R, dims, layers=None):
    """Floats of one workgroup's gradient partial: every distinct layer tensor once, then M_h | b_h | M_o | b_o."""
    layers = layers or [("W%d" % i, "b%d" % i) for i in range(len(dims))]
    seen, n = set(), 0
    for (w, b), (dout, din) in zip(layers, dims):
        if w not in seen:
            n += dout * din
        if b not in seen:
            n += dout
        seen.update((w, b))
    return n + (H + C) * R * (dims[-1][0] + 1)


def lr_plan(H, C, R, dims, layers=None):
    """The LDS plan of the low-rank kernels restated from DESIGN.md section 5.4a (floats; 160 KB): dims = [(out, in)] per layer,
    layers = their tensor names (None: all distinct).  -> (ok_fwd, ok_adj, gacc_in_lds, res_fwd >= 0, res_adj >= 0): each pass fits,
    the gradient partial lives in LDS, the stacked heads are LDS-resident in the forward / in the backward."""
    L = len(dims)
    HS = 16 * _ru(H, 16)
    DS = 16 * max(_ru(H, 16), max(_ru(d[0], 16) for d in dims))
    NT = _ru((H + C) * R, 16)
    fwd = 3 * DS + 4 * HS + 16 * _ru(C, 4) + 16 * NT
    adj = (4 + L) * DS + 8 * HS + 16 * _ru(C, 4) + 32 * NT
    gacc = adj + theta_size(H, C, R, dims, layers) <= LDS_LIMIT_FLOATS
    if gacc:
        adj += theta_size(H, C, R, dims, layers)
    res = (H + C) * R * ((dims[-1][0] + 1) | 1)
    return (fwd <= LDS_LIMIT_FLOATS, adj <= LDS_LIMIT_FLOATS, gacc, fwd + res <= LDS_LIMIT_FLOATS, adj + res <= LDS_LIMIT_FLOATS)
