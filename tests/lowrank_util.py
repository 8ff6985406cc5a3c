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


def restated_forward(p, z, H, C, R, nl):
    """dz/dt matrix [B, H, C] in fp64 from a parameter dict of arrays: hh = the shared Linear+ReLU stack, P = M_h(hh) viewed [H, R]
    (row index h R + r), Q = M_o(hh) viewed [R, C] (row index r C + c), M = tanh(P @ Q)."""
    t = {k: torch.as_tensor(np.asarray(v)).double() for k, v in p.items()}
    hh = torch.as_tensor(z).double()
    hh = torch.relu(hh @ t["W0"].T + t["b0"])
    for _ in range(nl - 1):
        hh = torch.relu(hh @ t["W1"].T + t["b1"])
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
