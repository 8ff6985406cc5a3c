"""Helpers of the online-inference tests: the g19 goldens (tools/gen_golden_stream.py -> tests/golden/g19_*.npz, MANIFEST_stream.json)
stepped through ``NeuralCDE.online``."""
import json
import os
import warnings

import numpy as np
import torch

import golden_util as gu

CASES = ["g19_a_rect", "g19_b_linear_ffill", "g19_c_rect_static", "g19_d_linear_single_step", "g19_e_rect_time2"]
TIGHT_Z = 2e-5      # forward bound of the project's reference goldens, |delta| / max |ref| (tests/test_control_grad_gpu.py:21)
_CACHE = {}


def load(name):
    if name not in _CACHE:      # read once, shared by the tests, never modified
        f = dict(np.load(os.path.join(gu.GOLD, name + ".npz")))
        _CACHE[name] = (f, json.loads(str(f["meta"])))
    return _CACHE[name]


def model_of(f, meta, device, dtype=torch.float32, **override):
    import ncde_amd
    model = ncde_amd.NeuralCDE(**dict(meta["ctor"], **override))
    sd = {k: torch.from_numpy(f["sd_" + k]) for k in meta["state_dict_keys"]}
    model.load_state_dict({k: v for k, v in sd.items() if k in model.state_dict()})
    return model.to(device=device, dtype=dtype)


def handle_of(model, meta, batch=None):
    return model.online(batch or meta["dims"]["B"], initial_value_if_nan=meta["initial_value_if_nan"], time_index=meta["time_index"])


def rows(f, device, dtype=torch.float32):
    """-> (observations [L, B, C] with their NaNs, static features or None)"""
    x = torch.from_numpy(f["x"]).to(device=device, dtype=dtype).transpose(0, 1).contiguous()
    st = torch.from_numpy(f["static"]).to(device=device, dtype=dtype) if "static" in f else None
    return x, st


def step_through(handle, x, static, quiet=True):
    """One call per observation -> (outputs [L, B, n_out], z [L, B, H], last filled rows [L, B, C]) as numpy."""
    outs, zs, lasts = [], [], []
    with warnings.catch_warnings():
        if quiet:
            warnings.simplefilter("ignore")
        for k in range(x.size(0)):
            outs.append(handle.step(x[k], static=static).cpu().numpy())
            zs.append(handle.z.cpu().numpy().copy())
            lasts.append(handle.last_row.cpu().numpy().copy())
    return np.stack(outs), np.stack(zs), np.stack(lasts)


def knot_rows(meta):
    """Index of observation k's row in the golden's coefficient / hidden sequence."""
    return 2 if meta["path"] == "rectilinear" else 1
