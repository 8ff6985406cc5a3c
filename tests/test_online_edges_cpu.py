"""The online step at its edges, on the CPU: the fp64 reference helper (tests/stream_ref.py) against the reference project's own
goldens, then the torch-op step of ``NeuralCDE.online`` -- the semantics the fused kernel implements -- in fp32 and fp64 on the
cases of tests/stream_edges.py: staggered streams, a per-row mask, reset(mask), the time channel, strided rows, missing data.

Bounds (stream_edges.tol): fp32 within a QUARTER of the project's forward bound 2e-5 against the fp64 reference -- the drift rule of
tools/gen_golden_stream.py, checked here for every seed the GPU tests use; fp64 within 1e-10.  Fill copies, untouched state, rows per
call and streams alone are compared bit for bit."""
import numpy as np
import pytest
import torch

import golden_util as gu
import stream_edges as se
import stream_ref as sr
import stream_util as su

DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
PATHS = pytest.mark.parametrize("path", ["rectilinear", "linear"])


@pytest.mark.parametrize("name", su.CASES)
def test_reference_helper_reproduces_the_goldens(name):
    """prefix_reference is independent of online.py; on the reference project's own fp64 results it is exact to round-off."""
    f, m = su.load(name)
    x, st = su.rows(f, "cpu")
    z, out = sr.prefix_reference(su.model_of(f, m, "cpu"), x, None, st, m["initial_value_if_nan"], m["time_index"])
    q = su.knot_rows(m)
    e_z, e_out = gu.relerr(z, np.swapaxes(f["hidden64"][:, ::q], 0, 1)), gu.relerr(out, np.swapaxes(f["out64"], 0, 1))
    print("%s: prefix_reference vs the golden's fp64: z %.3e out %.3e" % (name, e_z, e_out))
    assert e_z <= 1e-10 and e_out <= 1e-10, (e_z, e_out)
    rect = m["path"] == "rectilinear"
    for b in range(x.size(1)):      # the path it builds: the reference builder's own rows, bit for bit
        c = sr.path64(f["x"][b:b + 1], rect, m["initial_value_if_nan"], m["time_index"]).numpy()
        assert np.array_equal(c[0], f["coeffs"][b].astype(np.float64))


def test_reference_helper_on_partial_streams():
    """A stream without a row answers the readout of z = 0, a stream without a new row repeats itself, and a stream's answers do not
    depend on its neighbours or on what it was offered while it did not receive."""
    x, A = se.staggered_rows()
    model = se.staggered_model("rectilinear", "cpu", torch.float32)
    z, out = se.staggered_reference("rectilinear")
    bias = model.final_linear.bias.detach().double().numpy()
    assert not z[:, 3].any() and np.array_equal(out[:, 3], np.broadcast_to(bias, out[:, 3].shape))
    assert not z[0, 1].any() and np.array_equal(out[2, 1], bias)
    for j in range(1, A.shape[0]):
        idle = ~A[j]
        assert np.array_equal(z[j][idle], z[j - 1][idle]) and np.array_equal(out[j][idle], out[j - 1][idle])
    b = 4
    z1, out1 = sr.prefix_reference(model, x[A[:, b], b:b + 1], None, None, se.STAG["init"], 0)
    assert np.array_equal(z1[:, 0], z[A[:, b], b]) and np.array_equal(out1[:, 0], out[A[:, b], b])


def test_the_new_golden_has_time_in_channel_2():
    f, m = su.load("g19_e_rect_time2")
    assert m["time_index"] == 2 and m["path"] == "rectilinear" and m["dims"]["C"] == 5
    assert not np.isnan(f["x"][:, :, 2]).any() and (np.diff(f["x"][:, :, 2], axis=1) > 0).all()
    assert np.isnan(f["x"][:, 0]).any() and np.isnan(f["x"][:, 1:, 0]).any()
    c = f["coeffs"]      # lagged rows: new time, old values
    assert np.array_equal(c[:, 1::2, 2], c[:, 2::2, 2]) and np.array_equal(np.delete(c[:, 1::2], 2, axis=2), np.delete(c[:, 0:-1:2], 2, axis=2))


@DTYPES
@PATHS
def test_staggered_streams(path, dtype):
    se.check_staggered("cpu", dtype, path)


@DTYPES
@PATHS
def test_per_row_mask_in_one_call(path, dtype):
    se.check_row_mask("cpu", dtype, path)


@DTYPES
@PATHS
def test_reset_mask_and_state_dict(path, dtype):
    se.check_reset("cpu", dtype, path)


@DTYPES
def test_time_index_last_channel(dtype):
    se.check_time_index("cpu", dtype)


@DTYPES
@PATHS
def test_strided_rows(path, dtype):
    se.check_strides("cpu", dtype, path)


@DTYPES
@PATHS
def test_missing_data(path, dtype):
    se.check_missing("cpu", dtype, path)


@pytest.mark.parametrize("name,path", [("H192", "rectilinear"), ("H192", "linear"), ("H352", "rectilinear"), ("H368", "rectilinear")])
def test_wide_seeds_do_not_drift(name, path):
    """The wide cases of the GPU tests: their fp32 torch-op step stays within a quarter of the bound against fp64."""
    model = se.wide_model(name, path)
    x = se.dev(se.wide_rows(name), "cpu")
    _, zs, _ = su.step_through(model.online(x.size(1)), x, None)
    e = gu.relerr(zs, se.wide_reference(name, path))
    print("wide %s %s: fp32 torch-op step vs fp64 %.3e" % (name, path, e))
    assert e <= su.TIGHT_Z / 4, e
    assert np.abs(zs[-1] - zs[0]).max() > 1e-3


@PATHS
@pytest.mark.parametrize("method", ["rk4", "midpoint"])
@pytest.mark.parametrize("spec,H,HH", se.STACKS, ids=[se.stack_id(s) for s in se.STACKS])
def test_stack_seeds_do_not_drift(spec, H, HH, method, path):
    """The layer-stack cases of the GPU tests: the oracle in fp32 stays within a quarter of the bound of itself in fp64."""
    case = se.stack_case(spec, H, HH, method, path)
    z32, z64 = se.stack_oracle(case, np.float32), se.stack_oracle(case)
    e = gu.relerr(z32, z64)
    print("stack %s %s %s: oracle fp32 vs fp64 %.3e" % (se.stack_id((spec, H, HH)), method, path, e))
    assert e <= su.TIGHT_Z / 4, e
    assert np.abs(z64[:, -1] - z64[:, 0]).max() > 1e-3
