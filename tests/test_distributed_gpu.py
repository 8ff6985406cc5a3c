"""Data-parallel training with the REAL model on one GPU: two processes, both on cuda:0, `gloo` backend (the
collective's transport does not matter here; what is exercised is `FlatGradAllReduce(single=False)` -- `.grad` aliased
into the flat bucket -- against `_FusedCdeint.backward`, which returns fresh gradient tensors that autograd must
accumulate into those views, followed by identical Adam updates).  The same code runs under RCCL with one GPU per rank."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import golden_util as gu
import ncde_amd
from ncde_amd import distributed as D

pytestmark = pytest.mark.gpu

B, L, C, H, HH, NL, OUT = 64, 12, 20, 32, 32, 3, 1
STEPS = 3
SHAPE = {"B": B, "L": L}      # the workers of the cfg2-shaped case get (1024, 200) through their arguments


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _make_model(adjoint, seq):
    torch.manual_seed(0)
    return ncde_amd.NeuralCDE(C, H, OUT, hidden_hidden_dim=HH, num_layers=NL, interpolation="rectilinear", adjoint=adjoint,
                              solver="rk4", return_sequences=seq).cuda()


def _data(lo, hi, seq):
    B, L = SHAPE["B"], SHAPE["L"]
    x = gu.data.make_rectilinear_coeffs(B, L, C - 1, missing=0.3, seed=21)
    n = L if seq else 1
    y = (ncde_amd.data.uniform01(3, B * n, stream=2) > 0.5).astype(np.float32).reshape(B, n, 1)
    if not seq:
        y = y[:, 0]
    return torch.from_numpy(x[lo:hi]).cuda(), torch.from_numpy(y[lo:hi]).cuda()


def _train(model, x, y):
    bucket = D.FlatGradAllReduce(model.parameters())
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    loss_fn = torch.nn.BCEWithLogitsLoss()
    first = None
    for _ in range(STEPS):
        D.train_step(model, bucket, opt, x, y, loss_fn)
        if first is None:
            first = bucket.gathered().detach().clone().cpu()      # gradient at the common initial parameters
    torch.cuda.synchronize()
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu()
    return flat, first, bucket


def _worker(rank, world, port, out_dir, adjoint, seq, shape=None):
    if shape:
        SHAPE.update(shape)
    B = SHAPE["B"]
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    r, _, w = D.init_process_group("gloo")
    assert (r, w) == (rank, world)
    lo, hi = D.shard_bounds(B, rank, world)
    x, y = _data(lo, hi, seq)
    model = _make_model(adjoint, seq)
    flat, grad, bucket = _train(model, x, y)
    assert not bucket.single
    off = 0
    for p in model.parameters():        # backward accumulated straight into the bucket: the views were never replaced
        assert p.grad.data_ptr() == bucket.flat[off:off + p.numel()].data_ptr()
        off += p.numel()
    torch.save({"params": flat, "grad": grad}, os.path.join(out_dir, "rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("adjoint,seq", [(True, False), (False, True)])
def test_two_rank_neuralcde_data_parallel_on_one_gpu(adjoint, seq, tmp_path, gpu_lib):
    port = _free_port()
    mp.spawn(_worker, args=(2, port, str(tmp_path), adjoint, seq), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "rank0.pt")
    r1 = torch.load(tmp_path / "rank1.pt")
    assert torch.equal(r0["params"], r1["params"])           # replicas stay bit-identical
    assert torch.equal(r0["grad"], r1["grad"])
    # a single process on the full batch: mean loss over 64 samples == average of the two 32-sample mean-loss gradients
    x, y = _data(0, SHAPE["B"], seq)
    flat, grad, _ = _train(_make_model(adjoint, seq), x, y)
    scale = float(grad.abs().max())
    eg = float((grad - r0["grad"]).abs().max()) / scale
    ep = float((flat - r0["params"]).abs().max())
    print("dp vs single process: first-step gradient %.2e (rel. to max), parameters after %d Adam steps %.2e (abs)" % (eg, STEPS, ep))
    assert eg <= 1e-5, eg        # summation order only (32 + 32 samples vs 64 in one launch)
    # Adam divides by sqrt(v): an element whose gradient is small by cancellation turns fp32 summation noise into an update
    # difference of up to ~lr * (relative error of that element); lr = 1e-2, 3 steps
    assert ep <= 1e-3, ep


@pytest.mark.parametrize("adjoint", [True, False])
def test_two_rank_data_parallel_at_the_benchmarked_shape(adjoint, tmp_path, gpu_lib):
    """The same two-rank run at BASELINE cfg2/cfg3's per-sample shape (200 observations -> 399 rectilinear knots, C = 20, H = HH = 32),
    512 samples per rank: the flat-bucket all-reduce runs with the kernels the benchmark times (ncde_fwd_fast_bf3 / ncde_adj_fast3),
    replicas stay bit-identical and the first-step gradient equals the single-process one on the 1024-sample batch.  adjoint=False
    (VERDICT round 4, item 8): the recording forward + exact discrete backward, the mode every shipped experiment of the reference trains in."""
    shape = {"B": 1024, "L": 200}
    port = _free_port()
    mp.spawn(_worker, args=(2, port, str(tmp_path), adjoint, False, shape), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "rank0.pt")
    r1 = torch.load(tmp_path / "rank1.pt")
    assert torch.equal(r0["params"], r1["params"]) and torch.equal(r0["grad"], r1["grad"])
    SHAPE.update(shape)
    try:
        x, y = _data(0, 1024, False)
        flat, grad, _ = _train(_make_model(adjoint, False), x, y)
    finally:
        SHAPE.update({"B": B, "L": L})
    eg = float((grad - r0["grad"]).abs().max()) / float(grad.abs().max())
    assert eg <= 2e-5, eg


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs on one node: RCCL with more than one rank (the pool's boxes have one)")
def test_bench_two_gpus_over_rccl(gpu_lib):
    """bench.py --gpus 2 under torch.distributed.run (started before anything touches a GPU in this process tree's child), `nccl`
    (= RCCL) backend, one rank per GPU: the world>1 branches of the benchmark -- barrier, all-reduce of the flat gradient bucket,
    max-over-ranks timing, weak AND strong legs -- run for real, and the record says how many ranks RCCL saw."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--full"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["rccl_ranks"] == 2 and rec["scaling"] == "weak" and rec["ms_allreduce"] > 0
    assert rec["config"]["global_batch"] == 2 * 4096 and "strong" in rec and rec["strong"]["global_batch"] == 4096
    assert abs(rec["value"] - 2 * 4096 * 398 / (rec["ms_per_step"] * 1e-3)) / rec["value"] < 1e-6


def test_bench_world_size_two_branches_on_one_gpu(gpu_lib):
    """The same launch on a ONE-GPU box: two ranks, both on cuda:0, gloo instead of RCCL (NCDE_BENCH_BACKEND) -- the world > 1
    code of bench.py (probe all-reduce, barrier + max-over-ranks timing, all-reduce timing, the strong-scaling leg, rank-0-only
    output) executes on hardware; only the transport differs from the driver's 2/4/8-GPU runs."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--full"]
    env = dict(os.environ, NCDE_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["rccl_ranks"] == 2 and rec["collective_backend"] == "gloo" and rec["ms_allreduce"] > 0
    assert rec["strong"]["global_batch"] == 4096 and rec["strong"]["batch_per_gpu"] == 2048
    assert "cpu_baseline" not in rec      # rank 0 at N = 1 only


def test_bench_starts_its_own_ranks_without_a_launcher(gpu_lib):
    """a bare `python bench.py --gpus 2` (no torch.distributed.run around it, WORLD_SIZE unset) must not
    die on an assertion -- it starts the two ranks itself as a CHILD process before touching the GPU, relays rank 0's one JSON line and
    returns the child's code.  On this one-GPU box over gloo, both ranks on cuda:0 (NCDE_BENCH_BACKEND)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(NCDE_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--no-extras"],
                         capture_output=True, text=True, timeout=900, cwd=root, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, out.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["rccl_ranks"] == 2 and rec["collective_backend"] == "gloo"
    assert abs(rec["value"] - 2 * 4096 * 398 / (rec["ms_per_step"] * 1e-3)) / rec["value"] < 1e-6
