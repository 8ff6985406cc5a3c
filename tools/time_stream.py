"""Per-observation latency of online inference at cfg2 dimensions (C 20, H = HH = 32, three layers, rectilinear, rk4; run on the GPU box).

    python tools/time_stream.py [--out profiles/online_step_latency.json]      # ROUNDS=5 STEPS=200 REPS=10
    python tools/time_stream.py --interpolation linear,cubic_hermite           # the Hermite step (ncde_stream_step_hermite) next to the
                                                                               # linear step at the same shape: legs alternate in ONE process
    python tools/time_stream.py --vector-field minimal --batches 16,4096 --prefixes ""      # the field step (ncde_stream_step_field) next
    python tools/time_stream.py --vector-field-type evaluate --batches 16,4096 --prefixes ""  # to the torch-op step on the same weights
    python tools/time_stream.py --vector-field low-rank --interpolation linear --batches 16,4096 --prefixes "" --append --out F
                                                                               # the low-rank step (ncde_stream_step_lowrank), any path
    python tools/time_stream.py --interpolation cubic_hermite --vector-field minimal --batches 16,4096 --prefixes "" --append --out F
                                                                               # the field step on the Hermite path; --append collects
                                                                               # the runs of several invocations in one file
    python tools/time_stream.py --interpolation rectilinear,linear --hybrid 0,100 --prefixes ""      # the hybrid step (ncde_stream_step_hybrid,
                                                                               # DESIGN.md 5.14 "Hybrid step") next to the rectilinear and the
                                                                               # linear step of the same build, on the same weights

Legs, per batch size B in {1, 16, 256, 4096}:
  online step      handle.step(x_k) of NeuralCDE.online, one new observation per call (one launch of ncde_stream_step)
  prefix k         what a server has without it: one NeuralCDE(return_sequences=False) call on the prefix of k observations
                   (k in {10, 100, 399}; the prefix's coefficients are built BEFORE the clock starts, which flatters this leg)
  hybrid P%        with --hybrid P[,P..]: a linear handle over the same weights with rectilinear_indices = the upper half of the
                   channels, on rows whose sparse channels are observed, at a new value, on P % of the (stream, row) pairs and NaN
                   elsewhere: at 0 % no tile ever takes the second piece (S stages per row), at 100 % every stream takes it at every
                   row (2 S stages, the rectilinear step's count)
  torch-op step    with --vector-field / --vector-field-type other than original / matmul: a second handle over the same weights held
                   on the torch-op step (online.py::_advance_torch) -- the route such a handle took before its step kernel existed, and
                   the yardstick of that kernel
Every call is followed by a device synchronise inside the timed window -- a server reads the prediction before the next observation
arrives -- and the clock is the host's.  Every leg is warmed up, then the legs are timed ALTERNATING for ROUNDS rounds (STEPS online
steps / REPS prefix calls per round); one line per (leg, round) so that the spread is visible, then median, min and max per leg.
One 16-stream tile occupies one compute unit, so B <= 16 runs on a single CU: latency-bound by design."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import ncde_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the medians and spreads here as JSON")
    ap.add_argument("--batches", default="1,16,256,4096")
    ap.add_argument("--prefixes", default="10,100,399")
    ap.add_argument("--interpolation", default="rectilinear", help="the causal control path: rectilinear, linear or cubic_hermite; a comma "
                    "list times one online leg per path (the prefix legs run on the first)")
    ap.add_argument("--vector-field", default="original", help="original, minimal or low-rank (the fields with a step kernel)")
    ap.add_argument("--sparsity", type=float, default=0.5, help="low-rank: rank = ceil(C (1 - sparsity))")
    ap.add_argument("--append", action="store_true", help="--out holds {\"runs\": [...]}: add this run to it instead of overwriting")
    ap.add_argument("--vector-field-type", default="matmul", help="matmul, evaluate or derivative")
    ap.add_argument("--hybrid", default="", help="comma list of percentages: one hybrid leg each, the sparse channels changing on that share of the rows")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    ROUNDS, STEPS, REPS = (int(os.environ.get(k, d)) for k, d in (("ROUNDS", 5), ("STEPS", 200), ("REPS", 10)))
    c = dict(bench.CONFIGS["cfg2"])
    prefixes = [int(k) for k in args.prefixes.split(",") if k]
    field = dict(vector_field=args.vector_field, vector_field_type=args.vector_field_type)
    if args.vector_field == "low-rank":
        field["sparsity"] = args.sparsity
    variant = (args.vector_field, args.vector_field_type) != ("original", "matmul")
    L = max(prefixes + [STEPS]) + 1
    paths = args.interpolation.split(",")
    assert all(p in ("rectilinear", "linear", "cubic_hermite") for p in paths), paths
    path = paths[0]
    shares = [int(v) for v in args.hybrid.split(",") if v]
    report = {"dims": {k: c[k] for k in ("C", "H", "HH", "nl")}, "interpolation": paths, "hybrid": shares, "field": field, "rounds": ROUNDS, "steps": STEPS, "reps": REPS, "legs": []}
    for B in (int(b) for b in args.batches.split(",")):
        torch.manual_seed(0)
        model = ncde_amd.NeuralCDE(c["C"], c["H"], 1, hidden_hidden_dim=c["HH"], num_layers=c["nl"], interpolation=path, solver="rk4", **field).cuda()
        x = torch.from_numpy(ncde_amd.data.synthetic_series(B, L, c["C"] - 1, missing=c["missing"], seed=1234)).cuda()
        rows = x.transpose(0, 1).contiguous()
        handles = {path: model.online(B)}
        for q in paths[1:]:      # the same weights on the other paths
            other = ncde_amd.NeuralCDE(c["C"], c["H"], 1, hidden_hidden_dim=c["HH"], num_layers=c["nl"], interpolation=q, solver="rk4", **field).cuda()
            other.load_state_dict(model.state_dict())
            handles[q] = other.online(B)
        leg_rows = {}      # legs that step rows of their own
        sparse = list(range(c["C"] - c["C"] // 2, c["C"]))
        for share in shares:
            lin = model
            if path != "linear":
                lin = ncde_amd.NeuralCDE(c["C"], c["H"], 1, hidden_hidden_dim=c["HH"], num_layers=c["nl"], interpolation="linear", solver="rk4", **field).cuda()
                lin.load_state_dict(model.state_dict())
            name = "hybrid %d%%" % share
            handles[name] = lin.online(B, rectilinear_indices=sparse)
            g = torch.Generator(device="cpu").manual_seed(4321 + share)
            seen = (torch.rand(L, B, generator=g) * 100.0 < share).cuda()
            value = torch.arange(L, dtype=torch.float32, device="cuda")[:, None, None] * 0.01 + torch.rand(L, B, len(sparse), generator=g).cuda()
            hr = rows.clone()
            hr[:, :, sparse] = torch.where(seen[:, :, None], value, torch.full_like(value, float("nan")))
            leg_rows[name] = hr
        if variant:      # the same handle class, held on the torch-op step (its once-only warning is not the subject here)
            handles["torch-op"] = model.online(B)
            handles["torch-op"]._route[("cuda", torch.float32)] = False
        if path == "rectilinear":
            coeffs = {k: ncde_amd.linear_interpolation_coeffs(x[:, :k].contiguous(), rectilinear=0, initial_value_if_nan=0.0) for k in prefixes}
        else:
            build = ncde_amd.hermite_cubic_coefficients_with_backward_differences if path == "cubic_hermite" else ncde_amd.linear_interpolation_coeffs
            coeffs = {k: build(x[:, :k].contiguous(), initial_value_if_nan=0.0, forward_fill=True) for k in prefixes}

        def online(n, q=path):
            handle, own = handles[q], leg_rows.get(q, rows)
            handle.reset()
            handle.step(own[0])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(1, n + 1):
                handle.step(own[k])
                torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n

        def prefix(k, n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                with torch.no_grad():
                    model(coeffs[k])
                torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n

        legs = [("online step" if q == path else "online " + q, lambda q=q: online(STEPS, q)) for q in paths] + [(q, lambda q=q: online(STEPS, q)) for q in leg_rows] + ([("torch-op step", lambda: online(STEPS, "torch-op"))] if variant else []) + [("prefix %d" % k, lambda k=k: prefix(k, REPS)) for k in prefixes]
        for q in handles:
            online(20, q)
        for k in prefixes:
            prefix(k, 2)
        times = {name: [] for name, _ in legs}
        for r in range(ROUNDS):
            for name, fn in legs:
                dt = fn()
                times[name].append(dt)
                print("B %5d round %d  %-20s %10.1f us/call" % (B, r, name, dt * 1e6), flush=True)
        for name, _ in legs:
            v = times[name]
            rec = {"B": B, "leg": name, "median_us": statistics.median(v) * 1e6, "min_us": min(v) * 1e6, "max_us": max(v) * 1e6}
            report["legs"].append(rec)
            print("B %5d median   %-20s %10.1f us/call  (min %.1f, max %.1f over %d rounds)" % (B, name, rec["median_us"], rec["min_us"], rec["max_us"], ROUNDS),
                  flush=True)
    if args.out:
        if args.append:
            runs = []
            if os.path.exists(args.out):
                with open(args.out) as fh:
                    runs = json.load(fh)["runs"]
            report = {"runs": runs + [report]}
        with open(args.out, "w") as fh:
            json.dump(report, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
