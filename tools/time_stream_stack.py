"""Per-observation latency of online inference of a StackedNeuralCDE (run on the GPU box): the one-launch step against the chain.

    python tools/time_stream_stack.py [--out profiles/online_stack_latency.json]      # ROUNDS=5 STEPS=200

Legs, per stack (hidden_dims [32, 32] and [32, 32, 32] on 20 channels, rk4) and batch size B in {16, 4096}, on the same weights:
  one launch   handle.step(x_k) of StackedNeuralCDE.online(one_launch=True): every layer in one launch of ncde_stream_stack_step
  chain        the yardstick, what exists without it (and what the handle does by default): one NeuralCDE.online handle per layer, chained by hand -- one launch of
               ncde_stream_step and one Python round trip per layer
Every call is followed by a device synchronise inside the timed window and the clock is the host's, as in tools/time_stream.py.  Both
legs are warmed up, then timed ALTERNATING for ROUNDS rounds of STEPS steps; one line per (leg, round), then median, min and max."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ncde_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the medians and spreads here as JSON")
    ap.add_argument("--batches", default="16,4096")
    ap.add_argument("--stacks", default="32,32;32,32,32", help="hidden_dims of the stacks to time, ';' between stacks")
    ap.add_argument("--channels", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    ROUNDS, STEPS = (int(os.environ.get(k, d)) for k, d in (("ROUNDS", 5), ("STEPS", 200)))
    C = args.channels
    report = {"channels": C, "method": "rk4", "rounds": ROUNDS, "steps": STEPS, "legs": []}
    for dims in ([int(h) for h in s.split(",")] for s in args.stacks.split(";")):
        for B in (int(b) for b in args.batches.split(",")):
            torch.manual_seed(0)
            model = ncde_amd.StackedNeuralCDE(C, dims, 1, return_sequences=True).cuda()
            x = torch.from_numpy(ncde_amd.data.synthetic_series(B, STEPS + 1, C - 1, missing=0.3, seed=1234)).cuda()
            rows = x.transpose(0, 1).contiguous()
            fused = model.online(B, one_launch=True)
            chain = [ncde.online(B) for ncde in model.ncdes]

            def one_launch(row):
                return fused.step(row)

            def chained(row):
                for lay in chain:
                    row = lay.step(row)
                return row

            def run(step, handles, n):
                for h in handles:
                    h.reset()
                step(rows[0])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(1, n + 1):
                    step(rows[k])
                    torch.cuda.synchronize()
                return (time.perf_counter() - t0) / n

            legs = [("one launch", lambda n: run(one_launch, [fused], n)), ("chain", lambda n: run(chained, chain, n))]
            for _, fn in legs:
                fn(20)
            assert fused.fused is True, "the stack did not take the one-launch route"
            assert torch.equal(one_launch(rows[21]), chained(rows[21]))      # (both legs stand after 21 rows: the same answer)
            times = {name: [] for name, _ in legs}
            for r in range(ROUNDS):
                for name, fn in legs:
                    dt = fn(STEPS)
                    times[name].append(dt)
                    print("%s B %5d round %d  %-12s %10.1f us/call" % (dims, B, r, name, dt * 1e6), flush=True)
            for name, _ in legs:
                v = times[name]
                rec = {"hidden_dims": dims, "B": B, "leg": name, "median_us": statistics.median(v) * 1e6, "min_us": min(v) * 1e6, "max_us": max(v) * 1e6}
                report["legs"].append(rec)
                print("%s B %5d median   %-12s %10.1f us/call  (min %.1f, max %.1f over %d rounds)" % (dims, B, name, rec["median_us"], rec["min_us"],
                                                                                                      rec["max_us"], ROUNDS), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(report, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
