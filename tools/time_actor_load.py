"""Timing: one policy refresh of an MlpActor, [64, 64] and [128, 128, 128] on the 19-float row, from an
nn.Sequential whose parameters live on the device, in two ways
  (a) actor.load_(module)                           ctr_actor_load: one launch into the existing blob
  (b) MlpActor.from_torch(module, scale, device)    a new actor: parameters to the host, ctr_actor_pack
                                                    there, a new device blob, the copy up
each as the GPU sees it (HIP events around the calls, on an otherwise idle stream: the span the
stream is held, gaps included) and as the host sees it (wall clock around the call and a stream
synchronise after it).  The two ways alternate, REPEATS rounds of CALLS calls each after a warm-up;
a round's figure is its mean per call, and the median, lowest and highest round are reported with
the ratio (b) / (a) of the medians.  --only-a makes CALLS loads and nothing else: the run to put under
rocprofv3 --kernel-trace --stats for k_actor_load's own time.
usage: python tools/time_actor_load.py [--json PATH] [--hidden 64,64] [--only-a]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-ctr-reach_amd"))
from ctr_reach_amd.policy import MlpActor  # noqa: E402

DEVICE = "cuda:0"
SCALE = [0.001, 0.001, 0.001, 0.087, 0.087, 0.087]
CALLS, REPEATS, WARM = 1000, 7, 20


def make_seq(hidden, in_dim=19, seed=1):
    torch.manual_seed(seed)
    dims = [in_dim] + list(hidden)
    mods = []
    for a, b in zip(dims[:-1], dims[1:]):
        mods += [nn.Linear(a, b), nn.ReLU()]
    mods += [nn.Linear(dims[-1], 6), nn.Tanh()]
    return nn.Sequential(*mods).to(DEVICE)


def gpu_round(call):
    """us per call: events around CALLS back-to-back calls."""
    stream = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(CALLS):
        call()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / CALLS


def host_round(call):
    """us per call: wall clock around each call and the synchronise after it."""
    total = 0.0
    for _ in range(CALLS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        total += time.perf_counter() - t0
    return total * 1e6 / CALLS


def spread(rounds):
    return {"median_us": round(statistics.median(rounds), 3), "min_us": round(min(rounds), 3),
            "max_us": round(max(rounds), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--hidden", default=None, help="one network, e.g. 64,64 (default: [64,64] and [128,128,128])")
    ap.add_argument("--only-a", action="store_true", help="CALLS loads only (for a kernel trace)")
    args = ap.parse_args()
    shapes = [tuple(int(w) for w in args.hidden.split(","))] if args.hidden else [(64, 64), (128, 128, 128)]
    out = {"device": torch.cuda.get_device_name(0), "calls_per_round": CALLS, "rounds": REPEATS, "cases": {}}
    for hidden in shapes:
        seq = make_seq(hidden)
        actor = MlpActor.from_torch(seq, SCALE, DEVICE)
        if args.only_a:
            for _ in range(CALLS):
                actor.load_(seq)
            torch.cuda.synchronize()
            continue
        ways = {"(a) load_": lambda: actor.load_(seq),
                "(b) from_torch": lambda: MlpActor.from_torch(seq, SCALE, DEVICE)}
        for call in ways.values():
            for _ in range(WARM):
                call()
        torch.cuda.synchronize()
        rounds = {name: {"gpu": [], "host": []} for name in ways}
        for _ in range(REPEATS):                      # alternating: both ways see the same machine
            for name, call in ways.items():
                rounds[name]["gpu"].append(gpu_round(call))
                rounds[name]["host"].append(host_round(call))
        tag = "[%s]" % ",".join(map(str, hidden))
        case = out["cases"][tag] = {"blob_bytes": int(actor.blob.numel())}
        for name in ways:
            case[name] = {k: spread(v) for k, v in rounds[name].items()}
        for k in ("gpu", "host"):
            case["ratio_b_over_a_" + k] = round(case["(b) from_torch"][k]["median_us"] / case["(a) load_"][k]["median_us"], 2)
            for name in ways:
                s = case[name][k]
                print("%-16s %-15s %-5s %9.2f us  (%.2f .. %.2f)" % (tag, name, k, s["median_us"], s["min_us"], s["max_us"]),
                      flush=True)
            print("%-16s (b) / (a)       %-5s %9.2f" % (tag, k, case["ratio_b_over_a_" + k]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
