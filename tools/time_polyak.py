"""Timing: the end of one learner update, the Polyak step of both target networks and the refresh of
their two blobs, for [64, 64] and [128, 128, 128] actor + critic pairs on a 13-float observation
(rows of 19, critic inputs of 25), in three ways
  (a) polyak_([(actor_targ, policy, policy_targ), (critic_targ_dev, critic, critic_targ)], tau):
      one ctr_polyak launch
  (b) as examples/train_ddpg_her.py does it with --device-targets: the per-parameter lerp_ loop over
      both networks, then actor_targ.load_(policy_targ) and critic_targ_dev.load_(critic_targ)
  (c) torch._foreach_lerp_ over both networks' parameters, then the same two load_: the cheapest
      torch-only way
each as the GPU sees it: HIP events around CALLS back-to-back updates on an otherwise idle stream, the
span the stream is held per update, the gaps the host leaves included.  The three ways alternate in
one process, REPEATS rounds each after a warm-up; a round's figure is its mean per update, and the
median, lowest and highest round are reported.  (a) "is faster" than another way in a cell when its
highest round lies below the other's lowest.  --only-a makes CALLS updates of (a) and nothing else:
the run to put under rocprofv3 --kernel-trace --stats for the kernel's own time.
usage: python tools/time_polyak.py [--json PATH] [--only-a]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-ctr-reach_amd"))
from ctr_reach_amd.policy import MlpActor, MlpCritic, polyak_  # noqa: E402

DEVICE = "cuda:0"
TAU = 0.001
SCALE = [0.001, 0.001, 0.001, 0.087, 0.087, 0.087]
CALLS, REPEATS, WARM = 1000, 7, 20
SHAPES = ((64, 64), (128, 128, 128))


def mlp(n_in, hidden, n_out, tanh, seed, grad):
    torch.manual_seed(seed)
    dims = [n_in] + list(hidden)
    mods = []
    for a, b in zip(dims[:-1], dims[1:]):
        mods += [nn.Linear(a, b), nn.ReLU()]
    mods.append(nn.Linear(dims[-1], n_out))
    if tanh:
        mods.append(nn.Tanh())
    net = nn.Sequential(*mods).to(DEVICE)
    for p in net.parameters():
        p.requires_grad_(grad)
    return net


def gpu_round(call):
    """us per update: events around CALLS back-to-back updates."""
    stream = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(CALLS):
        call()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / CALLS


def spread(rounds):
    return {"median_us": round(statistics.median(rounds), 3), "min_us": round(min(rounds), 3),
            "max_us": round(max(rounds), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--only-a", action="store_true", help="CALLS updates of (a) only per cell (for a kernel trace)")
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "calls_per_round": CALLS, "rounds": REPEATS, "tau": TAU, "cases": {}}
    for hidden in SHAPES:
        policy, critic = mlp(19, hidden, 6, True, 1, True), mlp(25, hidden, 1, False, 2, True)
        policy_targ, critic_targ = mlp(19, hidden, 6, True, 3, False), mlp(25, hidden, 1, False, 4, False)
        actor_targ = MlpActor.from_torch(policy_targ, SCALE, DEVICE)
        critic_dev = MlpCritic.from_torch(critic_targ, DEVICE)
        pairs = ((policy, policy_targ), (critic, critic_targ))
        online = [p.detach() for net, _ in pairs for p in net.parameters()]
        target = [p for _, targ in pairs for p in targ.parameters()]
        triples = [(actor_targ, policy, policy_targ), (critic_dev, critic, critic_targ)]

        def way_a():
            polyak_(triples, TAU)

        def way_b():
            with torch.no_grad():
                for net, targ in pairs:
                    for p, pt in zip(net.parameters(), targ.parameters()):
                        pt.lerp_(p, TAU)
            actor_targ.load_(policy_targ)
            critic_dev.load_(critic_targ)

        def way_c():
            with torch.no_grad():
                torch._foreach_lerp_(target, online, TAU)
            actor_targ.load_(policy_targ)
            critic_dev.load_(critic_targ)

        if args.only_a:
            for _ in range(CALLS):
                way_a()
            torch.cuda.synchronize()
            continue
        ways = {"(a) polyak_": way_a, "(b) lerp_ loop + 2 load_": way_b, "(c) _foreach_lerp_ + 2 load_": way_c}
        for call in ways.values():
            for _ in range(WARM):
                call()
        torch.cuda.synchronize()
        rounds = {name: [] for name in ways}
        for _ in range(REPEATS):                          # alternating: the three ways see the same machine
            for name, call in ways.items():
                rounds[name].append(gpu_round(call))
        tag = "[%s]" % ",".join(map(str, hidden))
        case = out["cases"][tag] = {name: spread(r) for name, r in rounds.items()}
        a, b, c = (case[name] for name in ways)
        case["launches"] = {"(a) polyak_": 1, "(b) lerp_ loop + 2 load_": len(target) + 2,
                            "(c) _foreach_lerp_ + 2 load_": "foreach's + 2"}
        case["ratio_b_over_a"] = round(b["median_us"] / a["median_us"], 2)
        case["ratio_c_over_a"] = round(c["median_us"] / a["median_us"], 2)
        case["a_faster_than_b_beyond_spread"] = bool(a["max_us"] < b["min_us"])
        case["a_faster_than_c_beyond_spread"] = bool(a["max_us"] < c["min_us"])
        for name in ways:
            s = case[name]
            print("%-16s %-30s %9.2f us  (%.2f .. %.2f)" % (tag, name, s["median_us"], s["min_us"], s["max_us"]), flush=True)
        print("%-16s (b) / (a) %.2f, beyond the spread: %s;  (c) / (a) %.2f, beyond the spread: %s"
              % (tag, case["ratio_b_over_a"], case["a_faster_than_b_beyond_spread"], case["ratio_c_over_a"],
                 case["a_faster_than_c_beyond_spread"]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
