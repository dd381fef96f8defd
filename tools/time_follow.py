"""Timing of waypoint following: microseconds per step over 64-step launches at 65 536 envs on the
headline config (compliant model, scipy RK45, one system) with autoreset=False and an MLP actor
[64, 64], HIP events around 8 back-to-back 64-step calls, best of 3.  One line per process (a fresh
process per line: every line starts from the same reset):
  --line a        rollout(actor, 64)                                   (no goal changes: the baseline)
  --line b        follow(actor, waypoints, hold=8), K = 8              (the goal moves every 8 steps)
  --line b-reach  the same with reach=True                             (... or when the waypoint is reached)
  --line c        follow(..., fused=False)                             (set_goal + act + step_raw per step)
Line a also runs on an older library (CTR_REACH_AMD_LIB naming it): it needs ctr_rollout only.
The waypoints are reachable tips: the reset tips of eight other envs (seeds 101..108).
usage: python tools/time_follow.py --line a|b|b-reach|c [--envs N] [--append PATH] [--tag TEXT]"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-ctr-reach_amd"))
from ctr_reach_amd import CtrReachVecEnv  # noqa: E402
from ctr_reach_amd.policy import MlpActor  # noqa: E402

K, HOLD, STEPS, REPEATS = 8, 8, 64, 3


def make_env(n, seed=0):
    env = CtrReachVecEnv(n, device="cuda:0", seed=seed, record_info=False, autoreset=False)
    env.reset()
    return env


def make_actor(env, hidden=(64, 64), seed=1):
    torch.manual_seed(seed)
    dims = [env.obs_dim + 6] + list(hidden)
    mods = []
    for a, b in zip(dims[:-1], dims[1:]):
        mods += [nn.Linear(a, b), nn.ReLU()]
    mods += [nn.Linear(dims[-1], 6), nn.Tanh()]
    return MlpActor.from_torch(nn.Sequential(*mods), env.action_space.high, "cuda:0")


def timed(call, calls, warm):
    """us per step: best of REPEATS runs of ``calls`` 64-step calls."""
    stream = torch.cuda.current_stream()
    for _ in range(warm):
        call()
    runs = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(calls):
            call()
        e1.record(stream)
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) * 1e3 / (calls * STEPS))
    return {"us_per_step": round(min(runs), 3), "runs": [round(r, 3) for r in runs], "calls": calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--line", required=True, choices=("a", "b", "b-reach", "c"))
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--append", default=None, help="JSON document to add this line's record to")
    ap.add_argument("--tag", default="", help="which library, which process")
    args = ap.parse_args()
    n = args.envs
    env = make_env(n)
    actor = make_actor(env)
    if args.line == "a":
        name = "(a) rollout"
        res = timed(lambda: env.rollout(actor, STEPS), 8, 2)
    else:
        wp = torch.stack([make_env(n, seed=101 + k).achieved_goal.clone() for k in range(K)], dim=1).contiguous()
        if args.line == "c":
            name = "(c) follow, fused=False"
            res = timed(lambda: env.follow(actor, wp, HOLD, fused=False), 2, 1)
        else:
            reach = args.line == "b-reach"
            name = "(b) follow, reach %s" % ("on" if reach else "off")
            res = timed(lambda: env.follow(actor, wp, HOLD, reach=reach), 8, 2)
    res.update(line=name, tag=args.tag)
    print("%-28s %-24s %8.2f us/step   %s" % (name, args.tag, res["us_per_step"], res["runs"]), flush=True)
    if args.append:
        doc = {"device": torch.cuda.get_device_name(0), "envs": n, "steps_per_call": STEPS, "waypoints": K,
               "hold": HOLD, "actor": [64, 64], "repeats": REPEATS, "lines": []}
        if os.path.exists(args.append):
            with open(args.append) as f:
                doc = json.load(f)
        doc["lines"].append(res)
        with open(args.append, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
