"""Timing: the part of one learner update that DdpgLearner replaces -- the critic's regression step
and the policy's step, each forward, loss, backward and Adam -- for [64, 64] and [128, 128, 128]
actor + critic pairs on a 13-float observation (rows of 19, critic inputs of 25) at B = 256 and
B = 4096, in three ways
  (a) learner.critic_step(obs, action, target); learner.actor_step(obs): four launches
  (b) as examples/train_ddpg_her.py does it without --device-update: the two losses, backward and
      torch.optim.Adam as constructed there
  (c) (b) with torch.optim.Adam(fused=True), where this torch has it: the cheapest torch-only way
each as the GPU sees it: HIP events around CALLS back-to-back updates on an otherwise idle stream, the
span the stream is held per update, the gaps the host leaves included.  The ways alternate in one
process, REPEATS rounds each after a warm-up; a round's figure is its mean per update, and the
median, lowest and highest round are reported.  (a) "is faster" than another way in a cell when its
highest round lies below the other's lowest.  --only-a makes CALLS updates of (a) and nothing else:
the run to put under rocprofv3 --kernel-trace --stats for the kernels' own times.
usage: python tools/time_update.py [--json PATH] [--only-a]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-ctr-reach_amd"))
from ctr_reach_amd.learner import DdpgLearner  # noqa: E402

DEVICE = "cuda:0"
ACTOR_LR, CRITIC_LR = 1e-4, 1e-3
SCALE = [0.001, 0.001, 0.001, 0.087, 0.087, 0.087]
CALLS, REPEATS, WARM = 1000, 7, 20
SHAPES = ((64, 64), (128, 128, 128))
BATCHES = (256, 4096)


def mlp(n_in, hidden, n_out, tanh, seed, grad):
    torch.manual_seed(seed)
    dims = [n_in] + list(hidden)
    mods = []
    for a, b in zip(dims[:-1], dims[1:]):
        mods += [nn.Linear(a, b), nn.ReLU()]
    mods.append(nn.Linear(dims[-1], n_out))
    if tanh:
        mods.append(nn.Tanh())
    return nn.Sequential(*mods).to(DEVICE).requires_grad_(grad)


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


def torch_way(hidden, obs, action, target, scale, fused):
    """The example's update of the two online networks; None where this torch refuses fused Adam."""
    policy, critic = mlp(19, hidden, 6, True, 1, True), mlp(25, hidden, 1, False, 2, True)
    kw = {"fused": True} if fused else {}
    try:
        policy_opt = torch.optim.Adam(policy.parameters(), lr=ACTOR_LR, **kw)
        critic_opt = torch.optim.Adam(critic.parameters(), lr=CRITIC_LR, **kw)
    except (RuntimeError, TypeError, ValueError):
        return None

    def update():
        critic_loss = F.mse_loss(critic(torch.cat((obs, action / scale), dim=1)).squeeze(1), target)
        critic_opt.zero_grad(set_to_none=True)
        critic_loss.backward()
        critic_opt.step()
        policy_loss = -critic(torch.cat((obs, policy(obs)), dim=1)).mean()
        policy_opt.zero_grad(set_to_none=True)
        policy_loss.backward()
        policy_opt.step()

    return update


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--only-a", action="store_true", help="CALLS updates of (a) only per cell (for a kernel trace)")
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "calls_per_round": CALLS, "rounds": REPEATS, "cases": {}}
    scale = torch.tensor(SCALE, device=DEVICE)
    for hidden in SHAPES:
        for B in BATCHES:
            g = torch.Generator(device="cpu").manual_seed(B)
            obs = (torch.rand((B, 19), generator=g) * 2 - 1).to(DEVICE)
            action = ((torch.rand((B, 6), generator=g) * 2 - 1) * torch.tensor(SCALE)).to(DEVICE)
            target = (torch.rand((B,), generator=g) * 2 - 1).to(DEVICE)
            learner = DdpgLearner(mlp(19, hidden, 6, True, 1, False), mlp(25, hidden, 1, False, 2, False), scale=SCALE,
                                  actor_lr=ACTOR_LR, critic_lr=CRITIC_LR, max_batch=B)

            def way_a():
                learner.critic_step(obs, action, target)
                learner.actor_step(obs)

            if args.only_a:
                for _ in range(CALLS):
                    way_a()
                torch.cuda.synchronize()
                continue
            ways = {"(a) critic_step + actor_step": way_a,
                    "(b) torch autograd + Adam": torch_way(hidden, obs, action, target, scale, False)}
            fused = torch_way(hidden, obs, action, target, scale, True)
            if fused is not None:
                try:
                    fused()
                    torch.cuda.synchronize()
                    ways["(c) torch autograd + Adam(fused=True)"] = fused
                except RuntimeError:
                    fused = None
            for call in ways.values():
                for _ in range(WARM):
                    call()
            torch.cuda.synchronize()
            rounds = {name: [] for name in ways}
            for _ in range(REPEATS):                      # alternating: the ways see the same machine
                for name, call in ways.items():
                    rounds[name].append(gpu_round(call))
            tag = "[%s] B=%d" % (",".join(map(str, hidden)), B)
            case = out["cases"][tag] = {name: spread(r) for name, r in rounds.items()}
            names = list(ways)
            a, b = case[names[0]], case[names[1]]
            case["ratio_b_over_a"] = round(b["median_us"] / a["median_us"], 2)
            case["a_faster_than_b_beyond_spread"] = bool(a["max_us"] < b["min_us"])
            if fused is not None:
                c = case[names[2]]
                case["ratio_c_over_a"] = round(c["median_us"] / a["median_us"], 2)
                case["a_faster_than_c_beyond_spread"] = bool(a["max_us"] < c["min_us"])
            else:
                case["(c) torch autograd + Adam(fused=True)"] = "not available in this torch"
            for name in ways:
                s = case[name]
                print("%-22s %-40s %9.2f us  (%.2f .. %.2f)" % (tag, name, s["median_us"], s["min_us"], s["max_us"]),
                      flush=True)
            print("%-22s (b) / (a) %.2f, beyond the spread: %s;  (c) / (a) %s, beyond the spread: %s"
                  % (tag, case["ratio_b_over_a"], case["a_faster_than_b_beyond_spread"], case.get("ratio_c_over_a", "-"),
                     case.get("a_faster_than_c_beyond_spread", "-")), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
