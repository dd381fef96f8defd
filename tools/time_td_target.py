"""Timing: one learner update's batch and DDPG target, B = 256 and 4 096, target networks [64, 64] and
[128, 128, 128] on a 13-float observation (rows of 19, critic inputs of 25), in two ways
  (a) her.sample_td(B, actor_targ, critic_targ, gamma) and the two load_ of the targets
      (ctr_her_sample_td: the sampler's two scans and one kernel; ctr_actor_load, ctr_critic_load)
  (b) her.sample(B) and the torch float32 target networks and target arithmetic, as
      examples/train_ddpg_her.py does it without --device-targets: cat, the target policy, cat, the
      target critic, r + gamma (1 - done) q
each as the GPU sees it: HIP events around CALLS back-to-back updates on an otherwise idle stream, the
span the stream is held per update, the gaps the host leaves included.  The two ways alternate in
one process, REPEATS rounds each after a warm-up; a round's figure is its mean per update, and the
median, lowest and highest round are reported.  (a) "is faster" in a cell when its highest round
lies below (b)'s lowest.  --only-a makes CALLS updates of (a) and nothing else: the run to put under
rocprofv3 --kernel-trace --stats for the kernels' own time.
usage: python tools/time_td_target.py [--json PATH] [--only-a]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-ctr-reach_amd"))
from ctr_reach_amd import CtrReachVecEnv  # noqa: E402
from ctr_reach_amd.policy import ExploreNoise, MlpActor, MlpCritic  # noqa: E402

DEVICE = "cuda:0"
GAMMA = 0.99
CALLS, REPEATS, WARM = 1000, 7, 20
BATCHES = (256, 4096)
SHAPES = ((64, 64), (128, 128, 128))


def mlp(n_in, hidden, n_out, tanh, seed):
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
        p.requires_grad_(False)
    return net


def store():
    """A 4 096-env store of 10-step episodes, filled by one collect of 40 steps."""
    venv = CtrReachVecEnv(4096, device=DEVICE, seed=0, max_steps_per_episode=10)
    her = venv.enable_her()
    venv.reset()
    behaviour = MlpActor.from_torch(mlp(19, (32,), 6, True, 5), venv.action_space.high, DEVICE)
    venv.collect(behaviour, 40, ExploreNoise(0.2, random_eps=0.3, seed=0))
    torch.cuda.synchronize()
    assert len(her) > 0
    return venv, her


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
    venv, her = store()
    out = {"device": torch.cuda.get_device_name(0), "calls_per_round": CALLS, "rounds": REPEATS,
           "stored_rows": len(her), "cases": {}}
    for hidden in SHAPES:
        policy_targ, critic_targ = mlp(19, hidden, 6, True, 1), mlp(25, hidden, 1, False, 2)
        actor_targ = MlpActor.from_torch(policy_targ, venv.action_space.high, DEVICE)
        critic_dev = MlpCritic.from_torch(critic_targ, DEVICE)
        for B in BATCHES:
            def way_a():
                batch = her.sample_td(B, actor_targ, critic_dev, GAMMA)
                actor_targ.load_(policy_targ)
                critic_dev.load_(critic_targ)
                return batch["target"]

            def way_b():
                batch = her.sample(B)
                next_obs = batch["next_obs"]
                with torch.no_grad():
                    q_next = critic_targ(torch.cat((next_obs, policy_targ(next_obs)), dim=1)).squeeze(1)
                    return batch["reward"] + GAMMA * (1.0 - batch["done"]) * q_next

            if args.only_a:
                for _ in range(CALLS):
                    way_a()
                torch.cuda.synchronize()
                continue
            ways = {"(a) sample_td + 2 load_": way_a, "(b) sample + torch targets": way_b}
            for call in ways.values():
                for _ in range(WARM):
                    call()
            torch.cuda.synchronize()
            rounds = {name: [] for name in ways}
            for _ in range(REPEATS):                      # alternating: both ways see the same machine
                for name, call in ways.items():
                    rounds[name].append(gpu_round(call))
            tag = "B=%d [%s]" % (B, ",".join(map(str, hidden)))
            case = out["cases"][tag] = {name: spread(r) for name, r in rounds.items()}
            a, b = (case[name] for name in ways)
            case["ratio_b_over_a"] = round(b["median_us"] / a["median_us"], 2)
            case["a_faster_beyond_spread"] = bool(a["max_us"] < b["min_us"])
            for name in ways:
                s = case[name]
                print("%-24s %-28s %9.2f us  (%.2f .. %.2f)" % (tag, name, s["median_us"], s["min_us"], s["max_us"]), flush=True)
            print("%-24s (b) / (a) %.2f, (a) faster beyond the spread: %s" % (tag, case["ratio_b_over_a"],
                                                                              case["a_faster_beyond_spread"]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
