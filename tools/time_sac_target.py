"""Timing: SAC's batch with its soft target, and the whole SAC update around it, for [64, 64] and
[128, 128, 128] networks on a 13-float observation (rows of 19, critic inputs of 25) at B = 256 and
B = 4 096.

The batch and its target, in two ways
  (a) her.sample_sac(B, pi_dev, critic1_targ, critic2_targ, gamma, learner.log_alpha)
  (b) the target as examples/train_ddpg_her.py's main_sac writes it without --device-targets:
      her.sample(B), pi_dev.sample(next_obs, counter), the two target critics' calls, torch.minimum and
      r + gamma (1 - done) (q - alpha logp) in torch on the device
The whole update, in the same two ways: the target, SacLearner.critic_step, SacLearner.actor_step,
pi_dev.load_(policy) and one polyak_ of the two target critics
each as the GPU sees it: HIP events around CALLS back-to-back calls on an otherwise idle stream, the
span the stream is held per call, the gaps the host leaves included.  The ways alternate in one
process, REPEATS rounds each after a warm-up; a round's figure is its mean per call, and the median,
lowest and highest round are reported.  (a) "is faster" than (b) in a cell when its highest round
lies below (b)'s lowest.  --only-a makes CALLS calls of the target's (a) per cell and nothing else:
the run to put under rocprofv3 --kernel-trace --stats for the kernels' own times.
usage: python tools/time_sac_target.py [--json PATH] [--only-a]"""
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
from ctr_reach_amd.learner import SacLearner  # noqa: E402
from ctr_reach_amd.policy import ExploreNoise, GaussianActor, MlpActor, MlpCritic, polyak_  # noqa: E402

DEVICE = "cuda:0"
GAMMA, SAC_LR, SAC_TAU = 0.99, 3e-4, 0.005
SCALE = [0.001, 0.001, 0.001, 0.087, 0.087, 0.087]
CALLS, REPEATS, WARM = 1000, 7, 20
SHAPES = ((64, 64), (128, 128, 128))
BATCHES = (256, 4096)


def mlp(n_in, hidden, n_out, seed):
    torch.manual_seed(seed)
    dims = [n_in] + list(hidden)
    mods = []
    for a, b in zip(dims[:-1], dims[1:]):
        mods += [nn.Linear(a, b), nn.ReLU()]
    mods.append(nn.Linear(dims[-1], n_out))
    return nn.Sequential(*mods).to(DEVICE).requires_grad_(False)


def store():
    """A 4 096-env store of 10-step episodes, filled by one collect of 40 steps."""
    venv = CtrReachVecEnv(4096, device=DEVICE, seed=0, max_steps_per_episode=10)
    her = venv.enable_her()
    venv.reset()
    torch.manual_seed(5)
    behaviour = nn.Sequential(nn.Linear(19, 32), nn.ReLU(), nn.Linear(32, 6), nn.Tanh()).to(DEVICE).requires_grad_(False)
    venv.collect(MlpActor.from_torch(behaviour, venv.action_space.high, DEVICE), 40, ExploreNoise(0.2, random_eps=0.3, seed=0))
    torch.cuda.synchronize()
    assert len(her) > 0
    return venv, her


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


def spread(rounds):
    return {"median_us": round(statistics.median(rounds), 3), "min_us": round(min(rounds), 3),
            "max_us": round(max(rounds), 3)}


def measure(tag, ways, cases):
    """The ways (the first is (a), the second (b)) alternating; the cell's entry of ``cases``."""
    for call in ways.values():
        for _ in range(WARM):
            call()
    torch.cuda.synchronize()
    rounds = {name: [] for name in ways}
    for _ in range(REPEATS):                              # alternating: the ways see the same machine
        for name, call in ways.items():
            rounds[name].append(gpu_round(call))
    case = cases[tag] = {name: spread(r) for name, r in rounds.items()}
    names = list(ways)
    a, b = case[names[0]], case[names[1]]
    case["ratio_b_over_a"] = round(b["median_us"] / a["median_us"], 2)
    case["a_faster_than_b_beyond_spread"] = bool(a["max_us"] < b["min_us"])
    for name in names:
        s = case[name]
        print("%-26s %-36s %9.2f us  (%.2f .. %.2f)" % (tag, name, s["median_us"], s["min_us"], s["max_us"]), flush=True)
    print("%-26s (b) / (a) %.2f, (a) faster beyond the spread: %s" % (tag, case["ratio_b_over_a"],
                                                                      case["a_faster_than_b_beyond_spread"]), flush=True)


def run(only_a, out):
    venv, her = store()
    out["stored_rows"] = len(her)
    cases = out["cases"]
    for hidden in SHAPES:
        for B in BATCHES:
            policy = mlp(19, hidden, 12, 1)
            critics = [mlp(25, hidden, 1, 2), mlp(25, hidden, 1, 3)]
            targets = [mlp(25, hidden, 1, 2), mlp(25, hidden, 1, 3)]
            learner = SacLearner(policy, critics[0], critics[1], scale=SCALE, actor_lr=SAC_LR, critic_lr=SAC_LR,
                                 alpha_lr=SAC_LR, max_batch=B, seed=0)
            pi_dev = GaussianActor.from_torch(policy, venv.action_space.high, DEVICE, seed=0)
            targets_dev = [MlpCritic.from_torch(t, DEVICE) for t in targets]
            count = [0]

            def target_a():
                return her.sample_sac(B, pi_dev, targets_dev[0], targets_dev[1], GAMMA, learner.log_alpha)

            def target_b():
                batch = her.sample(B)
                nxt = pi_dev.sample(batch["next_obs"], counter=(1 << 40) + count[0])
                count[0] += 1
                q = torch.minimum(targets_dev[0](batch["next_obs"], nxt["unit"]),
                                  targets_dev[1](batch["next_obs"], nxt["unit"]))
                batch["target"] = batch["reward"] + GAMMA * (1.0 - batch["done"]) * (q - learner.alpha * nxt["logp"])
                return batch

            def update(target):
                batch = target()
                learner.critic_step(batch["obs"], batch["action"], batch["target"])
                learner.actor_step(batch["obs"])
                pi_dev.load_(policy)
                polyak_([(targets_dev[0], critics[0], targets[0]), (targets_dev[1], critics[1], targets[1])], SAC_TAU)

            if only_a:
                for _ in range(CALLS):
                    target_a()
                torch.cuda.synchronize()
                continue
            cell = "[%s] B=%d" % (",".join(map(str, hidden)), B)
            measure("target " + cell, {"(a) sample_sac": target_a, "(b) sample + gauss + 2 critics + torch": target_b}, cases)
            measure("update " + cell, {"(a) update on sample_sac": lambda: update(target_a),
                                       "(b) update on the torch target": lambda: update(target_b)}, cases)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--only-a", action="store_true", help="CALLS calls of sample_sac only per cell (for a kernel trace)")
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "calls_per_round": CALLS, "rounds": REPEATS, "cases": {}}
    run(args.only_a, out)
    if args.json and not args.only_a:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
