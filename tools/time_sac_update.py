"""Timing: 40 SAC updates from one call against the five-call loop, for [64, 64] and [128, 128, 128]
networks on a 13-float observation (rows of 19, critic inputs of 25) at B = 256 and B = 4 096, on
tools/time_sac_target.py's store.

  (a) learner.update(her, pi_dev, targets, B, gamma, tau, updates=40, history=hist)       (ctr_sac_update)
  (b) examples/train_ddpg_her.py's loop with --sac --device-targets, 40 times: her.sample_sac,
      learner.critic_step, learner.actor_step, pi_dev.load_(policy), polyak_ of the two target critics, and
      the example's accumulation of the two losses in torch
each measured twice per round: as the GPU sees it (HIP events around the 40 updates on an otherwise
idle stream, the gaps the host leaves included) and as the host sees it (a clock from the first call to
the end of torch.cuda.synchronize()).  The ways alternate in one process, REPEATS rounds each after a
warm-up; figures are per update (a round's time / 40), and the median, lowest and highest round are
reported.  (a) "is faster" than (b) in a cell when its highest round lies below (b)'s lowest.
--only-a makes ROUNDS_A calls of (a) per cell and nothing else: the run to put under rocprofv3
--kernel-trace --stats for the launch count and the kernels' own times; --only-b the same of (b), for
the replaced kernels' times beside them.
usage: python tools/time_sac_update.py [--json PATH] [--only-a | --only-b]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-ctr-reach_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ctr_reach_amd.learner import SacLearner  # noqa: E402
from ctr_reach_amd.policy import GaussianActor, MlpCritic, polyak_  # noqa: E402
from time_sac_target import BATCHES, DEVICE, GAMMA, SAC_LR, SAC_TAU, SCALE, SHAPES, mlp, store  # noqa: E402

UPDATES, REPEATS, WARM, ROUNDS_A = 40, 15, 3, 5


def world(venv, hidden, B):
    policy = mlp(19, hidden, 12, 1)
    critics = [mlp(25, hidden, 1, 2), mlp(25, hidden, 1, 3)]
    targets = [mlp(25, hidden, 1, 2), mlp(25, hidden, 1, 3)]
    learner = SacLearner(policy, critics[0], critics[1], scale=SCALE, actor_lr=SAC_LR, critic_lr=SAC_LR, alpha_lr=SAC_LR,
                         max_batch=B, seed=0)
    pi_dev = GaussianActor.from_torch(policy, venv.action_space.high, DEVICE, seed=0)
    targets_dev = [MlpCritic.from_torch(t, DEVICE) for t in targets]
    return policy, critics, targets, learner, pi_dev, targets_dev


def one_round(call):
    """(GPU us, host us) per update of one round of UPDATES updates."""
    stream = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record(stream)
    call()
    e1.record(stream)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    return e0.elapsed_time(e1) * 1e3 / UPDATES, (t1 - t0) * 1e6 / UPDATES


def spread(rounds):
    return {"median_us": round(statistics.median(rounds), 3), "min_us": round(min(rounds), 3),
            "max_us": round(max(rounds), 3)}


def measure(tag, ways, cases):
    for call in ways.values():
        for _ in range(WARM):
            call()
    torch.cuda.synchronize()
    rounds = {name: ([], []) for name in ways}
    for _ in range(REPEATS):                              # alternating: the ways see the same machine
        for name, call in ways.items():
            gpu, host = one_round(call)
            rounds[name][0].append(gpu)
            rounds[name][1].append(host)
    case = cases[tag] = {name: {"gpu": spread(r[0]), "host": spread(r[1])} for name, r in rounds.items()}
    a, b = (case[name] for name in ways)
    for clock in ("gpu", "host"):
        case["ratio_b_over_a_" + clock] = round(b[clock]["median_us"] / a[clock]["median_us"], 2)
        case["a_faster_than_b_beyond_spread_" + clock] = bool(a[clock]["max_us"] < b[clock]["min_us"])
    for name in ways:
        g, h = case[name]["gpu"], case[name]["host"]
        print("%-22s %-24s GPU %8.2f us (%.2f .. %.2f)   host %8.2f us (%.2f .. %.2f)  per update"
              % (tag, name, g["median_us"], g["min_us"], g["max_us"], h["median_us"], h["min_us"], h["max_us"]), flush=True)
    print("%-22s (b) / (a): GPU %.2f, host %.2f; (a) faster beyond the spread: GPU %s, host %s"
          % (tag, case["ratio_b_over_a_gpu"], case["ratio_b_over_a_host"], case["a_faster_than_b_beyond_spread_gpu"],
             case["a_faster_than_b_beyond_spread_host"]), flush=True)


def run(only, out):
    venv, her = store()
    out["stored_rows"] = len(her)
    for hidden in SHAPES:
        for B in BATCHES:
            policy, critics, targets, learner, pi_dev, targets_dev = world(venv, hidden, B)
            pairs = list(zip(targets_dev, targets))
            hist = torch.zeros((UPDATES, 5), dtype=torch.float32, device=DEVICE)

            def way_a():
                learner.update(her, pi_dev, pairs, B, GAMMA, SAC_TAU, updates=UPDATES, history=hist)

            def way_b():
                critic_sum = torch.zeros((), device=DEVICE)
                policy_sum = torch.zeros((), device=DEVICE)
                for _ in range(UPDATES):
                    batch = her.sample_sac(B, pi_dev, targets_dev[0], targets_dev[1], GAMMA, learner.log_alpha)
                    learner.critic_step(batch["obs"], batch["action"], batch["target"])
                    learner.actor_step(batch["obs"])
                    pi_dev.load_(policy)
                    polyak_([(targets_dev[0], critics[0], targets[0]), (targets_dev[1], critics[1], targets[1])], SAC_TAU)
                    critic_sum += learner.critic_loss.mean()
                    policy_sum += learner.actor_loss

            if only:
                for _ in range(ROUNDS_A):
                    (way_a if only == "a" else way_b)()
                torch.cuda.synchronize()
                continue
            cell = "[%s] B=%d" % (",".join(map(str, hidden)), B)
            measure(cell, {"(a) one update call": way_a, "(b) the five-call loop": way_b}, out["cases"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--only-a", action="store_true", help="ROUNDS_A calls of (a) only per cell (for a kernel trace)")
    ap.add_argument("--only-b", action="store_true", help="ROUNDS_A rounds of (b) only per cell (for a kernel trace)")
    args = ap.parse_args()
    only = "a" if args.only_a else ("b" if args.only_b else None)
    out = {"device": torch.cuda.get_device_name(0), "updates_per_round": UPDATES, "rounds": REPEATS, "cases": {}}
    run(only, out)
    if args.json and not only:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
