"""Timing: 40 DDPG or TD3 updates from one call against the example's eager loop, for [64, 64] and
[128, 128, 128] networks on a 13-float observation (rows of 19, critic inputs of 25) at B = 256 and
B = 4 096, on tools/time_sac_target.py's store.

  (a) learner.update(her, actor_targ, targets, B, gamma, tau, ..., updates=40, actor=actor, history=hist)
      (ctr_ddpg_update; TD3 with policy_delay 2)
  (b) examples/train_ddpg_her.py's loop with --device-update or --td3, 40 times: her.sample_td / sample_td3,
      learner.critic_step, and (TD3: on every second update) learner.actor_step and polyak_ of the two or
      three targets, with the example's accumulation of the losses in torch, and the iteration's one
      actor.load_(policy) at the end.  The library leaves those calls as they were, so (b) is the parent's
      behaviour.
each measured twice per round: as the GPU sees it (HIP events around the 40 updates on an otherwise
idle stream, the gaps the host leaves included) and as the host sees it (a clock from the first call to
the end of torch.cuda.synchronize()).  The ways alternate in one process, REPEATS rounds each after WARM
warm-up rounds; figures are per update (a round's time / 40), and the median, lowest and highest round
are reported.  (a) "is faster" than (b) in a cell when its highest round lies below (b)'s lowest.
--only-a makes ROUNDS_A calls of (a) per cell and nothing else: the run to put under rocprofv3
--kernel-trace --stats for the launch count and the kernels' own times; --only-b the same of (b), for
the replaced kernels' times beside them.  --cell I restricts a run to cell I (0..7, in the order printed),
so that a trace can be split by cell.
usage: python tools/time_ddpg_update.py [--json PATH] [--only-a | --only-b] [--cell I]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-ctr-reach_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ctr_reach_amd.learner import DdpgLearner, Td3Learner  # noqa: E402
from ctr_reach_amd.policy import MlpActor, MlpCritic, polyak_  # noqa: E402
from time_sac_target import BATCHES, DEVICE, GAMMA, SCALE, SHAPES, mlp, store  # noqa: E402
from time_sac_update import measure  # noqa: E402

import torch.nn as nn  # noqa: E402

UPDATES, ROUNDS_A = 40, 5
TAU, ACTOR_LR, CRITIC_LR = 0.001, 1e-4, 1e-3                    # the example's
SIGMA, CLIP, DELAY = 0.2, 0.5, 2


def tanh_mlp(n_in, hidden, seed):
    return nn.Sequential(*list(mlp(n_in, hidden, 6, seed)), nn.Tanh())


def world(venv, hidden, B, td3):
    policy, policy_targ = tanh_mlp(19, hidden, 1), tanh_mlp(19, hidden, 1)
    n = 2 if td3 else 1
    critics = [mlp(25, hidden, 1, 2 + y) for y in range(n)]
    targets = [mlp(25, hidden, 1, 2 + y) for y in range(n)]
    if td3:
        learner = Td3Learner(policy, critics[0], critics[1], scale=SCALE, actor_lr=ACTOR_LR, critic_lr=CRITIC_LR, max_batch=B)
    else:
        learner = DdpgLearner(policy, critics[0], scale=SCALE, actor_lr=ACTOR_LR, critic_lr=CRITIC_LR, max_batch=B)
    high = venv.action_space.high
    actor, actor_targ = MlpActor.from_torch(policy, high, DEVICE), MlpActor.from_torch(policy_targ, high, DEVICE)
    targets_dev = [MlpCritic.from_torch(t, DEVICE) for t in targets]
    return policy, policy_targ, critics, targets, learner, actor, actor_targ, targets_dev


def run(only, cell_only, out):
    venv, her = store()
    out["stored_rows"] = len(her)
    index = -1
    for td3 in (False, True):
        for hidden in SHAPES:
            for B in BATCHES:
                index += 1
                if cell_only is not None and index != cell_only:
                    continue
                policy, policy_targ, critics, targets, learner, actor, actor_targ, targets_dev = world(venv, hidden, B, td3)
                pairs = [(actor_targ, policy_targ)] + list(zip(targets_dev, targets))
                triples = [(net, online, targ) for (net, targ), online in zip(pairs, [policy] + critics)]
                hist = torch.zeros((UPDATES, 3 if td3 else 2), dtype=torch.float32, device=DEVICE)
                state = {"updates": 0}

                def way_a():
                    if td3:
                        learner.update(her, actor_targ, pairs, B, GAMMA, TAU, SIGMA, CLIP, DELAY, updates=UPDATES, actor=actor,
                                       history=hist)
                    else:
                        learner.update(her, actor_targ, pairs, B, GAMMA, TAU, updates=UPDATES, actor=actor, history=hist)

                def way_b():
                    critic_sum = torch.zeros((), device=DEVICE)
                    policy_sum = torch.zeros((), device=DEVICE)
                    for _ in range(UPDATES):
                        if td3:
                            batch = her.sample_td3(B, actor_targ, targets_dev[0], targets_dev[1], GAMMA, SIGMA, CLIP)
                            learner.critic_step(batch["obs"], batch["action"], batch["target"])
                            critic_sum += learner.critic_loss.mean()
                            state["updates"] += 1
                            if state["updates"] % DELAY == 0:
                                learner.actor_step(batch["obs"])
                                polyak_(triples, TAU)
                                policy_sum += learner.actor_loss
                            continue
                        batch = her.sample_td(B, actor_targ, targets_dev[0], GAMMA)
                        learner.critic_step(batch["obs"], batch["action"], batch["target"])
                        learner.actor_step(batch["obs"])
                        polyak_(triples, TAU)
                        critic_sum += learner.critic_loss
                        policy_sum += learner.actor_loss
                    actor.load_(policy)

                cell = "%s [%s] B=%d" % ("TD3" if td3 else "DDPG", ",".join(map(str, hidden)), B)
                if only:
                    print("cell %d: %s, %d rounds of (%s)" % (index, cell, ROUNDS_A, only), flush=True)
                    for _ in range(ROUNDS_A):
                        (way_a if only == "a" else way_b)()
                    torch.cuda.synchronize()
                    continue
                measure(cell, {"(a) one update call": way_a, "(b) the eager loop": way_b}, out["cases"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--only-a", action="store_true", help="ROUNDS_A calls of (a) only per cell (for a kernel trace)")
    ap.add_argument("--only-b", action="store_true", help="ROUNDS_A rounds of (b) only per cell (for a kernel trace)")
    ap.add_argument("--cell", type=int, default=None, help="only cell I of the eight (for a trace split by cell)")
    args = ap.parse_args()
    only = "a" if args.only_a else ("b" if args.only_b else None)
    from time_sac_update import REPEATS
    out = {"device": torch.cuda.get_device_name(0), "updates_per_round": UPDATES, "rounds": REPEATS, "cases": {}}
    run(only, args.cell, out)
    if args.json and not only:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
