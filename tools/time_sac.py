"""Timing: one SAC update on a fixed batch, for [64, 64] and [128, 128, 128] networks on a 13-float
observation (rows of 19, critic inputs of 25) at B = 256 and B = 4 096, in two ways
  (a) the device path of examples/train_ddpg_her.py --sac: GaussianActor.sample on next_obs, the two
      target critics (MlpCritic), the target in torch, SacLearner.critic_step and actor_step,
      GaussianActor.load_ and one polyak_ of the two target critics
  (b) a torch float32 SAC update as one would write it: the same target from torch target networks
      and randn_like noise, both critics' MSE under one Adam, the policy's loss under autograd with
      its Adam, the temperature's loss with its Adam, and a lerp_ loop over the target parameters
each as the GPU sees it: HIP events around CALLS back-to-back updates on an otherwise idle stream, the
span the stream is held per update, the gaps the host leaves included.  The ways alternate in one
process, REPEATS rounds each after a warm-up; a round's figure is its mean per update, and the median,
lowest and highest round are reported.  (a) "is faster" than (b) in a cell when its highest round
lies below (b)'s lowest.  The replay draw (her.sample) is the same call in both ways and is left out.
usage: python tools/time_sac.py [--json PATH]"""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-ctr-reach_amd"))
from ctr_reach_amd.learner import SacLearner  # noqa: E402
from ctr_reach_amd.policy import GaussianActor, MlpCritic, polyak_  # noqa: E402

DEVICE = "cuda:0"
GAMMA, TAU, LR, INIT_ALPHA, TARGET_ENTROPY = 0.99, 0.005, 3e-4, 1.0, -6.0
SCALE = [0.001, 0.001, 0.001, 0.087, 0.087, 0.087]
CALLS, REPEATS, WARM = 300, 7, 20
SHAPES = ((64, 64), (128, 128, 128))
BATCHES = (256, 4096)


def mlp(n_in, hidden, n_out, seed, grad=False):
    torch.manual_seed(seed)
    dims = [n_in] + list(hidden)
    mods = []
    for a, b in zip(dims[:-1], dims[1:]):
        mods += [nn.Linear(a, b), nn.ReLU()]
    mods.append(nn.Linear(dims[-1], n_out))
    return nn.Sequential(*mods).to(DEVICE).requires_grad_(grad)


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


def device_way(hidden, B, batch):
    obs, action, reward, next_obs, done = batch
    policy = mlp(19, hidden, 12, 1)
    critics = [mlp(25, hidden, 1, seed) for seed in (2, 3)]
    targets = [mlp(25, hidden, 1, seed) for seed in (2, 3)]
    learner = SacLearner(policy, critics[0], critics[1], scale=SCALE, actor_lr=LR, critic_lr=LR, alpha_lr=LR,
                         init_alpha=INIT_ALPHA, target_entropy=TARGET_ENTROPY, max_batch=B)
    pi_dev = GaussianActor.from_torch(policy, SCALE, DEVICE)
    targets_dev = [MlpCritic.from_torch(t, DEVICE) for t in targets]
    count = [0]

    def update():
        nxt = pi_dev.sample(next_obs, counter=(1 << 40) + count[0])
        count[0] += 1
        q = torch.minimum(targets_dev[0](next_obs, nxt["unit"]), targets_dev[1](next_obs, nxt["unit"]))
        target = reward + GAMMA * (1.0 - done) * (q - learner.alpha * nxt["logp"])
        learner.critic_step(obs, action, target)
        learner.actor_step(obs)
        pi_dev.load_(policy)
        polyak_([(targets_dev[0], critics[0], targets[0]), (targets_dev[1], critics[1], targets[1])], TAU)

    return update


def head(y):
    """The tanh-Gaussian head in torch: (unit action, logp)."""
    mu, s = y[:, :6], y[:, 6:].clamp(-20.0, 2.0)
    eps = torch.randn_like(mu)
    u = mu + s.exp() * eps
    logp = (-0.5 * eps * eps - s - 0.5 * math.log(2 * math.pi)).sum(dim=1) \
        - (2.0 * (math.log(2.0) - u - F.softplus(-2.0 * u))).sum(dim=1)
    return torch.tanh(u), logp


def torch_way(hidden, B, batch):
    obs, action, reward, next_obs, done = batch
    scale = torch.tensor(SCALE, device=DEVICE)
    policy = mlp(19, hidden, 12, 1, grad=True)
    critics = [mlp(25, hidden, 1, seed, grad=True) for seed in (2, 3)]
    targets = [mlp(25, hidden, 1, seed) for seed in (2, 3)]
    log_alpha = torch.tensor(math.log(INIT_ALPHA), device=DEVICE, requires_grad=True)
    policy_opt = torch.optim.Adam(policy.parameters(), lr=LR)
    critic_opt = torch.optim.Adam(list(critics[0].parameters()) + list(critics[1].parameters()), lr=LR)
    alpha_opt = torch.optim.Adam([log_alpha], lr=LR)

    def update():
        with torch.no_grad():
            a, logp = head(policy(next_obs))
            x = torch.cat((next_obs, a), dim=1)
            q = torch.minimum(targets[0](x), targets[1](x)).squeeze(1)
            target = reward + GAMMA * (1.0 - done) * (q - log_alpha.exp() * logp)
        x = torch.cat((obs, action / scale), dim=1)
        critic_loss = F.mse_loss(critics[0](x).squeeze(1), target) + F.mse_loss(critics[1](x).squeeze(1), target)
        critic_opt.zero_grad(set_to_none=True)
        critic_loss.backward()
        critic_opt.step()
        a, logp = head(policy(obs))
        x = torch.cat((obs, a), dim=1)
        policy_loss = (log_alpha.exp().detach() * logp - torch.minimum(critics[0](x), critics[1](x)).squeeze(1)).mean()
        policy_opt.zero_grad(set_to_none=True)
        policy_loss.backward()         # (the critics' gradients from this pass are dropped by their zero_grad)
        policy_opt.step()
        alpha_loss = -(log_alpha * (logp.detach().mean() + TARGET_ENTROPY))
        alpha_opt.zero_grad(set_to_none=True)
        alpha_loss.backward()
        alpha_opt.step()
        with torch.no_grad():
            for net, targ in zip(critics, targets):
                for p, pt in zip(net.parameters(), targ.parameters()):
                    pt.lerp_(p, TAU)

    return update


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "calls_per_round": CALLS, "rounds": REPEATS, "cases": {}}
    for hidden in SHAPES:
        for B in BATCHES:
            g = torch.Generator(device="cpu").manual_seed(B)
            batch = tuple(t.to(DEVICE) for t in (
                torch.rand((B, 19), generator=g) * 2 - 1, (torch.rand((B, 6), generator=g) * 2 - 1) * torch.tensor(SCALE),
                -torch.ones(B), torch.rand((B, 19), generator=g) * 2 - 1, (torch.rand(B, generator=g) < 0.05).float()))
            ways = {"(a) device SAC update": device_way(hidden, B, batch), "(b) torch float32 SAC update": torch_way(hidden, B, batch)}
            for call in ways.values():
                for _ in range(WARM):
                    call()
            torch.cuda.synchronize()
            rounds = {name: [] for name in ways}
            for _ in range(REPEATS):                              # alternating: the ways see the same machine
                for name, call in ways.items():
                    rounds[name].append(gpu_round(call))
            tag = "update [%s] B=%d" % (",".join(map(str, hidden)), B)
            case = out["cases"][tag] = {name: spread(r) for name, r in rounds.items()}
            a, b = (case[name] for name in ways)
            case["ratio_b_over_a"] = round(b["median_us"] / a["median_us"], 2)
            case["a_faster_than_b_beyond_spread"] = bool(a["max_us"] < b["min_us"])
            for name in ways:
                s = case[name]
                print("%-28s %-30s %9.2f us  (%.2f .. %.2f)" % (tag, name, s["median_us"], s["min_us"], s["max_us"]), flush=True)
            print("%-28s (b) / (a) %.2f, (a) faster beyond the spread: %s" % (tag, case["ratio_b_over_a"],
                                                                          case["a_faster_than_b_beyond_spread"]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
