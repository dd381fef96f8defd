"""DDPG + HER on CtrReachVecEnv: the loop the device-side pieces were built for, small and readable
(not a tuned trainer).

Every iteration
  1. collects ``steps_per_iter`` steps of every env with the current policy and exploration noise,
     recorded into the HER store: ``venv.collect(actor, steps, noise)``, one launch per refill period;
  2. draws relabelled batches on the device: ``her.sample(batch_size)``;
  3. makes the DDPG critic and actor updates in torch on them, and the Polyak update of the targets;
  4. refreshes the kernels' copy of the policy from the learner's parameters: ``actor.load_(policy)``,
     one launch, no copy to the host.
Everything is ordered on one stream and nothing is read back inside an iteration; the losses are
read once at its end.

The policy is ``Linear, ReLU, ..., Linear, Tanh`` (what ``MlpActor.from_torch`` takes) on
HERGoalEnvWrapper's flat row, and the action is ``scale * policy(row)`` with ``scale`` the action
space's high, so the critic sees actions in [-1, 1].  HER follows the reference's config
(ctr_reach_amd/her.py): strategy ``future``, ``n_sampled_goal`` 4, batch 256.  The learning rates,
``tau`` and ``gamma`` are stable-baselines DDPG's defaults; the noise is this example's choice.

The first episodes are cut short at random (the envs start with clocks spread over the time limit):
episodes enter the store when they end, so otherwise it would stay empty for a whole time limit and
then fill in bursts.  While the store is empty ``sample`` returns zero rows, which teach nothing and
harm nothing.

With ``--device-targets`` (``main(..., device_targets=True)``) step 2 also makes the DDPG target on
the device: an ``MlpActor`` for the target policy and an ``MlpCritic`` for the target critic are built
once, ``her.sample_td(batch_size, actor_targ, critic_targ, gamma)`` returns the batch with ``target``
in one launch, and after each Polyak update both blobs are refreshed with ``load_``.  The torch
target networks stay the owners of the float32 parameters; the blobs are their bf16 view, so the
targets then come from bf16 weights and activations (ctr_reach_amd/policy.py, ``emulate``) instead
of torch's float32 arithmetic.

With ``--device-polyak`` (``main(..., device_polyak=True)``, which implies the device targets) the
Polyak update moves to the device as well: the per-parameter ``lerp_`` loop and the two ``load_``
become one ``polyak_`` call, one launch that updates the float32 target parameters in place and
repacks both blobs from them.  The torch target modules still own those parameters, so their
``state_dict()`` is what it was.

With ``--device-update`` (``main(..., device_update=True)``, which implies ``--device-polyak``) step 3
leaves torch as well: the online networks are built with ``requires_grad_(False)`` and no torch
optimiser, and a ``DdpgLearner`` (ctr_reach_amd/learner.py) makes the critic's step (forward, MSE
against ``target``, backward, Adam) and the policy's step (policy forward, critic forward, backward
through both, Adam), two launches each, in float32 on those parameters in place.  An update is then
``sample_td``, ``critic_step``, ``actor_step`` and ``polyak_``, none of it autograd; the action is
divided by ``scale`` inside ``critic_step``.  The modules still own the parameters.

With ``--td3`` (``main(..., td3=True)``, which implies ``--device-update``) the same loop trains TD3
(Fujimoto et al. 2018) instead of DDPG: a second critic with its target and its ``MlpCritic``, the
target from the smaller of the two target critics on a noise-smoothed target action
(``her.sample_td3(batch_size, actor_targ, critic_targ_dev, critic2_targ_dev, gamma, TARGET_NOISE,
NOISE_CLIP)``, still one launch behind the sampler's scans), both critics regressed on it by one
``Td3Learner.critic_step`` (two launches), and on every ``POLICY_DELAY``-th update the policy's step
under critic 1 and one ``polyak_`` of the three target networks.  ``TARGET_NOISE`` 0.2, ``NOISE_CLIP``
0.5 and ``POLICY_DELAY`` 2 are TD3's published defaults and stable-baselines'.  The critic loss
reported is the mean of the two critics'.

With ``--sac`` (``main(..., sac=True)``; an error together with ``--td3``, and it implies nothing of the
DDPG path) the loop trains SAC (Haarnoja et al. 2018, with the learned temperature) instead: a policy
with a 12-row head (six means, six log standard deviations, no Tanh) as a ``GaussianActor`` ``pi_dev``,
two critics with their targets (``MlpCritic`` blobs) and no target policy.  Collection is per step
``venv.step(pi_dev.sample(venv.actor_rows(), counter=step, row_base=venv.env_base)["action"])`` with the
fused HER feed, two launches a step: the policy's own noise explores.  An update is ``her.sample``, the
next action and its log-probability from ``pi_dev.sample(next_obs, counter)``, the two target critics on
it, ``target = r + gamma (1 - done) (min(Q1', Q2') - alpha logp')`` in torch on the device,
``SacLearner.critic_step`` (``Td3Learner``'s), ``SacLearner.actor_step`` (the policy's step under both
critics and the temperature's), ``pi_dev.load_(policy)`` and one ``polyak_`` of the two target critics.
``SAC_LR`` 3e-4, ``SAC_TAU`` 0.005, ``init_alpha`` 1 and ``target_entropy`` -6 are stable-baselines SAC's
defaults with ``ent_coef='auto'``.  ``pi_dev.mean_actor()`` gives the trained policy's deterministic mean
to ``venv.rollout`` / ``follow`` for evaluation.

With ``--sac --device-targets`` (``main(..., sac=True, device_targets=True)``) the first four of those
steps are one call: ``her.sample_sac(batch_size, pi_dev, targets_dev[0], targets_dev[1], GAMMA,
learner.log_alpha)`` returns the batch with ``target``, made in the sampler's launch from the current
policy's sample on ``next_obs``, the two target critics and the temperature read on the device.  The
noise is keyed by the replay draw itself, whose seed is not the collection's, so no counter offset is
needed.

With ``--sac --device-collect`` (``main(..., sac=True, device_collect=True)``; a ValueError without
``--sac``, whose exploration alone is the policy's own sample) the per-step collection loop becomes one
call, ``venv.collect_gauss(pi_dev, steps_per_iter, counter=step)``: the policy's stochastic head runs
inside the fused period kernel, one launch per refill period instead of two per step, with the same
draws (step ``j`` of the call under ``counter + j``, an env's noise row its global id), so the envs and
the HER store are what the per-step loop leaves, bit for bit.  With ``--device-targets`` as well an
iteration is then one launch per refill period on the env side and four calls per update.

With ``--sac --update-call`` (``main(..., sac=True, update_call=True)``; a ValueError without ``--sac``; it
implies ``--device-targets``) the iteration's whole inner loop is one call,
``learner.update(her, pi_dev, [(targets_dev[0], targets[0]), (targets_dev[1], targets[1])], batch_size, GAMMA,
SAC_TAU, updates=updates_per_iter, history=hist)`` (ctr_sac_update): the same updates bit for bit, five
launches each instead of nine, the sampler's scans once per iteration, and no host work between the
updates.  The iteration's losses come from ``hist`` ([updates, 5]: the two critic losses, the policy's
loss, logp_mean, log_alpha per update) in the iteration's one host read.

With ``--update-run`` (``main(..., update_run=True)``; DDPG and ``--td3``; it implies ``--device-update``; a
ValueError with ``--sac``, whose flag is ``--update-call``) the inner loop of DDPG or TD3 is one call as well,
``learner.update(her, actor_targ, [(actor_targ, policy_targ), (critic_targ_dev, critic_targ), ...], batch_size,
GAMMA, TAU, updates=updates_per_iter, actor=actor, history=hist)`` (ctr_ddpg_update; TD3 also passes
``TARGET_NOISE``, ``NOISE_CLIP`` and ``POLICY_DELAY``): the same updates bit for bit, five launches for an
update with a policy step and three for one without, the sampler's scans once per iteration, no ``polyak_``
and no ``actor.load_`` (``actor``'s blob is repacked by every policy step).  The iteration's losses come from
``hist`` ([updates, 2] or [updates, 3]: the critic losses, then the actor loss of the updates that made a
policy step).

usage: python examples/train_ddpg_her.py [--num-envs N] [--iterations I] [--steps-per-iter S]
           [--batch-size B] [--updates-per-iter U] [--hidden 64,64] [--seed 0] [--device cuda]
           [--device-targets] [--device-polyak] [--device-update] [--td3] [--sac] [--device-collect] [--update-call]
           [--update-run]"""
import argparse
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-ctr-reach_amd"))
from ctr_reach_amd import CtrReachVecEnv  # noqa: E402
from ctr_reach_amd.learner import DdpgLearner, SacLearner, Td3Learner  # noqa: E402
from ctr_reach_amd.policy import ExploreNoise, GaussianActor, MlpActor, MlpCritic, polyak_  # noqa: E402

GAMMA, TAU, ACTOR_LR, CRITIC_LR = 0.99, 0.001, 1e-4, 1e-3
N_SAMPLED_GOAL, STRATEGY = 4, "future"
SIGMA, RANDOM_EPS = 0.2, 0.3
TARGET_NOISE, NOISE_CLIP, POLICY_DELAY = 0.2, 0.5, 2                         # TD3 (--td3)
SAC_LR, SAC_TAU, INIT_ALPHA, TARGET_ENTROPY = 3e-4, 0.005, 1.0, -6.0          # SAC (--sac)


def mlp(n_in, hidden, n_out, tanh):
    dims = [n_in] + list(hidden)
    mods = []
    for a, b in zip(dims[:-1], dims[1:]):
        mods += [nn.Linear(a, b), nn.ReLU()]
    mods.append(nn.Linear(dims[-1], n_out))
    if tanh:
        mods.append(nn.Tanh())
    return nn.Sequential(*mods)


def main(num_envs=4096, iterations=50, steps_per_iter=20, batch_size=256, updates_per_iter=40, hidden=(64, 64), seed=0,
         device="cuda", device_targets=False, device_polyak=False, device_update=False, td3=False, sac=False,
         device_collect=False, update_call=False, update_run=False):
    if sac and td3:
        raise ValueError("--sac and --td3 are two algorithms: choose one")
    if device_collect and not sac:
        raise ValueError("--device-collect is SAC's collection (venv.collect_gauss): use it with --sac")
    if update_call and not sac:
        raise ValueError("--update-call is SAC's update (SacLearner.update): use it with --sac")
    if update_run and sac:
        raise ValueError("--update-run is DDPG's and TD3's update (DdpgLearner.update, Td3Learner.update): SAC's is "
                         "--update-call")
    if sac:
        return main_sac(num_envs, iterations, steps_per_iter, batch_size, updates_per_iter, hidden, seed, device,
                        device_targets or update_call, device_collect, update_call)
    device = torch.device(device)
    device_update = device_update or td3 or update_run
    device_polyak = device_polyak or device_update
    device_targets = device_targets or device_polyak
    torch.manual_seed(seed)
    venv = CtrReachVecEnv(num_envs, device=device, seed=seed)
    her = venv.enable_her(n_sampled_goal=N_SAMPLED_GOAL, goal_selection_strategy=STRATEGY)
    venv.reset()
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    venv.t.copy_(torch.randint(0, venv.max_steps_per_episode, (num_envs,), generator=g, dtype=torch.int32))

    d = venv.obs_dim + 6
    scale = torch.tensor(venv.action_space.high, dtype=torch.float32, device=device)
    policy, critic = mlp(d, hidden, 6, True).to(device), mlp(d + 6, hidden, 1, False).to(device)
    policy_targ, critic_targ = mlp(d, hidden, 6, True).to(device), mlp(d + 6, hidden, 1, False).to(device)
    policy_targ.load_state_dict(policy.state_dict())
    critic_targ.load_state_dict(critic.state_dict())
    for p in list(policy_targ.parameters()) + list(critic_targ.parameters()):
        p.requires_grad_(False)
    critic2 = critic2_targ = critic2_targ_dev = None
    if td3:                                                                  # the twin critic and its target
        critic2 = mlp(d + 6, hidden, 1, False).to(device).requires_grad_(False)
        critic2_targ = mlp(d + 6, hidden, 1, False).to(device).requires_grad_(False)
        critic2_targ.load_state_dict(critic2.state_dict())
    learner = None
    if td3:
        policy.requires_grad_(False)
        critic.requires_grad_(False)
        learner = Td3Learner(policy, critic, critic2, scale=venv.action_space.high, actor_lr=ACTOR_LR, critic_lr=CRITIC_LR,
                             max_batch=batch_size)
    elif device_update:                                                        # the masters are written by the kernels
        policy.requires_grad_(False)
        critic.requires_grad_(False)
        learner = DdpgLearner(policy, critic, scale=venv.action_space.high, actor_lr=ACTOR_LR, critic_lr=CRITIC_LR,
                              max_batch=batch_size)
    else:
        policy_opt = torch.optim.Adam(policy.parameters(), lr=ACTOR_LR)
        critic_opt = torch.optim.Adam(critic.parameters(), lr=CRITIC_LR)

    actor = MlpActor.from_torch(policy, venv.action_space.high, device)      # once; load_ from here on
    noise = ExploreNoise(SIGMA, random_eps=RANDOM_EPS, seed=seed)
    actor_targ = critic_targ_dev = None
    if device_targets:                                                       # the targets' bf16 view, once
        actor_targ = MlpActor.from_torch(policy_targ, venv.action_space.high, device)
        critic_targ_dev = MlpCritic.from_torch(critic_targ, device)
    if td3:
        critic2_targ_dev = MlpCritic.from_torch(critic2_targ, device)
    losses = []
    updates = 0
    hist = torch.zeros((updates_per_iter, 3 if td3 else 2), dtype=torch.float32, device=device) if update_run else None
    for it in range(iterations):
        venv.collect(actor, steps_per_iter, noise)
        if update_run:                                                       # the iteration's updates: one call
            if td3:
                first = -(learner.update_count + 1) % POLICY_DELAY           # the first update with a policy step
                learner.update(her, actor_targ, [(actor_targ, policy_targ), (critic_targ_dev, critic_targ),
                                                 (critic2_targ_dev, critic2_targ)], batch_size, GAMMA, TAU, TARGET_NOISE,
                               NOISE_CLIP, POLICY_DELAY, updates=updates_per_iter, actor=actor, history=hist)
                stepped = hist[first::POLICY_DELAY, 2]
                # the iteration's only host read
                c, p = torch.stack((0.5 * hist[:, :2].sum(), stepped.sum())).tolist()
                losses.append((c / max(updates_per_iter, 1), p / max(stepped.numel(), 1)))
            else:
                learner.update(her, actor_targ, [(actor_targ, policy_targ), (critic_targ_dev, critic_targ)], batch_size,
                               GAMMA, TAU, updates=updates_per_iter, actor=actor, history=hist)
                h = hist.sum(0).tolist()                                     # the iteration's only host read
                losses.append((h[0] / max(updates_per_iter, 1), h[1] / max(updates_per_iter, 1)))
            continue
        critic_sum = torch.zeros((), device=device)
        policy_sum = torch.zeros((), device=device)
        policy_updates = 0
        for _ in range(updates_per_iter):
            if td3:                                                          # sample_td3, the twin step; every 2nd: the rest
                batch = her.sample_td3(batch_size, actor_targ, critic_targ_dev, critic2_targ_dev, GAMMA, TARGET_NOISE,
                                       NOISE_CLIP)
                learner.critic_step(batch["obs"], batch["action"], batch["target"])
                critic_sum += learner.critic_loss.mean()
                updates += 1
                if updates % POLICY_DELAY == 0:
                    learner.actor_step(batch["obs"])
                    polyak_([(actor_targ, policy, policy_targ), (critic_targ_dev, critic, critic_targ),
                             (critic2_targ_dev, critic2, critic2_targ)], TAU)
                    policy_sum += learner.actor_loss
                    policy_updates += 1
                continue
            if device_update:                                                # sample_td, two steps, polyak_: no autograd
                batch = her.sample_td(batch_size, actor_targ, critic_targ_dev, GAMMA)
                learner.critic_step(batch["obs"], batch["action"], batch["target"])
                learner.actor_step(batch["obs"])
                polyak_([(actor_targ, policy, policy_targ), (critic_targ_dev, critic, critic_targ)], TAU)
                critic_sum += learner.critic_loss
                policy_sum += learner.actor_loss
                continue
            if device_targets:
                batch = her.sample_td(batch_size, actor_targ, critic_targ_dev, GAMMA)
                obs, target = batch["obs"], batch["target"]
            else:
                batch = her.sample(batch_size)
                obs, next_obs = batch["obs"], batch["next_obs"]
                with torch.no_grad():
                    q_next = critic_targ(torch.cat((next_obs, policy_targ(next_obs)), dim=1)).squeeze(1)
                    target = batch["reward"] + GAMMA * (1.0 - batch["done"]) * q_next
            critic_loss = F.mse_loss(critic(torch.cat((obs, batch["action"] / scale), dim=1)).squeeze(1), target)
            critic_opt.zero_grad(set_to_none=True)
            critic_loss.backward()
            critic_opt.step()
            policy_loss = -critic(torch.cat((obs, policy(obs)), dim=1)).mean()
            policy_opt.zero_grad(set_to_none=True)
            policy_loss.backward()         # (the critic's gradients from this pass are dropped by its zero_grad)
            policy_opt.step()
            if device_polyak:                                                # the update and both blobs: one launch
                polyak_([(actor_targ, policy, policy_targ), (critic_targ_dev, critic, critic_targ)], TAU)
            else:
                with torch.no_grad():
                    for net, targ in ((policy, policy_targ), (critic, critic_targ)):
                        for p, pt in zip(net.parameters(), targ.parameters()):
                            pt.lerp_(p, TAU)
                if device_targets:
                    actor_targ.load_(policy_targ)
                    critic_targ_dev.load_(critic_targ)
            critic_sum += critic_loss.detach()
            policy_sum += policy_loss.detach()
        actor.load_(policy)
        # the iteration's only host read
        losses.append((critic_sum.item() / max(updates_per_iter, 1),
                       policy_sum.item() / max(policy_updates if td3 else updates_per_iter, 1)))
    return dict(critic2=critic2, critic2_targ=critic2_targ, critic2_targ_dev=critic2_targ_dev,
                actor=actor, policy=policy, critic=critic, policy_targ=policy_targ, critic_targ=critic_targ,
                actor_targ=actor_targ, critic_targ_dev=critic_targ_dev, learner=learner, losses=losses,
                rollout_stats=venv.rollout_stats, venv=venv, her=her)


def main_sac(num_envs, iterations, steps_per_iter, batch_size, updates_per_iter, hidden, seed, device,
             device_targets=False, device_collect=False, update_call=False):
    """``main(..., sac=True)``: the same loop with SAC's pieces (the module docstring)."""
    device = torch.device(device)
    torch.manual_seed(seed)
    venv = CtrReachVecEnv(num_envs, device=device, seed=seed)
    her = venv.enable_her(n_sampled_goal=N_SAMPLED_GOAL, goal_selection_strategy=STRATEGY)
    venv.reset()
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    venv.t.copy_(torch.randint(0, venv.max_steps_per_episode, (num_envs,), generator=g, dtype=torch.int32))

    d = venv.obs_dim + 6
    policy = mlp(d, hidden, 12, False).to(device).requires_grad_(False)       # six means, six log standard deviations
    critics = [mlp(d + 6, hidden, 1, False).to(device).requires_grad_(False) for _ in range(2)]
    targets = [mlp(d + 6, hidden, 1, False).to(device).requires_grad_(False) for _ in range(2)]
    for critic, targ in zip(critics, targets):
        targ.load_state_dict(critic.state_dict())
    learner = SacLearner(policy, critics[0], critics[1], scale=venv.action_space.high, actor_lr=SAC_LR, critic_lr=SAC_LR,
                         alpha_lr=SAC_LR, init_alpha=INIT_ALPHA, target_entropy=TARGET_ENTROPY, max_batch=batch_size, seed=seed)
    pi_dev = GaussianActor.from_torch(policy, venv.action_space.high, device, seed=seed)
    targets_dev = [MlpCritic.from_torch(targ, device) for targ in targets]
    losses = []
    step = update = 0
    hist = torch.zeros((updates_per_iter, 5), dtype=torch.float32, device=device) if update_call else None
    for it in range(iterations):
        if device_collect:                                                   # the same steps, one launch per refill period
            venv.collect_gauss(pi_dev, steps_per_iter, counter=step)
            step += steps_per_iter
        else:
            for _ in range(steps_per_iter):                                  # the policy's sample, the step with its HER feed
                venv.step(pi_dev.sample(venv.actor_rows(), counter=step, row_base=venv.env_base)["action"])
                step += 1
        if update_call:                                                      # the iteration's updates: one call
            learner.update(her, pi_dev, list(zip(targets_dev, targets)), batch_size, GAMMA, SAC_TAU,
                           updates=updates_per_iter, history=hist)
            h = hist.sum(0).tolist()                                         # the iteration's only host read
            losses.append((0.5 * (h[0] + h[1]) / max(updates_per_iter, 1), h[2] / max(updates_per_iter, 1)))
            continue
        critic_sum = torch.zeros((), device=device)
        policy_sum = torch.zeros((), device=device)
        for _ in range(updates_per_iter):
            if device_targets:                                               # the batch and its soft target: one call
                batch = her.sample_sac(batch_size, pi_dev, targets_dev[0], targets_dev[1], GAMMA, learner.log_alpha)
                target = batch["target"]
            else:
                batch = her.sample(batch_size)
                # the sampling draws and the collection draws share the key: keep their counters apart
                nxt = pi_dev.sample(batch["next_obs"], counter=(1 << 40) + update)
                update += 1
                q = torch.minimum(targets_dev[0](batch["next_obs"], nxt["unit"]),
                                  targets_dev[1](batch["next_obs"], nxt["unit"]))
                target = batch["reward"] + GAMMA * (1.0 - batch["done"]) * (q - learner.alpha * nxt["logp"])
            learner.critic_step(batch["obs"], batch["action"], target)
            learner.actor_step(batch["obs"])
            pi_dev.load_(policy)
            polyak_([(targets_dev[0], critics[0], targets[0]), (targets_dev[1], critics[1], targets[1])], SAC_TAU)
            critic_sum += learner.critic_loss.mean()
            policy_sum += learner.actor_loss
        # the iteration's only host read
        losses.append((critic_sum.item() / max(updates_per_iter, 1), policy_sum.item() / max(updates_per_iter, 1)))
    return dict(policy=policy, pi_dev=pi_dev, critic=critics[0], critic2=critics[1], critic_targ=targets[0],
                critic2_targ=targets[1], critic_targ_dev=targets_dev[0], critic2_targ_dev=targets_dev[1], learner=learner,
                losses=losses, alpha=learner.alpha, venv=venv, her=her)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--steps-per-iter", type=int, default=20)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--updates-per-iter", type=int, default=40)
    ap.add_argument("--hidden", default="64,64", help="hidden widths, multiples of 32")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--device-targets", action="store_true",
                    help="the DDPG target from her.sample_td (bf16 target networks); with --sac the soft target from "
                         "her.sample_sac")
    ap.add_argument("--device-polyak", action="store_true",
                    help="the Polyak update and both blob refreshes in one polyak_ launch (implies --device-targets)")
    ap.add_argument("--device-update", action="store_true",
                    help="the critic's and the policy's updates from a DdpgLearner, no autograd (implies --device-polyak)")
    ap.add_argument("--td3", action="store_true",
                    help="TD3: twin critics, smoothed clipped double-Q targets, delayed policy updates (implies --device-update)")
    ap.add_argument("--sac", action="store_true",
                    help="SAC: a tanh-Gaussian policy, twin critics, the learned temperature (not with --td3)")
    ap.add_argument("--device-collect", action="store_true",
                    help="with --sac: the policy's samples inside the fused period kernel (venv.collect_gauss), one "
                         "launch per refill period instead of two per step")
    ap.add_argument("--update-call", action="store_true",
                    help="with --sac: an iteration's updates from one learner.update call (implies --device-targets)")
    ap.add_argument("--update-run", action="store_true",
                    help="DDPG and --td3: an iteration's updates from one learner.update call (implies --device-update)")
    args = ap.parse_args()
    out = main(args.num_envs, args.iterations, args.steps_per_iter, args.batch_size, args.updates_per_iter,
               tuple(int(w) for w in args.hidden.split(",")), args.seed, args.device, args.device_targets,
               args.device_polyak, args.device_update, args.td3, args.sac, args.device_collect, args.update_call,
               args.update_run)
    for it, (c, p) in enumerate(out["losses"]):
        print("iteration %3d: critic loss %.4g, policy loss %.4g" % (it, c, p))
    if args.sac:
        print("alpha %.4g; %d rows in the HER store" % (float(out["alpha"]), len(out["her"])))
    else:
        stats = out["rollout_stats"]
        episodes, successes = int(stats["episodes"].sum()), int(stats["successes"].sum())
        print("%d episodes finished, %d reached their goal; %d rows in the HER store" % (episodes, successes, len(out["her"])))
