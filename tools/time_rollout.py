"""Timing: microseconds per step over a 20-step refill period at 65 536 envs on the headline config
(compliant model, scipy RK45, one system, pooled auto-reset), HIP events around 32 back-to-back
periods (each with its refill), best of 3, for
  (a) step_many with recorded actions                      (open loop: the benchmark's fused period)
  (a') step_many replaying the actions (b) applied         (open loop on (b)'s trajectory)
  (b) rollout with an MLP actor [64, 64] and [128, 128, 128]   (closed loop, one launch per period)
  (c) act + step_raw per step                              (ctr_actor and ctr_step, two launches)
  (d) a torch float32 nn.Sequential + step_raw per step    (the eager policy)
With a library that lacks ctr_rollout (CTR_REACH_AMD_LIB naming an older build) only (a) runs.
usage: python tools/time_rollout.py [--envs N] [--json PATH] [--only-a]"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-ctr-reach_amd"))
from ctr_reach_amd import CtrReachVecEnv  # noqa: E402

R, PERIODS, REPEATS, WARM = 20, 32, 3, 8


def make_env(n):
    env = CtrReachVecEnv(n, device="cuda:0", seed=0, record_info=False, refill_interval=R)
    env.reset()
    g0 = torch.Generator(device="cpu")
    g0.manual_seed(2)
    env.t.copy_(torch.randint(0, 150, (n,), generator=g0, dtype=torch.int32))     # steady-state episode clocks
    return env


def make_seq(hidden, in_dim, seed=1):
    torch.manual_seed(seed)
    dims = [in_dim] + list(hidden)
    mods = []
    for a, b in zip(dims[:-1], dims[1:]):
        mods += [nn.Linear(a, b), nn.ReLU()]
    mods += [nn.Linear(dims[-1], 6), nn.Tanh()]
    return nn.Sequential(*mods).to("cuda:0")


def timed(period):
    """us per step: best of REPEATS runs of PERIODS periods."""
    stream = torch.cuda.current_stream()
    for _ in range(WARM):
        period()
    runs = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(PERIODS):
            period()
        e1.record(stream)
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) * 1e3 / (PERIODS * R))
    return {"us_per_step": min(runs), "runs": [round(r, 3) for r in runs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--json", default=None)
    ap.add_argument("--only-a", action="store_true", help="time (a) only (run-to-run spread; an older library)")
    args = ap.parse_args()
    n = args.envs
    out = {"device": torch.cuda.get_device_name(0), "envs": n, "period_steps": R, "periods": PERIODS,
           "repeats": REPEATS, "cases": {}}

    def report(name, res):
        out["cases"][name] = res
        print("%-44s %7.2f us/step   %s" % (name, res["us_per_step"], res["runs"]), flush=True)

    env = make_env(n)
    hi = torch.tensor(env.action_space.high, device="cuda:0")
    g = torch.Generator(device="cuda:0")
    g.manual_seed(1)
    acts = [((torch.rand((n, 6), generator=g, device="cuda:0") * 2 - 1) * hi).contiguous() for _ in range(R)]
    report("(a) step_many, recorded actions", timed(lambda: env.step_many(acts)))
    if args.only_a:
        pass
    elif not hasattr(env.lib, "ctr_rollout"):
        print("this library has no ctr_rollout: (b), (c), (d) skipped")
    else:
        from ctr_reach_amd.policy import MlpActor
        for hidden in ((64, 64), (128, 128, 128)):
            seq = make_seq(hidden, env.obs_dim + 6)
            actor = MlpActor.from_torch(seq, env.action_space.high, "cuda:0")
            tag = "[%s]" % ",".join(map(str, hidden))
            env = make_env(n)
            report("(b) rollout " + tag, timed(lambda: env.rollout(actor, R)))
            # the same trajectory open loop: the rollout's recorded actions replayed by step_many from
            # the same start (the closed loop steers the robots elsewhere than uniform actions do, and
            # a step lasts as long as its slowest wave's FK), so (b) - (a') is the actor's own cost
            env = make_env(n)
            rec = [env.rollout(actor, R, record_actions=True) for _ in range(WARM + REPEATS * PERIODS)]
            env = make_env(n)
            it = iter(rec)
            report("(a') step_many, the actions of (b) " + tag, timed(lambda: env.step_many(list(next(it)))))
            del rec, it
            env = make_env(n)

            def eager_actor():
                for _ in range(R):
                    env.step_raw(env.act(actor))
            report("(c) act + step_raw " + tag, timed(eager_actor))
            env = make_env(n)

            def eager_torch():
                with torch.no_grad():
                    for _ in range(R):
                        env.step_raw((seq(env.actor_rows()) * hi).contiguous())
            report("(d) torch f32 Sequential + step_raw " + tag, timed(eager_torch))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
