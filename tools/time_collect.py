"""Timing of the data-collection half of a DDPG + HER iteration: microseconds per step over a 20-step
refill period at 65 536 envs on the headline config (compliant model, scipy RK45, one system, pooled
auto-reset) with an MLP actor [64, 64], tools/time_rollout.py's protocol (HIP events around 32
back-to-back periods, each with its refill, best of 3), every line in a fresh process:
  (a) rollout                         on --parent-lib (an older build of the library) and on this
                                      build's, --spread runs each, interleaved: did k_rollout keep its speed
  (b) collect, HER                    the actor and the HER recording in one launch per period
  (b) collect, HER + noise            ... with the exploration noise (sigma 0.3, random_eps 0.3)
  (c) act + explore + step_raw, HER   the same, eager: ctr_actor, ctr_explore, ctr_step_her per step
With --gauss, SAC's collection instead (a GaussianActor [64, 64] with the same hidden layers' seed),
--spread fresh processes of every line, the two builds interleaved:
  (d) collect_gauss                   the policy's sample and the HER recording in one launch per period
  (e) sample + step_raw, HER          the same, eager: torch.cat of the rows, ctr_gauss_act, ctr_step_her per
                                      step; on --parent-lib (the yardstick of (d)) and on this build's
  (a), (b) collect, HER               on both builds: did k_rollout and k_collect keep their times
usage: python tools/time_collect.py [--envs N] [--parent-lib PATH] [--spread K] [--json PATH] [--gauss]
       python tools/time_collect.py --case NAME      (one line, in this process; what the above starts)"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-ctr-reach_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CASES = ("rollout", "collect_her", "collect_her_noise", "eager_her_noise", "collect_gauss", "eager_gauss")
HIDDEN = (64, 64)


def run_case(name, n):
    import torch
    from time_rollout import R, make_env, make_seq, timed
    from ctr_reach_amd import CtrReachVecEnv
    from ctr_reach_amd.policy import MlpActor

    def make_her_env():
        env = CtrReachVecEnv(n, device="cuda:0", seed=0, record_info=False, refill_interval=R)
        env.enable_her()
        env.reset()
        g0 = torch.Generator(device="cpu")
        g0.manual_seed(2)
        env.t.copy_(torch.randint(0, 150, (n,), generator=g0, dtype=torch.int32))     # steady-state episode clocks
        # the store's clocks follow the env's: every open episode is at the env's step
        env._her.cur_t.copy_(env.t)
        return env

    env = make_env(n) if name == "rollout" else make_her_env()
    if name in ("collect_gauss", "eager_gauss"):
        from ctr_reach_amd.policy import GaussianActor
        seq = make_seq(HIDDEN, env.obs_dim + 6)[:-2]          # the hidden layers; a 12-row head, no Tanh
        torch.manual_seed(3)
        seq.append(torch.nn.Linear(HIDDEN[-1], 12).to("cuda:0"))
        pi = GaussianActor.from_torch(seq, env.action_space.high, "cuda:0", seed=1)
        step = [0]                                            # the running draw counter

        def fused():
            env.collect_gauss(pi, R, counter=step[0])
            step[0] += R

        def eager():
            for _ in range(R):
                env.step_raw(pi.sample(env.actor_rows(), counter=step[0], row_base=env.env_base)["action"])
                step[0] += 1

        res = timed(fused if name == "collect_gauss" else eager)
        res.update(case=name, envs=n, device=torch.cuda.get_device_name(0),
                   lib="--parent-lib" if os.environ.get("CTR_REACH_AMD_LIB") else "this build")
        return res
    actor = MlpActor.from_torch(make_seq(HIDDEN, env.obs_dim + 6), env.action_space.high, "cuda:0")
    if name == "rollout":
        res = timed(lambda: env.rollout(actor, R))
    else:
        from ctr_reach_amd.policy import ExploreNoise
        noise = ExploreNoise(0.3, random_eps=0.3, seed=1)
        if name == "collect_her":
            res = timed(lambda: env.collect(actor, R))
        elif name == "collect_her_noise":
            res = timed(lambda: env.collect(actor, R, noise))
        else:
            def eager():
                for _ in range(R):
                    env.step_raw(env.explore(env.act(actor), noise))
            res = timed(eager)
    res.update(case=name, envs=n, device=torch.cuda.get_device_name(0),
               lib="--parent-lib" if os.environ.get("CTR_REACH_AMD_LIB") else "this build")
    return res


def fresh(name, n, lib=None):
    env = dict(os.environ)
    if lib:
        env["CTR_REACH_AMD_LIB"] = lib
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--envs", str(n)], env=env,
                         capture_output=True, text=True, timeout=600)
    if out.returncode:
        raise RuntimeError("%s failed (exit %d):\n%s" % (name, out.returncode, out.stderr[-2000:]))
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--case", choices=CASES, default=None)
    ap.add_argument("--parent-lib", default=None, help="an older build of libctr_reach_amd.so, for (a)")
    ap.add_argument("--spread", type=int, default=3, help="fresh-process runs of (a) per library")
    ap.add_argument("--json", default=None)
    ap.add_argument("--gauss", action="store_true", help="SAC's collection: (d), (e) and (a), (b) on both builds")
    args = ap.parse_args()
    if args.case:
        print(json.dumps(run_case(args.case, args.envs)))
        return
    lines = []

    def line(label, name, lib=None):
        res = fresh(name, args.envs, lib)
        res["label"] = label
        lines.append(res)
        print(json.dumps(res), flush=True)

    for k in range(args.spread):                       # interleaved: both builds see the same machine
        if args.parent_lib:
            line("(a) rollout, parent build, run %d" % k, "rollout", os.path.abspath(args.parent_lib))
        line("(a) rollout, this build, run %d" % k, "rollout")
        if not args.gauss:
            continue
        for label, name in (("(b) collect, HER", "collect_her"), ("(e) sample + step_raw, fused HER", "eager_gauss")):
            if args.parent_lib:
                line("%s, parent build, run %d" % (label, k), name, os.path.abspath(args.parent_lib))
            line("%s, this build, run %d" % (label, k), name)
        line("(d) collect_gauss, this build, run %d" % k, "collect_gauss")
    if not args.gauss:
        line("(b) collect, HER", "collect_her")
        line("(b) collect, HER + noise", "collect_her_noise")
        line("(c) act + explore + step_raw, fused HER", "eager_her_noise")
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"lines": lines}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
