"""CtrReachVecEnv.rollout (ctr_rollout: the MLP actor inside the fused period kernel) leaves exactly
what act + step_raw, one launch each per step, leave: state, outputs, terminal rows, the reset
pool, the refill count, the applied actions and the per-env episode statistics, bit for bit, with
auto-resets and both done causes inside the launches.  Shapes as in test_gpu_step_many.py, as are
the 64-step default period and the moving goal-tolerance schedule."""
import numpy as np
import pytest

from test_oracle_uy import uy_systems as _uy_systems

pytestmark = pytest.mark.gpu

KEYS = ("joints", "desired_goal", "achieved_goal", "t", "epoch", "system", "obs", "reward", "done", "success", "error",
        "status", "terminal_obs", "terminal_achieved", "pool_r", "pool_q0", "pool_dg")
OFF_KEYS = ("joints", "desired_goal", "achieved_goal", "t", "epoch", "system", "obs", "reward", "done", "success",
            "error", "status")


def _pair(cuda, n, R=4, **kw):
    from ctr_reach_amd import CtrReachVecEnv
    mk = lambda: CtrReachVecEnv(n, device=cuda, seed=7, max_steps_per_episode=5, refill_interval=R,  # noqa: E731
                                select_systems=[0, 1, 2, 3], **kw)
    a, b = mk(), mk()
    for e in (a, b):
        e.goal_tolerance.current_tol = 0.03
        e.reset()
    return a, b


def _actor(env, cuda, hidden, seed=2):
    """U(+-1/sqrt(fan_in)) weights, the output layer scaled up so that the actions use the box."""
    from ctr_reach_amd.policy import MlpActor
    rng = np.random.default_rng(seed)
    dims = [env.obs_dim + 6] + list(hidden) + [6]
    layers = []
    for l in range(len(dims) - 1):
        s = (1.0 if l < len(hidden) else 8.0) / np.sqrt(dims[l])
        layers.append((rng.uniform(-s, s, (dims[l + 1], dims[l])).astype(np.float32),
                       rng.uniform(-s, s, dims[l + 1]).astype(np.float32)))
    return MlpActor(layers, env.action_space.high, device=cuda)


def _same(a, b, keys, where):
    import torch
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(getattr(a, k), getattr(b, k)), (where, k)


class _EagerStats(object):
    """The statistics ctr_rollout accumulates, formed in torch from the eager loop's outputs."""

    def __init__(self, env):
        import torch
        n, dev = env.num_envs, env.device
        self.s = dict(episodes=torch.zeros(n, dtype=torch.int32, device=dev),
                      successes=torch.zeros(n, dtype=torch.int32, device=dev),
                      error_sum=torch.zeros(n, dtype=torch.float64, device=dev),
                      length_sum=torch.zeros(n, dtype=torch.int32, device=dev))

    def step(self, env, t_before):
        import torch
        d = env.done.bool()
        self.s["episodes"] += d.to(torch.int32)
        self.s["successes"] += (d & env.success.bool()).to(torch.int32)
        self.s["error_sum"] += torch.where(d, env.error.to(torch.float64), torch.zeros_like(self.s["error_sum"]))
        self.s["length_sum"] += torch.where(d, t_before + 1, torch.zeros_like(t_before))


def _eager(env, actor, steps, stats=None):
    import torch
    acts = []
    for _ in range(steps):
        a = env.act(actor)
        t0 = env.t.clone()
        env.step_raw(a)
        acts.append(a)
        if stats is not None:
            stats.step(env, t0)
    return torch.stack(acts)


CONFIGS = [(300, {}), (1, {}), (65, {}), (300, dict(domain_rand=0.05)), (300, dict(obs_dtype="float64")),
           (300, dict(model="rigid")), (300, dict(uy=True)), (300, dict(uy=True, model="rigid")),
           (300, dict(uy=True, integrator="rk4", rk4_steps_per_m=100))]


HIDDEN = [(32,), (128, 128, 128), (256,), (224, 160)]
# every config with the first two; the wide ones (8 row tiles; 7 -> 5) with four of them
CASES = [(j, i) for j in (0, 1) for i in range(len(CONFIGS))] + [(j, i) for j in (2, 3) for i in (0, 2, 3, 5)]


def _rollout_lds(actor, kw):
    """What ctr_rollout's launcher adds up against a workgroup's 163 840 B of LDS: the blob (and 16 B
    to align it), the kernel's static LDS (90 240 B for the fixed-step RK4 on the compliant model,
    78 976 B for the other modes) and with domain randomisation 256 lanes' tube tables of 240 B."""
    fixed = 90240 if kw.get("integrator") == "rk4" and kw.get("model") != "rigid" else 78976
    return actor.blob.numel() + 16 + fixed + (256 * 240 if kw.get("domain_rand") else 0)


@pytest.mark.parametrize("n,kw,hidden", [CONFIGS[i] + (HIDDEN[j],) for j, i in CASES],
                         ids=["%d-kw%d-hidden%d" % (CONFIGS[i][0], i, j) for j, i in CASES])
def test_rollout_matches_act_and_step_bit_for_bit(cuda, n, kw, hidden):
    import torch
    R = 4
    kw = dict(kw)
    if kw.pop("uy", False):
        kw["ctr_systems_parameters"] = _uy_systems()
    a, b = _pair(cuda, n, R, **kw)
    actor = _actor(a, cuda, hidden)
    # the blob, the kernel's static LDS and the domain tables share the workgroup's 160 KB:
    # [128, 128, 128] (83 584 B) does not fit beside the domain tables, nor beside the fixed-step
    # RK4's static LDS; [256] (33 920 B) not beside the domain tables; [224, 160] (97 920 B) not even
    # beside the static LDS alone.  ctr_rollout refuses those with the byte counts and leaves the
    # env untouched
    too_big = _rollout_lds(actor, kw) > 160 * 1024
    assert too_big == {(32,): False, (128, 128, 128): "domain_rand" in kw or kw.get("integrator") == "rk4",
                       (256,): "domain_rand" in kw, (224, 160): True}[hidden]
    if too_big:
        from ctr_reach_amd._abi import CtrError
        with pytest.raises(CtrError, match="LDS"):
            b.rollout(actor, R)
        _same(a, b, KEYS, "refused")
        assert b.fused_launches == 0
        return
    if "ctr_systems_parameters" in kw and not kw.get("model") and not kw.get("integrator"):
        # the compliant model's scipy RK45 with y pre-curvature: its kernel would need scratch, so
        # ctr_rollout refuses the mode (as ctr_step_period does); act + step_raw is the way there
        with pytest.raises(RuntimeError, match="scratch"):
            b.rollout(actor, R)
        rc = b.lib.ctr_rollout(b.cfg, b._batch, actor._struct, R, b._out, 2, None, None)
        assert rc == -1 and b"ctr_actor + ctr_step" in b.lib.ctr_last_error()
        _same(a, b, KEYS, "refused mode")
        return
    stats = _EagerStats(a)
    for period in range(3):
        want = _eager(a, actor, R, stats)
        got = b.rollout(actor, R, record_actions=True)
        _same(a, b, KEYS, period)
        assert torch.equal(want, got), period
        for k, v in stats.s.items():
            assert torch.equal(v, b.rollout_stats[k]), (period, k)
    assert a.refills == b.refills
    assert b.fused_launches == 3 and a.fused_launches == 0
    # 5-step episodes: every env took at least 2 time-limit resets inside the fused launches
    assert int((b.epoch - 1).sum().item()) >= 2 * n
    assert int(b.rollout_stats["episodes"].min().item()) >= 2
    # the policy moved the robots: the actions differ between the envs and the steps
    assert len(torch.unique(got[..., 0])) > min(n, 8)


def test_rollout_without_autoreset(cuda):
    from ctr_reach_amd import CtrReachVecEnv
    n, k = 300, 6
    mk = lambda: CtrReachVecEnv(n, device=cuda, seed=3, autoreset=False, max_steps_per_episode=5,  # noqa: E731
                                select_systems=[0, 1, 2, 3])
    a, b = mk(), mk()
    for e in (a, b):
        e.goal_tolerance.current_tol = 0.03
        e.reset()
    actor = _actor(a, cuda, (64, 96))
    import torch
    want = _eager(a, actor, k)
    got = b.rollout(actor, k, record_actions=True)
    _same(a, b, OFF_KEYS, "off")
    assert torch.equal(want, got)
    assert b.fused_launches == 1 and getattr(b, "rollout_stats", None) is None
    assert int(b.t.min().item()) == k and bool(b.done.all().item())     # past the time limit, nobody reset


def _default_period_pair(cuda, **kw):
    """65 envs (a full wave and a one-lane wave) with the constructor's own refill_interval and
    pool_depth: a period is CTR_STEP_MANY_MAX steps."""
    from ctr_reach_amd import CtrReachVecEnv, _abi
    mk = lambda: CtrReachVecEnv(65, device=cuda, seed=7, max_steps_per_episode=5,  # noqa: E731
                                select_systems=[0, 1, 2, 3], **kw)
    a, b = mk(), mk()
    for e in (a, b):
        assert e.refill_interval == 64 == _abi.CTR_STEP_MANY_MAX
        assert e.pool_depth == (64 if e.autoreset else 0)
        e.goal_tolerance.current_tol = 0.03
        e.reset()
    return a, b


def test_a_default_period_is_one_launch_of_64_closed_loop_steps(cuda):
    import torch
    a, b = _default_period_pair(cuda)
    actor = _actor(a, cuda, (32,))
    stats = _EagerStats(a)
    for period in range(2):
        epoch = b.epoch.clone()
        want = _eager(a, actor, 64, stats)
        got = b.rollout(actor, 64, record_actions=True)
        _same(a, b, KEYS, period)
        assert torch.equal(want, got), period
        for k, v in stats.s.items():
            assert torch.equal(v, b.rollout_stats[k]), (period, k)
        assert b.fused_launches == period + 1 and a.refills == b.refills
        assert int((b.epoch - epoch).min().item()) >= 12      # a dozen pooled resets of every env in the launch
    st = b.rollout_stats
    assert int(st["successes"].sum().item()) > 0 and int((st["episodes"] - st["successes"]).sum().item()) > 0


def test_67_closed_loop_steps_without_autoreset_split_into_64_and_3(cuda):
    import torch
    a, b = _default_period_pair(cuda, autoreset=False)
    actor = _actor(a, cuda, (32,))
    want = _eager(a, actor, 67)
    got = b.rollout(actor, 67, record_actions=True)
    _same(a, b, OFF_KEYS, "64 + 3")
    assert torch.equal(want, got)
    assert b.fused_launches == 2
    assert int(b.t.min().item()) == 67 and bool(b.done.all().item())


# The goal-tolerance schedule (tests/test_gpu_step_many.py has the open-loop paths): rollout judges its
# steps with the tolerance the schedule holds at the call, as step() does.
SCHEDULE = dict(inc_tol_obs=False, initial_tol=0.05, final_tol=0.005, N_ts=8, function="linear", set_tol=0)
SCHEDULE_TS = (2, 5, 8)


def _scheduled(cuda, **kw):
    from ctr_reach_amd import CtrReachVecEnv
    e = CtrReachVecEnv(300, device=cuda, seed=7, max_steps_per_episode=5, refill_interval=4,
                       select_systems=[0, 1, 2, 3], goal_tolerance_parameters=dict(SCHEDULE), **kw)
    assert e.get_goal_tolerance() == 0.05
    e.reset()
    return e


def test_a_tolerance_update_reaches_rollout(cuda):
    import torch
    R = 4
    a, b = _scheduled(cuda), _scheduled(cuda)
    actor = _actor(a, cuda, (64, 96))
    prev = 0.05
    for ts in SCHEDULE_TS:
        for e in (a, b):
            e.update_goal_tolerance(ts)
        tol = a.get_goal_tolerance()
        assert tol == b.get_goal_tolerance() and tol < prev
        matters = False
        for _ in range(R):                # the reference: step(), which reads the schedule
            a.step(a.act(actor))
            err = a.error.double()
            matters = matters or bool(((err > tol + 1e-6) & (err < prev - 1e-6)).any().item())
        assert matters                    # (on the reference: the previous tolerance would show)
        b.rollout(actor, R)
        _same(a, b, KEYS, ts)
        assert bool((b.obs[:, 12] == torch.tensor(tol, dtype=torch.float64).to(b.obs.dtype)).all().item()), ts
        prev = tol
    assert b.fused_launches == len(SCHEDULE_TS)


def test_rollout_outputs_follow_the_schedule_in_plain_float64(cuda):
    """Without auto-reset (the tips stay): reward, success and done of a period's last step against
    the distance formed in numpy float64 and the schedule's current tolerance.  Rows within 1e-12
    of the tolerance are left out (the kernel's distance may differ in the last bit)."""
    import torch
    R = 4
    env = _scheduled(cuda, autoreset=False)
    actor = _actor(env, cuda, (64, 96))
    prev, matters = 0.05, 0
    for ts in SCHEDULE_TS:
        env.update_goal_tolerance(ts)
        tol = env.get_goal_tolerance()
        env.rollout(actor, R)
        torch.cuda.synchronize()
        d = np.linalg.norm(env.achieved_goal.cpu().numpy() - env.desired_goal.cpu().numpy(), axis=1)
        assert d.dtype == np.float64
        keep = np.abs(d - tol) > 1e-12
        assert keep.mean() >= 0.99
        reward = env.reward.cpu().numpy()
        assert np.array_equal(reward[keep], -(d > tol).astype(np.float32)[keep]), ts
        assert np.array_equal(env.success.cpu().numpy()[keep], (d < tol).astype(np.uint8)[keep]), ts
        t = env.t.cpu().numpy()
        assert np.array_equal(env.done.cpu().numpy(), ((reward == 0) | (t >= 5)).astype(np.uint8)), ts
        assert bool((env.obs[:, 12] == torch.tensor(tol, dtype=torch.float64).to(env.obs.dtype)).all().item())
        matters += int(((d > tol) != (d > prev))[keep].sum())
        prev = tol
    assert matters > 0                    # (the previous tolerance would have judged some env otherwise)


def test_rollout_splits_at_the_refill_boundary(cuda):
    R = 4
    a, b = _pair(cuda, 300, R)
    actor = _actor(a, cuda, (64, 96))
    r0 = b.refills
    _eager(a, actor, 2 * R)
    b.rollout(actor, 2 * R)
    _same(a, b, KEYS, "split")
    assert b.fused_launches == 2 and b.refills - r0 == 2 and a.refills == b.refills
    # a rollout that starts inside a period ends at the period's refill
    _eager(a, actor, 1)
    b.step_raw(b.act(actor))
    _eager(a, actor, R + 1)
    b.rollout(actor, R + 1)
    _same(a, b, KEYS, "split inside")
    assert b.fused_launches == 4 and a.refills == b.refills and b._steps_since_refill == 2


@pytest.mark.parametrize("kw", [dict(pack_outputs=True),
                                dict(integrator="rk4", rk4_steps_per_m=400, model="compliant")])
def test_ineligible_envs_raise_and_stay_untouched(cuda, kw):
    a, b = _pair(cuda, 300, 4, **kw)
    actor = _actor(a, cuda, (32,))
    with pytest.raises(RuntimeError):
        b.rollout(actor, 4)
    _same(a, b, KEYS, "ineligible")
    assert b.fused_launches == 0 and a.refills == b.refills


def test_every_env_finishes_episodes(cuda):
    a, b = _pair(cuda, 300, 4)
    actor = _actor(a, cuda, (32,))
    b.rollout(actor, 12)
    st = b.rollout_stats
    assert int(st["episodes"].min().item()) >= 2
    assert bool((st["successes"] <= st["episodes"]).all().item())
    assert bool((st["length_sum"] <= 5 * st["episodes"]).all().item()) and bool((st["length_sum"] >= st["episodes"]).all().item())
    b.reset_rollout_stats()
    assert int(b.rollout_stats["episodes"].sum().item()) == 0
