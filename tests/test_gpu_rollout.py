"""CtrReachVecEnv.rollout (ctr_rollout: the MLP actor inside the fused period kernel) leaves exactly
what act + step_raw, one launch each per step, leave: state, outputs, terminal rows, the reset
pool, the refill count, the applied actions and the per-env episode statistics, bit for bit, with
auto-resets and both done causes inside the launches.  Shapes as in test_gpu_step_many.py."""
import numpy as np
import pytest

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


def _uy_systems():
    """The registered systems with a y pre-curvature on two tubes: the kernels' MODE bit 1."""
    from ctr_reach_amd.systems import default_systems_parameters
    p = default_systems_parameters()
    for name in p:
        p[name]["tube_0"]["y_curvature"] = 3.0
        p[name]["tube_1"]["y_curvature"] = -2.0
    return p


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


@pytest.mark.parametrize("hidden", [(32,), (128, 128, 128)])
@pytest.mark.parametrize("n,kw", CONFIGS)
def test_rollout_matches_act_and_step_bit_for_bit(cuda, n, kw, hidden):
    import torch
    R = 4
    kw = dict(kw)
    if kw.pop("uy", False):
        kw["ctr_systems_parameters"] = _uy_systems()
    a, b = _pair(cuda, n, R, **kw)
    actor = _actor(a, cuda, hidden)
    # the blob, the kernel's static LDS and the domain tables share the workgroup's 160 KB: the
    # largest network does not fit beside the domain tables, nor beside the fixed-step RK4's static
    # LDS; ctr_rollout refuses those with the byte counts and leaves the env untouched
    too_big = hidden == (128, 128, 128) and ("domain_rand" in kw or kw.get("integrator") == "rk4")
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
