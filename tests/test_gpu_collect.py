"""CtrReachVecEnv.collect (ctr_collect: the actor, the exploration noise and the HER recording inside
the fused period kernel) leaves exactly what act + explore + step_raw with the fused HER feed, one
launch each per step, leave: state, outputs, terminal rows, the reset pool, the refill count, every
buffer of the HER store, the applied actions and the per-env episode statistics, bit for bit, with
auto-resets, both done causes and wrapping store slots inside the launches."""
import numpy as np
import pytest

from test_gpu_rollout import KEYS, OFF_KEYS, SCHEDULE, SCHEDULE_TS, _actor, _EagerStats, _same
from test_oracle_uy import uy_systems as _uy_systems

pytestmark = pytest.mark.gpu

HER_KEYS = ("state", "step_rows", "dg", "tol", "len", "epoch", "cur_t", "cur_epoch")
R = 4


def _noise(kind):
    from ctr_reach_amd.policy import ExploreNoise
    return {None: None, "gauss": ExploreNoise(0.3, seed=5), "full": ExploreNoise(0.3, random_eps=0.3, seed=5)}[kind]


def _make(cuda, n, her=True, systems=(0, 1, 2, 3), env_base=0, **kw):
    """test_gpu_rollout._pair's env (float32 observations), with a 3-slot HER store: 5-step episodes
    at tolerance 0.03 end by success and by the time limit, and the slots wrap."""
    from ctr_reach_amd import CtrReachVecEnv
    kw.setdefault("max_steps_per_episode", 5)
    kw.setdefault("refill_interval", R)
    e = CtrReachVecEnv(n, device=cuda, seed=7, env_base=env_base, select_systems=list(systems), **kw)
    e.goal_tolerance.current_tol = 0.03
    if her:
        e.enable_her(slots=3)
    e.reset()
    return e


def _eager(env, actor, noise, steps, stats=None):
    """The unfused collection: act, explore, step_raw (which records into the fused HER feed)."""
    import torch
    acts = []
    for _ in range(steps):
        a = env.act(actor)
        if noise is not None:
            a = env.explore(a, noise)
        t0 = env.t.clone()
        env.step_raw(a)
        acts.append(a)
        if stats is not None:
            stats.step(env, t0)
    return torch.stack(acts)


def _same_store(a, b, where):
    import torch
    torch.cuda.synchronize()
    bits = {torch.float32: torch.int32, torch.float64: torch.int64}
    for k in HER_KEYS:
        # as bits: the state rows hold the float64 achieved goals, whose halves read as float32 may be NaNs
        x, y = getattr(a._her, k), getattr(b._her, k)
        assert torch.equal(x.view(bits.get(x.dtype, x.dtype)), y.view(bits.get(y.dtype, y.dtype))), (where, "her." + k)


def _check_periods(cuda, a, b, actor, noise, periods=4):
    import torch
    n = a.num_envs
    stats = _EagerStats(a)
    for period in range(periods):
        want = _eager(a, actor, noise, R, stats)
        got = b.collect(actor, R, noise, record_actions=True)
        _same(a, b, KEYS, period)
        _same_store(a, b, period)
        assert torch.equal(want, got), period
        for k, v in stats.s.items():
            assert torch.equal(v, b.rollout_stats[k]), (period, k)
        assert a.refills == b.refills
    assert b.fused_launches == periods and a.fused_launches == 0
    assert int(b.rollout_stats["episodes"].min().item()) >= 2
    # the store holds episodes ended by success and by the time limit
    her = b._her
    L = her.len.view(n, her.slots).long()
    last = her.reward.permute(2, 0, 1).gather(2, (L - 1).clamp(min=0).unsqueeze(-1)).squeeze(-1)
    print("n = %d: stored episodes ended by success %d, by the time limit %d"
          % (n, int(((L > 0) & (last == 0)).sum().item()), int(((L == 5) & (last < 0)).sum().item())))
    # (a single env keeps its last two finished episodes: with this seed both ran to the time limit,
    # so the two causes are asked of the batches only)
    if n > 1:
        assert bool(((L > 0) & (last == 0)).any().item()) and bool(((L == 5) & (last < 0)).any().item())
    assert bool((L > 0).any().item())
    sa, sb = a._her.sample(256, seed=9), b._her.sample(256, seed=9)
    torch.cuda.synchronize()
    assert sorted(sa) == sorted(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    return got


GRID = [(n, systems, noise, hidden) for n in (300, 65, 1) for systems in ((0,), (0, 1, 2, 3))
        for noise in (None, "gauss", "full") for hidden in ((32,), (128, 128, 128))]


@pytest.mark.parametrize("n,systems,noise,hidden", GRID,
                         ids=["%d-sys%d-%s-h%d" % (n, len(s), k, len(h)) for n, s, k, h in GRID])
def test_collect_matches_act_explore_and_step_bit_for_bit(cuda, n, systems, noise, hidden):
    import torch
    a, b = _make(cuda, n, systems=systems), _make(cuda, n, systems=systems)
    actor = _actor(a, cuda, hidden)
    assert actor.in_dim == (19 if len(systems) == 1 else 20)
    got = _check_periods(cuda, a, b, actor, _noise(noise))
    if noise is not None and n > 1:
        # the noise reached the env: the applied actions are not the actor's
        assert not torch.equal(got[-1], b.act(actor))


@pytest.mark.parametrize("kw", [dict(domain_rand=0.05), dict(model="rigid"),
                                dict(uy=True, integrator="rk4", rk4_steps_per_m=100)],
                         ids=["domain_rand", "rigid", "uy_rk4"])
def test_collect_in_the_other_kernel_modes(cuda, kw):
    kw = dict(kw)
    if kw.pop("uy", False):
        kw["ctr_systems_parameters"] = _uy_systems()
    a, b = _make(cuda, 300, **kw), _make(cuda, 300, **kw)
    _check_periods(cuda, a, b, _actor(a, cuda, (32,)), _noise("full"))


def test_collect_without_noise_is_rollout_with_a_store(cuda):
    import torch
    b, c = _make(cuda, 300), _make(cuda, 300, her=False)
    actor = _actor(b, cuda, (64, 96))
    for period in range(2):
        got = b.collect(actor, R, None, record_actions=True)
        want = c.rollout(actor, R, record_actions=True)
        _same(c, b, KEYS, period)
        assert torch.equal(want, got)
        for k, v in c.rollout_stats.items():
            assert torch.equal(v, b.rollout_stats[k]), (period, k)


def test_collect_without_autoreset(cuda):
    import torch
    a, b = _make(cuda, 300, autoreset=False), _make(cuda, 300, autoreset=False)
    actor, noise = _actor(a, cuda, (64, 96)), _noise("full")
    want = _eager(a, actor, noise, 6)
    got = b.collect(actor, 6, noise, record_actions=True)
    _same(a, b, OFF_KEYS, "off")
    _same_store(a, b, "off")
    assert torch.equal(want, got)
    assert b.fused_launches == 1 and getattr(b, "rollout_stats", None) is None
    # past the time limit nobody was reset: every env closed its one episode and records nothing more
    assert bool(b.done.all().item()) and bool((b._her.cur_t == -1).all().item())
    assert int((b._her.len > 0).sum().item()) == 300 and int(b._her.len.max().item()) == 5


def test_67_collected_steps_without_autoreset_split_into_64_and_3(cuda):
    import torch
    from ctr_reach_amd import _abi
    mk = lambda: _make(cuda, 65, autoreset=False, refill_interval=64)  # noqa: E731
    a, b = mk(), mk()
    assert _abi.CTR_STEP_MANY_MAX == 64
    actor, noise = _actor(a, cuda, (32,)), _noise("gauss")
    want = _eager(a, actor, noise, 67)
    got = b.collect(actor, 67, noise, record_actions=True)
    _same(a, b, OFF_KEYS, "64 + 3")
    _same_store(a, b, "64 + 3")
    assert torch.equal(want, got)
    assert b.fused_launches == 2 and int(b.t.min().item()) == 67


def test_a_tolerance_update_reaches_collect_and_the_store(cuda):
    mk = lambda: _make(cuda, 300, goal_tolerance_parameters=dict(SCHEDULE))  # noqa: E731
    a, b = mk(), mk()
    actor, noise = _actor(a, cuda, (64, 96)), _noise("full")
    tols = []
    for ts in SCHEDULE_TS[:2]:
        for e in (a, b):
            e.update_goal_tolerance(ts)
        tol = a.get_goal_tolerance()
        tols.append(tol)
        _eager(a, actor, noise, R)
        b.collect(actor, R, noise)
        _same(a, b, KEYS, ts)
        _same_store(a, b, ts)
        assert bool((b.obs[:, 12] == np.float32(tol)).all().item()), ts
    assert tols[0] != tols[1]
    closed = b._her.tol[b._her.len > 0]
    # episodes closed in the second call were judged, and stored, with the second tolerance
    assert bool((closed == tols[1]).any().item()) and bool(((closed == tols[0]) | (closed == tols[1])).all().item())


def _untouched(a, b, where):
    _same(a, b, KEYS, where)
    if a._her is not None and b._her is not None:
        _same_store(a, b, where)
    assert b.fused_launches == 0 and a.refills == b.refills


def test_collect_needs_the_fused_her_feed(cuda):
    a, b = _make(cuda, 300, her=False), _make(cuda, 300, her=False)
    actor = _actor(a, cuda, (32,))
    with pytest.raises(RuntimeError, match=r"enable_her\(\)"):
        b.collect(actor, R)
    _untouched(a, b, "no her")
    a, b = _make(cuda, 300), _make(cuda, 300)
    b._her.fused = False
    with pytest.raises(RuntimeError, match=r"enable_her\(\)"):
        b.collect(actor, R, _noise("full"))
    _untouched(a, b, "unfused")
    from ctr_reach_amd import CtrReachVecEnv
    c = CtrReachVecEnv(300, device=cuda, seed=7, max_steps_per_episode=5, refill_interval=R, obs_dtype="float64")
    with pytest.raises(ValueError, match="float32"):
        c.enable_her(slots=3)
    c.reset()
    with pytest.raises(RuntimeError, match=r"enable_her\(\)"):
        c.collect(_actor(c, cuda, (32,)), R)
    assert c.fused_launches == 0


def test_collect_refusals_leave_the_env_and_the_store_untouched(cuda):
    from ctr_reach_amd._abi import CtrError
    a, b = _make(cuda, 300), _make(cuda, 300)
    with pytest.raises(CtrError, match="LDS"):               # [224, 160]: 97 920 B beside 78 976 B of static LDS
        b.collect(_actor(a, cuda, (224, 160)), R, _noise("full"))
    _untouched(a, b, "LDS")
    # rollout() and step_many() keep refusing an env with the HER feed
    with pytest.raises(RuntimeError, match="not with the HER feed"):
        b.rollout(_actor(a, cuda, (32,)), R)
    assert b.step_many_ineligible() == "not with the HER feed" and b.collect_ineligible() is None
    _untouched(a, b, "rollout")
    # the compliant model's scipy RK45 with y pre-curvature: the kernel would need scratch
    kw = dict(ctr_systems_parameters=_uy_systems())
    a, b = _make(cuda, 300, **kw), _make(cuda, 300, **kw)
    actor = _actor(a, cuda, (32,))
    with pytest.raises(RuntimeError, match="scratch"):
        b.collect(actor, R, _noise("full"))
    rc = b.lib.ctr_collect(b.cfg, b._batch, actor._struct, None, b._her._h, R, b._out, 2, None, None)
    assert rc == -1 and b"scratch" in b.lib.ctr_last_error()
    _untouched(a, b, "mode 1")
    # the lane-pair mode
    kw = dict(integrator="rk4", rk4_steps_per_m=400, model="compliant")
    a, b = _make(cuda, 300, **kw), _make(cuda, 300, **kw)
    with pytest.raises(RuntimeError, match="lane-pair"):
        b.collect(_actor(a, cuda, (32,)), R)
    _untouched(a, b, "lane pair")


def test_collect_does_not_depend_on_the_sharding(cuda):
    import torch
    full, lo, hi = _make(cuda, 300), _make(cuda, 150), _make(cuda, 150, env_base=150)
    actor, noise = _actor(full, cuda, (32,)), _noise("full")
    for e in (full, lo, hi):
        e.collect(actor, 2 * R, noise)
    torch.cuda.synchronize()
    for k in ("joints", "obs", "t", "epoch"):
        assert torch.equal(torch.cat((getattr(lo, k), getattr(hi, k))), getattr(full, k)), k
    rows = full._her.step_rows                                # [slots, t, n, 8]
    assert torch.equal(rows[:, :, :150], lo._her.step_rows) and torch.equal(rows[:, :, 150:], hi._her.step_rows)
    assert torch.equal(full._her.len.view(300, 3)[150:], hi._her.len.view(150, 3))
