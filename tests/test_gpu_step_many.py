"""CtrReachVecEnv.step_many (ctr_step_many: the steps of a refill period in one launch, each wave
taking its envs through all of them) leaves exactly what stepping one launch at a time leaves:
state, outputs, terminal rows, the reset pool and the refill count, bit for bit, with auto-resets
inside the fused launches; it splits at refill boundaries; the envs it cannot run keep the
step-by-step capture and raise from step_many.  Also at the constructor's own period length
(64 steps = CTR_STEP_MANY_MAX in one launch, 64 + 3 without auto-reset), and under a goal-tolerance
schedule that moves between the periods: step_raw, step_many, the tail refill and a fresh capture
leave the bits of a twin driven through step(), and reward, success and done follow the current
tolerance in plain float64."""
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


def _actions(env, cuda, count, seed=4):
    import torch
    rng = np.random.default_rng(seed)
    return [torch.tensor((rng.uniform(-1, 1, (env.num_envs, 6)) * env.action_space.high).astype(np.float32),
                         device=cuda) for _ in range(count)]


def _same(a, b, keys, where):
    import torch
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(getattr(a, k), getattr(b, k)), (where, k)


# kernel modes: {} 0, rigid 4; with y pre-curvature 1, rigid 5, fixed-step RK4 on the compliant model 3
# (without it that is the lane-pair step, which step_many refuses)
@pytest.mark.parametrize("n,kw", [(300, {}), (1, {}), (65, {}), (300, dict(domain_rand=0.05)),
                                  (300, dict(obs_dtype="float64")), (300, dict(model="rigid")),
                                  (300, dict(uy=True)), (300, dict(uy=True, model="rigid")),
                                  (300, dict(uy=True, integrator="rk4", rk4_steps_per_m=100))])
def test_step_many_matches_eager_steps_bit_for_bit(cuda, n, kw):
    R = 4
    kw = dict(kw)
    if kw.pop("uy", False):
        kw["ctr_systems_parameters"] = _uy_systems()
    a, b = _pair(cuda, n, R, **kw)
    if "ctr_systems_parameters" in kw:
        assert any(a.cfg.systems[s].Uy[i] != 0.0 for s in range(a.n_systems) for i in range(3))
    acts = _actions(a, cuda, 3 * R)
    for period in range(3):
        chunk = acts[period * R:(period + 1) * R]
        for x in chunk:
            a.step_raw(x)
        b.step_many(chunk)
        _same(a, b, KEYS, period)
    assert a.refills == b.refills
    assert b.fused_launches == 3 and a.fused_launches == 0
    # 5-step episodes: every env took at least 2 time-limit resets inside the fused launches
    assert int((b.epoch - 1).sum().item()) >= 2 * n


def test_step_many_without_autoreset(cuda):
    from ctr_reach_amd import CtrReachVecEnv
    n, k = 300, 6
    mk = lambda: CtrReachVecEnv(n, device=cuda, seed=3, autoreset=False, max_steps_per_episode=5,  # noqa: E731
                                select_systems=[0, 1, 2, 3])
    a, b = mk(), mk()
    for e in (a, b):
        e.goal_tolerance.current_tol = 0.03
        e.reset()
    acts = _actions(a, cuda, k)
    for x in acts:
        a.step_raw(x)
    b.step_many(acts)
    _same(a, b, OFF_KEYS, "off")
    assert b.fused_launches == 1
    assert int(b.t.min().item()) == k and bool(b.done.all().item())     # past the time limit, nobody reset


def test_step_many_splits_at_the_refill_boundary(cuda):
    R = 4
    a, b = _pair(cuda, 300, R)
    acts = _actions(a, cuda, 2 * R)
    r0 = b.refills
    for x in acts:
        a.step_raw(x)
    b.step_many(acts)
    _same(a, b, KEYS, "split")
    assert b.fused_launches == 2 and b.refills - r0 == 2 and a.refills == b.refills
    # a launch that starts inside a period ends at the period's refill
    a.step_raw(acts[0])
    b.step_raw(acts[0])
    for x in acts[1:R + 2]:
        a.step_raw(x)
    b.step_many(acts[1:R + 2])
    _same(a, b, KEYS, "split inside")
    assert b.fused_launches == 4 and a.refills == b.refills and b._steps_since_refill == 2


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


def test_a_default_period_is_one_launch_of_64_steps(cuda):
    import torch
    a, b = _default_period_pair(cuda)
    acts = _actions(a, cuda, 128)
    reached = timed_out = torch.zeros(65, dtype=torch.bool, device=cuda)
    for period in range(2):
        chunk = acts[64 * period:64 * (period + 1)]
        epoch = b.epoch.clone()
        for x in chunk:
            a.step_raw(x)
            reached = reached | (a.done.bool() & a.success.bool())
            timed_out = timed_out | (a.done.bool() & ~a.success.bool())
        b.step_many(chunk)
        _same(a, b, KEYS, period)
        assert b.fused_launches == period + 1 and a.refills == b.refills
        # 5-step episodes: a dozen pooled resets of every env inside the launch
        assert int((b.epoch - epoch).min().item()) >= 12
    assert bool(reached.any().item()) and bool(timed_out.any().item())      # both done causes
    assert a.fused_launches == 0 and a.sweeps == b.sweeps == 0


def test_67_steps_without_autoreset_split_into_64_and_3(cuda):
    a, b = _default_period_pair(cuda, autoreset=False)
    acts = _actions(a, cuda, 67)
    for x in acts:
        a.step_raw(x)
    b.step_many(acts)
    _same(a, b, OFF_KEYS, "64 + 3")
    assert b.fused_launches == 2
    assert int(b.t.min().item()) == 67 and bool(b.done.all().item())


# The goal-tolerance schedule (the reference's training curriculum): every path that launches a
# step judges it with the tolerance the schedule holds at the call.  The reference of these tests
# is a twin env driven through step().
SCHEDULE = dict(inc_tol_obs=False, initial_tol=0.05, final_tol=0.005, N_ts=8, function="linear", set_tol=0)
SCHEDULE_TS = (2, 5, 8)


def _scheduled(cuda, **kw):
    from ctr_reach_amd import CtrReachVecEnv
    e = CtrReachVecEnv(300, device=cuda, seed=7, max_steps_per_episode=5, refill_interval=4,
                       select_systems=[0, 1, 2, 3], goal_tolerance_parameters=dict(SCHEDULE), **kw)
    assert e.get_goal_tolerance() == 0.05
    e.reset()
    return e


def _between(err, tol_a, tol_b):
    """Some env's distance lies between the two tolerances: its outcome depends on which one ran."""
    lo, hi = min(tol_a, tol_b), max(tol_a, tol_b)
    return bool(((err.double() > lo + 1e-6) & (err.double() < hi - 1e-6)).any().item())


def _drive(path, env, chunk):
    if path == "step_raw":
        for x in chunk:
            env.step_raw(x)
    elif path == "graph":
        g = env.capture_steps(chunk)          # a fresh capture: it takes the tolerance of now
        g.replay()
        return g                              # (the caller keeps it alive while it runs)
    else:
        env.step_many(chunk)


@pytest.mark.parametrize("path", ["step_raw", "step_many", "tail", "graph"])
def test_a_tolerance_update_reaches_every_step_path(cuda, path):
    import torch
    R = 4
    a, b = _scheduled(cuda), _scheduled(cuda, tail_refill=path == "tail")
    acts = _actions(a, cuda, len(SCHEDULE_TS) * R)
    prev = 0.05
    for p, ts in enumerate(SCHEDULE_TS):
        for e in (a, b):
            e.update_goal_tolerance(ts)
        tol = a.get_goal_tolerance()
        assert tol == b.get_goal_tolerance() and abs(tol - (0.05 - 0.045 * ts / 8)) < 1e-15 and tol < prev
        chunk = acts[p * R:(p + 1) * R]
        matters = False
        for x in chunk:
            a.step(x)
            matters = matters or _between(a.error, prev, tol)
        assert matters                    # (on the reference: the previous tolerance would show)
        g = _drive(path, b, chunk)
        _same(a, b, KEYS, (path, ts))
        del g
        assert bool((b.obs[:, 12] == torch.tensor(tol, dtype=torch.float64).to(b.obs.dtype)).all().item()), (path, ts)
        prev = tol
    assert b.tail_launches == (len(SCHEDULE_TS) if path == "tail" else 0)
    assert b.fused_launches == (0 if path == "step_raw" else len(SCHEDULE_TS))


def test_a_captured_period_keeps_the_tolerance_it_was_captured_with(cuda):
    """capture_steps captures the tolerance: a replay after update_goal_tolerance is the period of an
    env whose schedule stayed where it was (a fresh capture takes the new value: the "graph" case of
    the test above)."""
    import torch
    R = 4
    a, b = _scheduled(cuda), _scheduled(cuda)
    acts = _actions(a, cuda, 2 * R)
    for e in (a, b):
        e.update_goal_tolerance(2)
    old = a.get_goal_tolerance()
    g = b.capture_steps(acts[:R])
    for x in acts[:R]:
        a.step(x)
    g.replay()
    _same(a, b, KEYS, "captured")
    b.update_goal_tolerance(5)            # a stays at ts = 2
    new = b.get_goal_tolerance()
    for x, buf in zip(acts[R:], g.actions):
        buf.copy_(x)
    matters = False
    for x in acts[R:]:
        a.step(x)
        matters = matters or _between(a.error, old, new)
    assert matters and new < old
    g.replay()
    _same(a, b, KEYS, "replayed after the update")
    assert bool((b.obs[:, 12] == torch.tensor(old, dtype=torch.float64).to(b.obs.dtype)).all().item())


@pytest.mark.parametrize("path", ["step_raw", "step_many"])
def test_outputs_follow_the_schedule_in_plain_float64(cuda, path):
    """Without auto-reset (the tips stay): reward, success and done of a period's last step against
    the distance formed in numpy float64 and the schedule's current tolerance.  Rows within 1e-12
    of the tolerance are left out (the kernel's distance may differ in the last bit)."""
    import torch
    R = 4
    env = _scheduled(cuda, autoreset=False)
    acts = _actions(env, cuda, len(SCHEDULE_TS) * R)
    prev, matters = 0.05, 0
    for p, ts in enumerate(SCHEDULE_TS):
        env.update_goal_tolerance(ts)
        tol = env.get_goal_tolerance()
        _drive(path, env, acts[p * R:(p + 1) * R])
        torch.cuda.synchronize()
        d = np.linalg.norm(env.achieved_goal.cpu().numpy() - env.desired_goal.cpu().numpy(), axis=1)
        assert d.dtype == np.float64
        keep = np.abs(d - tol) > 1e-12
        assert keep.mean() >= 0.99
        reward = env.reward.cpu().numpy()
        assert np.array_equal(reward[keep], -(d > tol).astype(np.float32)[keep]), (path, ts)
        assert np.array_equal(env.success.cpu().numpy()[keep], (d < tol).astype(np.uint8)[keep]), (path, ts)
        t = env.t.cpu().numpy()
        assert np.array_equal(env.done.cpu().numpy(), ((reward == 0) | (t >= 5)).astype(np.uint8)), (path, ts)
        assert bool((env.obs[:, 12] == torch.tensor(tol, dtype=torch.float64).to(env.obs.dtype)).all().item())
        matters += int(((d > tol) != (d > prev))[keep].sum())
        prev = tol
    assert matters > 0                    # (the previous tolerance would have judged some env otherwise)


@pytest.mark.parametrize("fused", [True, False])
def test_her_stores_the_updated_tolerance_with_the_episode(cuda, fused):
    """Episodes recorded after an update (inside the step, or by ctr_her_record after it) carry the
    new tolerance: it is what relabelled rewards are computed with."""
    from ctr_reach_amd import CtrReachVecEnv
    env = CtrReachVecEnv(300, device=cuda, seed=7, max_steps_per_episode=5, refill_interval=4,
                         select_systems=[0, 1, 2, 3], goal_tolerance_parameters=dict(SCHEDULE))
    her = env.enable_her(slots=3)
    her.fused = fused
    env.reset()
    env.update_goal_tolerance(5)
    tol = env.get_goal_tolerance()
    assert tol != 0.05
    for x in _actions(env, cuda, 5):
        env.step_raw(x)
    closed = her.len > 0
    assert int(closed.sum().item()) >= 300            # 5-step episodes: every env closed one
    assert bool((her.tol[closed] == tol).all().item())


@pytest.mark.parametrize("kw", [dict(pack_outputs=True),
                                dict(integrator="rk4", rk4_steps_per_m=400, model="compliant")])
def test_ineligible_envs_keep_the_stepwise_capture(cuda, kw):
    R = 4
    a, b = _pair(cuda, 300, R, **kw)
    acts = _actions(a, cuda, R)
    with pytest.raises(RuntimeError):
        b.step_many(acts)
    g = b.capture_steps(acts)
    assert not g.fused
    for rep in range(2):
        for x in acts:
            a.step_raw(x)
        g.replay()
        _same(a, b, KEYS, rep)
    assert b.fused_launches == 0 and a.refills == b.refills


def test_fused_period_switch_selects_the_capture(cuda):
    R = 4
    a, b = _pair(cuda, 300, R)
    _, d = _pair(cuda, 300, R, fused_period=False)
    acts = _actions(a, cuda, 2 * R)
    gb, gd = b.capture_steps(acts), d.capture_steps(acts)
    assert gb.fused and not gd.fused
    assert b.fused_launches == 0                      # the capture launched nothing
    for x in acts:
        a.step_raw(x)
    gb.replay()
    gd.replay()
    _same(a, b, KEYS, "fused")
    _same(a, d, KEYS, "stepwise")
    assert b.fused_launches == 2 and d.fused_launches == 0
    assert a.refills == b.refills == d.refills


def test_environment_variable_selects_the_stepwise_capture(cuda, monkeypatch):
    R = 4
    monkeypatch.setenv("CTR_FUSED_PERIOD", "0")
    a, b = _pair(cuda, 300, R)                        # fused_period=True by keyword, overridden
    assert not b.fused_period
    monkeypatch.delenv("CTR_FUSED_PERIOD")
    acts = _actions(a, cuda, R)
    g = b.capture_steps(acts)
    assert not g.fused
    for x in acts:
        a.step_raw(x)
    g.replay()
    _same(a, b, KEYS, "env var")
    assert b.fused_launches == 0 and a.refills == b.refills
    b.step_many(acts)                                 # the switch is about the capture only
    assert b.fused_launches == 1
