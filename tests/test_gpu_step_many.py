"""CtrReachVecEnv.step_many (ctr_step_many: the steps of a refill period in one launch, each wave
taking its envs through all of them) leaves exactly what stepping one launch at a time leaves:
state, outputs, terminal rows, the reset pool and the refill count, bit for bit, with auto-resets
inside the fused launches; it splits at refill boundaries; the envs it cannot run keep the
step-by-step capture and raise from step_many."""
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


def _uy_systems():
    """The registered systems with a y pre-curvature on two tubes: the kernels' MODE bit 1."""
    from ctr_reach_amd.systems import default_systems_parameters
    p = default_systems_parameters()
    for name in p:
        p[name]["tube_0"]["y_curvature"] = 3.0
        p[name]["tube_1"]["y_curvature"] = -2.0
    return p


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
