"""CtrReachVecEnv.set_goal (ctr_set_goal) and CtrReachVecEnv.follow (ctr_follow: every env walks its own
waypoint list inside the fused period kernel).

set_goal is checked against torch on the env's own tensors.  follow(fused=True) is checked, bit for
bit, against a reference loop written here with the API the env had before: direct writes of
``desired_goal`` and ``obs[:, 9:12]``, then act + step_raw, and the bookkeeping in torch -- the state,
the outputs, the cursors, the per-waypoint records and the applied actions, with both causes of an
advance (the hold running out, the waypoint reached) and the end of the path inside the launches.
Shapes as in test_gpu_rollout.py; the tolerance is 0.03.

Measured shares (test_both_advance_causes_happen, 300 envs x 3 waypoints, hold 4, 15 steps): see
DESIGN 4.0i."""
import numpy as np
import pytest

from test_gpu_rollout import OFF_KEYS, _actor, _same
from test_oracle_uy import uy_systems as _uy_systems

pytestmark = pytest.mark.gpu

TOL = 0.03
EXTRA = ("terminal_obs", "terminal_achieved")      # (not written without auto-reset: they stay zero)


def _kw(kw):
    kw = dict(kw)
    if kw.pop("uy", False):
        kw["ctr_systems_parameters"] = _uy_systems()
    return kw


def _env(cuda, n, seed=7, **kw):
    from ctr_reach_amd import CtrReachVecEnv
    kw.setdefault("autoreset", False)
    e = CtrReachVecEnv(n, device=cuda, seed=seed, max_steps_per_episode=5, select_systems=[0, 1, 2, 3], **_kw(kw))
    e.goal_tolerance.current_tol = TOL
    e.reset()
    return e


def _waypoints(cuda, env, K, **kw):
    """[N, K, 3] reachable waypoints: the even ones are the reset tips of other envs of the same
    configuration (another seed each: about a workspace away, so the hold runs out on most), the
    odd ones the env's own tip of now (a few steps of a bounded policy stay within the tolerance of
    it, so they are reached early)."""
    import torch
    cols = []
    for k in range(K):
        if k % 2:
            cols.append(env.achieved_goal.clone())
        else:
            cols.append(_env(cuda, env.num_envs, seed=100 + k, **kw).achieved_goal.clone())
    return torch.stack(cols, dim=1).contiguous()


class _Ref(object):
    """The reference loop's cursors and records, in follow()'s layout."""

    def __init__(self, n, K, dev):
        import torch
        nan = float("nan")
        self.cursor = torch.zeros(n, dtype=torch.int32, device=dev)
        self.held = torch.zeros(n, dtype=torch.int32, device=dev)
        self.tip = torch.full((n, K, 3), nan, dtype=torch.float64, device=dev)
        self.error = torch.full((n, K), nan, dtype=torch.float32, device=dev)
        self.steps = torch.zeros((n, K), dtype=torch.int32, device=dev)
        self.reached = torch.zeros((n, K), dtype=torch.uint8, device=dev)
        self.early = torch.zeros((n, K), dtype=torch.bool, device=dev)    # advanced before the hold ran out


def _reference(env, actor, wp, hold, reach, steps, ref=None):
    """``steps`` rounds of: move the goal of the envs that start a waypoint (direct writes), act,
    step_raw, and the advance bookkeeping in torch.  Returns (ref, actions [steps, N, 6])."""
    import torch
    n, K = wp.shape[0], wp.shape[1]
    ref = ref if ref is not None else _Ref(n, K, env.device)
    ar = torch.arange(n, device=env.device)
    acts = []
    for _ in range(steps):
        at = ref.cursor.clamp(max=K - 1).long()
        start = (ref.cursor < K) & (ref.held == 0)
        g = wp[ar, at]
        env.desired_goal[start] = g[start]
        env.obs[start, 9:12] = (g - env.achieved_goal)[start].to(env.obs.dtype)
        a = env.act(actor)
        env.step_raw(a)
        acts.append(a)
        on = ref.cursor < K
        ref.held = ref.held + on.to(torch.int32)
        ok = env.success.bool()
        adv = on & ((ref.held >= hold) | (ok & bool(reach)))
        ea, ka = ar[adv], at[adv]
        ref.tip[ea, ka] = env.achieved_goal[adv]
        ref.error[ea, ka] = env.error[adv]
        ref.steps[ea, ka] = ref.held[adv]
        ref.reached[ea, ka] = env.success[adv]
        ref.early[ea, ka] = ref.held[adv] < hold
        ref.cursor = ref.cursor + adv.to(torch.int32)
        ref.held = torch.where(adv, torch.zeros_like(ref.held), ref.held)
    return ref, (torch.stack(acts) if acts else None)


def _bits(t):
    """Bit equality that takes NaN == NaN (the unvisited waypoints)."""
    import torch
    if t.dtype == torch.float64:
        return t.contiguous().view(torch.int64)
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32)
    return t.contiguous()


def _same_result(ref, res, where):
    import torch
    torch.cuda.synchronize()
    for k in ("cursor", "held", "tip", "error", "steps", "reached"):
        assert torch.equal(_bits(getattr(ref, k)), _bits(getattr(res, k))), (where, k)


def _snapshot(env):
    keys = OFF_KEYS + EXTRA + (("pool",) if env.pool is not None else ())
    return {k: getattr(env, k).clone() for k in keys}


def _unchanged(env, snap, where, but=()):
    import torch
    torch.cuda.synchronize()
    for k, v in snap.items():
        if k not in but:
            assert torch.equal(_bits(getattr(env, k)), _bits(v)), (where, k)


# ---------------------------------------------------------------------------- 1. set_goal
@pytest.mark.parametrize("obs_dtype", ["float32", "float64"])
@pytest.mark.parametrize("masked", [False, True])
def test_set_goal_against_torch(cuda, obs_dtype, masked):
    import torch
    n = 300
    env = _env(cuda, n, autoreset=True, refill_interval=4, obs_dtype=obs_dtype)
    rng = np.random.default_rng(3)
    for _ in range(3):                     # outputs and a pool worth comparing
        env.step_raw(torch.tensor((rng.uniform(-1, 1, (n, 6)) * env.action_space.high).astype(np.float32), device=cuda))
    snap = _snapshot(env)
    assert "pool" in snap and env.n_systems == 4 and env.obs.shape == (n, 14)
    goal = torch.tensor(rng.uniform(-0.1, 0.1, (n, 3)), dtype=torch.float64, device=cuda)
    mask = torch.tensor(rng.uniform(size=n) < 0.5, device=cuda) if masked else None
    out = env.set_goal(goal, mask=mask)
    assert out["desired_goal"] is env.desired_goal and out["observation"] is env.obs
    m = mask if masked else torch.ones(n, dtype=torch.bool, device=cuda)
    assert 0 < int(m.sum().item()) and (not masked or int(m.sum().item()) < n)
    want_dg = torch.where(m[:, None], goal, snap["desired_goal"])
    want_obs = snap["obs"].clone()
    want_obs[:, 9:12] = torch.where(m[:, None], (goal - snap["achieved_goal"]).to(env.obs.dtype), snap["obs"][:, 9:12])
    torch.cuda.synchronize()
    assert torch.equal(env.desired_goal, want_dg)
    assert torch.equal(env.obs, want_obs)
    assert not torch.equal(env.obs, snap["obs"])
    _unchanged(env, snap, "set_goal", but=("desired_goal", "obs"))
    # [1, 3] is broadcast
    env.set_goal([[0.01, -0.02, 0.1]])
    torch.cuda.synchronize()
    one = torch.tensor([0.01, -0.02, 0.1], dtype=torch.float64, device=cuda)
    assert torch.equal(env.desired_goal, one.expand(n, 3))
    assert torch.equal(env.obs[:, 9:12], (one - env.achieved_goal).to(env.obs.dtype))
    with pytest.raises(ValueError):
        env.set_goal(goal[:7])


# ---------------------------------------------------------------------------- 2. follow against the reference loop
CONFIGS = [(300, {}), (1, {}), (65, {}), (300, dict(domain_rand=0.05)), (300, dict(obs_dtype="float64")),
           (300, dict(model="rigid")), (300, dict(uy=True, model="rigid")),
           (300, dict(uy=True, integrator="rk4", rk4_steps_per_m=100))]
HIDDEN = [(32,), (128, 128, 128)]
# [128, 128, 128] where the LDS budget allows: not beside the domain tables, nor beside the static
# LDS of the fixed-step RK4 on the compliant model (test_refusals_leave_the_env_untouched has those)
CASES = [(0, i) for i in range(len(CONFIGS))] + [(1, i) for i in (0, 1, 2, 4, 5, 6)]
K, HOLD = 3, 4


@pytest.mark.parametrize("reach", [False, True], ids=["hold", "reach"])
@pytest.mark.parametrize("n,kw,hidden", [CONFIGS[i] + (HIDDEN[j],) for j, i in CASES],
                         ids=["%d-kw%d-hidden%d" % (CONFIGS[i][0], i, j) for j, i in CASES])
def test_follow_matches_the_reference_loop_bit_for_bit(cuda, n, kw, hidden, reach):
    import torch
    a, b = _env(cuda, n, **kw), _env(cuda, n, **kw)
    actor = _actor(a, cuda, hidden)
    launches = 0
    # 10 steps end in the middle of a hold, 12 = K * hold, 15 run past the end of the path
    for steps in (10, 12, 15):
        wp = _waypoints(cuda, a, K, **kw)
        ref, want = _reference(a, actor, wp, HOLD, reach, steps)
        res = b.follow(actor, wp, HOLD, reach=reach, steps=steps, record_actions=True)
        launches += 1
        _same(a, b, OFF_KEYS + EXTRA, steps)
        _same_result(ref, res, steps)
        assert torch.equal(want, res.actions), steps
        assert b.fused_launches == launches and a.fused_launches == 0
        if steps == 10:
            if not reach:
                assert bool((res.cursor == 2).all().item()) and bool((res.held == 2).all().item())
            # a second call resumes from the cursors the first one left (and ends past the path)
            ref, want = _reference(a, actor, wp, HOLD, reach, 5, ref)
            got = b.follow(actor, wp, HOLD, reach=reach, steps=5, record_actions=True, resume=res)
            launches += 1
            assert got is res
            _same(a, b, OFF_KEYS + EXTRA, "resumed")
            _same_result(ref, res, "resumed")
            assert torch.equal(want, res.actions)
        assert bool((ref.cursor == K).all().item())
    # the envs stepped past the end towards their last waypoint, which was recorded before
    assert bool((res.cursor == K).all().item()) and not bool(torch.isnan(res.tip).any().item())
    assert bool((a.desired_goal == wp[:, K - 1]).all().item())
    # the policy moved the robots
    assert n == 1 or len(torch.unique(res.actions[..., 0])) > min(n, 8)


def test_steps_default_to_the_whole_path(cuda):
    import torch
    a, b = _env(cuda, 65), _env(cuda, 65)
    actor = _actor(a, cuda, (32,))
    wp = _waypoints(cuda, a, K)
    ref, _ = _reference(a, actor, wp, HOLD, False, K * HOLD)
    res = b.follow(actor, wp.cpu().numpy(), HOLD)              # (numpy waypoints, as paths makes them)
    _same(a, b, OFF_KEYS, "default")
    _same_result(ref, res, "default")
    assert res.actions is None and bool((res.steps == HOLD).all().item()) and bool((res.cursor == K).all().item())
    assert res.tip.shape == (65, K, 3) and res.error.shape == res.steps.shape == res.reached.shape == (65, K)
    assert torch.equal(res.tip[:, K - 1], b.achieved_goal)


# ---------------------------------------------------------------------------- 3. fused=False
@pytest.mark.parametrize("n,kw", [CONFIGS[0], CONFIGS[4]], ids=["300-kw0", "300-kw4"])
def test_the_python_loop_equals_the_fused_follow(cuda, n, kw):
    import torch
    a, b = _env(cuda, n, **kw), _env(cuda, n, **kw)
    actor = _actor(a, cuda, (32,))
    wp = _waypoints(cuda, a, K, **kw)
    ra = a.follow(actor, wp, HOLD, reach=True, steps=10, fused=False, record_actions=True)
    rb = b.follow(actor, wp, HOLD, reach=True, steps=10, record_actions=True)
    _same(a, b, OFF_KEYS + EXTRA, "eager")
    _same_result(ra, rb, "eager")
    assert torch.equal(ra.actions, rb.actions)
    assert a.fused_launches == 0 and b.fused_launches == 1
    a.follow(actor, wp, HOLD, reach=True, steps=5, fused=False, resume=ra)
    b.follow(actor, wp, HOLD, reach=True, steps=5, resume=rb)
    _same(a, b, OFF_KEYS + EXTRA, "eager resumed")
    _same_result(ra, rb, "eager resumed")
    assert bool((rb.cursor == K).all().item())


# ---------------------------------------------------------------------------- 4. the launch split
@pytest.mark.parametrize("reach", [False, True], ids=["hold", "reach"])
def test_72_steps_split_into_64_and_8_at_a_waypoint_switch(cuda, reach):
    import torch
    from ctr_reach_amd import _abi
    n, k9, hold = 65, 9, 8
    assert _abi.CTR_STEP_MANY_MAX == 64
    a, b = _env(cuda, n), _env(cuda, n)
    actor = _actor(a, cuda, (32,))
    wp = _waypoints(cuda, a, k9)
    ref, want = _reference(a, actor, wp, hold, reach, 72)
    res = b.follow(actor, wp, hold, reach=reach, steps=72, record_actions=True)
    _same(a, b, OFF_KEYS + EXTRA, "64 + 8")
    _same_result(ref, res, "64 + 8")
    assert torch.equal(want, res.actions)
    assert b.fused_launches == 2
    assert bool((res.cursor == k9).all().item())
    if not reach:
        # every env took waypoint 8 in the second launch's first step (its prologue moved the goal)
        assert bool((res.steps == hold).all().item())


# ---------------------------------------------------------------------------- 5. both advance causes
def test_both_advance_causes_happen(cuda, oracle_mod):
    """In the reference loop's result: at least 5 % of the (env, waypoint) pairs advance early (the
    waypoint reached) and at least 5 % by the hold running out; the same shares from the CPU
    (oracle.step + MlpActor.emulate, whose actions differ from the kernel's in the last bits)."""
    import torch
    n = 300
    a = _env(cuda, n)
    actor = _actor(a, cuda, (32,))
    wp = _waypoints(cuda, a, K)
    q0, sysid = a.joints.cpu().numpy().copy(), a.system.cpu().numpy().copy()
    ag0, obs0 = a.achieved_goal.cpu().numpy().copy(), a.obs.cpu().numpy().astype(np.float64)
    ref, _ = _reference(a, actor, wp, HOLD, True, 15)
    torch.cuda.synchronize()
    assert bool((ref.cursor == K).all().item())
    early = float(ref.early.float().mean().item())
    late = float((ref.steps == HOLD).float().mean().item())
    print("reference loop: early %.3f, hold ran out %.3f" % (early, late))
    assert early >= 0.05 and late >= 0.05 and abs(early + late - 1.0) < 1e-6
    # the same loop on the CPU
    systems = oracle_mod.make_systems(select=[0, 1, 2, 3])
    w = wp.cpu().numpy()
    q, ag, obs = q0, ag0, obs0               # (the reset's state and observation, from the device)
    c, h = np.zeros(n, int), np.zeros(n, int)
    dg = np.zeros((n, 3))
    n_early = n_late = 0
    for _ in range(15):
        start = (c < K) & (h == 0)
        g = w[np.arange(n), np.minimum(c, K - 1)]
        dg[start] = g[start]
        obs[start, 9:12] = (g - ag)[start]
        rows = np.concatenate((obs.astype(np.float32), ag.astype(np.float32), dg.astype(np.float32)), axis=1)
        act = actor.emulate(rows)[0].astype(np.float32)
        r = oracle_mod.step(q, act, dg, 0, TOL, system=sysid, systems=systems, multi=True)   # (done is not used)
        q, ag, obs = r["joints"], r["achieved_goal"], r["observation"].copy()
        on = c < K
        h = h + on
        adv = on & ((h >= HOLD) | r["is_success"])
        n_early += int((adv & (h < HOLD)).sum())
        n_late += int((adv & (h >= HOLD)).sum())
        c = c + adv
        h = np.where(adv, 0, h)
    assert n_early + n_late == n * K
    print("CPU loop: early %.3f, hold ran out %.3f" % (n_early / (n * K), n_late / (n * K)))
    assert n_early >= 0.05 * n * K and n_late >= 0.05 * n * K


# ---------------------------------------------------------------------------- 6. known answers
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "python"])
def test_known_answers_with_an_actor_that_stands_still(cuda, fused):
    """An all-zero actor: the action is 0 and the joints never move.  Waypoint 0 is the env's tip
    (reached on the first step), waypoint 1 a metre beside it (never reached)."""
    import torch
    from ctr_reach_amd.policy import MlpActor
    n, hold = 300, 4
    env = _env(cuda, n)
    dims = [env.obs_dim + 6, 32, 6]
    actor = MlpActor([(np.zeros((dims[l + 1], dims[l]), np.float32), np.zeros(dims[l + 1], np.float32)) for l in range(2)],
                     env.action_space.high, device=cuda)
    tip0, q0 = env.achieved_goal.clone(), env.joints.clone()
    wp = torch.stack((tip0, tip0 + torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64, device=cuda)), dim=1)
    res = env.follow(actor, wp, hold, reach=True, steps=1 + hold, fused=fused, record_actions=True)
    torch.cuda.synchronize()
    assert bool((res.actions == 0).all().item())
    assert torch.equal(env.joints, q0)
    assert bool((res.cursor == 2).all().item()) and bool((res.held == 0).all().item())
    assert bool((res.steps[:, 0] == 1).all().item()) and bool((res.reached[:, 0] == 1).all().item())
    assert bool((res.error[:, 0] < TOL).all().item())
    assert bool((res.steps[:, 1] == hold).all().item()) and bool((res.reached[:, 1] == 0).all().item())
    assert bool(((res.error[:, 1].double() - 1.0).abs() < TOL).all().item())
    assert torch.equal(res.tip[:, 1], env.achieved_goal)
    assert torch.equal(res.tip[:, 0], env.achieved_goal)          # (the same joints: the same FK)
    assert float((res.tip[:, 0] - tip0).abs().max().item()) < 1e-9
    assert torch.equal(env.desired_goal, wp[:, 1])
    assert torch.equal(env.obs[:, 9:12], (wp[:, 1] - env.achieved_goal).to(env.obs.dtype))


# ---------------------------------------------------------------------------- 7. refusals
def _refusal_case(cuda, name):
    """(env, actor hidden, waypoints builder kwargs, hold, wrong-shape flag, the exception, its words)."""
    n = 65
    if name == "autoreset":
        return _env(cuda, n, autoreset=True, refill_interval=4), (32,), 4, False, RuntimeError, "autoreset=False"
    if name == "her":
        from ctr_reach_amd import CtrReachVecEnv
        e = CtrReachVecEnv(n, device=cuda, seed=7, autoreset=False, max_steps_per_episode=5, select_systems=[0, 1, 2, 3])
        e.goal_tolerance.current_tol = TOL
        e.enable_her()
        e.reset()
        return e, (32,), 4, False, RuntimeError, "HER"
    if name == "mode1":
        return _env(cuda, n, uy=True), (32,), 4, False, RuntimeError, "scratch"
    if name == "lane-pair":
        return (_env(cuda, n, integrator="rk4", rk4_steps_per_m=400, model="compliant"), (32,), 4, False, RuntimeError,
                "lane-pair")
    if name == "shape":
        return _env(cuda, n), (32,), 4, True, ValueError, "waypoints"
    if name == "hold":
        return _env(cuda, n), (32,), 0, False, ValueError, "hold"
    assert name == "lds"
    return _env(cuda, n, domain_rand=0.05), (128, 128, 128), 4, False, RuntimeError, "83584 B"


@pytest.mark.parametrize("name", ["autoreset", "her", "mode1", "lane-pair", "shape", "hold", "lds"])
def test_refusals_leave_the_env_untouched(cuda, name):
    import torch
    env, hidden, hold, wrong, exc, words = _refusal_case(cuda, name)
    actor = _actor(env, cuda, hidden)
    wp = torch.zeros((env.num_envs, K, 3), dtype=torch.float64, device=cuda) + 0.05
    if wrong:
        wp = wp[:, :, :2]
    snap = _snapshot(env)
    launches = env.fused_launches
    with pytest.raises(exc, match=words) as info:
        env.follow(actor, wp, hold, reach=True)
    if name == "lds":                      # the byte counts: blob, static LDS, domain tables, the workgroup's LDS
        for w in ("78976 B", "61440 B", "163840 B"):
            assert w in str(info.value)
    _unchanged(env, snap, name)
    assert env.fused_launches == launches
    if name == "her":
        with pytest.raises(RuntimeError, match="HER"):
            env.set_goal(wp[:, 0])
        _unchanged(env, snap, "set_goal with HER")
    if name == "mode1":
        # the C entry point refuses the mode by name, as ctr_rollout does
        from ctr_reach_amd import FollowResult, _abi
        r = FollowResult(env.num_envs, K, cuda)
        w = wp.transpose(0, 1).contiguous()
        fw = _abi.CtrFollow(_abi.ptr(w), K, 4, 1, 0, _abi.ptr(r.cursor), _abi.ptr(r.held), None, None, None, None)
        assert env.lib.ctr_follow(env.cfg, env._batch, actor._struct, fw, 4, env._out, None, None) == -1
        assert b"y pre-curvature" in env.lib.ctr_last_error() and b"ctr_actor + ctr_step" in env.lib.ctr_last_error()
        _unchanged(env, snap, "ctr_follow, mode 1")
        # ... and the Python loop is the way there
        env.follow(actor, wp, 4, reach=True, steps=2, fused=False)


def test_null_record_arrays_are_not_wanted(cuda):
    """Any of the four per-waypoint pointers may be NULL: the cursors still move."""
    import torch
    from ctr_reach_amd import FollowResult, _abi
    n = 65
    a, b = _env(cuda, n), _env(cuda, n)
    actor = _actor(a, cuda, (32,))
    wp = _waypoints(cuda, a, K)
    ref, _ = _reference(a, actor, wp, HOLD, True, 10)
    r = FollowResult(n, K, cuda)
    w = wp.transpose(0, 1).contiguous()
    fw = _abi.CtrFollow(_abi.ptr(w), K, HOLD, 1, 0, _abi.ptr(r.cursor), _abi.ptr(r.held), None, None, None, None)
    b.cfg.tol = TOL
    rc = b.lib.ctr_follow(b.cfg, b._batch, actor._struct, fw, 10, b._out, None, None)
    assert rc == 0, b.lib.ctr_last_error()
    _same(a, b, OFF_KEYS, "no records")
    assert torch.equal(ref.cursor, r.cursor) and torch.equal(ref.held, r.held)
    assert bool(torch.isnan(r.tip).all().item()) and int(r.steps.sum().item()) == 0
