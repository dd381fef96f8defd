"""CtrReachVecEnv.step_many with the period's refill in the step kernel's tail (ctr_step_period)
leaves what ctr_step_many followed by ctr_pool_refill leaves, bit for bit: the reference of every
case is the same env with tail_refill=False.  Compared after every period: the state, every
output, the status words, the pool slots an env can still take, and how many resets sit suspended.

3-step episodes and 4-step periods: every env resets in every period (some twice), so a wave has
more new resets than its 32 lane pairs take in one pass, and suspended resets are claimed, resumed
and finished in later periods.  The sizes pick the paths:
- n = 1 and 65: one workgroup and one sub-list, within ctr_pool_refill's budget rule (65 has a
  ragged second wave);
- n = 300 with 3-step episodes: two workgroups, but the period's resets do not fit the carry lists
  (3 sub-lists of 200), so the reference runs without the budget and the waves' guess is corrected
  by k_tail_close (TAIL_FIX_ALL);
- n = 300 and 1 000 with 8-step episodes: 2 and 4 workgroups appending to 2 of 3 and 4 of 8
  sub-lists, and about n / 2 new resets a period, which fits the rule (one pass: at most 384 and
  1 024 resets) in most periods.  Suspended resets then sit on several sub-lists at a launch, the
  claim phase looks them up across them, and in the periods that fit the rule the last workgroup
  flips the lists itself, as the reference does;
- the 9-slot ring puts suspended resets within refill_lead + k of their env (TAIL_FIX_NEAR).

A ctr_pool_refill resumes whatever is suspended, after either kind of period.  So an explicit one
after a tail period changes nothing only while nothing is suspended (checked without lists, and
with lists allocated but empty); with suspended resets the check is that the queue is empty and
that tail and reference stay equal through the extra refill."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATE = ("joints", "desired_goal", "achieved_goal", "t", "epoch", "system", "obs", "reward", "done", "success",
         "error", "status", "terminal_obs", "terminal_achieved", "desired_joints", "starting_joints",
         "starting_position")
POOL_MISS = 16
R = 4
PERIODS = 6


def _env(cuda, n, tail, R=R, **kw):
    from ctr_reach_amd import CtrReachVecEnv
    kw.setdefault("select_systems", [0])
    kw.setdefault("max_steps_per_episode", 3)
    e = CtrReachVecEnv(n, device=cuda, seed=7, refill_interval=R, tail_refill=tail, **kw)
    e.goal_tolerance.current_tol = 0.03
    e.reset()
    return e


def _actions(env, cuda, count, seed=4):
    import torch
    rng = np.random.default_rng(seed)
    return [torch.tensor((rng.uniform(-1, 1, (env.num_envs, 6)) * env.action_space.high).astype(np.float32),
                         device=cuda) for _ in range(count)]


def _usable(env):
    """[P, n] mask of the pool slots holding a reset their env can still take (epoch + 1 .. epoch + P)."""
    lead = (env.pool_r.long() - env.epoch.long().unsqueeze(0) - 1) % (1 << 32)
    return lead < env.pool_depth


def _same(a, b, where, pool=True):
    import torch
    torch.cuda.synchronize()
    for k in STATE:
        assert torch.equal(getattr(a, k), getattr(b, k)), (where, k)
    assert not bool((b.status & POOL_MISS).any().item()), (where, "pool miss")
    if pool:
        ma, mb = _usable(a), _usable(b)
        assert torch.equal(ma, mb), (where, "usable slots")
        assert torch.equal(a.pool[ma], b.pool[mb]), (where, "pool")
        assert int(b.refill[0].item()) == 0, (where, "queue not empty")
        assert sum(a.carried()) == sum(b.carried()), (where, "suspended", a.carried(), b.carried())


def _run(cuda, n, kw, R=R, periods=PERIODS):
    a, b = _env(cuda, n, False, R, **kw), _env(cuda, n, True, R, **kw)
    acts = _actions(a, cuda, periods * R)
    carried = 0
    for p in range(periods):
        chunk = acts[p * R:(p + 1) * R]
        a.step_many(chunk)
        b.step_many(chunk)
        _same(a, b, p)
        carried = max(carried, sum(b.carried()))
    assert b.tail_launches == periods and a.tail_launches == 0
    assert a.refills == b.refills and a.fused_launches == b.fused_launches
    # every env took a reset at least every max_steps steps (3-step episodes, R = 4: in every period)
    assert int(b.epoch.min().item()) >= 1 + periods * R // b.max_steps_per_episode
    return a, b, carried


@pytest.mark.parametrize("n,kw,suspends", [
    (1, {}, True), (65, {}, True), (300, {}, False),
    (65, dict(refill_budget=1), True), (65, dict(refill_budget=3), True), (300, dict(refill_budget=3), False),
    (300, dict(refill_budget=0), False),
    (65, dict(pool_depth=9, refill_budget=1), True),
    (300, dict(domain_rand=0.05), False), (65, dict(domain_rand=0.05), True),
    (300, dict(obs_dtype="float64"), False),
    (300, dict(select_systems=[0, 1, 2, 3]), False), (65, dict(select_systems=[0, 1, 2, 3]), True),
    (65, dict(model="rigid"), True)])
def test_tail_refill_matches_the_trailing_refill_bit_for_bit(cuda, n, kw, suspends):
    a, b, carried = _run(cuda, n, kw)
    assert (b.carry is not None) == (kw.get("refill_budget", 6) != 0)
    if suspends:
        assert carried > 0                      # resets really were suspended, claimed and finished


def _parity(env):
    import torch
    return int(env.carry[512:516].view(torch.int32).item())          # CarryHdr.parity


@pytest.mark.parametrize("n,subs", [(300, 2), (1000, 4)])
def test_suspended_resets_on_several_sub_lists(cuda, n, subs):
    """Several workgroups, mostly within the budget rule: periods leave suspended resets on at least
    `subs` sub-lists, and the next period's claim phase looks them up across the sub-lists, resumes
    and finishes them.  In the periods that fit the rule the last workgroup flips the lists itself,
    as the trailing refill does (k_tail_close has nothing to do)."""
    import torch
    kw = dict(max_steps_per_episode=8)
    a, b = _env(cuda, n, False, **kw), _env(cuda, n, True, **kw)
    acts = _actions(a, cuda, PERIODS * R)
    seen = set()                        # how many were suspended, period by period
    claimed_across = flipped = 0
    for p in range(PERIODS):
        before = b.carry[:512].view(torch.int32).view(2, 64)[_parity(b)]     # the list this period reads
        claimed_across += int((before > 0).sum().item()) >= subs
        par = _parity(b)
        chunk = acts[p * R:(p + 1) * R]
        a.step_many(chunk)
        b.step_many(chunk)
        _same(a, b, p)
        flipped += _parity(b) == par ^ 1
        counts = b.carry[:512].view(torch.int32).view(2, 64)[_parity(b)]
        # (more than `subs` sub-lists when one fills up and its pairs go to the next: the small last
        # workgroup of n = 300 finishes early, claims most of the list and fills its 200 records)
        if sum(b.carried()):
            assert int((counts > 0).sum().item()) >= subs, (p, counts[:8].tolist())
            assert sum(b.carried()) == int(counts.sum().item())
        seen.add(sum(b.carried()))
    assert b.tail_launches == PERIODS and len(seen) > 1
    assert claimed_across >= 2          # periods that started with suspended resets on several sub-lists
    assert flipped >= 2                 # periods whose last workgroup closed the refill itself
    # plain refills on both resume what is left the same way
    for _ in range(4):
        a.refill_pool()
        b.refill_pool()
    _same(a, b, "plain refills")


def test_two_step_periods(cuda):
    a, b, carried = _run(cuda, 65, {}, R=2, periods=8)
    assert carried > 0


def test_a_default_period_of_64_steps_with_its_refill_is_one_launch(cuda):
    """The constructor's own refill_interval and pool_depth (64 / 64: no budget, no lists): a period
    is CTR_STEP_MANY_MAX steps and a dozen resets of every env, then the refill of all of them."""
    from ctr_reach_amd import CtrReachVecEnv, _abi
    mk = lambda tail: CtrReachVecEnv(65, device=cuda, seed=7, max_steps_per_episode=5,  # noqa: E731
                                     select_systems=[0, 1, 2, 3], tail_refill=tail)
    a, b = mk(False), mk(True)
    for e in (a, b):
        assert e.refill_interval == 64 == _abi.CTR_STEP_MANY_MAX and e.pool_depth == 64 and e.carry is None
        e.goal_tolerance.current_tol = 0.03
        e.reset()
    acts = _actions(a, cuda, 128)
    for p in range(2):
        epoch = b.epoch.clone()
        a.step_many(acts[64 * p:64 * (p + 1)])
        b.step_many(acts[64 * p:64 * (p + 1)])
        _same(a, b, p)
        assert int((b.epoch - epoch).min().item()) >= 12
    assert b.tail_launches == 2 and a.tail_launches == 0
    assert a.refills == b.refills and a.fused_launches == b.fused_launches == 2
    assert int(b.epoch.max().item()) > 1 + 128 // 5          # more resets than the time limit gives: goals were reached


def test_tail_refill_matches_synchronous_resets(cuda):
    """The n = 65 trajectory equals resets computed at the step that needs them (no pool)."""
    import torch
    s = _env(cuda, 65, False, pool_depth=0)
    b = _env(cuda, 65, True)
    acts = _actions(b, cuda, PERIODS * R)
    for p in range(PERIODS):
        chunk = acts[p * R:(p + 1) * R]
        for x in chunk:
            s.step_raw(x)
        b.step_many(chunk)
        torch.cuda.synchronize()
        for k in STATE:
            assert torch.equal(getattr(s, k), getattr(b, k)), (p, k)
    assert b.tail_launches == PERIODS and s.sweeps == PERIODS * R


def test_an_explicit_refill_after_a_tail_period(cuda):
    import torch
    # nothing suspended (no budget): the extra refill finds nothing and changes nothing
    a, b, _ = _run(cuda, 300, dict(refill_budget=0), periods=2)
    pool = b.pool.clone()
    b.refill_pool()
    torch.cuda.synchronize()
    assert torch.equal(pool, b.pool) and int(b.refill[0].item()) == 0
    # lists allocated but empty (n = 300, 3-step episodes: k_tail_close finishes every reset in most
    # periods): no byte of the pool, no count and no record changes; the refill flips its parity
    # word, as it does after any period, which only names the (empty) list read next
    a, b = _env(cuda, 300, False), _env(cuda, 300, True)
    acts = _actions(a, cuda, PERIODS * R)
    checked = 0
    for p in range(PERIODS):
        a.step_many(acts[p * R:(p + 1) * R])
        b.step_many(acts[p * R:(p + 1) * R])
        _same(a, b, p)
        if sum(b.carried()) == 0:
            pool, carry, par = b.pool.clone(), b.carry.clone(), _parity(b)
            a.refill_pool()
            b.refill_pool()
            torch.cuda.synchronize()
            assert torch.equal(pool, b.pool) and int(b.refill[0].item()) == 0
            assert torch.equal(carry[:512], b.carry[:512]) and torch.equal(carry[516:], b.carry[516:])
            assert _parity(b) == par ^ 1 and b.carried() == (0, 0)
            _same(a, b, (p, "after the extra refill"))
            checked += 1
    assert checked > 0
    # suspended resets: the queue is empty, the refill resumes them as after a ctr_pool_refill
    a, b = _env(cuda, 65, False), _env(cuda, 65, True)
    acts = _actions(a, cuda, PERIODS * R)
    for p in range(PERIODS):
        chunk = acts[p * R:(p + 1) * R]
        a.step_many(chunk)
        b.step_many(chunk)
        if p == 1:
            assert sum(b.carried()) > 0 and int(b.refill[0].item()) == 0
            a.refill_pool()
            b.refill_pool()
        _same(a, b, p)


def test_tail_periods_alternate_with_closed_loop_steps(cuda):
    a, b = _env(cuda, 65, False), _env(cuda, 65, True)
    acts = _actions(a, cuda, PERIODS * R)
    for p in range(PERIODS):
        chunk = acts[p * R:(p + 1) * R]
        for e in (a, b):
            if p % 2:
                for x in chunk:
                    e.step(x)
            else:
                e.step_many(chunk)
        _same(a, b, p)
    assert b.tail_launches == PERIODS // 2


def test_checkpoint_with_suspended_resets(cuda):
    a, b = _env(cuda, 65, False), _env(cuda, 65, True)
    acts = _actions(a, cuda, 6 * R)
    for p in range(3):
        a.step_many(acts[p * R:(p + 1) * R])
        b.step_many(acts[p * R:(p + 1) * R])
    assert sum(b.carried()) > 0
    sa, sb = a.state_dict(), b.state_dict()
    a.step_many(acts[:R])
    b.step_many(acts[:R])
    a.load_state_dict(sa)
    b.load_state_dict(sb)
    _same(a, b, "restored")
    for p in range(3, 6):
        a.step_many(acts[p * R:(p + 1) * R])
        b.step_many(acts[p * R:(p + 1) * R])
        _same(a, b, p)


def test_a_captured_period_replays_like_eager_periods(cuda):
    """One period captured, replayed 4 times (the same actions): the lists alternate under replay."""
    a, b = _env(cuda, 65, False), _env(cuda, 65, True)
    acts = _actions(a, cuda, R)
    g = b.capture_steps(acts)
    assert g.fused and b.tail_launches == 0
    for rep in range(4):
        a.step_many(acts)
        g.replay()
        _same(a, b, rep)
    assert b.tail_launches == 4 and a.refills == b.refills


def test_the_switches_keep_the_trailing_refill(cuda, monkeypatch):
    monkeypatch.setenv("CTR_TAIL_REFILL", "0")
    c = _env(cuda, 65, True)
    monkeypatch.setenv("CTR_TAIL_REFILL", "1")
    b = _env(cuda, 65, False)
    monkeypatch.delenv("CTR_TAIL_REFILL")
    a = _env(cuda, 65, False)
    acts = _actions(a, cuda, 2 * R)
    for p in range(2):
        for e in (a, b, c):
            e.step_many(acts[p * R:(p + 1) * R])
        _same(a, b, p)
        _same(a, c, p)
    assert c.tail_launches == 0 and a.tail_launches == 0 and b.tail_launches == 2
    # a chunk that is not a whole period keeps ctr_step_many and the refill launch
    a.step_many(acts[:2])
    b.step_many(acts[:2])
    a.step_many(acts[2:R])
    b.step_many(acts[2:R])
    _same(a, b, "split")
    assert b.tail_launches == 2


def test_y_pre_curvature_on_the_compliant_rk45_keeps_the_refill_launch(cuda):
    """The one step_many mode ctr_step_period refuses (its kernel would need scratch): step_many
    runs it through ctr_step_many and ctr_pool_refill whatever tail_refill says."""
    from test_oracle_uy import uy_systems
    kw = dict(ctr_systems_parameters=uy_systems())
    a, b = _env(cuda, 65, False, **kw), _env(cuda, 65, True, **kw)
    assert b.tail_refill and not b._tail_eligible()
    acts = _actions(a, cuda, 2 * R)
    for q in range(2):
        a.step_many(acts[q * R:(q + 1) * R])
        b.step_many(acts[q * R:(q + 1) * R])
        _same(a, b, q)
    assert b.tail_launches == 0 and b.fused_launches == 2 and a.refills == b.refills
    # the rigid model with the same tubes is eligible
    c = _env(cuda, 65, True, model="rigid", **kw)
    r = _env(cuda, 65, False, model="rigid", **kw)
    r.step_many(acts[:R])
    c.step_many(acts[:R])
    _same(r, c, "rigid")
    assert c.tail_launches == 1


@pytest.mark.parametrize("kw", [dict(integrator="rk4", rk4_steps_per_m=400, model="compliant"),
                                dict(integrator="rk4", rk4_steps_per_m=100, model="rigid"),
                                dict(pack_outputs=True), dict(her=True)])
def test_refused_modes_fall_back_and_match(cuda, kw):
    kw = dict(kw)
    her = kw.pop("her", False)
    a, b = _env(cuda, 65, False, **kw), _env(cuda, 65, True, **kw)
    acts = _actions(a, cuda, 2 * R)
    if her:
        for e in (a, b):
            e.enable_her(slots=2)
        with pytest.raises(RuntimeError):
            b.step_many(acts[:R])
        for x in acts:
            a.step_raw(x)
            b.step_raw(x)
    else:
        with pytest.raises(RuntimeError):
            b.step_many(acts[:R])
        ga, gb = a.capture_steps(acts), b.capture_steps(acts)
        assert not gb.fused
        ga.replay()
        gb.replay()
    _same(a, b, "fallback", pool=False)
    assert b.tail_launches == 0 and a.refills == b.refills
