"""CtrReachVecEnv.collect_gauss (ctr_collect_gauss: SAC's tanh-Gaussian policy sampled inside the fused
period kernel, with the HER recording) leaves exactly what the per-step loop
``step_raw(pi.sample(actor_rows(), counter=c + j, row_base=env_base)["action"])`` with the fused HER feed
leaves: state, outputs, terminal rows, the reset pool, the refill count, every buffer of the HER store,
the applied actions and the per-env episode statistics, bit for bit; the draw counter runs on across
the launches of a call and across 2^32, and the noise row is the global env id."""
import numpy as np
import pytest

from test_gpu_collect import _make, _same_store
from test_gpu_gauss_actor import _random_layers
from test_gpu_rollout import KEYS, _actor, _EagerStats, _same
from test_oracle_uy import uy_systems as _uy_systems

pytestmark = pytest.mark.gpu

R = 4                                   # test_gpu_collect._make's refill_interval


def _policy(env, cuda, hidden, seed=7):
    from ctr_reach_amd.policy import GaussianActor
    layers = _random_layers(np.random.default_rng(3), hidden, env.obs_dim + 6)
    return GaussianActor(layers, env.action_space.high, cuda, seed=seed)


def _eager(env, pi, steps, counter, stats=None):
    """The unfused collection: the policy's sample on the env's rows, then step_raw (which records
    into the fused HER feed): two launches a step."""
    import torch
    acts = []
    for j in range(steps):
        a = pi.sample(env.actor_rows(), counter=counter + j, row_base=env.env_base)["action"]
        t0 = env.t.clone()
        env.step_raw(a)
        acts.append(a)
        if stats is not None:
            stats.step(env, t0)
    return torch.stack(acts)


def _check_periods(a, b, pi, counter=0, periods=4):
    """``periods`` refill periods on a (eager) and b (collect_gauss), compared after each; with four
    periods (three 5-step episodes) the store must hold what makes the comparison mean something."""
    import torch
    n = a.num_envs
    stats = _EagerStats(a)
    launches = b.fused_launches
    for period in range(periods):
        want = _eager(a, pi, R, counter + R * period, stats)
        got = b.collect_gauss(pi, R, counter=counter + R * period, record_actions=True)
        _same(a, b, KEYS, period)
        _same_store(a, b, period)
        assert torch.equal(want, got), period
        for k, v in stats.s.items():
            assert torch.equal(v, b.rollout_stats[k]), (period, k)
        assert a.refills == b.refills
    assert b.fused_launches == launches + periods and a.fused_launches == 0
    full = periods >= 4
    if full:
        assert int(b.rollout_stats["episodes"].min().item()) >= 2
    # no case passes on an empty store: it holds episodes ended by success and by the time limit
    her = b._her
    L = her.len.view(n, her.slots).long()
    last = her.reward.permute(2, 0, 1).gather(2, (L - 1).clamp(min=0).unsqueeze(-1)).squeeze(-1)
    print("n = %d: stored episodes ended by success %d, by the time limit %d"
          % (n, int(((L > 0) & (last == 0)).sum().item()), int(((L == 5) & (last < 0)).sum().item())))
    if n > 1 and full:
        assert bool(((L > 0) & (last == 0)).any().item()) and bool(((L == 5) & (last < 0)).any().item())
    if full:
        assert bool((L > 0).any().item())
    sa, sb = a._her.sample(256, seed=9), b._her.sample(256, seed=9)
    torch.cuda.synchronize()
    assert sorted(sa) == sorted(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    return got


GRID = [(n, systems, hidden) for n in (300, 65, 1) for systems in ((0,), (0, 1, 2, 3))
        for hidden in ((32,), (128, 128, 128))]


@pytest.mark.parametrize("n,systems,hidden", GRID, ids=["%d-sys%d-h%d" % (n, len(s), len(h)) for n, s, h in GRID])
def test_collect_gauss_matches_sample_and_step_bit_for_bit(cuda, n, systems, hidden):
    a, b = _make(cuda, n, systems=systems), _make(cuda, n, systems=systems)
    pi = _policy(a, cuda, hidden)
    assert pi.in_dim == (19 if len(systems) == 1 else 20)
    _check_periods(a, b, pi, counter=11)


def test_the_counter_runs_on_across_the_launches_of_a_call(cuda):
    """One call of 8 steps (two launches) = calls of 3 and 5 steps with counter and counter + 3 (the
    second split at the refill boundary again) = the eager loop."""
    import torch
    a, b, c = _make(cuda, 65), _make(cuda, 65), _make(cuda, 65)
    pi = _policy(a, cuda, (32,))
    want = _eager(a, pi, 8, 100)
    one = b.collect_gauss(pi, 8, counter=100, record_actions=True)
    two = torch.cat((c.collect_gauss(pi, 3, counter=100, record_actions=True),
                     c.collect_gauss(pi, 5, counter=103, record_actions=True)))
    assert b.fused_launches == 2 and c.fused_launches == 3
    for e, got in ((b, one), (c, two)):
        _same(a, e, KEYS, "8 steps")
        _same_store(a, e, "8 steps")
        assert torch.equal(want, got)
        assert a.refills == e.refills
    # a step's draw is its counter's: the same steps under another counter apply other actions
    d = _make(cuda, 65)
    assert not torch.equal(d.collect_gauss(pi, 1, counter=101, record_actions=True)[0], want[0])


@pytest.mark.parametrize("counter", [2 ** 32 - 2, (1 << 40) + 5], ids=["wraps_low_word", "high_word"])
def test_the_counter_is_a_64_bit_sum(cuda, counter):
    """counter = 2^32 - 2 over 4 steps: the low word wraps and the high word changes inside one launch."""
    a, b = _make(cuda, 65), _make(cuda, 65)
    pi = _policy(a, cuda, (32,))
    _check_periods(a, b, pi, counter=counter, periods=1)


def test_the_noise_row_is_the_global_env_id(cuda):
    import torch
    a, b, zero = _make(cuda, 65, env_base=1000), _make(cuda, 65, env_base=1000), _make(cuda, 65)
    assert a.env_base == 1000
    pi = _policy(a, cuda, (32,))
    mean = b.act(pi.mean_actor())                          # the deterministic policy on the first step's rows
    want = _eager(a, pi, R, 5)                             # row_base = 1000
    got = b.collect_gauss(pi, R, counter=5, record_actions=True)
    _same(a, b, KEYS, "env_base")
    _same_store(a, b, "env_base")
    assert torch.equal(want, got)
    # an env_base = 0 env built with the same seed applies other actions in its first step
    other = zero.collect_gauss(pi, 1, counter=5, record_actions=True)
    assert not torch.equal(other[0], got[0])
    # the noise reached the env: the applied actions are not the policy's mean
    assert not torch.equal(got[0], mean)


@pytest.mark.parametrize("kw", [dict(domain_rand=0.05), dict(model="rigid"),
                                dict(uy=True, integrator="rk4", rk4_steps_per_m=100)],
                         ids=["domain_rand", "rigid", "uy_rk4"])
def test_collect_gauss_in_the_other_kernel_modes(cuda, kw):
    kw = dict(kw)
    if kw.pop("uy", False):
        kw["ctr_systems_parameters"] = _uy_systems()
    a, b = _make(cuda, 300, **kw), _make(cuda, 300, **kw)
    _check_periods(a, b, _policy(a, cuda, (32,)))


def _untouched(a, b, where):
    _same(a, b, KEYS, where)
    if a._her is not None and b._her is not None:
        _same_store(a, b, where)
    assert b.fused_launches == 0 and a.refills == b.refills


def test_collect_gauss_refusals_leave_the_env_untouched(cuda):
    a, b = _make(cuda, 300, her=False), _make(cuda, 300, her=False)
    pi = _policy(a, cuda, (32,))
    with pytest.raises(RuntimeError, match=r"enable_her\(\)"):
        b.collect_gauss(pi, R, counter=0)
    _untouched(a, b, "no her")
    a, b = _make(cuda, 300), _make(cuda, 300)
    with pytest.raises(TypeError, match="GaussianActor"):
        b.collect_gauss(_actor(a, cuda, (32,)), R, counter=0)
    with pytest.raises(TypeError, match="GaussianActor"):
        b.collect_gauss(pi.mean_actor(), R, counter=0)
    _untouched(a, b, "MlpActor")
    # the compliant model's scipy RK45 with y pre-curvature: the kernel would need scratch
    kw = dict(ctr_systems_parameters=_uy_systems())
    a, b = _make(cuda, 300, **kw), _make(cuda, 300, **kw)
    pi = _policy(a, cuda, (32,))
    with pytest.raises(RuntimeError, match="scratch"):
        b.collect_gauss(pi, R, counter=0)
    rc = b.lib.ctr_collect_gauss(b.cfg, b._batch, pi._struct, pi.seed, 0, b._her._h, R, b._out, 2, None, None)
    msg = b.lib.ctr_last_error()
    assert rc == -1 and msg.startswith(b"ctr_collect_gauss: ") and b"scratch" in msg
    _untouched(a, b, "mode 1")
