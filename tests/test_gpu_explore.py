"""CtrReachVecEnv.explore (ctr_explore: the exploration noise as a launch of its own) against
policy.ExploreNoise.emulate, its numpy restatement: the random branch and the choice between the
branches bit for bit, the Gaussian branch to the f32 logf / sinf / cosf error measured on the
MI355X; the rows do not depend on the sharding; sigma = 0 and random_eps = 0 keep the bits."""
import numpy as np
import pytest

from test_gpu_rollout import _actor

pytestmark = pytest.mark.gpu

# max |device - emulate| / scale of the Gaussian branch (sigma 0.3, random_eps 0, the actor's
# actions, the 300 envs of `world`), measured on an MI355X against the float64 restatement:
# 2.024e-07.  It is the error of f32 logf, sqrtf, sinf, cosf and of the f32 products and the
# fused multiply-add around them (an ulp of a value in [1, 2) is 2^-23 = 1.19e-07), not a statistical
# figure.  The test allows 4x.
GAUSS_ERR_MEASURED = 2.024e-07


def _env(cuda, n, env_base=0):
    from ctr_reach_amd import CtrReachVecEnv
    e = CtrReachVecEnv(n, device=cuda, seed=7, env_base=env_base, max_steps_per_episode=5, refill_interval=4,
                       select_systems=[0, 1, 2, 3])
    e.goal_tolerance.current_tol = 0.03
    e.reset()
    return e


def _walk(env, actions):
    """Seven steps with fixed action rows: episodes of 5 steps at most, some ended by success, so
    the clocks and the reset numbers differ between the envs."""
    for a in actions:
        env.step_raw(a)


def _fixed_actions(cuda, n, steps=7, seed=3):
    import torch
    from ctr_reach_amd.systems import default_kwargs
    from ctr_reach_amd.vec_env import action_space
    rng = np.random.default_rng(seed)
    kw = default_kwargs()
    high = action_space(kw["extension_action_limit"], kw["rotation_action_limit"]).high
    return [torch.tensor((rng.uniform(-1, 1, (n, 6)) * high).astype(np.float32), device=cuda) for _ in range(steps)]


@pytest.fixture(scope="module")
def world(cuda):
    """300 envs walked seven steps, an actor's actions on them, and the keys of their next step."""
    import torch
    env = _env(cuda, 300)
    _walk(env, _fixed_actions(cuda, 300))
    actor = _actor(env, cuda, (32,))
    act = env.act(actor)
    torch.cuda.synchronize()
    t, epoch = env.t.cpu().numpy(), env.epoch.cpu().numpy()
    assert len(np.unique(t)) >= 3 and len(np.unique(epoch)) >= 2
    return dict(env=env, act=act, t=t, epoch=epoch, genv=np.arange(300), scale=env.action_space.high)


def _noise(*a, **kw):
    from ctr_reach_amd.policy import ExploreNoise
    return ExploreNoise(*a, **kw)


def _emulate(w, noise, act):
    return noise.emulate(w["genv"], w["epoch"], w["t"], act.cpu().numpy(), w["scale"])


def test_random_branch_matches_emulate_bit_for_bit(world):
    noise = _noise(0.3, random_eps=1.0, seed=5)
    got = world["env"].explore(world["act"].clone(), noise).cpu().numpy()
    want = _emulate(world, noise, world["act"])
    assert noise.last_random.all()
    assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32))
    assert np.array_equal(got.astype(np.float64), want)
    assert (np.abs(got) <= world["scale"]).all() and len(np.unique(got[:, 0])) > 250


def test_gaussian_branch_matches_emulate_to_the_f32_functions_error(world):
    noise = _noise(0.3, random_eps=0.0, seed=5)
    got = world["env"].explore(world["act"].clone(), noise).cpu().numpy().astype(np.float64)
    want = _emulate(world, noise, world["act"])
    scale = world["scale"].astype(np.float64)
    err = np.abs(got - want) / scale
    print("gaussian branch: max |device - emulate| / scale = %.3e" % err.max())
    assert err.max() <= 4 * GAUSS_ERR_MEASURED, err.max()
    # a row clipped on one side only is within the same bound of the face (the clamp is continuous)
    one_sided = (np.abs(got) == scale) != (np.abs(want) == scale)
    assert (err[one_sided] <= 4 * GAUSS_ERR_MEASURED).all()
    # the noise is there: unclipped, sigma 0.3 of the box moves an action by 0.3 sqrt(2 / pi) = 0.24 of
    # it on average; the clip takes at most the outward half of that away
    moved = np.abs(got - world["act"].cpu().numpy()) / scale
    assert 0.08 < moved.mean() < 0.27 and 0.0 < (np.abs(got) == scale).mean() < 0.9


def test_mixed_rows_take_the_branch_emulate_takes(world):
    noise = _noise(0.3, random_eps=0.3, seed=5)
    got = world["env"].explore(world["act"].clone(), noise).cpu().numpy()
    want = _emulate(world, noise, world["act"])
    rnd = noise.last_random
    assert 40 < rnd.sum() < 150                                   # 300 rows at 0.3
    assert np.array_equal(got[rnd].view(np.uint32), want[rnd].astype(np.float32).view(np.uint32))
    scale = world["scale"].astype(np.float64)
    err = np.abs(got.astype(np.float64) - want) / scale
    assert err[~rnd].max() <= 4 * GAUSS_ERR_MEASURED
    # ... and only those: a Gaussian row is not a uniform row of the same key
    other = _noise(0.3, random_eps=1.0, seed=5)
    uniform = _emulate(world, other, world["act"])
    assert (np.abs(got.astype(np.float64) - uniform)[~rnd].max(axis=1) > 0).all()


def test_rows_do_not_depend_on_the_sharding(cuda, world):
    import torch
    acts = _fixed_actions(cuda, 300)
    lo, hi = _env(cuda, 150, 0), _env(cuda, 150, 150)
    _walk(lo, [a[:150].contiguous() for a in acts])
    _walk(hi, [a[150:].contiguous() for a in acts])
    full = world["env"]
    torch.cuda.synchronize()
    assert torch.equal(torch.cat((lo.t, hi.t)), full.t) and torch.equal(torch.cat((lo.epoch, hi.epoch)), full.epoch)
    noise = _noise(0.3, random_eps=0.3, seed=5)
    want = full.explore(world["act"].clone(), noise)
    got = torch.cat((lo.explore(world["act"][:150].clone(), noise), hi.explore(world["act"][150:].clone(), noise)))
    assert torch.equal(got, want)
    # the second shard's rows are not the first's: the key has the global env id
    assert not torch.equal(hi.explore(world["act"][:150].clone(), noise), got[:150])


@pytest.mark.parametrize("n", [300, 65, 1])
def test_noop_keeps_the_bits_and_small_batches_match(cuda, n):
    import torch
    env = _env(cuda, n)
    _walk(env, _fixed_actions(cuda, n, steps=3))
    act = _fixed_actions(cuda, n, steps=1, seed=9)[0]
    act[0, 0] = -0.0
    act[0, 1] = 5.0                                               # outside the box: stays there
    same = env.explore(act.clone(), _noise(0.0, random_eps=0.0, seed=5))
    assert torch.equal(same.view(torch.int32), act.view(torch.int32))
    assert env.explore(act, _noise(0.0)) is act                   # in place on a contiguous float32 tensor
    noise = _noise(0.3, random_eps=1.0, seed=5)
    got = env.explore(act.clone(), noise).cpu().numpy()
    want = noise.emulate(np.arange(n), env.epoch.cpu().numpy(), env.t.cpu().numpy(), act.cpu().numpy(),
                         env.action_space.high)
    assert np.array_equal(got.astype(np.float64), want)
    with pytest.raises(ValueError):
        env.explore(torch.zeros((n + 1, 6), device=cuda), noise)
