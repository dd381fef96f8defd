"""HerReplayBuffer.sample_td3 (ctr_her_sample_td3): ctr_her_sample's batch, bit for bit, plus TD3's
clipped double-Q target of every drawn row: the target policy's action, smoothed by clipped Gaussian
noise keyed by (seed, counter, row), and the smaller of two target critics on it.  q1_next, q2_next
and target are bit-equal to the stand-alone launches on the kernel's own next_action and to the
float32 restatement of the target; the smoothed action is held to policy.TargetSmoothing within 4x
the error measured on an MI355X; sigma = 0 with one critic twice is sample_td bit for bit; clip =
inf is any clip the draw does not reach; a draw does not depend on the batch size; the dynamic LDS
region is sized by the largest of the three blobs; an empty store gives the networks on zero rows;
the call can be captured into a graph."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GAMMA = 0.99
DRAW_SEED = 11
COUNTER = 3
SIGMA, CLIP = 0.2, 0.5

# max |next_action - TargetSmoothing.emulate(11, 3, row, a')| over the B = 300 draws of both stores
# below (sigma 0.2, clip 0.5, a' from the stand-alone unit-scale actor), measured on an MI355X against
# the float64 restatement.  It is the error of f32 logf, sqrtf, sinf, cosf, of the two f32 products
# around them and of the f32 sum (half an ulp of a value in [0.5, 1) is 2.98e-08), not a
# statistical figure: 1.420e-07 on the one-system store, 1.750e-07 on the four-system one.  The test
# allows 4x.
SMOOTH_ERR_MEASURED = 1.750e-07


def _layers(rng, dims, out_gain=1.0):
    layers = []
    for l in range(len(dims) - 1):
        s = 1.0 / np.sqrt(dims[l])
        layers.append((rng.uniform(-s, s, (dims[l + 1], dims[l])).astype(np.float32),
                       rng.uniform(-s, s, dims[l + 1]).astype(np.float32)))
    W, b = layers[-1]
    layers[-1] = (W * np.float32(out_gain), b * np.float32(out_gain))
    return layers


def _store(cuda, systems):
    """A 96-env store with 5-step episodes and 3 slots, filled by one collect of 20 steps."""
    from ctr_reach_amd import CtrReachVecEnv
    from ctr_reach_amd.policy import ExploreNoise, MlpActor
    env = CtrReachVecEnv(96, device=cuda, seed=7, max_steps_per_episode=5, refill_interval=4, select_systems=list(systems))
    env.goal_tolerance.current_tol = 0.03
    her = env.enable_her(slots=3)
    env.reset()
    rng = np.random.default_rng(2)
    behaviour = MlpActor(_layers(rng, [env.obs_dim + 6, 32, 6], out_gain=8.0), env.action_space.high, device=cuda)
    env.collect(behaviour, 20, ExploreNoise(0.2, random_eps=0.3, seed=1))
    return her


def _networks(cuda, obs_dim, actor_hidden=(64, 96), critic1_hidden=(96, 64), critic2_hidden=(32,), seed=21):
    """(the target policy with some scale, the same weights with a scale of ones, critic 1, critic 2's
    layers); the policy's output layer is scaled up so that tanh leaves its linear range."""
    from ctr_reach_amd.policy import MlpActor, MlpCritic
    rng = np.random.default_rng(seed)
    la = _layers(rng, [obs_dim + 6] + list(actor_hidden) + [6], out_gain=8.0)
    l1 = _layers(rng, [obs_dim + 12] + list(critic1_hidden) + [1])
    l2 = _layers(rng, [obs_dim + 12] + list(critic2_hidden) + [1])
    scale = np.array([0.001, 0.001, 0.001, 0.087, 0.087, 0.087])
    return MlpActor(la, scale, device=cuda), MlpActor(la, np.ones(6), device=cuda), MlpCritic(l1, device=cuda), l2


def _balanced_critic2(cuda, her, actor, critic1, layers2, counter):
    """Critic 2 with its output bias moved so that q2 - q1 has median 0 on the sample_td rows of the
    draw (a stand-alone ctr_critic pass): min(q1, q2) then picks both critics."""
    import torch
    from ctr_reach_amd.policy import MlpCritic
    her._counter = counter
    rows = her.sample_td(300, actor, critic1, GAMMA, seed=DRAW_SEED, return_next=True)
    q2 = MlpCritic(layers2, device=cuda)(rows["next_obs"], rows["next_action"])
    torch.cuda.synchronize()
    shift = np.float32(np.median((q2 - rows["q_next"]).cpu().numpy()))
    W, b = layers2[-1]
    return MlpCritic(layers2[:-1] + [(W, b - shift)], device=cuda)


@pytest.fixture(scope="module", params=[(0,), (0, 1, 2, 3)], ids=["one_system", "four_systems"])
def twin(cuda, request):
    """Two identically built and filled buffers and the target networks (built once, not modified:
    sampling writes the buffers' scan scratch only)."""
    import torch
    a, b = _store(cuda, request.param), _store(cuda, request.param)
    assert a.obs_dim == (13 if len(request.param) == 1 else 14)
    torch.cuda.synchronize()
    assert len(a) > 0
    actor, unit_actor, critic1, layers2 = _networks(cuda, a.obs_dim)
    critic2 = _balanced_critic2(cuda, a, actor, critic1, layers2, COUNTER)
    return a, b, actor, unit_actor, critic1, critic2


def _draw(her, B, actor, critic1, critic2, counter=COUNTER, seed=DRAW_SEED, sigma=SIGMA, clip=CLIP):
    her._counter = counter
    out = her.sample_td3(B, actor, critic1, critic2, GAMMA, sigma=sigma, clip=clip, seed=seed, return_index=True,
                         return_next=True)
    assert her._counter == counter + 1
    return out


def _target32(reward, done, q1, q2):
    """The target as the header states it: float32, the smaller q, two roundings."""
    r, d, q1, q2 = (t.cpu().numpy() for t in (reward, done, q1, q2))
    assert r.dtype == d.dtype == q1.dtype == q2.dtype == np.float32
    return np.where(d != 0, r, np.float32(GAMMA) * np.minimum(q1, q2) + r)


def _check_against_stand_alone(out, critic1, critic2):
    """q1_next, q2_next and target from the kernel's own next_action."""
    import torch
    q1, q2 = critic1(out["next_obs"], out["next_action"]), critic2(out["next_obs"], out["next_action"])
    torch.cuda.synchronize()
    assert torch.equal(out["q1_next"], q1) and torch.equal(out["q2_next"], q2)
    tg = out["target"].cpu().numpy()
    assert np.array_equal(tg.view(np.uint32), _target32(out["reward"], out["done"], q1, q2).view(np.uint32))
    done, rew = out["done"].cpu().numpy(), out["reward"].cpu().numpy()
    assert np.array_equal(tg[done != 0], rew[done != 0])


def _check_noise(out, unit_actor, counter=COUNTER, sigma=SIGMA, clip=CLIP):
    """next_action against the float64 restatement on a' from the stand-alone unit-scale actor (whose
    1.0f * tanhf(y) keeps the bits of the kernel's tanhf: tests/test_gpu_td_target.py).  -> the error."""
    import torch
    from ctr_reach_amd.policy import TargetSmoothing
    a1 = unit_actor(out["next_obs"])
    torch.cuda.synchronize()
    a1 = a1.cpu().numpy()
    got = out["next_action"].cpu().numpy()
    B = got.shape[0]
    want = TargetSmoothing(sigma, clip).emulate(DRAW_SEED, counter, np.arange(B), a1)
    err = np.abs(got.astype(np.float64) - want).max()
    print("B = %d: max |next_action - emulate| = %.3e" % (B, err))
    assert err <= 4 * SMOOTH_ERR_MEASURED, err
    assert (np.abs(got) <= 1).all()
    moved = got.astype(np.float64) - a1.astype(np.float64)
    assert (np.abs(moved) <= clip + 2.0 ** -24).all(), np.abs(moved).max()
    return a1, got, moved, err


def test_batch_target_and_noise(twin):
    import torch
    a, b, actor, unit_actor, critic1, critic2 = twin
    got = {}
    for B in (1, 65, 300):
        out = got[B] = _draw(a, B, actor, critic1, critic2)
        b._counter = COUNTER
        ref = b.sample(B, seed=DRAW_SEED, return_index=True)
        torch.cuda.synchronize()
        assert b._counter == COUNTER + 1
        for k in ("obs", "action", "reward", "next_obs", "done", "index"):
            assert torch.equal(out[k], ref[k]), (B, k)
        assert set(out) == set(ref) | {"target", "q1_next", "q2_next", "next_action"}
        assert out["target"].shape == out["q1_next"].shape == out["q2_next"].shape == (B,)
        assert out["next_action"].shape == (B, 6)
        _check_against_stand_alone(out, critic1, critic2)
        _check_noise(out, unit_actor)
    out = got[300]
    done, rew = out["done"].cpu().numpy(), out["reward"].cpu().numpy()
    assert (done == 1).any() and (done == 0).any() and (rew == 0).any() and (rew == -1).any()
    q1, q2, tg = (out[k].cpu().numpy() for k in ("q1_next", "q2_next", "target"))
    assert 0.25 <= (q2 < q1).mean() <= 0.75, (q2 < q1).mean()
    live = done == 0
    assert (q1[live] < q2[live]).any() and (q2[live] < q1[live]).any()
    assert not np.array_equal(tg[live], rew[live]) and len(np.unique(q1)) > 100 and len(np.unique(q2)) > 100
    # the noise is there, clipped where it is large, and the box holds where the action is near a face
    a1, na, moved, _ = _check_noise(out, unit_actor)
    bar = 4 * SMOOTH_ERR_MEASURED
    far = np.abs(a1) <= 1 - CLIP - 1e-3                    # a' + e cannot reach the box
    assert (far & (np.abs(moved) >= CLIP - bar)).any() and (far & (np.abs(moved) < CLIP - bar) & (moved != 0)).any()
    assert 0.05 < np.abs(moved[far]).mean() < 0.2          # sigma sqrt(2 / pi) = 0.16 unclipped
    assert (np.abs(na) == 1).any()
    # a row of a draw does not depend on the batch size: rows 0..64 of the 300 are the 65
    for k in got[65]:
        assert torch.equal(got[300][k][:65], got[65][k]), k
        assert torch.equal(got[300][k][:1], got[1][k]), k
    # another counter is another draw, of rows and of noise
    other = _draw(a, 65, actor, critic1, critic2, counter=COUNTER + 1)
    torch.cuda.synchronize()
    assert not torch.equal(other["obs"], got[65]["obs"])
    _check_noise(other, unit_actor, counter=COUNTER + 1)
    # the scale of the target policy is not read; without return_next / return_index the same target
    again = _draw(a, 65, unit_actor, critic1, critic2)
    a._counter = COUNTER
    plain = a.sample_td3(65, actor, critic1, critic2, GAMMA, seed=DRAW_SEED)
    torch.cuda.synchronize()
    assert torch.equal(again["target"], got[65]["target"]) and torch.equal(again["next_action"], got[65]["next_action"])
    assert set(plain) == {"obs", "action", "reward", "next_obs", "done", "target"}
    assert torch.equal(plain["target"], got[65]["target"])


def test_no_noise_and_one_critic_is_sample_td(twin):
    import torch
    a, _, actor, unit_actor, critic1, critic2 = twin
    for B in (65, 300):
        out = _draw(a, B, actor, critic1, critic1, sigma=0.0)
        a._counter = COUNTER
        ref = a.sample_td(B, actor, critic1, GAMMA, seed=DRAW_SEED, return_index=True, return_next=True)
        torch.cuda.synchronize()
        for k in ("obs", "action", "reward", "next_obs", "done", "index", "target", "next_action"):
            assert torch.equal(out[k].view(torch.int32), ref[k].view(torch.int32)), (B, k)
        assert torch.equal(out["q1_next"], ref["q_next"]) and torch.equal(out["q2_next"], ref["q_next"])
    # sigma = 0 with the two critics: the unsmoothed action, the smaller q
    out = _draw(a, 300, actor, critic1, critic2, sigma=0.0)
    torch.cuda.synchronize()
    assert torch.equal(out["next_action"], ref["next_action"])
    _check_against_stand_alone(out, critic1, critic2)


def test_an_infinite_clip_is_any_clip_the_draw_does_not_reach(twin):
    import torch
    from ctr_reach_amd.policy import TargetSmoothing
    a, _, actor, unit_actor, critic1, critic2 = twin
    z = TargetSmoothing(SIGMA, np.inf).gaussians(DRAW_SEED, COUNTER, np.arange(300))
    reach = float(np.float32(SIGMA)) * np.abs(z).max()
    assert reach > CLIP                                    # (the default clip does cut this draw)
    free = _draw(a, 300, actor, critic1, critic2, clip=float("inf"))
    wide = _draw(a, 300, actor, critic1, critic2, clip=reach + 0.01)
    cut = _draw(a, 300, actor, critic1, critic2)
    torch.cuda.synchronize()
    for k in free:
        assert torch.equal(free[k], wide[k]), k
    assert not torch.equal(free["next_action"], cut["next_action"])
    _check_against_stand_alone(free, critic1, critic2)
    _check_noise(free, unit_actor, clip=np.inf)


def test_critic2_alone_sizes_the_lds_region(cuda, twin):
    """A 91 776 B critic 2 behind a small actor and a small critic 1: the dynamic region is sized by the
    largest of the three blobs, which is staged last."""
    import torch
    from ctr_reach_amd.policy import MlpCritic
    a = twin[0]
    actor, unit_actor, critic1, layers2 = _networks(cuda, a.obs_dim, (32,), (32,), (256, 128), seed=33)
    critic2 = MlpCritic(layers2, device=cuda)
    assert critic2.blob.numel() > 64 * 1024 > 8 * max(actor.blob.numel(), critic1.blob.numel())
    out = _draw(a, 300, actor, critic1, critic2, counter=9)
    torch.cuda.synchronize()
    _check_against_stand_alone(out, critic1, critic2)
    _check_noise(out, unit_actor, counter=9)
    assert len(np.unique(out["q2_next"].cpu().numpy())) > 100
    # ... and as critic 1, and as both
    for c1, c2 in ((critic2, critic1), (critic2, critic2)):
        out = _draw(a, 65, actor, c1, c2, counter=9)
        torch.cuda.synchronize()
        _check_against_stand_alone(out, c1, c2)


def test_an_empty_store_gives_the_networks_on_zero_rows(cuda):
    import torch
    from ctr_reach_amd import CtrReachVecEnv
    from ctr_reach_amd.policy import MlpCritic
    env = CtrReachVecEnv(96, device=cuda, seed=7, max_steps_per_episode=5)
    her = env.enable_her(slots=3)
    env.reset()                                           # episodes are open, none is stored
    actor, unit_actor, critic1, layers2 = _networks(cuda, 13)
    critic2 = MlpCritic(layers2, device=cuda)
    out = _draw(her, 65, actor, critic1, critic2, counter=0)
    torch.cuda.synchronize()
    assert (out["index"][:, 0] == -1).all() and not out["index"][:, 1:].any()
    for k in ("obs", "action", "reward", "next_obs", "done"):
        assert not out[k].any(), k
    _check_noise(out, unit_actor, counter=0)
    _check_against_stand_alone(out, critic1, critic2)
    q = torch.minimum(out["q1_next"], out["q2_next"]).cpu().numpy()
    assert q.any() and np.array_equal(out["target"].cpu().numpy(), np.float32(GAMMA) * q + np.float32(0))


def test_the_call_can_be_captured_into_a_graph(twin):
    import torch
    a, _, actor, unit_actor, critic1, critic2 = twin
    eager = _draw(a, 65, actor, critic1, critic2, counter=5)   # (the kernels' first launches are not the captured ones)
    torch.cuda.synchronize()
    a._counter = 5
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                          # three launches on one stream: no parallel branches
        out = a.sample_td3(65, actor, critic1, critic2, GAMMA, sigma=SIGMA, clip=CLIP, seed=DRAW_SEED, return_index=True,
                           return_next=True)
    for replay in range(2):                                # a replay draws the captured counter again
        for k in out:
            out[k].zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k in eager:
            assert torch.equal(out[k], eager[k]), (replay, k)
