"""HerReplayBuffer.sample_sac (ctr_her_sample_sac): ctr_her_sample's batch, bit for bit, plus SAC's
soft target of every drawn row: the current policy's stochastic action on next_obs under the noise
of the draw's own (seed, counter), its log-probability, the two target critics on it and
target = r + gamma (1 - done) (min(q1, q2) - alpha logp) with alpha = exp(log_alpha) read on the
device.  next_action and next_logp are bit-equal to the stand-alone ctr_gauss_act on a second,
identically filled buffer's next_obs, q1_next and q2_next to the stand-alone ctr_critic, target to
the float32 restatement; for policies of 1, 2 and 3 hidden layers; a row does not depend on the
batch size; each of the three blobs alone may size the LDS region; the two critics may be one; an
empty store gives the networks on zero rows; a captured graph reads the temperature at each replay.

What the inputs cover (log standard deviations above, inside and below the clip, saturated and
unsaturated actions, both critics giving the minimum, both values of done and reward) is asserted on
the stand-alone call's logits and on the reference values, never on the kernel under test."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GAMMA = 0.99
DRAW_SEED = 11
COUNTER = 3
LOG_ALPHAS = (0.0, float(np.float32(np.log(0.2))), -30.0)
# The policy's head: the mean rows times MEAN_GAIN; the log-std rows times STD_GAIN with STD_BIAS added,
# two dimensions each around the upper clip end, inside, and around the lower end, so that the shares
# of clipped and open log standard deviations do not hang on how much the store's rows vary.
MEAN_GAIN, STD_GAIN = 4.0, 8.0
STD_BIAS = (5.0, 1.5, -6.0, -12.0, -19.5, -25.0)
SCALE = np.array([0.001, 0.001, 0.001, 0.087, 0.087, 0.087])
BATCH_KEYS = ("obs", "action", "reward", "next_obs", "done", "index")


def _layers(rng, dims, out_gain=1.0):
    layers = []
    for l in range(len(dims) - 1):
        s = 1.0 / np.sqrt(dims[l])
        layers.append((rng.uniform(-s, s, (dims[l + 1], dims[l])).astype(np.float32),
                       rng.uniform(-s, s, dims[l + 1]).astype(np.float32)))
    W, b = layers[-1]
    layers[-1] = (W * np.float32(out_gain), b * np.float32(out_gain))
    return layers


def _policy_layers(rng, obs_dim, hidden):
    """A 12-row policy whose log standard deviations reach both clip ends (the header of this file)."""
    layers = _layers(rng, [obs_dim + 6] + list(hidden) + [12])
    W, b = (t.copy() for t in layers[-1])
    W[:6] *= np.float32(MEAN_GAIN)
    b[:6] *= np.float32(MEAN_GAIN)
    W[6:] *= np.float32(STD_GAIN)
    b[6:] = b[6:] * np.float32(STD_GAIN) + np.asarray(STD_BIAS, dtype=np.float32)
    layers[-1] = (W, b)
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


class Nets(object):
    """The policy handed to sample_sac (some scale, a seed of its own: neither is read), the same weights
    keyed by the draw seed for the stand-alone reference, and the two critics."""

    def __init__(self, cuda, obs_dim, policy_hidden=(64, 96), critic1_hidden=(96, 64), critic2_hidden=(32,), seed=21):
        from ctr_reach_amd.policy import GaussianActor, MlpCritic
        rng = np.random.default_rng(seed)
        self.cuda = cuda
        self.policy_layers = _policy_layers(rng, obs_dim, policy_hidden)
        self.policy = GaussianActor(self.policy_layers, SCALE, device=cuda, seed=999)
        self.reference = GaussianActor(self.policy_layers, SCALE, device=cuda, seed=DRAW_SEED)
        self.critic1 = MlpCritic(_layers(rng, [obs_dim + 12] + list(critic1_hidden) + [1]), device=cuda)
        self.layers2 = _layers(rng, [obs_dim + 12] + list(critic2_hidden) + [1])
        self.critic2 = MlpCritic(self.layers2, device=cuda)

    def balance(self, ref_buffer, counter=COUNTER):
        """Critic 2's output bias moved so that q2 - q1 has median 0 on the reference rows of the draw
        (stand-alone launches on the second buffer): min(q1, q2) then picks both critics."""
        from ctr_reach_amd.policy import MlpCritic
        ref = _reference(ref_buffer, self, 300, counter)
        shift = np.float32(np.median(ref["q2"].cpu().numpy() - ref["q1"].cpu().numpy()))
        W, b = self.layers2[-1]
        self.layers2 = self.layers2[:-1] + [(W, b - shift)]
        self.critic2 = MlpCritic(self.layers2, device=self.cuda)
        return self


def _reference(ref_buffer, nets, B, counter=COUNTER, critic1=None, critic2=None):
    """The stand-alone launches: the second buffer's ``sample``, ctr_gauss_act keyed (DRAW_SEED, counter,
    row_base 0) on its next_obs, the two ctr_critic calls on that action."""
    import torch
    ref_buffer._counter = counter
    ref = ref_buffer.sample(B, seed=DRAW_SEED, return_index=True)
    assert ref_buffer._counter == counter + 1
    st = nets.reference.sample(ref["next_obs"], counter=counter, row_base=0, logits=True)
    ref.update(unit=st["unit"], logp=st["logp"], logits=st["logits"])
    ref["q1"] = (critic1 or nets.critic1)(ref["next_obs"], st["unit"])
    ref["q2"] = (critic2 or nets.critic2)(ref["next_obs"], st["unit"])
    torch.cuda.synchronize()
    return ref


def _log_alpha(cuda, value):
    import torch
    return torch.tensor(float(value), dtype=torch.float32, device=cuda)


def _draw(her, B, nets, log_alpha, counter=COUNTER, policy=None, critic1=None, critic2=None, **kw):
    import torch
    her._counter = counter
    kw.setdefault("return_index", True)
    kw.setdefault("return_next", True)
    out = her.sample_sac(B, policy or nets.policy, critic1 or nets.critic1, critic2 or nets.critic2, GAMMA, log_alpha,
                         seed=DRAW_SEED, **kw)
    assert her._counter == counter + 1
    torch.cuda.synchronize()
    return out


def _bits(t):
    import torch
    return t.view(torch.int32)


def _target32(reward, done, q1, q2, logp, log_alpha):
    """The target as the header states it, in numpy float32: alpha from a float64 exp rounded once."""
    r, d, q1, q2, lp = (t.cpu().numpy() for t in (reward, done, q1, q2, logp))
    assert r.dtype == d.dtype == q1.dtype == q2.dtype == lp.dtype == np.float32
    g32 = np.float32(GAMMA)
    a32 = np.float32(np.exp(np.float64(np.float32(log_alpha))))
    want = np.where(d != 0, r, g32 * (np.minimum(q1, q2) - a32 * lp) + r)
    assert want.dtype == np.float32
    return want


def _check(out, ref, log_alpha, critic1, critic2):
    """Checks 1 and 2 of one draw against its reference: the batch, the action, its log-probability and
    the Qs bit for bit, the target against the float32 restatement."""
    import torch
    for k in BATCH_KEYS:
        assert torch.equal(out[k], ref[k]), k
    assert set(out) == set(BATCH_KEYS) | {"target", "q1_next", "q2_next", "next_action", "next_logp"}
    B = out["obs"].shape[0]
    assert out["target"].shape == out["q1_next"].shape == out["q2_next"].shape == out["next_logp"].shape == (B,)
    assert out["next_action"].shape == (B, 6)
    assert torch.equal(_bits(out["next_action"]), _bits(ref["unit"]))
    assert torch.equal(_bits(out["next_logp"]), _bits(ref["logp"]))
    q1, q2 = critic1(out["next_obs"], out["next_action"]), critic2(out["next_obs"], out["next_action"])
    torch.cuda.synchronize()
    assert torch.equal(_bits(out["q1_next"]), _bits(q1)) and torch.equal(_bits(out["q2_next"]), _bits(q2))
    assert torch.equal(_bits(q1), _bits(ref["q1"])) and torch.equal(_bits(q2), _bits(ref["q2"]))
    want = _target32(ref["reward"], ref["done"], ref["q1"], ref["q2"], ref["logp"], log_alpha)
    tg = out["target"].cpu().numpy()
    assert np.isfinite(want).all()
    assert np.array_equal(tg.view(np.uint32), want.view(np.uint32))
    done, rew = ref["done"].cpu().numpy(), ref["reward"].cpu().numpy()
    assert np.array_equal(tg[done != 0], rew[done != 0])
    return tg


@pytest.fixture(scope="module", params=[(0,), (0, 1, 2, 3)], ids=["one_system", "four_systems"])
def twin(cuda, request):
    """Two identically built and filled buffers and the networks (built once, not modified: sampling
    writes the buffers' scan scratch only), and the references of the draws the tests share."""
    import torch
    a, b = _store(cuda, request.param), _store(cuda, request.param)
    assert a.obs_dim == (13 if len(request.param) == 1 else 14)
    torch.cuda.synchronize()
    assert len(a) > 0
    nets = Nets(cuda, a.obs_dim).balance(b)
    refs = {B: _reference(b, nets, B) for B in (1, 65, 300)}
    return a, b, nets, refs


def test_the_inputs_cover_the_head_the_minimum_and_the_flags(twin):
    """Check 4, on the stand-alone call's outputs and the reference values of the 300 draws."""
    _, _, _, refs = twin
    ref = refs[300]
    raw = ref["logits"].cpu().numpy()[:, 6:]
    above, below = (raw > 2).mean(), (raw < -20).mean()
    inside = ((raw >= -20) & (raw <= 2)).mean()
    unit = np.abs(ref["unit"].cpu().numpy())
    q1, q2, done, rew = (ref[k].cpu().numpy() for k in ("q1", "q2", "done", "reward"))
    print("log std above 2: %.3f, below -20: %.3f, inside: %.3f; |unit| == 1: %.3f, < 0.5: %.3f; q2 < q1: %.3f; "
          "done: %.3f; reward -1: %.3f" % (above, below, inside, (unit == 1).mean(), (unit < 0.5).mean(), (q2 < q1).mean(),
                                           (done != 0).mean(), (rew == -1).mean()))
    assert above >= 0.05 and below >= 0.05 and inside >= 0.30, (above, below, inside)
    assert (unit == 1).any() and (unit < 0.5).any()
    assert 0.25 <= (q2 < q1).mean() <= 0.75, (q2 < q1).mean()
    assert (done == 1).any() and (done == 0).any() and (rew == 0).any() and (rew == -1).any()
    assert np.isfinite(ref["logp"].cpu().numpy()).all()
    assert len(np.unique(q1)) > 100 and len(np.unique(q2)) > 100


def test_batch_action_logp_qs_and_target(cuda, twin):
    """Checks 1, 2, 5, 6 and 7."""
    import torch
    a, b, nets, refs = twin
    got = {}
    for la in LOG_ALPHAS:
        for B in (1, 65, 300):
            out = got[la, B] = _draw(a, B, nets, _log_alpha(cuda, la))
            _check(out, refs[B], la, nets.critic1, nets.critic2)
    # the temperature is in the target: three values, three targets on the rows that bootstrap
    live = refs[300]["done"].cpu().numpy() == 0
    tg = [got[la, 300]["target"].cpu().numpy()[live] for la in LOG_ALPHAS]
    assert live.any() and not np.array_equal(tg[0], tg[1]) and not np.array_equal(tg[1], tg[2]) \
        and not np.array_equal(tg[0], tg[2])
    assert not np.array_equal(tg[0], refs[300]["reward"].cpu().numpy()[live])
    # a row of a draw does not depend on the batch size: rows 0..64 of the 300 are the 65, row 0 is the 1
    for la in LOG_ALPHAS:
        for k in got[la, 65]:
            assert torch.equal(_bits(got[la, 300][k][:65]), _bits(got[la, 65][k])), (la, k)
            assert torch.equal(_bits(got[la, 300][k][:1]), _bits(got[la, 1][k])), (la, k)
    # another counter is another draw, of rows and of noise
    la = LOG_ALPHAS[1]
    other = _draw(a, 65, nets, _log_alpha(cuda, la), counter=COUNTER + 1)
    ref = _reference(b, nets, 65, counter=COUNTER + 1)
    assert not torch.equal(other["obs"], got[la, 65]["obs"])
    assert not torch.equal(other["next_action"], got[la, 65]["next_action"])
    _check(other, ref, la, nets.critic1, nets.critic2)
    same_rows_old_noise = nets.reference.sample(ref["next_obs"], counter=COUNTER, row_base=0)["unit"]
    torch.cuda.synchronize()
    assert not torch.equal(other["next_action"], same_rows_old_noise)
    # without return_next / return_index: sample's keys plus target, the same bits
    plain = _draw(a, 65, nets, _log_alpha(cuda, la), return_index=False, return_next=False)
    assert set(plain) == {"obs", "action", "reward", "next_obs", "done", "target"}
    for k in plain:
        assert torch.equal(_bits(plain[k]), _bits(got[la, 65][k])), k
    # a 1-element temperature is the 0-d one; the policy's scale and its own seed are not read
    from ctr_reach_amd.policy import GaussianActor
    unit_policy = GaussianActor(nets.policy_layers, np.ones(6), device=cuda, seed=5)
    again = _draw(a, 65, nets, _log_alpha(cuda, la).reshape(1), policy=unit_policy)
    for k in again:
        assert torch.equal(_bits(again[k]), _bits(got[la, 65][k])), k


@pytest.mark.parametrize("hidden", [(32,), (64, 96), (32, 64, 32)], ids=["1_hidden", "2_hidden", "3_hidden"])
def test_policies_of_one_two_and_three_hidden_layers(cuda, twin, hidden):
    """Check 3: gauss_logits takes the output bias of rows 8..11 by the number of hidden layers."""
    a, b, _, _ = twin
    nets = Nets(cuda, a.obs_dim, policy_hidden=hidden, seed=40 + len(hidden))
    for B in (65, 300):
        ref = _reference(b, nets, B, counter=6)
        out = _draw(a, B, nets, _log_alpha(cuda, LOG_ALPHAS[1]), counter=6)
        _check(out, ref, LOG_ALPHAS[1], nets.critic1, nets.critic2)
    raw = ref["logits"].cpu().numpy()[:, 6:]
    assert (raw > 2).any() and (raw < -20).any() and ((raw >= -20) & (raw <= 2)).any()
    assert len(np.unique(ref["logits"].cpu().numpy()[:, 8:])) > 100        # rows 8..11: the second half of the tile


@pytest.mark.parametrize("large", ["policy", "critic1", "critic2"])
def test_each_blob_alone_sizes_the_lds_region(cuda, twin, large):
    """Check 8: a (256, 128) network, more than 8 times the other two blobs, in each of the three places."""
    a, b, _, _ = twin
    hidden = {"policy": (32,), "critic1": (32,), "critic2": (32,)}
    hidden[large] = (256, 128)
    nets = Nets(cuda, a.obs_dim, hidden["policy"], hidden["critic1"], hidden["critic2"], seed=33)
    sizes = {"policy": nets.policy.blob.numel(), "critic1": nets.critic1.blob.numel(), "critic2": nets.critic2.blob.numel()}
    assert sizes[large] > 64 * 1024 and sizes[large] > 8 * max(v for k, v in sizes.items() if k != large), sizes
    for la in (LOG_ALPHAS[0], LOG_ALPHAS[1]):
        ref = _reference(b, nets, 300, counter=9)
        out = _draw(a, 300, nets, _log_alpha(cuda, la), counter=9)
        _check(out, ref, la, nets.critic1, nets.critic2)
    assert len(np.unique(out["q1_next"].cpu().numpy())) > 100 and len(np.unique(out["q2_next"].cpu().numpy())) > 100


def test_the_two_critics_may_be_one(cuda, twin):
    """Check 9."""
    import torch
    a, b, nets, _ = twin
    for critic in (nets.critic1, nets.critic2):
        ref = _reference(b, nets, 65, critic1=critic, critic2=critic)
        out = _draw(a, 65, nets, _log_alpha(cuda, LOG_ALPHAS[1]), critic1=critic, critic2=critic)
        _check(out, ref, LOG_ALPHAS[1], critic, critic)
        assert torch.equal(_bits(out["q1_next"]), _bits(out["q2_next"]))


def test_an_empty_store_gives_the_networks_on_zero_rows(cuda):
    """Check 10."""
    import torch
    from ctr_reach_amd import CtrReachVecEnv

    def empty():
        env = CtrReachVecEnv(96, device=cuda, seed=7, max_steps_per_episode=5)
        her = env.enable_her(slots=3)
        env.reset()                                       # episodes are open, none is stored
        return her

    a, b = empty(), empty()
    nets = Nets(cuda, 13)
    for la in LOG_ALPHAS[:2]:
        ref = _reference(b, nets, 65, counter=0)
        out = _draw(a, 65, nets, _log_alpha(cuda, la), counter=0)
        assert (out["index"][:, 0] == -1).all() and not out["index"][:, 1:].any()
        for k in ("obs", "action", "reward", "next_obs", "done"):
            assert not out[k].any(), k
        tg = _check(out, ref, la, nets.critic1, nets.critic2)
        # the networks ran: the zero row's logits are the biases' doing, the noise differs row by row
        assert ref["logits"].cpu().numpy().any() and len(np.unique(out["next_logp"].cpu().numpy())) > 32
        assert tg.any() and torch.isfinite(out["target"]).all()


def test_a_captured_graph_reads_the_temperature_at_each_replay(cuda, twin):
    """Check 11."""
    import torch
    a, b, nets, _ = twin
    first, second = LOG_ALPHAS[1], -1.25
    log_alpha = _log_alpha(cuda, first)
    ref = _reference(b, nets, 65, counter=5)
    eager = _draw(a, 65, nets, log_alpha, counter=5)     # (the kernels' first launches are not the captured ones)
    _check(eager, ref, first, nets.critic1, nets.critic2)
    a._counter = 5
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                          # three launches on one stream: no parallel branches
        out = a.sample_sac(65, nets.policy, nets.critic1, nets.critic2, GAMMA, log_alpha, seed=DRAW_SEED, return_index=True,
                           return_next=True)
    for replay in range(2):                                # a replay draws the captured counter again
        for k in out:
            out[k].zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k in eager:
            assert torch.equal(_bits(out[k]), _bits(eager[k])), (replay, k)
    log_alpha.fill_(second)                                # no recapture: the kernel reads the value on the device
    for k in out:
        out[k].zero_()
    graph.replay()
    torch.cuda.synchronize()
    tg = _check(out, ref, second, nets.critic1, nets.critic2)
    live = ref["done"].cpu().numpy() == 0
    assert live.any() and not np.array_equal(tg[live], eager["target"].cpu().numpy()[live])
