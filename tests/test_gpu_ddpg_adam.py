"""DdpgLearner's Adam step and its bookkeeping on the GPU: from the gradients a step stored, the numpy
float32 restatement (learner.adam_reference, held to torch.optim.Adam in tests/test_host_ddpg.py)
gives the parameters, m, v and pow bit for bit, over three consecutive steps and for two pairs of
betas; a step repeated from a restored state repeats every bit; a captured pair of steps replays as
eager steps do; the actor's step leaves the critic alone and nothing is written beside the gradient
and state tensors; and the two losses go down on a fixed batch."""
import numpy as np
import pytest

import ddpg_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(0x4B3C2D1E)
GAP = 8


class _Carver(object):
    """``alloc`` for a DdpgLearner: zeroed tensors carved from one buffer of sentinels, each starting
    at an odd float offset with GAP sentinel floats behind it."""

    def __init__(self, cuda, floats=1 << 20):
        import torch
        self.buf = torch.from_numpy(np.full(floats, SENTINEL, dtype=np.uint32).view(np.float32)).to(cuda)
        self.guard = np.ones(floats, dtype=bool)
        self.off = 1

    def __call__(self, shape):
        n = int(np.prod(shape))
        view = self.buf[self.off:self.off + n].view(*shape)
        view.zero_()
        self.guard[self.off:self.off + n] = False
        self.off += n + GAP + (n + GAP) % 2
        assert self.off < self.buf.numel()
        return view

    def intact(self):
        return bool((R.bits(self.buf.cpu().numpy())[self.guard] == SENTINEL).all())


def _setup(cuda, seed=0, a_hidden=(32,), c_hidden=(32,), in_dim=19, B=70, **kw):
    from ctr_reach_amd.learner import DdpgLearner
    policy, critic, rows, actions, target = R.make(seed, a_hidden, c_hidden, in_dim, B)
    learner = DdpgLearner(R.to_device(policy, cuda), R.to_device(critic, cuda), max_batch=B, **kw)
    return learner, tuple(t.to(cuda) for t in (rows, actions, target))


def _snapshot(learner):
    """Every output of a step, on the host."""
    import torch
    torch.cuda.synchronize()
    out = {}
    for name, net in (("actor", learner._actor), ("critic", learner._critic)):
        out[name] = dict(p=R.host(net.params), g=R.host(net.grads), m=R.host(net.m), v=R.host(net.v),
                         pow=net.pow.cpu().numpy().copy())
    out["losses"] = np.array([float(learner.critic_loss), float(learner.actor_loss)], dtype=np.float32)
    return out


def _assert_same(a, b, tag):
    for name in ("actor", "critic"):
        for key in ("p", "g", "m", "v"):
            for l, (x, y) in enumerate(zip(a[name][key], b[name][key])):
                for which, s, t in zip("Wb", x, y):
                    assert np.array_equal(R.bits(s), R.bits(t)), (tag, name, key, which, l)
        assert np.array_equal(R.bits(a[name]["pow"]), R.bits(b[name]["pow"])), (tag, name, "pow")
    assert np.array_equal(R.bits(a["losses"]), R.bits(b["losses"])), (tag, "losses", a["losses"], b["losses"])


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.75)])
@pytest.mark.parametrize("a_hidden,c_hidden,in_dim", [((32,), (32,), 19), ((64, 96), (256, 128), 20)])
def test_three_steps_are_the_restatement_bit_for_bit(cuda, betas, a_hidden, c_hidden, in_dim):
    from ctr_reach_amd.learner import adam_reference
    learner, (rows, actions, target) = _setup(cuda, 1, a_hidden, c_hidden, in_dim, 70, betas=betas, actor_lr=1e-4,
                                              critic_lr=1e-3)
    before = _snapshot(learner)
    for name in ("actor", "critic"):                                       # the zero state
        assert all(not a.any() and not b.any() for key in ("m", "v") for a, b in before[name][key])
        assert before[name]["pow"].tolist() == [1.0, 1.0]
    for step in range(1, 4):
        learner.critic_step(rows, actions, target)
        mid = _snapshot(learner)
        learner.actor_step(rows)
        after = _snapshot(learner)
        for name, old, new, lr in (("critic", before, mid, 1e-3), ("actor", mid, after, 1e-4)):
            pw = None
            for l in range(len(new[name]["g"])):
                for w in (0, 1):
                    g = new[name]["g"][l][w]
                    assert np.isfinite(g).all() and np.abs(g).max() > 0
                    p1, m1, v1, pw = adam_reference(old[name]["p"][l][w], g, old[name]["m"][l][w], old[name]["v"][l][w],
                                                    old[name]["pow"], lr, betas, 1e-8)
                    for key, want in (("p", p1), ("m", m1), ("v", v1)):
                        got = new[name][key][l][w]
                        bad = np.flatnonzero(R.bits(got).reshape(-1) != R.bits(want).reshape(-1))
                        assert bad.size == 0, (step, name, key, l, w, bad.size, got.reshape(-1)[bad[:4]].tolist(),
                                               want.reshape(-1)[bad[:4]].tolist())
                    assert not np.array_equal(p1, old[name]["p"][l][w])    # (the step moved the tensor)
            assert np.array_equal(R.bits(new[name]["pow"]), R.bits(pw)), (step, name, new[name]["pow"], pw)
        # the critic's step writes nothing of the actor's, the actor's nothing of the critic's
        for key in ("p", "g", "m", "v"):
            for (a, b), (a1, b1) in zip(before["actor"][key], mid["actor"][key]):
                assert np.array_equal(R.bits(a), R.bits(a1)) and np.array_equal(R.bits(b), R.bits(b1)), ("actor", key, step)
            for (a, b), (a1, b1) in zip(mid["critic"][key], after["critic"][key]):
                assert np.array_equal(R.bits(a), R.bits(a1)) and np.array_equal(R.bits(b), R.bits(b1)), ("critic", key, step)
        assert np.array_equal(mid["critic"]["pow"], after["critic"]["pow"])
        before = after
    want = np.array([np.float32(betas[0]) ** 3, np.float32(betas[1]) ** 3])
    assert np.allclose(after["actor"]["pow"], want, rtol=1e-6) and np.allclose(after["critic"]["pow"], want, rtol=1e-6)


def _restore(learner, snap, state):
    import torch
    for name, net in (("actor", learner._actor), ("critic", learner._critic)):
        for (W, b), (W0, b0) in zip(net.params, snap[name]["p"]):
            W.copy_(torch.from_numpy(W0))
            b.copy_(torch.from_numpy(b0))
    learner.load_state_dict(state)


def test_the_same_step_twice_gives_the_same_bits(cuda):
    learner, (rows, actions, target) = _setup(cuda, 2, (64, 96), (32, 64), 20, 3 * R.T + 5)
    learner.critic_step(rows, actions, target)                             # (a nonzero state to start from)
    learner.actor_step(rows)
    start, state = _snapshot(learner), learner.state_dict()
    assert all(t.data_ptr() != mine.data_ptr() for t, mine in zip(state["actor"]["m"][0], learner._actor.m[0]))
    runs = []
    for _ in range(2):
        _restore(learner, start, state)
        learner.critic_step(rows, actions, target)
        learner.actor_step(rows)
        runs.append(_snapshot(learner))
    _assert_same(runs[0], runs[1], "rerun")
    assert not np.array_equal(runs[0]["actor"]["p"][0][0], start["actor"]["p"][0][0])
    assert np.array_equal(state["critic"]["pow"].cpu().numpy(), start["critic"]["pow"])      # (a clone: it stayed)


def test_a_captured_pair_of_steps_replays_as_eager_steps(cuda):
    import torch
    learner, (rows, actions, target) = _setup(cuda, 3, (64, 96), (32, 64), 19, 70)
    twin, _ = _setup(cuda, 3, (64, 96), (32, 64), 19, 70)
    for _ in range(3):
        twin.critic_step(rows, actions, target)
        twin.actor_step(rows)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    learner.critic_step(rows, actions, target)                             # (the kernels' first launch is not the captured one)
    learner.actor_step(rows)
    assert torch.cuda.memory_allocated() == before                         # a step allocates nothing
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                          # a synchronisation in here raises
        learner.critic_step(rows, actions, target)
        learner.actor_step(rows)
    graph.replay()
    graph.replay()
    _assert_same(_snapshot(learner), _snapshot(twin), "replayed")


@pytest.mark.parametrize("a_hidden,c_hidden,in_dim,B", [((32,), (32,), 19, 1), ((64, 96), (32,), 20, 3 * R.T + 5)])
def test_nothing_is_written_beside_the_tensors(cuda, a_hidden, c_hidden, in_dim, B):
    carver = _Carver(cuda)
    learner, (rows, actions, target) = _setup(cuda, 4, a_hidden, c_hidden, in_dim, B, alloc=carver)
    assert learner.actor_grads[0][0].data_ptr() % 8 == 4                   # (tensors that start at any float)
    for _ in range(2):
        learner.critic_step(rows, actions, target)
        learner.actor_step(rows)
    snap = _snapshot(learner)
    assert carver.intact()
    for name in ("actor", "critic"):
        assert all(a.any() and b.any() for key in ("g", "m", "v") for a, b in snap[name][key])


def test_the_losses_go_down_on_a_fixed_batch(cuda, capsys):
    """[32] nets, B = 70, seed 0 (torch float32 on the CPU: the critic's loss 0.366 -> 0.090 in 100
    steps at lr 1e-3, the actor's 0.193 -> 0.108 in 200 steps at lr 1e-4)."""
    import torch
    learner, (rows, actions, target) = _setup(cuda, 0)
    critic_losses, actor_losses = [], []
    for _ in range(100):
        learner.critic_step(rows, actions, target)
        critic_losses.append(learner.critic_loss.clone())
    for _ in range(200):
        learner.actor_step(rows)
        actor_losses.append(learner.actor_loss.clone())
    torch.cuda.synchronize()
    c0, c1, a0, a1 = (float(x) for x in (critic_losses[0], critic_losses[-1], actor_losses[0], actor_losses[-1]))
    with capsys.disabled():
        print("\ncritic loss %.4g -> %.4g in 100 steps, actor loss %.4g -> %.4g in 200 steps" % (c0, c1, a0, a1))
    assert np.isfinite([c0, c1, a0, a1]).all()
    assert c1 < 0.5 * c0
    assert a1 < a0
