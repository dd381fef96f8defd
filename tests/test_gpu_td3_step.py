"""Td3Learner.critic_step (ctr_td3_critic_step): both critics' regression in the two launches of one
call, against two DdpgLearner.critic_step calls on cloned parameters: after each of three consecutive
steps every parameter, gradient, m, v, pow and both losses are bit-equal, for critics of equal and
of different shapes, with and without the action scale, at B = 1, a ragged tile and a ragged second
tile in slot 0; a repeated step repeats every bit; actor_step is DdpgLearner's under critic 1 and
leaves both critics alone; a captured step replays as eager steps do; and nothing is written beside
the workspace, the gradient and the state tensors."""
import ctypes

import numpy as np
import pytest

import ddpg_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(0x4B3C2D1E)
GAP = 8
SCALE = [0.001, 0.001, 0.001, 0.087, 0.087, 0.087]
PAIRS = [((32,), (32,)), ((64, 96), (32,)), ((128, 128, 128), (256, 128))]
BATCHES = [1, 3 * R.T + 5, R.T * R.SLOTS + 5]           # 1, 53, 1 029


def _make(seed, h1, h2, c_in, B):
    """(policy, critic 1, critic 2, rows, actions, target) on the CPU: torch's default init, U(-1, 1) data."""
    import torch
    g = torch.Generator().manual_seed(2000 + seed)
    state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    nets = R.mlp(c_in - 6, (32,), 6, True), R.mlp(c_in, h1, 1, False), R.mlp(c_in, h2, 1, False)
    torch.random.set_rng_state(state)
    data = tuple(torch.rand(shape, generator=g) * 2 - 1 for shape in ((B, c_in - 6), (B, 6), (B,)))
    return tuple(n.requires_grad_(False) for n in nets) + data


def _setup(cuda, seed, h1, h2, c_in, B, scale=None, **kw):
    """A Td3Learner and the two DdpgLearners it is held to, each on its own clones, and the batch."""
    from ctr_reach_amd.learner import DdpgLearner, Td3Learner
    policy, c1, c2, rows, actions, target = _make(seed, h1, h2, c_in, B)
    td3 = Td3Learner(R.to_device(policy, cuda), R.to_device(c1, cuda), R.to_device(c2, cuda), scale=scale, max_batch=B, **kw)
    singles = [DdpgLearner(R.to_device(policy, cuda), R.to_device(c, cuda), scale=scale, max_batch=B) for c in (c1, c2)]
    return td3, singles, tuple(t.to(cuda) for t in (rows, actions, target))


def _net_snapshot(net):
    return dict(p=R.host(net.params), g=R.host(net.grads), m=R.host(net.m), v=R.host(net.v), pow=net.pow.cpu().numpy().copy())


def _snapshot(td3):
    import torch
    torch.cuda.synchronize()
    return dict(actor=_net_snapshot(td3._actor), critic1=_net_snapshot(td3._critics[0]), critic2=_net_snapshot(td3._critics[1]),
                closs=td3.critic_loss.cpu().numpy().copy(), aloss=td3.actor_loss.cpu().numpy().copy())


def _single_snapshot(singles):
    import torch
    torch.cuda.synchronize()
    return dict(critic1=_net_snapshot(singles[0]._critic), critic2=_net_snapshot(singles[1]._critic),
                closs=np.array([float(s.critic_loss) for s in singles], dtype=np.float32))


def _assert_net_same(a, b, tag):
    for key in ("p", "g", "m", "v"):
        assert len(a[key]) == len(b[key])
        for l, (x, y) in enumerate(zip(a[key], b[key])):
            for which, s, t in zip("Wb", x, y):
                assert np.array_equal(R.bits(s), R.bits(t)), (tag, key, which, l)
    assert np.array_equal(R.bits(a["pow"]), R.bits(b["pow"])), (tag, "pow")


def _assert_same(a, b, tag, names=("critic1", "critic2")):
    for name in names:
        _assert_net_same(a[name], b[name], (tag, name))
    assert np.array_equal(R.bits(a["closs"]), R.bits(b["closs"])), (tag, "losses", a["closs"], b["closs"])


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("c_in", [25, 26])
@pytest.mark.parametrize("h1,h2", PAIRS)
def test_three_twin_steps_are_two_single_steps_bit_for_bit(cuda, h1, h2, c_in, B):
    for scale in (None, SCALE):
        td3, singles, (rows, actions, target) = _setup(cuda, 1, h1, h2, c_in, B, scale=scale)
        start = _snapshot(td3)
        _assert_same(start, dict(_single_snapshot(singles), closs=np.zeros(2, np.float32)), "start")
        for step in range(1, 4):
            td3.critic_step(rows, actions, target)
            for s in singles:
                s.critic_step(rows, actions, target)
            got, want = _snapshot(td3), _single_snapshot(singles)
            _assert_same(got, want, (scale is not None, step))
            assert np.isfinite(got["closs"]).all() and (got["closs"] > 0).all()
            for name in ("critic1", "critic2"):
                assert all(np.abs(g).max() > 0 for pair in got[name]["g"] for g in pair), (name, step)
                assert not np.array_equal(got[name]["p"][0][0], start[name]["p"][0][0])
            _assert_net_same(got["actor"], start["actor"], "the policy is not touched")
        want_pow = np.array([np.float32(0.9) ** 3, np.float32(0.999) ** 3])
        assert np.allclose(got["critic1"]["pow"], want_pow, rtol=1e-6) and np.allclose(got["critic2"]["pow"], want_pow, rtol=1e-6)
        if (h1, h2) == PAIRS[0]:
            # equal shapes are not equal critics: each plane worked on its own
            assert not np.array_equal(got["critic1"]["p"][0][0], got["critic2"]["p"][0][0])
            assert got["closs"][0] != got["closs"][1]


def _restore(td3, snap, state):
    import torch
    for name, net in (("actor", td3._actor), ("critic1", td3._critics[0]), ("critic2", td3._critics[1])):
        for (W, b), (W0, b0) in zip(net.params, snap[name]["p"]):
            W.copy_(torch.from_numpy(W0))
            b.copy_(torch.from_numpy(b0))
    td3.load_state_dict(state)


def test_the_same_step_twice_gives_the_same_bits(cuda):
    td3, _, (rows, actions, target) = _setup(cuda, 2, (64, 96), (32,), 26, 3 * R.T + 5, scale=SCALE)
    td3.critic_step(rows, actions, target)                                 # (a nonzero state to start from)
    td3.actor_step(rows)
    start, state = _snapshot(td3), td3.state_dict()
    assert set(state) == {"actor", "critic1", "critic2"}
    assert all(t.data_ptr() != mine.data_ptr() for t, mine in zip(state["critic2"]["m"][0], td3._critics[1].m[0]))
    runs = []
    for _ in range(2):
        _restore(td3, start, state)
        td3.critic_step(rows, actions, target)
        td3.actor_step(rows)
        runs.append(_snapshot(td3))
    _assert_same(runs[0], runs[1], "rerun", names=("actor", "critic1", "critic2"))
    assert np.array_equal(R.bits(runs[0]["aloss"]), R.bits(runs[1]["aloss"]))
    assert not np.array_equal(runs[0]["critic2"]["p"][0][0], start["critic2"]["p"][0][0])
    assert np.array_equal(state["critic1"]["pow"].cpu().numpy(), start["critic1"]["pow"])      # (a clone: it stayed)


@pytest.mark.parametrize("h1,h2,c_in", [((64, 96), (32,), 25), ((32,), (256, 128), 26)])
def test_the_actor_step_is_ddpg_under_critic_1(cuda, h1, h2, c_in):
    td3, singles, (rows, actions, target) = _setup(cuda, 3, h1, h2, c_in, 3 * R.T + 5)
    for step in range(2):
        td3.critic_step(rows, actions, target)
        singles[0].critic_step(rows, actions, target)
        before = _snapshot(td3)
        td3.actor_step(rows)
        singles[0].actor_step(rows)
        after = _snapshot(td3)
        _assert_net_same(after["actor"], _net_snapshot(singles[0]._actor), ("actor", step))
        assert np.array_equal(R.bits(after["aloss"]), R.bits(singles[0].actor_loss.cpu().numpy()))
        assert not np.array_equal(after["actor"]["p"][0][0], before["actor"]["p"][0][0])
        _assert_same(after, before, ("the critics are only read", step))
    assert td3.actor_grads is td3._actor.grads and td3.critic_grads == (td3._critics[0].grads, td3._critics[1].grads)


def test_a_captured_twin_step_replays_as_eager_steps(cuda):
    import torch
    td3, _, (rows, actions, target) = _setup(cuda, 4, (64, 96), (32,), 25, 70)
    twin, _, _ = _setup(cuda, 4, (64, 96), (32,), 25, 70)
    for _ in range(3):
        twin.critic_step(rows, actions, target)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    td3.critic_step(rows, actions, target)                                 # (the kernels' first launch is not the captured one)
    assert torch.cuda.memory_allocated() == before                         # a step allocates nothing
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                          # two launches on one stream: no parallel branches
        td3.critic_step(rows, actions, target)
    graph.replay()
    graph.replay()
    _assert_same(_snapshot(td3), _snapshot(twin), "replayed")


class _Carver(object):
    """``alloc`` for a learner: zeroed tensors carved from one buffer of sentinels, each starting at an
    odd float offset with GAP sentinel floats behind it; ``take(nbytes)``: a 16-B aligned byte region."""

    def __init__(self, cuda, floats=1 << 22):                              # (the widest case's workspace is 2.7 M floats)
        import torch
        self.buf = torch.from_numpy(np.full(floats, SENTINEL, dtype=np.uint32).view(np.float32)).to(cuda)
        assert self.buf.data_ptr() % 16 == 0
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

    def take(self, nbytes):
        import torch
        assert nbytes % 4 == 0
        start = (self.off + GAP + 3) // 4 * 4                              # floats: 16-B aligned
        n = nbytes // 4
        view = self.buf[start:start + n].view(torch.uint8)
        self.guard[start:start + n] = False
        self.off = start + n + GAP + 1
        self.off += (self.off + 1) % 2
        assert self.off < self.buf.numel() and view.numel() == nbytes and view.data_ptr() % 16 == 0
        return view

    def intact(self):
        return bool((R.bits(self.buf.cpu().numpy())[self.guard] == SENTINEL).all())


@pytest.mark.parametrize("h1,h2,c_in,B", [((32,), (32,), 25, 1), ((64, 96), (32,), 26, 3 * R.T + 5),
                                          ((32,), (256, 128), 25, R.T * R.SLOTS + 5)])
def test_nothing_is_written_beside_the_workspace_and_the_tensors(cuda, h1, h2, c_in, B):
    from ctr_reach_amd import _abi
    carver = _Carver(cuda)
    td3, singles, (rows, actions, target) = _setup(cuda, 5, h1, h2, c_in, B, alloc=carver)
    assert td3.critic_grads[1][0][0].data_ptr() % 8 == 4                   # (tensors that start at any float)
    # a workspace of exactly ctr_td3_workspace_bytes, sentinels on either side
    need = int(_abi.load().ctr_td3_workspace_bytes(td3._actor_struct, td3._critic_structs[0], td3._critic_structs[1], B))
    assert need == td3.workspace.numel() == td3._ws_bytes
    td3.workspace = carver.take(need)
    td3._ws = ctypes.c_void_p(td3.workspace.data_ptr())
    for _ in range(2):
        td3.critic_step(rows, actions, target)
        td3.actor_step(rows)
        singles[0].critic_step(rows, actions, target)
        singles[0].actor_step(rows)
        singles[1].critic_step(rows, actions, target)
    snap = _snapshot(td3)
    assert carver.intact()
    for name in ("actor", "critic1", "critic2"):
        assert all(a.any() and b.any() for key in ("g", "m", "v") for a, b in snap[name][key])
    _assert_same(snap, _single_snapshot(singles), "carved")
    _assert_net_same(snap["actor"], _net_snapshot(singles[0]._actor), "carved actor")
