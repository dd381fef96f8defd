"""MlpActor.load_ (ctr_actor_load: the packer as a kernel) writes, from device-resident parameters,
the bytes ctr_actor_pack gives on the host for the same values -- every byte of the blob, the
padding included, with the host's rounding of NaNs, infinities, denormals and ties; it is ordered
on the stream like any launch, can be captured into a graph, refuses tensors it would have to
convert, and keeps or drops the host copies as asked."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# 6 -> 32 row padding, 19 -> 32 column padding and unaligned rows; two tiles -> three; 16 k-steps and
# several tiles; 384 B under the LDS budget
SHAPES = [((32,), 19), ((64, 96), 20), ((32, 256, 32), 20), ((224, 160), 19)]

# +-0, +-inf, quiet and signalling NaNs of both signs with payloads, the smallest and the largest
# denormal, the largest finite float (rounds to infinity), a tie that rounds down to even
# (1 + 2^-8), one just above it (rounds up), a tie that rounds up to even (1 + 3 * 2^-8)
SPECIALS = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC12345, 0x7F800001, 0xFF800001,
                     0x7FBFFFFF, 0x00000001, 0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x3F808000, 0x3F808001, 0x3F818000],
                    dtype=np.uint32)


def _layers(rng, hidden, in_dim, specials=False):
    """U(+-1/sqrt(fan_in)) weights and biases (numpy); with ``specials`` the special values planted
    in every layer: all of them over each weight matrix (its first and last element among the
    places) and six of them in each bias."""
    dims = [in_dim] + list(hidden) + [6]
    layers = []
    for l in range(len(dims) - 1):
        s = 1.0 / np.sqrt(dims[l])
        W = rng.uniform(-s, s, (dims[l + 1], dims[l])).astype(np.float32)
        b = rng.uniform(-s, s, dims[l + 1]).astype(np.float32)
        if specials:
            where = np.concatenate(([0, W.size - 1], rng.choice(np.arange(1, W.size - 1), SPECIALS.size - 2, replace=False)))
            W.reshape(-1).view(np.uint32)[where] = SPECIALS
            b.view(np.uint32)[rng.choice(b.size, 6, replace=False)] = SPECIALS[[1, 3, 5, 6, 9, 11]]
            assert np.array_equal(np.sort(W.reshape(-1).view(np.uint32)[where]), np.sort(SPECIALS))
        layers.append((W, b))
    return layers


def _host_pack(actor, layers):
    """ctr_actor_pack of ``layers`` (numpy) into a host buffer prefilled with 0xAB."""
    from ctr_reach_amd import _abi
    lib = _abi.load()
    nb = lib.ctr_actor_blob_bytes(actor._struct)
    out = np.full(nb, 0xAB, dtype=np.uint8)
    n = len(layers)
    W = (ctypes.c_void_p * n)(*[np.ascontiguousarray(w).ctypes.data for w, _ in layers])
    b = (ctypes.c_void_p * n)(*[np.ascontiguousarray(v).ctypes.data for _, v in layers])
    assert lib.ctr_actor_pack(actor._struct, W, b, out.ctypes.data) == 0
    return out


def _device(layers, cuda):
    import torch
    return [(torch.from_numpy(W).to(cuda), torch.from_numpy(b).to(cuda)) for W, b in layers]


def _actor(layers, cuda):
    from ctr_reach_amd.policy import MlpActor
    return MlpActor(layers, np.array([0.001, 0.001, 0.001, 0.087, 0.087, 0.087]), device=cuda)


def _blob(actor):
    import torch
    torch.cuda.synchronize()
    return actor.blob.cpu().numpy()


@pytest.mark.parametrize("hidden,in_dim", SHAPES)
def test_the_blob_is_the_host_packers_bytes(cuda, hidden, in_dim):
    rng = np.random.default_rng(40 + len(hidden) + in_dim)
    actor = _actor(_layers(rng, hidden, in_dim), cuda)
    first = _blob(actor).copy()
    new = _layers(rng, hidden, in_dim, specials=True)
    want = _host_pack(actor, new)
    assert want.size == actor.blob.numel() and not np.array_equal(want, first)
    actor.blob.fill_(0xAB)                               # the kernel must not rely on zeroed padding
    ptr = actor.blob.data_ptr()
    assert actor.load_(_device(new, cuda)) is actor
    got = _blob(actor)
    assert actor.blob.data_ptr() == ptr == actor._struct.blob            # in place
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (hidden, in_dim, bad.size, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


def _env(cuda, her=False):
    from ctr_reach_amd import CtrReachVecEnv
    e = CtrReachVecEnv(256, device=cuda, seed=7, max_steps_per_episode=5, refill_interval=4, select_systems=[0, 1, 2, 3])
    e.goal_tolerance.current_tol = 0.03
    e.reset()
    return e


def _box_layers(rng, hidden, in_dim):
    """As the rollout tests' actor: the output layer scaled up so that the actions use the box."""
    layers = _layers(rng, hidden, in_dim)
    W, b = layers[-1]
    layers[-1] = (W * np.float32(8), b * np.float32(8))
    return layers


def test_a_load_is_ordered_on_the_stream(cuda):
    """load_, rollout and the actor's own launch back to back, nothing waited for in between: the
    rollout and the launch after it see the loaded weights, as a twin env with an actor freshly
    built from them does."""
    import torch
    from ctr_reach_amd.policy import MlpActor
    rng = np.random.default_rng(5)
    hidden, in_dim = (64, 96), 20
    a, b = _env(cuda), _env(cuda)
    assert a.step_many_ineligible() is None
    old, new = _box_layers(rng, hidden, in_dim), _box_layers(rng, hidden, in_dim)
    actor = MlpActor(old, a.action_space.high, device=cuda)
    fresh = MlpActor(new, b.action_space.high, device=cuda)
    src = _device(new, cuda)
    rows = a.actor_rows().clone()
    torch.cuda.synchronize()
    actor.load_(src)
    got = a.rollout(actor, 4, record_actions=True)
    got_act = actor(rows)
    want = b.rollout(fresh, 4, record_actions=True)
    want_act = fresh(rows)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and torch.equal(got_act, want_act)
    for k in ("obs", "joints", "achieved_goal", "desired_goal", "t", "epoch", "reward", "done"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert not torch.equal(want_act, MlpActor(old, a.action_space.high, device=cuda)(rows))   # (the weights matter)


def test_a_captured_load_packs_what_the_parameters_hold_at_replay(cuda):
    import torch
    rng = np.random.default_rng(6)
    hidden, in_dim = (32, 256, 32), 20
    first = _layers(rng, hidden, in_dim)
    actor = _actor(first, cuda)
    src = _device(first, cuda)
    actor.load_(src)                                     # (the kernel's first launch is not the captured one)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                        # a synchronisation or an allocation in here raises
        actor.load_(src)
    new = _layers(rng, hidden, in_dim, specials=True)
    for (W, b), (W1, b1) in zip(src, new):
        W.copy_(torch.from_numpy(W1))
        b.copy_(torch.from_numpy(b1))
    actor.blob.fill_(0xAB)
    graph.replay()
    assert np.array_equal(_blob(actor), _host_pack(actor, new))


def test_tensors_that_would_need_a_copy_are_refused(cuda):
    import torch
    rng = np.random.default_rng(7)
    hidden, in_dim = (64, 96), 20
    layers = _layers(rng, hidden, in_dim)
    actor = _actor(layers, cuda)
    before = _blob(actor).copy()
    kept = actor.weights

    def refused(l, which, tensor, word):
        src = [list(p) for p in _device(_layers(rng, hidden, in_dim), cuda)]
        src[l][which] = tensor
        with pytest.raises(ValueError, match=word):
            actor.load_([tuple(p) for p in src])

    good = _device(_layers(rng, hidden, in_dim), cuda)
    refused(1, 0, good[1][0].double(), "float32")
    refused(2, 1, good[2][1].double(), "float32")
    refused(1, 0, torch.zeros((64, 96), device=cuda).t(), "contiguous")           # [96, 64], strides (1, 96)
    refused(0, 1, torch.zeros(128, device=cuda)[::2], "contiguous")
    refused(0, 0, torch.zeros((64, 19), device=cuda), "must be")
    refused(2, 0, torch.zeros((32, 96), device=cuda), "must be")
    refused(1, 1, torch.zeros((96, 1), device=cuda), "must be")
    refused(0, 0, good[0][0].cpu(), "is on cpu")
    refused(2, 1, good[2][1].cpu(), "is on cpu")
    refused(0, 0, good[0][0].cpu().numpy(), "torch tensor")
    with pytest.raises(ValueError, match="3 layers"):
        actor.load_(good[:2])
    assert np.array_equal(_blob(actor), before)
    assert actor.weights is kept                          # nor were the host copies dropped


def test_keep_host(cuda):
    import torch.nn as nn
    from ctr_reach_amd.policy import MlpActor
    rng = np.random.default_rng(8)
    hidden, in_dim = (64, 96), 20
    actor = _actor(_layers(rng, hidden, in_dim), cuda)
    new = _layers(rng, hidden, in_dim)
    rows = rng.uniform(-1, 1, (50, in_dim)).astype(np.float32)
    host = MlpActor(new, actor.scale, device=None)
    actor.load_(_device(new, cuda), keep_host=True)
    for got, want in zip(actor.emulate(rows), host.emulate(rows)):
        assert np.array_equal(got, want)
    assert np.array_equal(actor.reference(rows), host.reference(rows))
    assert np.array_equal(actor.packed, _blob(actor))
    actor.load_(_device(new, cuda))
    assert actor.weights is None and actor.biases is None and actor.packed is None
    for call in (actor.emulate, actor.reference):
        with pytest.raises(RuntimeError, match="keep_host=True"):
            call(rows)
    # a module, as from_torch takes it
    seq = nn.Sequential(nn.Linear(20, 64), nn.ReLU(), nn.Linear(64, 96), nn.ReLU(), nn.Linear(96, 6), nn.Tanh()).to(cuda)
    actor.load_(seq, keep_host=True)
    want = MlpActor.from_torch(seq, actor.scale, cuda)
    assert np.array_equal(_blob(actor), _blob(want))
    with pytest.raises(ValueError, match="nn.Tanh"):
        actor.load_(nn.Sequential(*list(seq)[:-1]))
