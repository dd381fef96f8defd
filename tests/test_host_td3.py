"""TD3 on the host (no GPU): ctr_her_sample_td3, ctr_td3_workspace_bytes and ctr_td3_critic_step are
declared, listed and exported; the ctypes mirror of ctr_her_td3_t matches the header; every refusal
the header lists returns CTR_EINVAL (-1) with a ctr_last_error that names the function, before any
HIP call (the device pointers are fake and never dereferenced); ctr_td3_workspace_bytes covers the
two critics' regions and the actor's step; policy.TargetSmoothing pins the keying of the smoothing
noise; Td3Learner and HerReplayBuffer.sample_td3 refuse what they would have to convert."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

from test_host_ddpg import WRITES_IN_PLACE, exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FNS = ("ctr_her_sample_td3", "ctr_td3_workspace_bytes", "ctr_td3_critic_step")


def _lib():
    from ctr_reach_amd import _abi
    return _abi, _abi.load()


def _actor(hidden=(64, 64), in_dim=19, blob=1 << 21):
    from ctr_reach_amd import _abi
    a = _abi.CtrActor()
    a.in_dim, a.n_hidden = in_dim, len(hidden)
    for l, w in enumerate(hidden):
        a.width[l] = w
    for i in range(6):
        a.scale[i] = 0.5
    a.blob = blob
    return a


def _critic(hidden=(64, 64), in_dim=25, blob=1 << 20):
    from ctr_reach_amd import _abi_critic
    c = _abi_critic.CtrCritic()
    c.in_dim, c.n_hidden = in_dim, len(hidden)
    for l, w in enumerate(hidden):
        c.width[l] = w
    c.blob = blob
    return c


def test_declared_listed_and_exported():
    _abi, lib = _lib()
    header = open(os.path.join(ROOT, "include", "ctr_reach_amd.h")).read()
    assert re.search(r"^int ctr_her_sample_td3\(const ctr_her_t \*her, int64_t batch_size, uint64_t seed, uint64_t counter,\n"
                     r" +const ctr_her_batch_t \*out, const ctr_her_td3_t \*td, void \*stream\);", header, re.M)
    assert re.search(r"^int64_t ctr_td3_workspace_bytes\(const ctr_actor_t \*actor, const ctr_critic_t \*critic1,\n"
                     r" +const ctr_critic_t \*critic2, int64_t max_B\);", header, re.M)
    assert re.search(r"^int ctr_td3_critic_step\(const ctr_critic_t \*const critic\[2\], const ctr_ddpg_net_t \*const net\[2\],",
                     header, re.M)
    for fn in FNS:
        assert fn in _abi.EXPORTED and hasattr(lib, fn), fn
    assert lib.ctr_abi_version() == _abi.CTR_ABI_VERSION == 17
    import ctr_reach_amd
    from ctr_reach_amd.learner import Td3Learner
    from ctr_reach_amd.policy import TargetSmoothing
    assert ctr_reach_amd.Td3Learner is Td3Learner and ctr_reach_amd.TargetSmoothing is TargetSmoothing
    assert hasattr(ctr_reach_amd.HerReplayBuffer, "sample_td3")


def test_struct_layout_matches_header(tmp_path):
    from ctr_reach_amd import _abi_td3
    cls = _abi_td3.CtrHerTd3
    lines = ['  printf("%zu\\n", sizeof(ctr_her_td3_t));']
    want = [ctypes.sizeof(cls)]
    for fname, _ in cls._fields_:
        lines.append('  printf("%%zu\\n", offsetof(ctr_her_td3_t, %s));' % fname)
        want.append(getattr(cls, fname).offset)
    lines.append('  printf("%d\\n", CTR_ABI_VERSION);')
    want.append(17)
    prog = tmp_path / "td3_layout.c"
    prog.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"ctr_reach_amd.h\"\nint main(void) {\n"
                    + "\n".join(lines) + "\n  return 0; }\n")
    exe = tmp_path / "td3_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(prog), "-o", str(exe)])
    assert list(map(int, subprocess.check_output([str(exe)]).split())) == want
    assert [f for f, _ in cls._fields_] == ["actor", "critic1", "critic2", "gamma", "sigma", "clip", "pad", "target",
                                            "q1_next", "q2_next", "next_action"]
    assert ctypes.sizeof(_abi_td3.CriticPair) == ctypes.sizeof(_abi_td3.NetPair) == 2 * ctypes.sizeof(ctypes.c_void_p)


# ------------------------------------------------------------------------------------------
# ctr_her_sample_td3

def _her(obs_dim=13, n=8):
    from ctr_reach_amd import _abi
    h = _abi.CtrHer()
    h.obs_dim, h.t_max, h.n_sampled_goal, h.strategy = obs_dim, 5, 4, _abi.CTR_HER_FUTURE
    h.n, h.env_base, h.slots, h.seed = n, 0, 3, 1
    for name in ("state", "step", "dg", "tol", "len", "epoch", "cur_t", "cur_epoch", "cdf"):
        setattr(h, name, 1 << 12)
    return h


NOARG = object()


def _td3_call(her=None, B=8, out="default", td="default", actor=NOARG, critic1=NOARG, critic2=NOARG, gamma=0.99, sigma=0.2,
              clip=0.5, target=1 << 14):
    from ctr_reach_amd import _abi_td3
    _abi, lib = _lib()
    her = her if her is not None else _her()
    if out == "default":
        out = _abi.CtrHerBatch()
        out.obs = out.action = out.reward = out.next_obs = out.done = 1 << 13
    if td == "default":
        td = _abi_td3.CtrHerTd3()
        actor = _actor() if actor is NOARG else actor
        critic1 = _critic() if critic1 is NOARG else critic1
        critic2 = _critic((32,), blob=3 << 20) if critic2 is NOARG else critic2
        for name, net in (("actor", actor), ("critic1", critic1), ("critic2", critic2)):
            if net is not None:
                setattr(td, name, ctypes.pointer(net))
        td.gamma, td.sigma, td.clip, td.target = gamma, sigma, clip, target
    return lib.ctr_her_sample_td3(her, B, 1, 0, out, td, None), lib.ctr_last_error()


def test_her_sample_td3_refusals():
    _abi, lib = _lib()

    def refused(word, **kw):
        rc, msg = _td3_call(**kw)
        assert rc == -1 and b"ctr_her_sample_td3" in msg and word in msg, (word, kw, rc, msg)

    # what ctr_her_sample refuses
    assert lib.ctr_her_sample_td3(None, 8, 1, 0, None, None, None) == -1
    assert b"ctr_her_sample_td3" in lib.ctr_last_error() and b"her is NULL" in lib.ctr_last_error()
    bad = _her()
    bad.obs_dim = 15
    refused(b"obs_dim", her=bad)
    bad = _her()
    bad.slots = 1
    refused(b"slots", her=bad)
    refused(b"bad batch", out=None)
    refused(b"bad batch", B=-1)
    refused(b"empty store", her=_her(n=0))
    out = _abi.CtrHerBatch()
    out.obs = out.action = out.reward = out.next_obs = 1 << 13
    refused(b"output missing", out=out)
    out.done = 1 << 13
    out.next_obs = (1 << 13) + 4
    refused(b"16-byte aligned", out=out)
    # what ctr_her_sample_td refuses, of each of the three networks
    refused(b"td is NULL", td=None)
    refused(b"target", target=None)
    refused(b"actor is NULL", actor=None)
    refused(b"is NULL", critic1=None)
    refused(b"is NULL", critic2=None)
    refused(b"actor: n_hidden", actor=_actor(()))
    a = _actor()
    a.blob = None
    refused(b"actor: blob", actor=a)
    refused(b"actor->in_dim", actor=_actor(in_dim=20))
    refused(b"actor->in_dim", her=_her(obs_dim=14))
    for which in ("critic1", "critic2"):
        refused(b"critic: every hidden width", **{which: _critic((64, 48))})
        refused(b"CTR_ACTOR_MAX_BYTES", **{which: _critic((256, 256))})
        refused(b"critic: blob is NULL", **{which: _critic(blob=None)})
        refused(b"critic: blob must be 16-B aligned", **{which: _critic(blob=(1 << 20) + 4)})
        refused(b"in_dim must be her->obs_dim + 12", **{which: _critic(in_dim=26)})
    refused(b"in_dim must be her->obs_dim + 12", her=_her(obs_dim=14), actor=_actor(in_dim=20))
    # its own
    nan, inf = float("nan"), float("inf")
    for g in (nan, inf, -inf):
        refused(b"gamma", gamma=g)
    for s in (nan, inf, -inf, -1e-3):
        refused(b"sigma", sigma=s)
    for c in (nan, -1e-3, -inf):
        refused(b"clip", clip=c)
    # what it takes: no noise, no clip, the same critic twice, an actor whose scale is not a number
    assert _td3_call(B=0, sigma=0.0)[0] == 0
    assert _td3_call(B=0, clip=inf)[0] == 0
    assert _td3_call(B=0, clip=0.0)[0] == 0
    c = _critic()
    assert _td3_call(B=0, critic1=c, critic2=c)[0] == 0
    a = _actor()
    a.scale[2] = nan
    assert _td3_call(B=0, actor=a)[0] == 0
    # an empty draw is a no-op (and still a checked call)
    assert _td3_call(B=0, her=_her(obs_dim=14), actor=_actor(in_dim=20), critic1=_critic(in_dim=26),
                     critic2=_critic((32,), 26, 3 << 20))[0] == 0
    refused(b"td is NULL", B=0, td=None)


# ------------------------------------------------------------------------------------------
# ctr_td3_critic_step

FIELDS = ("W", "b", "gW", "gb", "mW", "mb", "vW", "vb")


def _ptrs(base, holes=()):
    return (ctypes.c_void_p * 4)(*[None if l in holes else base + 4096 * l for l in range(4)])


def _net(which=0, **over):
    """ctr_ddpg_net_t number `which` on fake, pairwise different device pointers; ``over``: a field's
    array, or None for a NULL one."""
    from ctr_reach_amd import _abi_ddpg
    n = _abi_ddpg.CtrDdpgNet()
    for i, name in enumerate(FIELDS):
        value = over.get(name, _ptrs((16 * which + i + 1) << 24))
        if value is not None:
            setattr(n, name, value)
    n.pow = over.get("pow", (16 * which + 15) << 24)
    return n


def _adam(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
    from ctr_reach_amd import _abi_ddpg
    return _abi_ddpg.CtrDdpgAdam(lr, beta1, beta2, eps)


WS, WS_BYTES = 64 << 24, 1 << 26
ROWS, ACTIONS, TARGET = 80 << 24, 81 << 24, 82 << 24


def _step(critics=NOARG, nets=NOARG, adam=NOARG, rows=ROWS, actions=ACTIONS, scale=None, target=TARGET, B=64, ws=WS,
          ws_bytes=WS_BYTES, loss=None):
    from ctr_reach_amd import _abi_td3
    _abi, lib = _lib()
    keep = []

    def pair(cls, items):
        if items is None:
            return None
        arr = cls()
        for i, item in enumerate(items):
            if item is not None:
                keep.append(item)
                arr[i] = ctypes.pointer(item)
        return arr

    critics = (_critic(), _critic((32,))) if critics is NOARG else critics
    nets = (_net(0), _net(1)) if nets is NOARG else nets
    adam = _adam() if adam is NOARG else adam
    rc = lib.ctr_td3_critic_step(pair(_abi_td3.CriticPair, critics), pair(_abi_td3.NetPair, nets), adam, rows, actions,
                                 scale, target, B, loss, ws, ws_bytes, None)
    return rc, lib.ctr_last_error()


def _step_refused(word, **kw):
    rc, msg = _step(**kw)
    assert rc == -1 and msg == word, (word, kw, rc, msg)


def test_a_good_twin_step_gets_to_b_zero():
    assert _step(B=0)[0] == 0
    assert _step(B=0, rows=None, actions=None, target=None)[0] == 0
    assert _step(B=0, critics=(_critic((128, 128, 128)), _critic((256, 128))))[0] == 0
    assert _step(B=0, critics=(_critic((32,), 26), _critic((64, 96), 26)))[0] == 0


def test_twin_step_refuses_null_arrays_and_entries():
    _step_refused(b"ctr_td3_critic_step: critic or net is NULL", critics=None)
    _step_refused(b"ctr_td3_critic_step: critic or net is NULL", nets=None)
    _step_refused(b"ctr_td3_critic_step: NULL entry in critic[2] or net[2]", critics=(_critic(), None))
    _step_refused(b"ctr_td3_critic_step: NULL entry in critic[2] or net[2]", critics=(None, _critic()))
    _step_refused(b"ctr_td3_critic_step: NULL entry in critic[2] or net[2]", nets=(_net(0), None))
    _step_refused(b"ctr_td3_critic_step: NULL entry in critic[2] or net[2]", nets=(None, _net(1)))
    _step_refused(b"ctr_td3_critic_step: adam is NULL", adam=None)


def test_twin_step_refuses_for_either_net_what_the_single_step_refuses():
    good = _critic()
    fn = b"ctr_td3_critic_step: critic: "
    for bad, word in ((_critic(in_dim=24), fn + b"in_dim must be obs_dim + 12 = 25 or 26"),
                      (_critic(()), fn + b"n_hidden must be in 1..CTR_ACTOR_MAX_HIDDEN (3)"),
                      (_critic((64, 48)), fn + b"every hidden width must be a multiple of 32 in 32..CTR_ACTOR_MAX_WIDTH (256)"),
                      (_critic((256, 256)), fn + b"the packed network (163840 B of weights + 2176 B of biases) exceeds "
                                                 b"CTR_ACTOR_MAX_BYTES = 98304 B of LDS")):
        _step_refused(word, critics=(bad, good))
        _step_refused(word, critics=(good, bad))
    _step_refused(b"ctr_td3_critic_step: the two critics must have the same in_dim", critics=(_critic(), _critic(in_dim=26)))
    for which in (0, 1):
        def nets(**over):
            pair = [_net(0), _net(1)]
            pair[which] = _net(which, **over)
            return tuple(pair)
        for name in FIELDS:
            _step_refused(b"ctr_td3_critic_step: NULL pointer array or pow in net", nets=nets(**{name: None}))
            # critic 0 has two hidden layers (layers 0..2 are read), critic 1 one (layers 0..1)
            _step_refused(b"ctr_td3_critic_step: NULL layer among W, b, gW, gb, mW, mb, vW, vb [0..n_hidden]",
                          nets=nets(**{name: _ptrs(50 << 24, holes=(1,))}))
        _step_refused(b"ctr_td3_critic_step: NULL pointer array or pow in net", nets=nets(pow=None))
        same = _ptrs(60 << 24)
        _step_refused(b"ctr_td3_critic_step: a gradient or state tensor is a parameter tensor", nets=nets(gW=same, W=same))
        _step_refused(b"ctr_td3_critic_step: a gradient or state tensor is a parameter tensor",
                      nets=nets(pow=((16 * which + 1) << 24) + 4096))  # pow is W[1]
    assert _step(B=0, nets=(_net(0), _net(1, W=_ptrs(50 << 24, holes=(2,)))))[0] == 0        # layer 2 of critic 1 is not read
    nan, inf = float("nan"), float("inf")
    for kw in ({"lr": nan}, {"beta1": inf}, {"eps": nan}):
        _step_refused(b"ctr_td3_critic_step: lr, beta1, beta2 and eps must be finite", adam=_adam(**kw))
    _step_refused(b"ctr_td3_critic_step: beta1 and beta2 must be in [0, 1)", adam=_adam(beta1=1.0))
    _step_refused(b"ctr_td3_critic_step: eps must be positive", adam=_adam(eps=0.0))
    for B in (-1, 65537, 1 << 40):
        _step_refused(b"ctr_td3_critic_step: B must be in 0..65536", B=B)
    for kw in ({"rows": None}, {"actions": None}, {"target": None}):
        _step_refused(b"ctr_td3_critic_step: rows, actions or target is NULL", **kw)


def test_twin_step_refuses_nets_that_share_a_tensor():
    first = _net(0)
    for name in FIELDS:
        for other in FIELDS:
            arr = _ptrs((16 + FIELDS.index(other) + 1) << 24)              # net 1's own array of `other` ...
            arr[1] = ctypes.cast(getattr(first, name), ctypes.POINTER(ctypes.c_void_p))[0]   # ... layer 1: net 0's `name`[0]
            _step_refused(b"ctr_td3_critic_step: the two nets share a parameter, gradient or state tensor",
                          nets=(first, _net(1, **{other: arr})))
    _step_refused(b"ctr_td3_critic_step: the two nets share a tensor (pow)", nets=(first, _net(1, pow=first.pow)))
    _step_refused(b"ctr_td3_critic_step: the two nets share a parameter, gradient or state tensor",
                  nets=(first, _net(1, pow=(3 << 24) + 4096)))  # net 1's pow is net 0's gW[1]
    arr = _ptrs((16 + 5) << 24)
    arr[0] = first.pow                                                     # net 1's mW[0] is net 0's pow
    _step_refused(b"ctr_td3_critic_step: the two nets share a parameter, gradient or state tensor", nets=(first, _net(1, mW=arr)))
    _step_refused(b"ctr_td3_critic_step: the two nets share a tensor (pow)", nets=(first, first))


def test_twin_step_workspace():
    _abi, lib = _lib()
    _step_refused(b"ctr_td3_critic_step: workspace is NULL", ws=None)
    _step_refused(b"ctr_td3_critic_step: workspace must be 16-B aligned", ws=WS + 8)
    a, c1, c2 = _actor((32,)), _critic(), _critic((32,))
    need = lib.ctr_td3_workspace_bytes(a, c1, c2, 64)
    one = lib.ctr_ddpg_workspace_bytes(a, c1, 64)
    assert need > one > 0
    _step_refused(b"ctr_td3_critic_step: workspace too small (ctr_ddpg_workspace_bytes)", ws_bytes=1024)
    _step_refused(b"ctr_td3_critic_step: workspace too small (ctr_td3_workspace_bytes)", ws_bytes=one)  # room for critic 1 alone
    _step_refused(b"ctr_td3_critic_step: workspace too small (ctr_td3_workspace_bytes)", ws_bytes=need - 1)
    assert _step(ws_bytes=need, B=0)[0] == 0
    _step_refused(b"ctr_td3_critic_step: workspace too small (ctr_ddpg_workspace_bytes)",
                  ws_bytes=need, B=65)  # one more tile than it was sized for


SHAPE_PAIRS = [((64, 64), (32,)), ((32,), (32,)), ((64, 96), (32,)), ((128, 128, 128), (256, 128))]


@pytest.mark.parametrize("in_dim", [25, 26])
def test_workspace_bytes(in_dim):
    _abi, lib = _lib()
    for h1, h2 in SHAPE_PAIRS:
        for ah in ((32,), (256, 128)):
            a, c1, c2 = _actor(ah, in_dim - 6), _critic(h1, in_dim), _critic(h2, in_dim)
            for B in (1, 16, 1029, 65536):
                need = lib.ctr_td3_workspace_bytes(a, c1, c2, B)
                r1 = lib.ctr_ddpg_workspace_bytes(a, c1, B)
                # a critic's own region: what the single step needs under an actor smaller than the critic
                small = _actor((32,), in_dim - 6)
                regions = [lib.ctr_ddpg_workspace_bytes(small, c, B) for c in (c1, c2)]
                assert min(regions) > 0 and all(r % 16 == 0 for r in regions)
                assert need % 16 == 0 and need >= r1 and need >= sum(regions), (h1, h2, ah, B, need, r1, regions)
                assert need == max(sum(regions), r1)
            for B in (0, -1, 65537):
                assert lib.ctr_td3_workspace_bytes(a, c1, c2, B) == -1
                assert b"ctr_td3_workspace_bytes" in lib.ctr_last_error() and b"max_B" in lib.ctr_last_error()
    a, c = _actor(), _critic()
    for args, word in (((None, c, c), b"actor is NULL"), ((a, None, c), b"critic is NULL"), ((a, c, None), b"critic is NULL"),
                       ((a, c, _critic(in_dim=26)), b"in_dim"), ((a, _critic((64, 48)), c), b"width"),
                       ((_actor(in_dim=20), c, c), b"in_dim"), ((a, c, _critic((256, 256))), b"CTR_ACTOR_MAX_BYTES")):
        assert lib.ctr_td3_workspace_bytes(*(args + (64,))) == -1
        assert b"ctr_td3_workspace_bytes" in lib.ctr_last_error() and word in lib.ctr_last_error(), lib.ctr_last_error()


# ------------------------------------------------------------------------------------------
# policy.TargetSmoothing: the keying of the smoothing noise

def test_target_smoothing_pins_the_keying():
    from ctr_reach_amd.policy import TargetSmoothing, philox4x32
    ts = TargetSmoothing(0.2, 0.5)
    index = np.arange(300)
    out = ts.emulate(11, 3, index, np.zeros((300, 6), np.float32))
    assert out.shape == (300, 6) and out.dtype == np.float64
    # the uniforms, restated from the specification: stream 7, blocks 0 and 1, words w0..w3 | w4, w5
    key = np.array([11, 0], dtype=np.uint32)
    w = np.concatenate([philox4x32(np.stack((np.full(300, blk), np.full(300, 3), index, np.full(300, 7 << 24)),
                                            axis=-1).astype(np.uint32), key) for blk in (0, 1)], axis=-1)[:, :6]
    u = (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    assert u.dtype == np.float32 and np.array_equal(u, ts.uniforms(11, 3, index))
    assert (u.astype(np.float64) * 2.0 ** 24 == np.floor(u.astype(np.float64) * 2.0 ** 24)).all()      # exact: 24 bits
    z = ts.gaussians(11, 3, index)
    assert abs(z.mean()) < 0.1 and 0.9 < z.std() < 1.1, (z.mean(), z.std())
    assert abs(z.mean() - -0.005) < 1e-3 and abs(z.std() - 1.005) < 1e-3, (z.mean(), z.std())
    # zero actions: the output is the clipped noise itself
    assert np.array_equal(out, np.clip(float(np.float32(0.2)) * z, -0.5, 0.5))
    at_clip = np.abs(out) == 0.5
    assert at_clip.sum() == 26, at_clip.sum()
    free = np.abs(float(np.float32(0.2)) * z)[~at_clip]
    assert (0.5 - free).min() > 2.5e-4, (0.5 - free).min()                  # no value near enough to flip under f32
    assert at_clip[:65].sum() == 6
    # rows are keyed by their index alone; another counter or seed is another draw
    assert np.array_equal(ts.emulate(11, 3, np.arange(65), np.zeros((65, 6))), out[:65])
    assert np.array_equal(ts.emulate(11, 3, [299, 7], np.zeros((2, 6))), out[[299, 7]])
    assert not np.array_equal(ts.emulate(11, 4, index, np.zeros((300, 6))), out)
    assert not np.array_equal(ts.emulate(12, 3, index, np.zeros((300, 6))), out)
    assert not np.array_equal(ts.emulate(11 + (1 << 32), 3, index, np.zeros((300, 6))), out)
    assert not np.array_equal(ts.emulate(11, 3 + (1 << 32), index, np.zeros((300, 6))), out)
    # the sum and the box
    a = np.random.default_rng(5).uniform(-1, 1, (300, 6)).astype(np.float32)
    sm = ts.emulate(11, 3, index, a)
    assert np.array_equal(sm, np.clip(a.astype(np.float64) + out, -1.0, 1.0)) and (np.abs(sm) <= 1).all()
    assert (np.abs(sm) == 1).any()


def test_target_smoothing_no_noise_and_no_clip():
    from ctr_reach_amd.policy import TargetSmoothing
    a = np.random.default_rng(6).uniform(-1, 1, (40, 6)).astype(np.float32)
    same = TargetSmoothing(0.0, 0.5).emulate(11, 3, np.arange(40), a)
    assert same.dtype == np.float64 and np.array_equal(same.astype(np.float32).view(np.uint32), a.view(np.uint32))
    z = TargetSmoothing(0.2, 0.5).gaussians(11, 3, np.arange(40))
    free = TargetSmoothing(0.2, np.inf).emulate(11, 3, np.arange(40), np.zeros((40, 6)))
    assert np.array_equal(free, float(np.float32(0.2)) * z)
    assert np.array_equal(TargetSmoothing(0.2, 0.0).emulate(11, 3, np.arange(40), a), a.astype(np.float64))
    for kw in ({"sigma": -0.1}, {"sigma": np.inf}, {"sigma": np.nan}, {"clip": -0.5}, {"clip": np.nan}):
        with pytest.raises(ValueError, match=list(kw)[0]):
            TargetSmoothing(**kw)


# ------------------------------------------------------------------------------------------
# Td3Learner and sample_td3: every ValueError comes before the library or a GPU is touched.

def _mlp(n_in, hidden, n_out, tanh, grad=False):
    import torch.nn as nn
    dims = [n_in] + list(hidden)
    mods = []
    for a, b in zip(dims[:-1], dims[1:]):
        mods += [nn.Linear(a, b), nn.ReLU()]
    mods.append(nn.Linear(dims[-1], n_out))
    if tanh:
        mods.append(nn.Tanh())
    return nn.Sequential(*mods).requires_grad_(grad)


def test_learner_refuses_what_it_would_have_to_convert_or_could_not_write():
    import torch
    from ctr_reach_amd.learner import Td3Learner
    policy, c1, c2 = _mlp(19, (64, 96), 6, True), _mlp(25, (32,), 1, False), _mlp(25, (64, 32), 1, False)
    with pytest.raises(ValueError, match=exact("policy layer 0: W" + WRITES_IN_PLACE)):
        Td3Learner(_mlp(19, (64,), 6, True, grad=True), c1, c2)
    with pytest.raises(ValueError, match=exact("critic1 layer 0: W" + WRITES_IN_PLACE)):
        Td3Learner(policy, _mlp(25, (32,), 1, False, grad=True), c2)
    half = _mlp(25, (32,), 1, False)
    half[2].bias.requires_grad_(True)
    with pytest.raises(ValueError, match=exact("critic2 layer 1: b" + WRITES_IN_PLACE)):
        Td3Learner(policy, c1, half)
    with pytest.raises(ValueError, match=exact("the actor ends with nn.Tanh")):
        Td3Learner(_mlp(19, (64,), 6, False), c1, c2)
    with pytest.raises(ValueError, match=exact("the critic2 ends with its output nn.Linear (no activation after it)")):
        Td3Learner(policy, c1, _mlp(25, (32,), 1, True))
    with pytest.raises(ValueError, match=exact("the policy's rows are obs_dim + 6 = 19 or 20 floats")):
        Td3Learner(_mlp(18, (64,), 6, True), c1, c2)
    with pytest.raises(ValueError, match=exact("the critic1's rows are obs_dim + 12 = 25 or 26 floats")):
        Td3Learner(policy, _mlp(19, (64,), 1, False), c2)
    with pytest.raises(ValueError, match=exact("the critic2 takes [row, action]: 19 + 6 inputs, not 26")):
        Td3Learner(policy, c1, _mlp(26, (32,), 1, False))
    with pytest.raises(ValueError, match=exact("critic1: hidden widths must be multiples of 32 in 32..256")):
        Td3Learner(policy, _mlp(25, (48,), 1, False), c2)
    with pytest.raises(ValueError, match=exact("the critic2 has 1..3 hidden layers and an output layer")):
        Td3Learner(policy, c1, _mlp(25, (32, 32, 32, 32), 1, False))
    with pytest.raises(ValueError, match=exact("critic2 layer 1: b must be float32, not torch.float64")):
        layers = [(m.weight, m.bias) for m in c1 if hasattr(m, "weight")]
        Td3Learner(policy, c1, [layers[0], (layers[1][0], layers[1][1].double())])
    with pytest.raises(ValueError, match=exact("critic1 layer 0: W must be contiguous")):
        Td3Learner(policy, [(torch.zeros((25, 32)).t(), torch.zeros(32)), (torch.zeros((1, 32)), torch.zeros(1))], c2)
    with pytest.raises(ValueError, match=exact("critic2 layer 0: W must be a torch tensor")):
        Td3Learner(policy, c1, [(np.zeros((32, 25), np.float32), torch.zeros(32)), (torch.zeros((1, 32)), torch.zeros(1))])
    with pytest.raises(ValueError, match=exact("critic1 and critic2 share a tensor: the twin step updates them side by side")):
        Td3Learner(policy, c1, c1)
    layers = [(m.weight, m.bias) for m in c1 if hasattr(m, "weight")]
    other = [(m.weight, m.bias) for m in _mlp(25, (32,), 1, False) if hasattr(m, "weight")]
    with pytest.raises(ValueError, match=exact("critic1 and critic2 share a tensor: the twin step updates them side by side")):
        Td3Learner(policy, layers, [other[0], (other[1][0], layers[1][1])])
    for kw, word in (({"betas": (1.0, 0.999)}, "betas must be in [0, 1)"), ({"betas": (0.9, -0.1)}, "betas must be in [0, 1)"),
                     ({"eps": 0.0}, "eps must be positive"), ({"eps": float("nan")}, "eps must be finite"),
                     ({"actor_lr": float("inf")}, "actor_lr must be finite"),
                     ({"critic_lr": float("nan")}, "critic_lr must be finite"),
                     ({"max_batch": 0}, "max_batch must be in 1..65536"), ({"max_batch": 65537}, "max_batch must be in 1..65536"),
                     ({"scale": [1.0] * 5}, "scale is six finite, non-zero floats"),
                     ({"scale": [1.0, 1.0, 0.0, 1.0, 1.0, 1.0]}, "scale is six finite, non-zero floats")):
        with pytest.raises(ValueError, match=exact(word)):
            Td3Learner(policy, c1, c2, **kw)
    with pytest.raises(ValueError, match=exact("the networks are on cpu: the learner's networks are on a GPU")):   # (all else in order)
        Td3Learner(policy, c1, c2, scale=[0.001] * 3 + [0.087] * 3)


def test_sample_td3_refuses_host_networks_and_bad_noise():
    """The checks come before anything is allocated or the library is called: a buffer that has only
    its device is enough to see them."""
    import torch
    from ctr_reach_amd.her import HerReplayBuffer
    from ctr_reach_amd.policy import MlpActor, MlpCritic
    rng = np.random.default_rng(3)

    def layers(dims):
        return [(rng.uniform(-1, 1, (dims[l + 1], dims[l])).astype(np.float32),
                 rng.uniform(-1, 1, dims[l + 1]).astype(np.float32)) for l in range(len(dims) - 1)]

    buf = HerReplayBuffer.__new__(HerReplayBuffer)
    buf.venv = types.SimpleNamespace(device=torch.device("cpu"))
    host_actor = MlpActor(layers([19, 64, 6]), np.full(6, 0.5, np.float32), device=None)
    host_critic = MlpCritic(layers([25, 32, 1]), device=None)
    cpu_actor = MlpActor(layers([19, 64, 6]), np.full(6, 0.5, np.float32), device="cpu")
    cpu_critic = MlpCritic(layers([25, 32, 1]), device="cpu")
    with pytest.raises(ValueError, match="sample_td3: the actor must be on the device"):
        buf.sample_td3(8, host_actor, cpu_critic, cpu_critic, 0.99)
    with pytest.raises(ValueError, match="sample_td3: the critic1 must be on the device"):
        buf.sample_td3(8, cpu_actor, host_critic, cpu_critic, 0.99)
    with pytest.raises(ValueError, match="sample_td3: the critic2 must be on the device"):
        buf.sample_td3(8, cpu_actor, cpu_critic, host_critic, 0.99)
    # on the networks' "device" the noise is looked at
    for kw, word in (({"gamma": float("nan")}, "gamma"), ({"sigma": -0.1}, "sigma"), ({"sigma": float("inf")}, "sigma"),
                     ({"clip": -0.5}, "clip"), ({"clip": float("nan")}, "clip")):
        args = dict(gamma=0.99)
        args.update(kw)
        with pytest.raises(ValueError, match="sample_td3: " + word):
            buf.sample_td3(8, cpu_actor, cpu_critic, cpu_critic, **args)
    buf.venv.device = torch.device("cuda", 0)
    with pytest.raises(ValueError, match="sample_td3: the actor is on cpu, the buffer on cuda:0"):
        buf.sample_td3(8, cpu_actor, cpu_critic, cpu_critic, 0.99)
