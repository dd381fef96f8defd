"""The MLP critic and the TD sampler on the host (no GPU): ctr_critic_blob_bytes, ctr_critic_pack,
ctr_critic, ctr_critic_load and ctr_her_sample_td refuse bad arguments with CTR_EINVAL (-1) and a
telling ctr_last_error before any HIP call (the device pointers are fake and never dereferenced);
ctr_critic_pack's bytes are an independent numpy restatement of the layout the header documents;
the ctypes structs match the header; MlpCritic.emulate is the specification."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(32,), (64, 96), (128, 128, 128), (256, 128)]


def _lib():
    from ctr_reach_amd import _abi
    return _abi, _abi.load()


def _critic(hidden=(64, 64), in_dim=25):
    from ctr_reach_amd import _abi_critic
    c = _abi_critic.CtrCritic()
    c.in_dim, c.n_hidden = in_dim, len(hidden)
    for l, w in enumerate(hidden):
        c.width[l] = w
    c.blob = 1 << 20
    return c


def _actor(hidden=(64, 64), in_dim=19):
    from ctr_reach_amd import _abi
    a = _abi.CtrActor()
    a.in_dim, a.n_hidden = in_dim, len(hidden)
    for l, w in enumerate(hidden):
        a.width[l] = w
    for i in range(6):
        a.scale[i] = 0.5
    a.blob = 1 << 21
    return a


def _refused(critic, word, shape=True):
    """Every critic entry point refuses `critic` with `word` in the message (shape=False: the two
    that read only the shape are left out)."""
    _abi, lib = _lib()
    W = (ctypes.c_void_p * 4)(16, 16, 16, 16)
    calls = [("ctr_critic", lambda: lib.ctr_critic(critic, 16, 16, 8, 16, None)),
             ("ctr_critic_load", lambda: lib.ctr_critic_load(critic, W, W, None))]
    if shape:
        calls += [("ctr_critic_blob_bytes", lambda: lib.ctr_critic_blob_bytes(critic)),
                  ("ctr_critic_pack", lambda: lib.ctr_critic_pack(critic, W, W, 16))]
    for name, call in calls:
        assert call() == -1, name
        assert word in lib.ctr_last_error(), (name, lib.ctr_last_error())


def test_exported_and_abi_number():
    _abi, lib = _lib()
    for name in ("ctr_critic_blob_bytes", "ctr_critic_pack", "ctr_critic_load", "ctr_critic", "ctr_her_sample_td"):
        assert name in _abi.EXPORTED and hasattr(lib, name), name
    assert lib.ctr_abi_version() == _abi.CTR_ABI_VERSION == 17


def test_critic_shapes_are_validated():
    for d in (24, 27):
        _refused(_critic(in_dim=d), b"in_dim")
    for nh in (0, 4):
        c = _critic()
        c.n_hidden = nh
        _refused(c, b"n_hidden")
    for w in (0, 48, 288):
        _refused(_critic((64, w)), b"width")
    _refused(_critic((256, 256)), b"CTR_ACTOR_MAX_BYTES")
    _abi, lib = _lib()
    assert lib.ctr_critic_blob_bytes(_critic((256, 256))) == -1
    msg = lib.ctr_last_error()
    assert b"critic" in msg and b"163840 B of weights" in msg and b"2176 B of biases" in msg, msg
    W = (ctypes.c_void_p * 4)(16, 16, 16, 16)
    assert lib.ctr_critic_blob_bytes(None) == -1 and b"critic is NULL" in lib.ctr_last_error()
    assert lib.ctr_critic_pack(None, W, W, 16) == -1
    assert lib.ctr_critic_load(None, W, W, None) == -1
    assert lib.ctr_critic(None, 16, 16, 8, 16, None) == -1
    # the sizes: the actor's, whose 6-row output tile is padded to 32 rows as the critic's 1-row tile is
    assert lib.ctr_critic_blob_bytes(_critic((32,))) == 2048 + 2048 + 256
    assert lib.ctr_critic_blob_bytes(_critic((128, 128, 128), 26)) == 81920 + 1664
    assert lib.ctr_critic_blob_bytes(_critic((256, 128))) == 90112 + 1664


def test_critic_blob_and_arrays_are_validated():
    _abi, lib = _lib()
    c = _critic()
    c.blob = None
    _refused(c, b"blob", shape=False)
    c.blob = (1 << 20) + 8
    _refused(c, b"16-B aligned", shape=False)
    assert lib.ctr_critic_blob_bytes(c) == 4096 + 8192 + 4096 + 640            # (the blob is not read)
    c = _critic()
    assert lib.ctr_critic(c, None, 16, 8, 16, None) == -1 and b"rows" in lib.ctr_last_error()
    assert lib.ctr_critic(c, 16, None, 8, 16, None) == -1
    assert lib.ctr_critic(c, 16, 16, 8, None, None) == -1
    assert lib.ctr_critic(c, 16, 16, -1, 16, None) == -1 and b"n out of range" in lib.ctr_last_error()
    assert lib.ctr_critic(c, None, None, 0, None, None) == 0                    # an empty batch
    W = (ctypes.c_void_p * 4)(16, 16, 16, 16)
    hole = (ctypes.c_void_p * 4)(16, None, 16, 16)
    assert lib.ctr_critic_load(c, None, W, None) == -1 and b"ctr_critic_load" in lib.ctr_last_error()
    assert lib.ctr_critic_load(c, W, hole, None) == -1 and b"NULL layer" in lib.ctr_last_error()
    assert lib.ctr_critic_pack(c, W, None, 16) == -1 and b"ctr_critic_pack" in lib.ctr_last_error()
    assert lib.ctr_critic_pack(c, hole, W, 16) == -1 and b"NULL layer" in lib.ctr_last_error()


def _her(obs_dim=13, n=8):
    from ctr_reach_amd import _abi
    h = _abi.CtrHer()
    h.obs_dim, h.t_max, h.n_sampled_goal, h.strategy = obs_dim, 5, 4, _abi.CTR_HER_FUTURE
    h.n, h.env_base, h.slots, h.seed = n, 0, 3, 1
    for name in ("state", "step", "dg", "tol", "len", "epoch", "cur_t", "cur_epoch", "cdf"):
        setattr(h, name, 1 << 12)
    return h


def _td_call(her=None, B=8, out="default", td="default", actor=None, critic=None, gamma=0.99, target=1 << 14):
    from ctr_reach_amd import _abi_critic
    _abi, lib = _lib()
    her = her if her is not None else _her()
    if out == "default":
        out = _abi.CtrHerBatch()
        out.obs = out.action = out.reward = out.next_obs = out.done = 1 << 13
    if td == "default":
        td = _abi_critic.CtrHerTd()
        actor = actor if actor is not None else _actor()
        critic = critic if critic is not None else _critic()
        td.actor, td.critic = ctypes.pointer(actor), ctypes.pointer(critic)
        td.gamma, td.target = gamma, target
    return lib.ctr_her_sample_td(her, B, 1, 0, out, td, None), lib.ctr_last_error()


def test_her_sample_td_refusals():
    from ctr_reach_amd import _abi_critic
    _abi, lib = _lib()

    def refused(word, **kw):
        rc, msg = _td_call(**kw)
        assert rc == -1 and word in msg, (word, rc, msg)

    # what ctr_her_sample refuses
    assert lib.ctr_her_sample_td(None, 8, 1, 0, None, None, None) == -1 and b"her is NULL" in lib.ctr_last_error()
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
    # its own
    refused(b"td is NULL", td=None)
    refused(b"target", target=None)
    td = _abi_critic.CtrHerTd()
    td.critic, td.gamma, td.target = ctypes.pointer(_critic()), 0.99, 1 << 14
    refused(b"actor is NULL", td=td)
    td = _abi_critic.CtrHerTd()
    td.actor, td.gamma, td.target = ctypes.pointer(_actor()), 0.99, 1 << 14
    refused(b"critic is NULL", td=td)
    refused(b"actor: n_hidden", actor=_actor(()))
    refused(b"critic: every hidden width", critic=_critic((64, 48)))
    refused(b"CTR_ACTOR_MAX_BYTES", critic=_critic((256, 256)))
    a = _actor()
    a.blob = None
    refused(b"actor: blob", actor=a)
    c = _critic()
    c.blob = (1 << 20) + 4
    refused(b"critic: blob must be 16-B aligned", critic=c)
    refused(b"actor->in_dim", actor=_actor(in_dim=20))
    refused(b"critic->in_dim", critic=_critic(in_dim=26))
    refused(b"actor->in_dim", her=_her(obs_dim=14))
    refused(b"critic->in_dim", her=_her(obs_dim=14), actor=_actor(in_dim=20))
    for g in (float("nan"), float("inf"), -float("inf")):
        refused(b"gamma", gamma=g)
    # the actor's scale is not read
    a = _actor()
    a.scale[2] = float("nan")
    assert _td_call(B=0, actor=a)[0] == 0
    # an empty draw is a no-op (and still a checked call)
    assert _td_call(B=0)[0] == 0
    refused(b"td is NULL", B=0, td=None)


def _layers(rng, hidden, in_dim):
    dims = [in_dim] + list(hidden) + [1]
    layers = []
    for l in range(len(dims) - 1):
        s = 1.0 / np.sqrt(dims[l])
        layers.append((rng.uniform(-s, s, (dims[l + 1], dims[l])).astype(np.float32),
                       rng.uniform(-s, s, dims[l + 1]).astype(np.float32)))
    return layers


def _bf16_bits(W):
    """Round to nearest even in integer arithmetic; every value here is finite."""
    u = np.ascontiguousarray(W, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _numpy_pack(layers, hidden, in_dim):
    """The blob as the header documents it ("MLP actor", with a 1-row output layer), from the
    matrices: fragments [tile][k-step][lane][8] per layer, then the biases padded to 32-row tiles."""
    dims = [in_dim] + list(hidden) + [1]
    frags, biases = [], []
    for l, (W, b) in enumerate(layers):
        rows, cols = dims[l + 1], dims[l]
        tiles = (rows + 31) // 32
        ksteps = 2 if l == 0 else cols // 16
        Wp = np.zeros((tiles * 32, ksteps * 16), dtype=np.uint16)
        Wp[:rows, :cols] = _bf16_bits(W)
        T, S, lane, j = np.meshgrid(np.arange(tiles), np.arange(ksteps), np.arange(64), np.arange(8), indexing="ij")
        h = lane >> 5
        k = 16 * S + 8 * h + j if l == 0 else 32 * (S >> 1) + 16 * (S & 1) + 8 * (j >> 2) + 4 * h + (j & 3)
        frags.append(Wp[32 * T + (lane & 31), k].reshape(-1).view(np.uint8))
        bp = np.zeros(tiles * 32, dtype=np.float32)
        bp[:rows] = b
        biases.append(bp.view(np.uint8))
    return np.concatenate(frags + biases)


@pytest.mark.parametrize("in_dim", [25, 26])
@pytest.mark.parametrize("hidden", SHAPES)
def test_pack_is_the_documented_layout(hidden, in_dim):
    from ctr_reach_amd.policy import MlpCritic
    _abi, lib = _lib()
    layers = _layers(np.random.default_rng(7 + in_dim + len(hidden)), hidden, in_dim)
    layers[0][0][3, 24] = np.float32(1.0 + 2.0 ** -8 + 2.0 ** -20)    # above the tie: up
    layers[0][0][4, in_dim - 1] = np.float32(1.0 + 2.0 ** -8)         # the tie: to even (down)
    crit = MlpCritic(layers, device=None)
    want = _numpy_pack(layers, hidden, in_dim)
    nb = lib.ctr_critic_blob_bytes(crit._struct)
    assert nb == want.size
    blob = np.full(nb, 0xAB, dtype=np.uint8)                          # unwritten padding would show
    n = len(layers)
    W = (ctypes.c_void_p * n)(*[w.ctypes.data for w in crit.weights])
    b = (ctypes.c_void_p * n)(*[v.ctypes.data for v in crit.biases])
    assert lib.ctr_critic_pack(crit._struct, W, b, blob.ctypes.data) == 0
    bad = np.flatnonzero(blob != want)
    assert bad.size == 0, (hidden, in_dim, bad.size, bad[:8].tolist())
    assert np.array_equal(crit._pack_host(), want)
    # (the restatement rounds as the header says)
    assert _bf16_bits(layers[0][0][3, 24]) == 0x3F81 and _bf16_bits(layers[0][0][4, in_dim - 1]) == 0x3F80


def test_struct_layout_matches_header(tmp_path):
    from ctr_reach_amd import _abi_critic
    lines, want = [], []
    for cname, cls in (("ctr_critic_t", _abi_critic.CtrCritic), ("ctr_her_td_t", _abi_critic.CtrHerTd)):
        lines.append('  printf("%%zu\\n", sizeof(%s));' % cname)
        want.append(ctypes.sizeof(cls))
        for fname, _ in cls._fields_:
            lines.append('  printf("%%zu\\n", offsetof(%s, %s));' % (cname, fname))
            want.append(getattr(cls, fname).offset)
    lines.append('  printf("%d\\n", CTR_ABI_VERSION);')
    want.append(17)
    prog = tmp_path / "critic_layout.c"
    prog.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"ctr_reach_amd.h\"\nint main(void) {\n"
                    + "\n".join(lines) + "\n  return 0; }\n")
    exe = tmp_path / "critic_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(prog), "-o", str(exe)])
    assert list(map(int, subprocess.check_output([str(exe)]).split())) == want


@pytest.mark.parametrize("in_dim", [25, 26])
def test_emulate_is_integer_arithmetic_on_small_integers(in_dim):
    """Where every value is a small integer no rounding of the specification acts, and emulate must
    be the plain integer MLP."""
    from ctr_reach_amd.policy import MlpCritic
    rng = np.random.default_rng(in_dim)
    hidden = (32, 64)
    dims = [in_dim] + list(hidden) + [1]
    layers = [(rng.integers(-1, 2, (dims[l + 1], dims[l])).astype(np.float32),
               rng.integers(-2, 3, dims[l + 1]).astype(np.float32)) for l in range(3)]
    crit = MlpCritic(layers, device=None)
    rows = rng.integers(-2, 3, (50, in_dim - 6))
    acts = rng.integers(-1, 2, (50, 6))
    z = np.concatenate([rows, acts], axis=1).astype(np.int64)
    for l, (W, b) in enumerate(layers):
        z = z @ W.astype(np.int64).T + b.astype(np.int64)
        if l < 2:
            z = np.maximum(z, 0)
            assert z.max() <= 256                                       # exact in bf16
    q = crit.emulate(rows, acts)
    assert q.shape == (50,) and np.array_equal(q, z[:, 0].astype(np.float64))
    assert np.array_equal(crit.reference(rows, acts), q)
    assert len(np.unique(q)) > 3


def test_mlp_critic_shape_checks():
    from ctr_reach_amd.policy import MlpCritic
    rng = np.random.default_rng(0)
    MlpCritic(_layers(rng, (32,), 25))
    with pytest.raises(ValueError, match="25 or 26"):
        MlpCritic(_layers(rng, (32,), 20))
    bad = _layers(rng, (32,), 25)
    bad[-1] = (np.zeros((6, 32), np.float32), np.zeros(6, np.float32))
    with pytest.raises(ValueError, match="1 row"):
        MlpCritic(bad)
    with pytest.raises(ValueError, match="multiples of 32"):
        MlpCritic(_layers(rng, (48,), 25))
    with pytest.raises(ValueError, match="hidden layers"):
        MlpCritic(_layers(rng, (32, 32, 32, 32), 25))
