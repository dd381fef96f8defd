"""ctr_polyak on the host (no GPU): the symbol is declared, listed and exported; the ctypes mirror of
ctr_polyak_net_t matches the header; every refusal the header lists returns CTR_EINVAL (-1) with a
ctr_last_error that names ctr_polyak, before any HIP call (the device pointers are fake and never
dereferenced); policy.polyak_ refuses what it would have to convert or could not write."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _ptrs(base, holes=()):
    return (ctypes.c_void_p * 4)(*[None if l in holes else base + 4096 * l for l in range(4)])


def _net(actor=None, critic=None, W="default", b="default", W_targ="default", b_targ="default"):
    """One ctr_polyak_net_t on fake, pairwise different device pointers."""
    from ctr_reach_amd import _abi_polyak
    n = _abi_polyak.CtrPolyakNet()
    if actor is not None:
        n.actor = ctypes.pointer(actor)
    if critic is not None:
        n.critic = ctypes.pointer(critic)
    for name, value, base in (("W", W, 1 << 24), ("b", b, 2 << 24), ("W_targ", W_targ, 3 << 24), ("b_targ", b_targ, 4 << 24)):
        if isinstance(value, str):
            value = _ptrs(base)
        if value is not None:
            setattr(n, name, value)
    return n


def _refused(nets, word, n_nets=None, tau=0.001):
    from ctr_reach_amd import _abi_polyak
    _abi, lib = _lib()
    arr = (_abi_polyak.CtrPolyakNet * max(len(nets), 1))(*nets)
    rc = lib.ctr_polyak(arr, len(nets) if n_nets is None else n_nets, tau, None)
    msg = lib.ctr_last_error()
    assert rc == -1 and b"ctr_polyak" in msg and word in msg, (word, rc, msg)


def test_declared_listed_and_exported():
    _abi, lib = _lib()
    header = open(os.path.join(ROOT, "include", "ctr_reach_amd.h")).read()
    assert re.search(r"^int ctr_polyak\(const ctr_polyak_net_t \*nets, int32_t n_nets, float tau, void \*stream\);",
                     header, re.M)
    assert "ctr_polyak" in _abi.EXPORTED and hasattr(lib, "ctr_polyak")
    assert lib.ctr_abi_version() == _abi.CTR_ABI_VERSION == 17


def test_struct_layout_matches_header(tmp_path):
    from ctr_reach_amd import _abi_polyak
    cls = _abi_polyak.CtrPolyakNet
    lines = ['  printf("%zu\\n", sizeof(ctr_polyak_net_t));']
    want = [ctypes.sizeof(cls)]
    for fname, _ in cls._fields_:
        lines.append('  printf("%%zu\\n", offsetof(ctr_polyak_net_t, %s));' % fname)
        want.append(getattr(cls, fname).offset)
    lines.append('  printf("%d\\n", CTR_POLYAK_MAX_NETS);')
    want.append(_abi_polyak.CTR_POLYAK_MAX_NETS)
    lines.append('  printf("%d\\n", CTR_ABI_VERSION);')
    want.append(17)
    prog = tmp_path / "polyak_layout.c"
    prog.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"ctr_reach_amd.h\"\nint main(void) {\n"
                    + "\n".join(lines) + "\n  return 0; }\n")
    exe = tmp_path / "polyak_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(prog), "-o", str(exe)])
    assert list(map(int, subprocess.check_output([str(exe)]).split())) == want
    assert [f for f, _ in cls._fields_] == ["actor", "critic", "W", "b", "W_targ", "b_targ"]


def test_nets_and_count_are_validated():
    _abi, lib = _lib()
    assert lib.ctr_polyak(None, 1, 0.001, None) == -1
    assert b"ctr_polyak" in lib.ctr_last_error() and b"nets is NULL" in lib.ctr_last_error()
    good = _net(actor=_actor())
    for n in (0, -1, 5):
        _refused([good], b"n_nets", n_nets=n)
    a, c = _actor(), _critic()
    _refused([_net(actor=a, critic=c)], b"exactly one")
    _refused([_net()], b"exactly one")
    _refused([good, _net()], b"net 1")                                   # (the second net is looked at too)


def test_shapes_and_blobs_are_validated():
    _refused([_net(actor=_actor(in_dim=21))], b"in_dim")
    _refused([_net(critic=_critic(in_dim=24))], b"in_dim")
    _refused([_net(actor=_actor(()))], b"n_hidden")
    _refused([_net(critic=_critic((64, 48)))], b"width")
    _refused([_net(critic=_critic((256, 256)))], b"CTR_ACTOR_MAX_BYTES")
    a = _actor()
    a.scale[3] = float("inf")
    _refused([_net(actor=a)], b"scale")
    _refused([_net(actor=_actor(blob=None))], b"blob is NULL")
    _refused([_net(critic=_critic(blob=(1 << 20) + 8))], b"16-B aligned")


def test_pointer_arrays_and_layers_are_validated():
    a = _actor()                                                           # two hidden layers: layers 0..2 are read
    for name in ("W", "b", "W_targ", "b_targ"):
        _refused([_net(actor=a, **{name: None})], b"is NULL")
        _refused([_net(actor=a, **{name: _ptrs(5 << 24, holes=(2,))})], b"NULL layer")
    # ... and layer 3 is not: the call gets as far as its last check
    _refused([_net(actor=a, W=_ptrs(5 << 24, holes=(3,)))], b"tau", tau=float("nan"))


def test_aliases_are_refused():
    a = _actor()
    same = _ptrs(7 << 24)
    _refused([_net(actor=a, W=same, W_targ=same)], b"same tensor")
    _refused([_net(actor=a, b=same, b_targ=same)], b"same tensor")
    mixed = _ptrs(3 << 24)
    mixed[0] = 9 << 24                                                     # only layer 2 coincides with W_targ's
    mixed[1] = 10 << 24
    _refused([_net(actor=a, W=mixed)], b"same tensor")
    c = _critic(blob=a.blob)
    _refused([_net(actor=a), _net(critic=c)], b"blob")
    _refused([_net(actor=a), _net(critic=_critic()), _net(actor=_actor((32,), blob=3 << 21)), _net(actor=a)], b"net 3")


def test_tau_is_validated():
    good = _net(actor=_actor())
    for tau in (float("nan"), -1e-6, 1.0001, float("inf"), -float("inf")):
        _refused([good], b"tau", tau=tau)


# ------------------------------------------------------------------------------------------
# policy.polyak_: a net whose "device" is the CPU has a blob and takes CPU tensors through every
# check; no call here gets as far as the library.

HIDDEN, IN_DIM = (64, 96), 20


def _layers(rng, hidden=HIDDEN, dims_in=IN_DIM, out=6):
    dims = [dims_in] + list(hidden) + [out]
    return [(rng.uniform(-1, 1, (dims[l + 1], dims[l])).astype(np.float32),
             rng.uniform(-1, 1, dims[l + 1]).astype(np.float32)) for l in range(len(dims) - 1)]


def _tensors(layers):
    import torch
    return [(torch.from_numpy(W.copy()), torch.from_numpy(b.copy())) for W, b in layers]


def _cpu_actor(rng):
    from ctr_reach_amd.policy import MlpActor
    return MlpActor(_layers(rng), np.full(6, 0.5, np.float32), device="cpu")


def test_polyak_refuses_a_host_only_net_and_bad_lists():
    from ctr_reach_amd.policy import MlpActor, MlpCritic, polyak_
    import ctr_reach_amd
    assert ctr_reach_amd.polyak_ is polyak_
    rng = np.random.default_rng(0)
    layers = _layers(rng)
    host = MlpActor(layers, np.full(6, 0.5, np.float32), device=None)
    with pytest.raises(RuntimeError, match="on the host"):
        polyak_([(host, _tensors(layers), _tensors(layers))], 0.001)
    with pytest.raises(RuntimeError, match="on the host"):
        host.polyak_(_tensors(layers), _tensors(layers), 0.001)
    crit_layers = _layers(rng, (32,), 25, 1)
    crit = MlpCritic(crit_layers, device=None)
    with pytest.raises(RuntimeError, match="on the host"):
        crit.polyak_(_tensors(crit_layers), _tensors(crit_layers), 0.5)
    net = _cpu_actor(rng)
    triple = (net, _tensors(layers), _tensors(layers))
    with pytest.raises(ValueError, match="1..4 triples"):
        polyak_([], 0.001)
    with pytest.raises(ValueError, match="1..4 triples"):
        polyak_([triple] * 5, 0.001)
    with pytest.raises(ValueError, match="1..4 triples"):
        polyak_([triple[:2]], 0.001)
    with pytest.raises(ValueError, match="MlpActor"):
        polyak_([(object(), triple[1], triple[2])], 0.001)
    for tau in (float("nan"), -0.1, 1.5):
        with pytest.raises(ValueError, match="tau"):
            polyak_([triple], tau)
    for which in (1, 2):                                                   # a wrong layer count, on either list
        short = list(triple)
        short[which] = short[which][:2]
        with pytest.raises(ValueError, match="3 layers"):
            polyak_([tuple(short)], 0.001)
    assert net.weights is not None and net._sources is None               # nothing was dropped or adopted


@pytest.mark.parametrize("role", ["online", "target"])
def test_polyak_refuses_tensors_it_would_have_to_convert(role):
    import torch
    from ctr_reach_amd.policy import polyak_
    rng = np.random.default_rng(1)
    net = _cpu_actor(rng)
    kept = net.weights

    def refused(l, which, tensor, word):
        lists = {"online": [list(p) for p in _tensors(_layers(rng))], "target": [list(p) for p in _tensors(_layers(rng))]}
        lists[role][l][which] = tensor
        with pytest.raises(ValueError, match=word) as err:
            polyak_([(net, [tuple(p) for p in lists["online"]], [tuple(p) for p in lists["target"]])], 0.001)
        assert role in str(err.value) and "layer %d" % l in str(err.value)

    good = _tensors(_layers(rng))
    refused(1, 0, good[1][0].double(), "float32")
    refused(2, 1, good[2][1].double(), "float32")
    refused(1, 0, torch.zeros((64, 96)).t(), "contiguous")                 # [96, 64], strides (1, 96)
    refused(0, 1, torch.zeros(128)[::2], "contiguous")
    refused(0, 0, torch.zeros((64, 19)), "must be")
    refused(2, 0, torch.zeros((32, 96)), "must be")
    refused(1, 1, torch.zeros((96, 1)), "must be")
    refused(0, 0, torch.zeros((64, 20), device="meta"), "is on meta")
    refused(2, 1, torch.zeros(6, device="meta"), "is on meta")
    refused(0, 0, good[0][0].numpy(), "torch tensor")
    assert net.weights is kept and net._sources is None


def test_polyak_refuses_a_target_that_requires_grad():
    import torch.nn as nn
    from ctr_reach_amd.policy import polyak_
    rng = np.random.default_rng(2)
    net = _cpu_actor(rng)
    online, target = _tensors(_layers(rng)), _tensors(_layers(rng))
    target[1][1].requires_grad_(True)
    with pytest.raises(ValueError, match="target layer 1: b requires grad"):
        polyak_([(net, online, target)], 0.001)
    # a module's parameters require grad until the trainer says otherwise; as the online list they may
    seq = nn.Sequential(nn.Linear(20, 64), nn.ReLU(), nn.Linear(64, 96), nn.ReLU(), nn.Linear(96, 6), nn.Tanh())
    with pytest.raises(ValueError, match="target layer 0: W requires grad"):
        polyak_([(net, online, seq)], 0.001)
    with pytest.raises(ValueError, match="nn.Tanh"):
        polyak_([(net, nn.Sequential(*list(seq)[:-1]), target)], 0.001)
    online[0][0].requires_grad_(True)
    target[1][1].requires_grad_(False)
    with pytest.raises(ValueError, match="target layer 2: W must be float32"):   # (the online list passed)
        polyak_([(net, online, target[:2] + [(target[2][0].double(), target[2][1])])], 0.001)
