"""ctr_ddpg_critic_step / ctr_ddpg_actor_step on the host (no GPU): the symbols are declared, listed
and exported; the ctypes mirrors match the header; every refusal the header lists returns CTR_EINVAL
(-1) with a ctr_last_error that names the function, before any HIP call (the device pointers are
fake and never dereferenced); ctr_ddpg_workspace_bytes; DdpgLearner's ValueErrors; and the numpy
float32 restatement of the Adam step (learner.adam_reference, which the GPU tests hold the kernel to
bit for bit) against torch.optim.Adam within a bound derived from the roundings that differ."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FNS = ("ctr_ddpg_workspace_bytes", "ctr_ddpg_critic_step", "ctr_ddpg_actor_step")


def _lib():
    from ctr_reach_amd import _abi
    return _abi, _abi.load()


def _actor(hidden=(64, 64), in_dim=19):
    from ctr_reach_amd import _abi
    a = _abi.CtrActor()
    a.in_dim, a.n_hidden = in_dim, len(hidden)
    for l, w in enumerate(hidden):
        a.width[l] = w
    return a                                                               # (scale and blob are not read)


def _critic(hidden=(64, 64), in_dim=25):
    from ctr_reach_amd import _abi_critic
    c = _abi_critic.CtrCritic()
    c.in_dim, c.n_hidden = in_dim, len(hidden)
    for l, w in enumerate(hidden):
        c.width[l] = w
    return c


def _ptrs(base, holes=()):
    return (ctypes.c_void_p * 4)(*[None if l in holes else base + 4096 * l for l in range(4)])


FIELDS = ("W", "b", "gW", "gb", "mW", "mb", "vW", "vb")


def _net(**over):
    """One ctr_ddpg_net_t on fake, pairwise different device pointers; ``over``: a field's array, or
    None for a NULL one."""
    from ctr_reach_amd import _abi_ddpg
    n = _abi_ddpg.CtrDdpgNet()
    for i, name in enumerate(FIELDS):
        value = over.get(name, _ptrs((i + 1) << 24))
        if value is not None:
            setattr(n, name, value)
    n.pow = over.get("pow", 15 << 24)
    return n


def _adam(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
    from ctr_reach_amd import _abi_ddpg
    return _abi_ddpg.CtrDdpgAdam(lr, beta1, beta2, eps)


WS, WS_BYTES = 32 << 24, 1 << 26
ROWS, ACTIONS, TARGET = 40 << 24, 41 << 24, 42 << 24
NOARG = object()


WRITES_IN_PLACE = " requires grad: the learner writes it in place, outside autograd"


def exact(text):
    """pytest.raises(match=...): the whole message and nothing else."""
    return "^" + re.escape(text) + "$"


def _critic_step(critic=NOARG, net=NOARG, adam=NOARG, rows=ROWS, actions=ACTIONS, scale=None, target=TARGET, B=64,
                 ws=WS, ws_bytes=WS_BYTES):
    _abi, lib = _lib()
    critic = _critic() if critic is NOARG else critic
    net = _net() if net is NOARG else net
    adam = _adam() if adam is NOARG else adam
    rc = lib.ctr_ddpg_critic_step(critic, net, adam, rows, actions, scale, target, B, None, ws, ws_bytes, None)
    return rc, lib.ctr_last_error()


def _actor_step(actor=NOARG, net=NOARG, adam=NOARG, critic=NOARG, cW=NOARG, cb=NOARG, rows=ROWS, B=64, ws=WS,
                ws_bytes=WS_BYTES):
    _abi, lib = _lib()
    actor = _actor() if actor is NOARG else actor
    net = _net() if net is NOARG else net
    adam = _adam() if adam is NOARG else adam
    critic = _critic() if critic is NOARG else critic
    cW = _ptrs(20 << 24) if cW is NOARG else cW
    cb = _ptrs(21 << 24) if cb is NOARG else cb
    rc = lib.ctr_ddpg_actor_step(actor, net, adam, critic, cW, cb, rows, B, None, ws, ws_bytes, None)
    return rc, lib.ctr_last_error()


def _both_refuse(word, **kw):
    """A refusal of an argument the two calls share."""
    for call, name in ((_critic_step, b"ctr_ddpg_critic_step"), (_actor_step, b"ctr_ddpg_actor_step")):
        rc, msg = call(**kw)
        assert rc == -1 and msg == name + b": " + word, (word, kw, rc, msg)


def test_declared_listed_and_exported():
    _abi, lib = _lib()
    header = open(os.path.join(ROOT, "include", "ctr_reach_amd.h")).read()
    assert re.search(r"^int64_t ctr_ddpg_workspace_bytes\(const ctr_actor_t \*actor, const ctr_critic_t \*critic, "
                     r"int64_t max_B\);", header, re.M)
    assert re.search(r"^int ctr_ddpg_critic_step\(const ctr_critic_t \*critic, const ctr_ddpg_net_t \*net,", header, re.M)
    assert re.search(r"^int ctr_ddpg_actor_step\(const ctr_actor_t \*actor, const ctr_ddpg_net_t \*net,", header, re.M)
    for fn in FNS:
        assert fn in _abi.EXPORTED and hasattr(lib, fn)
    assert lib.ctr_abi_version() == _abi.CTR_ABI_VERSION == 17
    import ctr_reach_amd
    from ctr_reach_amd.learner import DdpgLearner
    assert ctr_reach_amd.DdpgLearner is DdpgLearner


def test_struct_layouts_match_header(tmp_path):
    from ctr_reach_amd import _abi_ddpg
    lines, want = [], []
    for ctype, cls in (("ctr_ddpg_net_t", _abi_ddpg.CtrDdpgNet), ("ctr_ddpg_adam_t", _abi_ddpg.CtrDdpgAdam)):
        lines.append('  printf("%%zu\\n", sizeof(%s));' % ctype)
        want.append(ctypes.sizeof(cls))
        for fname, _ in cls._fields_:
            lines.append('  printf("%%zu\\n", offsetof(%s, %s));' % (ctype, fname))
            want.append(getattr(cls, fname).offset)
    lines.append('  printf("%d\\n", CTR_ABI_VERSION);')
    want.append(17)
    prog = tmp_path / "ddpg_layout.c"
    prog.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"ctr_reach_amd.h\"\nint main(void) {\n"
                    + "\n".join(lines) + "\n  return 0; }\n")
    exe = tmp_path / "ddpg_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(prog), "-o", str(exe)])
    assert list(map(int, subprocess.check_output([str(exe)]).split())) == want
    assert [f for f, _ in _abi_ddpg.CtrDdpgNet._fields_] == list(FIELDS) + ["pow"]
    assert [f for f, _ in _abi_ddpg.CtrDdpgAdam._fields_] == ["lr", "beta1", "beta2", "eps"]


def test_a_good_call_gets_to_b_zero():
    """Every check passes on the fake pointers and B = 0 returns before any launch."""
    assert _critic_step(B=0)[0] == 0
    assert _actor_step(B=0)[0] == 0
    assert _critic_step(B=0, rows=None, actions=None, target=None)[0] == 0


def test_null_structs():
    _both_refuse(b"critic is NULL", critic=None)
    _both_refuse(b"net is NULL", net=None)
    _both_refuse(b"adam is NULL", adam=None)
    rc, msg = _actor_step(actor=None)
    assert rc == -1 and b"ctr_ddpg_actor_step" in msg and b"actor is NULL" in msg


def test_shapes():
    _both_refuse(b"critic: in_dim must be obs_dim + 12 = 25 or 26", critic=_critic(in_dim=24))
    _both_refuse(b"critic: n_hidden must be in 1..CTR_ACTOR_MAX_HIDDEN (3)", critic=_critic(()))
    _both_refuse(b"critic: every hidden width must be a multiple of 32 in 32..CTR_ACTOR_MAX_WIDTH (256)", critic=_critic((64, 48)))
    _both_refuse(b"critic: the packed network (163840 B of weights + 2176 B of biases) exceeds CTR_ACTOR_MAX_BYTES = 98304 B of LDS",
                 critic=_critic((256, 256)))
    for actor, word in ((_actor(in_dim=21), b"in_dim"), (_actor(()), b"n_hidden"), (_actor((64, 300)), b"width"),
                        (_actor(in_dim=20), b"actor->in_dim + 6")):
        rc, msg = _actor_step(actor=actor)
        assert rc == -1 and b"ctr_ddpg_actor_step" in msg and word in msg, msg
    rc, msg = _actor_step(actor=_actor(in_dim=20), critic=_critic(in_dim=26), B=0)
    assert rc == 0, msg
    # every hidden-layer count, the two nets with different ones
    assert _actor_step(actor=_actor((32,)), critic=_critic((128, 128, 128)), B=0)[0] == 0


def test_pointer_arrays_and_layers():
    for name in FIELDS:
        _both_refuse(b"NULL pointer array or pow in net", net=_net(**{name: None}))
        _both_refuse(b"NULL layer among W, b, gW, gb, mW, mb, vW, vb [0..n_hidden]",
                     net=_net(**{name: _ptrs(50 << 24, holes=(2,))}))
        # two hidden layers: layer 3 is not read
        assert _critic_step(net=_net(**{name: _ptrs(50 << 24, holes=(3,))}), B=0)[0] == 0
    _both_refuse(b"NULL pointer array or pow in net", net=_net(pow=None))
    for kw in ({"cW": None}, {"cb": None}):
        rc, msg = _actor_step(**kw)
        assert rc == -1 and b"ctr_ddpg_actor_step" in msg and b"is NULL" in msg, msg
    for kw in ({"cW": _ptrs(20 << 24, holes=(1,))}, {"cb": _ptrs(21 << 24, holes=(2,))}):
        rc, msg = _actor_step(**kw)
        assert rc == -1 and b"ctr_ddpg_actor_step" in msg and b"NULL layer" in msg, msg


def test_aliases():
    for name in FIELDS[2:]:
        for param in ("W", "b"):
            same = _ptrs(60 << 24)
            _both_refuse(b"a gradient or state tensor is a parameter tensor", net=_net(**{name: same, param: same}))
    mixed = _ptrs(3 << 24)                                                 # gW's own pointers ...
    mixed[1] = (2 << 24) + 4096 * 2                                        # ... but layer 1's is b[2]
    _both_refuse(b"a gradient or state tensor is a parameter tensor", net=_net(gW=mixed))
    _both_refuse(b"a gradient or state tensor is a parameter tensor", net=_net(pow=(1 << 24) + 4096))  # pow is W[1]


def test_workspace():
    _both_refuse(b"workspace is NULL", ws=None)
    _both_refuse(b"workspace must be 16-B aligned", ws=WS + 8)
    _abi, lib = _lib()
    a, c = _actor(), _critic()
    need = lib.ctr_ddpg_workspace_bytes(a, c, 64)
    assert need > 0
    _both_refuse(b"workspace too small (ctr_ddpg_workspace_bytes)", ws_bytes=1024)
    rc, msg = _critic_step(ws_bytes=need - 1)                              # (the critic is the larger network here)
    assert rc == -1 and msg == b"ctr_ddpg_critic_step: workspace too small (ctr_ddpg_workspace_bytes)"
    assert _critic_step(ws_bytes=need, B=0)[0] == 0 and _actor_step(ws_bytes=need, B=0)[0] == 0
    rc, msg = _critic_step(ws_bytes=need, B=65)                            # one more tile than it was sized for
    assert rc == -1 and msg == b"ctr_ddpg_critic_step: workspace too small (ctr_ddpg_workspace_bytes)"


def test_workspace_bytes():
    _abi, lib = _lib()
    for a, c in ((_actor(), _critic()), (_actor((32,)), _critic((128, 128, 128))), (_actor((32, 256, 32), 20),
                                                                                    _critic((32,), 26))):
        sizes = [lib.ctr_ddpg_workspace_bytes(a, c, B) for B in (1, 16, 17, 70, 256, 1023, 1024, 1025, 4096, 65536)]
        assert all(s > 0 and s % 16 == 0 for s in sizes), sizes
        assert sizes == sorted(sizes) and sizes[0] == sizes[1] < sizes[2] < sizes[3]
        assert sizes[5] == sizes[6] == sizes[7] == sizes[-1]               # 64 slots of 16 rows: the bound
        for B in (0, -1, 65537):
            assert lib.ctr_ddpg_workspace_bytes(a, c, B) == -1
            assert b"ctr_ddpg_workspace_bytes" in lib.ctr_last_error() and b"max_B" in lib.ctr_last_error()
    assert lib.ctr_ddpg_workspace_bytes(None, _critic(), 64) == -1 and b"actor is NULL" in lib.ctr_last_error()
    assert lib.ctr_ddpg_workspace_bytes(_actor(), None, 64) == -1 and b"critic is NULL" in lib.ctr_last_error()
    assert lib.ctr_ddpg_workspace_bytes(_actor(in_dim=20), _critic(), 64) == -1
    assert b"ctr_ddpg_workspace_bytes" in lib.ctr_last_error()


def test_adam_constants_and_b():
    nan, inf = float("nan"), float("inf")
    for kw in ({"lr": nan}, {"lr": inf}, {"beta1": nan}, {"beta2": -inf}, {"eps": inf}, {"eps": nan}):
        _both_refuse(b"lr, beta1, beta2 and eps must be finite", adam=_adam(**kw))
    for kw in ({"beta1": -0.1}, {"beta1": 1.0}, {"beta2": 1.0}, {"beta2": 1.5}, {"beta2": -1e-3}):
        _both_refuse(b"beta1 and beta2 must be in [0, 1)", adam=_adam(**kw))
    for eps in (0.0, -1e-8):
        _both_refuse(b"eps must be positive", adam=_adam(eps=eps))
    assert _critic_step(adam=_adam(beta1=0.0, beta2=0.0, lr=0.0), B=0)[0] == 0
    for B in (-1, 65537, 1 << 40):
        _both_refuse(b"B must be in 0..65536", B=B)
    for kw in ({"rows": None}, {"actions": None}, {"target": None}):
        rc, msg = _critic_step(**kw)
        assert rc == -1 and msg == b"ctr_ddpg_critic_step: rows, actions or target is NULL", msg
    rc, msg = _actor_step(rows=None)
    assert rc == -1 and b"ctr_ddpg_actor_step" in msg and b"rows is NULL" in msg, msg


# ------------------------------------------------------------------------------------------
# DdpgLearner: every ValueError comes before the library or a GPU is touched.

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
    from ctr_reach_amd.learner import DdpgLearner
    policy, critic = _mlp(19, (64, 96), 6, True), _mlp(25, (32,), 1, False)
    with pytest.raises(ValueError, match=exact("policy layer 0: W" + WRITES_IN_PLACE)):
        DdpgLearner(_mlp(19, (64,), 6, True, grad=True), critic)
    with pytest.raises(ValueError, match=exact("critic layer 0: W" + WRITES_IN_PLACE)):
        DdpgLearner(policy, _mlp(25, (32,), 1, False, grad=True))
    half = _mlp(25, (32,), 1, False)
    half[2].bias.requires_grad_(True)
    with pytest.raises(ValueError, match=exact("critic layer 1: b" + WRITES_IN_PLACE)):
        DdpgLearner(policy, half)
    with pytest.raises(ValueError, match=exact("the actor ends with nn.Tanh")):
        DdpgLearner(_mlp(19, (64,), 6, False), critic)
    with pytest.raises(ValueError, match=exact("the critic ends with its output nn.Linear (no activation after it)")):
        DdpgLearner(policy, _mlp(25, (32,), 1, True))
    with pytest.raises(ValueError, match=exact("the policy's rows are obs_dim + 6 = 19 or 20 floats")):
        DdpgLearner(_mlp(18, (64,), 6, True), critic)
    with pytest.raises(ValueError, match=exact("the critic's rows are obs_dim + 12 = 25 or 26 floats")):
        DdpgLearner(policy, _mlp(19, (64,), 1, False))
    with pytest.raises(ValueError, match=exact("the critic takes [row, action]: 19 + 6 inputs, not 26")):
        DdpgLearner(policy, _mlp(26, (32,), 1, False))
    with pytest.raises(ValueError, match=exact("policy: hidden widths must be multiples of 32 in 32..256")):
        DdpgLearner(_mlp(19, (48,), 6, True), critic)
    with pytest.raises(ValueError, match=exact("the policy has 1..3 hidden layers and an output layer")):
        DdpgLearner(_mlp(19, (32, 32, 32, 32), 6, True), critic)
    with pytest.raises(ValueError, match=exact("policy layer 1: W must be [6, 64], not [5, 64]")):
        DdpgLearner(_mlp(19, (64,), 5, True), critic)
    with pytest.raises(ValueError, match=exact("critic layer 1: b must be float32, not torch.float64")):
        layers = [(m.weight, m.bias) for m in critic if hasattr(m, "weight")]
        DdpgLearner(policy, [layers[0], (layers[1][0], layers[1][1].double())])
    with pytest.raises(ValueError, match=exact("policy layer 0: W must be contiguous")):
        DdpgLearner([(torch.zeros((19, 32)).t(), torch.zeros(32)), (torch.zeros((6, 32)), torch.zeros(6))], critic)
    with pytest.raises(ValueError, match=exact("policy layer 0: W must be a torch tensor")):
        DdpgLearner([(np.zeros((32, 19), np.float32), torch.zeros(32)), (torch.zeros((6, 32)), torch.zeros(6))], critic)
    for kw, word in (({"betas": (1.0, 0.999)}, "betas must be in [0, 1)"), ({"betas": (0.9, -0.1)}, "betas must be in [0, 1)"),
                     ({"eps": 0.0}, "eps must be positive"), ({"eps": float("nan")}, "eps must be finite"),
                     ({"actor_lr": float("inf")}, "actor_lr must be finite"),
                     ({"critic_lr": float("nan")}, "critic_lr must be finite"),
                     ({"max_batch": 0}, "max_batch must be in 1..65536"), ({"max_batch": 65537}, "max_batch must be in 1..65536"),
                     ({"scale": [1.0] * 5}, "scale is six finite, non-zero floats"),
                     ({"scale": [1.0, 1.0, 0.0, 1.0, 1.0, 1.0]}, "scale is six finite, non-zero floats")):
        with pytest.raises(ValueError, match=exact(word)):
            DdpgLearner(policy, critic, **kw)
    with pytest.raises(ValueError, match=exact("the networks are on cpu: the learner's networks are on a GPU")):   # (all else in order)
        DdpgLearner(policy, critic, scale=[0.001] * 3 + [0.087] * 3)


# ------------------------------------------------------------------------------------------
# The restatement against torch.optim.Adam

def test_adam_reference_against_torch_adam(capsys):
    """torch's Adam (CPU, foreach=False) keeps beta^t, 1 - beta^t, lr / (1 - beta1^t) and sqrt(1 -
    beta2^t) in double precision and states the moments as lerp_ and mul_().addcmul_(); the
    restatement keeps everything in float32.  With u = 2^-24, to first order, per step t:
      * m': either side makes at most 4 roundings of terms no larger than M = |m| + |g|, the float32
        beta1 is off by u (u |m|) and 1 - beta1 by u beta1 / (1 - beta1) of (1 - beta1) |g| (u |g|):
        e_m' <= e_m + 10 u M;
      * v' (a sum of positive terms): 5 roundings either side, and as above u v + u g^2 for the float32
        beta2 and 1 - beta2: e_v' <= e_v + u (10 v' + v + g^2);
      * c_i = 1 - beta_i^t: the float32 power carries t conversions of beta_i and t - 1 products, the
        subtraction one more: relative r_i = 2 t u beta_i^t / c_i + u;
      * D = lr (m'/c_1) / (sqrt(v'/c_2) + eps): e_m' / (c_1 (sqrt(v'/c_2) + eps)) lr from m', and
        relative r_1 + (e_v'/v' + r_2) / 2 + 16 u from the rest (8 roundings and scalar conversions
        either side);
      * p' = p - D: one rounding either side, u (|p'| + |D|) each.
    Derived, not measured; the measured maximum of |difference| / bound is printed."""
    import torch
    from ctr_reach_amd.learner import adam_reference
    u = 2.0 ** -24
    worst = 0.0
    for betas, lr in (((0.9, 0.999), 1e-3), ((0.5, 0.75), 1e-4)):
        rng = np.random.default_rng(900)
        p = rng.uniform(-1, 1, (37, 19)).astype(np.float32)
        tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
        opt = torch.optim.Adam([tp], lr=lr, betas=betas, eps=1e-8, foreach=False)
        m, v, pw = np.zeros_like(p), np.zeros_like(p), np.ones(2, np.float32)
        e_m, e_v, e_p = np.zeros(p.shape), np.zeros(p.shape), np.zeros(p.shape)
        for t in range(1, 4):
            g = rng.uniform(-1, 1, p.shape).astype(np.float32)
            m0, v0 = m.astype(np.float64), v.astype(np.float64)
            p, m, v, pw = adam_reference(p, g, m, v, pw, lr, betas, 1e-8)
            tp.grad = torch.from_numpy(g.copy())
            opt.step()
            g64, m64, v64, p64 = (a.astype(np.float64) for a in (g, m, v, p))
            e_m = e_m + 10 * u * (np.abs(m0) + np.abs(g64))
            e_v = e_v + u * (10 * v64 + v0 + g64 * g64)
            c = [1.0 - b ** t for b in betas]
            r = [2 * t * u * b ** t / ci + u for b, ci in zip(betas, c)]
            den = np.sqrt(v64 / c[1]) + 1e-8
            D = np.abs(lr * (m64 / c[0]) / den)
            e_D = lr * e_m / (c[0] * den) + D * (r[0] + 0.5 * (e_v / v64 + r[1]) + 16 * u)
            e_p = e_p + e_D + 2 * u * (np.abs(p64) + D)
            diff = np.abs(p64 - tp.detach().numpy().astype(np.float64))
            assert (v64 > 0).all() and (diff <= e_p).all(), (betas, t, float((diff / e_p).max()))
            worst = max(worst, float((diff / e_p).max()))
            st = opt.state[tp]
            assert (np.abs(st["exp_avg"].numpy() - m64) <= e_m).all() and (np.abs(st["exp_avg_sq"].numpy() - v64) <= e_v).all()
        assert pw.dtype == np.float32 and abs(float(pw[0]) - betas[0] ** 3) < 8 * u
    with capsys.disabled():
        print("\nadam_reference against torch.optim.Adam over 3 steps: largest difference / bound %.3g" % worst)


def test_adam_reference_is_float32_throughout():
    from ctr_reach_amd.learner import adam_reference
    f = np.float32
    p, g, m, v = f(0.3), f(-0.7), f(0.01), f(0.002)
    p1, m1, v1, pw = adam_reference(np.array([p]), np.array([g]), np.array([m]), np.array([v]), [f(0.9), f(0.999)], 1e-3)
    b1, b2 = f(0.9), f(0.999)
    want_m = f(f(b1 * m) + f(f(f(1) - b1) * g))
    want_v = f(f(b2 * v) + f(f(f(f(1) - b2) * g) * g))
    pw1, pw2 = f(f(0.9) * b1), f(f(0.999) * b2)
    want_p = f(p - f(f(1e-3) * f(f(want_m / f(f(1) - pw1)) / f(f(np.sqrt(f(want_v / f(f(1) - pw2)))) + f(1e-8)))))
    assert m1[0] == want_m and v1[0] == want_v and p1[0] == want_p and pw[0] == pw1 and pw[1] == pw2
