"""SAC on the host (no GPU): the six new entry points are declared, listed and exported; the ctypes
mirror of ctr_sac_alpha_t matches the header; every refusal the header lists returns CTR_EINVAL (-1)
with a ctr_last_error that names the function, before any HIP call (the device pointers are fake and
never dereferenced); ctr_gauss_pack against a numpy restatement of the layout, and against
ctr_actor_pack of the first six rows; GaussianActor.emulate's formulas; sac_ref's loss gradient
against central finite differences; SacLearner's constructor errors."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ddpg_ref as R
import sac_ref as S
import test_host_td3 as H
from test_host_ddpg import WRITES_IN_PLACE, exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FNS = ("ctr_gauss_blob_bytes", "ctr_gauss_pack", "ctr_gauss_load", "ctr_gauss_act", "ctr_sac_workspace_bytes",
       "ctr_sac_actor_step")
_actor, _critic, _net, _adam, _ptrs, NOARG = H._actor, H._critic, H._net, H._adam, H._ptrs, H.NOARG


def _lib():
    from ctr_reach_amd import _abi
    return _abi, _abi.load()


def test_declared_listed_and_exported():
    _abi, lib = _lib()
    header = open(os.path.join(ROOT, "include", "ctr_reach_amd.h")).read()
    assert re.search(r"^int ctr_gauss_act\(const ctr_actor_t \*actor, const float \*rows, int64_t n, uint64_t seed, "
                     r"uint64_t counter,\n +int64_t row_base, int32_t deterministic, float \*actions, float \*unit, "
                     r"float \*logp,\n +float \*logits, void \*stream\);", header, re.M)
    assert re.search(r"^int ctr_sac_actor_step\(const ctr_actor_t \*actor, const ctr_ddpg_net_t \*net, "
                     r"const ctr_ddpg_adam_t \*adam,\n +const ctr_critic_t \*const critic\[2\]", header, re.M)
    for fn in FNS:
        assert fn in _abi.EXPORTED and hasattr(lib, fn), fn
    assert lib.ctr_abi_version() == _abi.CTR_ABI_VERSION == 17
    import ctr_reach_amd
    from ctr_reach_amd.learner import SacLearner
    from ctr_reach_amd.policy import GaussianActor
    assert ctr_reach_amd.SacLearner is SacLearner and ctr_reach_amd.GaussianActor is GaussianActor


def test_struct_layout_matches_header(tmp_path):
    from ctr_reach_amd import _abi_sac
    cls = _abi_sac.CtrSacAlpha
    lines = ['  printf("%zu\\n", sizeof(ctr_sac_alpha_t));']
    want = [ctypes.sizeof(cls)]
    for fname, _ in cls._fields_:
        lines.append('  printf("%%zu\\n", offsetof(ctr_sac_alpha_t, %s));' % fname)
        want.append(getattr(cls, fname).offset)
    lines.append('  printf("%d\\n", CTR_ABI_VERSION);')
    want.append(17)
    prog = tmp_path / "sac_layout.c"
    prog.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"ctr_reach_amd.h\"\nint main(void) {\n"
                    + "\n".join(lines) + "\n  return 0; }\n")
    exe = tmp_path / "sac_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(prog), "-o", str(exe)])
    assert list(map(int, subprocess.check_output([str(exe)]).split())) == want
    assert [f for f, _ in cls._fields_] == ["state", "grad", "lr", "learn"]
    assert ctypes.sizeof(_abi_sac.LayersPair) == 2 * ctypes.sizeof(ctypes.c_void_p)


# ------------------------------------------------------------------------------------------
# the Gaussian policy's entry points

def _act(actor=NOARG, rows=1 << 22, n=8, row_base=0, det=0):
    _abi, lib = _lib()
    actor = _actor() if actor is NOARG else actor
    rc = lib.ctr_gauss_act(actor, rows, n, 1, 2, row_base, det, 1 << 23, None, None, None, None)
    return rc, lib.ctr_last_error()


def test_gauss_entry_points_refuse():
    _abi, lib = _lib()

    def refused(word, **kw):
        rc, msg = _act(**kw)
        assert rc == -1 and b"ctr_gauss_act" in msg and word in msg, (word, kw, rc, msg)

    refused(b"actor is NULL", actor=None)
    refused(b"n_hidden", actor=_actor(()))
    refused(b"width", actor=_actor((64, 48)))
    refused(b"in_dim", actor=_actor(in_dim=25))
    refused(b"CTR_ACTOR_MAX_BYTES", actor=_actor((256, 256, 256)))
    a = _actor()
    a.scale[3] = float("inf")
    refused(b"scale", actor=a)
    refused(b"blob is NULL", actor=_actor(blob=None))
    refused(b"16-B aligned", actor=_actor(blob=(1 << 21) + 8))
    refused(b"n out of range", n=-1)
    refused(b"n out of range", n=1 << 31)
    refused(b"row_base", row_base=-1)
    refused(b"row_base", row_base=(1 << 32) - 7)
    refused(b"rows is NULL", rows=None)
    assert _act(n=0)[0] == 0 and _act(n=0, rows=None)[0] == 0 and _act(n=0, row_base=1 << 32)[0] == 0
    assert _act(n=0, actor=_actor((128, 128, 128), 20), det=1)[0] == 0
    # the blob's size, the packer and the loader: the actor's checks
    assert lib.ctr_gauss_blob_bytes(None) == -1 and lib.ctr_gauss_blob_bytes(_actor((64, 48))) == -1
    for hidden in ((32,), (64, 64), (128, 128, 128), (256, 128)):
        for in_dim in (19, 20):
            assert lib.ctr_gauss_blob_bytes(_actor(hidden, in_dim)) == lib.ctr_actor_blob_bytes(_actor(hidden, in_dim)) > 0
    buf = np.zeros(1 << 16, dtype=np.uint8)
    W, b = _ptrs(1 << 24), _ptrs(2 << 24)
    assert lib.ctr_gauss_pack(None, W, b, buf.ctypes.data) == -1
    assert lib.ctr_gauss_pack(_actor(), None, b, buf.ctypes.data) == -1 and b"ctr_gauss_pack" in lib.ctr_last_error()
    assert lib.ctr_gauss_pack(_actor(), W, b, None) == -1
    assert lib.ctr_gauss_pack(_actor(), _ptrs(1 << 24, holes=(2,)), b, buf.ctypes.data) == -1
    assert b"NULL layer" in lib.ctr_last_error()
    assert lib.ctr_gauss_load(None, W, b, None) == -1
    assert lib.ctr_gauss_load(_actor(), None, b, None) == -1 and b"ctr_gauss_load" in lib.ctr_last_error()
    assert lib.ctr_gauss_load(_actor(), W, _ptrs(2 << 24, holes=(0,)), None) == -1
    assert lib.ctr_gauss_load(_actor(blob=None), W, b, None) == -1 and b"blob" in lib.ctr_last_error()


def _numpy_pack(weights, biases, in_dim):
    """The blob's layout restated (csrc/ctr_actor.inc's header comment): per layer, per 32-row tile,
    per k-step of 16, per lane, 8 bf16; then every layer's f32 biases padded to whole 32-row tiles."""
    from ctr_reach_amd.policy import bf16_round
    frags, bias = [], []
    for l, (W, b) in enumerate(zip(weights, biases)):
        rows, cols = W.shape
        tiles = (rows + 31) // 32
        ksteps = 2 if l == 0 else cols // 16
        Wp = np.zeros((32 * tiles, 16 * ksteps), dtype=np.float32)
        Wp[:rows, :cols] = W
        bits = (bf16_round(Wp).view(np.uint32) >> np.uint32(16)).astype(np.uint16)
        out = np.zeros((tiles, ksteps, 64, 8), dtype=np.uint16)
        for lane in range(64):
            h, r = lane >> 5, lane & 31
            for j in range(8):
                for S_ in range(ksteps):
                    k = 16 * S_ + 8 * h + j if l == 0 else 32 * (S_ >> 1) + 16 * (S_ & 1) + 8 * (j >> 2) + 4 * h + (j & 3)
                    out[:, S_, lane, j] = bits[r::32, k]
        frags.append(out.reshape(-1).view(np.uint8))
        bp = np.zeros(32 * tiles, dtype=np.float32)
        bp[:rows] = b
        bias.append(bp.view(np.uint8))
    return np.concatenate(frags + bias)


@pytest.mark.parametrize("hidden,in_dim", [((32,), 19), ((64, 96), 20), ((128, 128, 128), 19)])
def test_gauss_pack_layout_and_the_sliced_actor(hidden, in_dim):
    from ctr_reach_amd.policy import GaussianActor, MlpActor
    rng = np.random.default_rng(len(hidden))
    dims = [in_dim] + list(hidden) + [12]
    layers = [(rng.standard_normal((o, i)).astype(np.float32), rng.standard_normal(o).astype(np.float32))
              for i, o in zip(dims[:-1], dims[1:])]
    scale = np.full(6, 0.5, dtype=np.float32)
    pi = GaussianActor(layers, scale)
    blob = pi._pack_host()
    want = _numpy_pack([W for W, _ in layers], [b for _, b in layers], in_dim)
    assert blob.shape == want.shape and np.array_equal(blob, want)
    # rows 6..11 of the output layer are there, and elsewhere the blob is the 6-row actor's
    sliced = MlpActor(layers[:-1] + [(layers[-1][0][:6], layers[-1][1][:6])], scale)._pack_host()
    assert sliced.shape == blob.shape
    # the bytes that hold rows 6..11: where a pack of zeros with every byte of those rows non-zero is non-zero
    every_byte = np.array([0x3F818181], dtype=np.uint32).view(np.float32)[0]      # bf16 0x3F82, f32 3F 81 81 81
    marked = [(np.zeros_like(W), np.zeros_like(b)) for W, b in layers]
    marked[-1][0][6:] = every_byte
    marked[-1][1][6:] = every_byte
    mask = GaussianActor(marked, scale)._pack_host() != 0
    assert mask.sum() == 6 * hidden[-1] * 2 + 6 * 4
    assert (blob != sliced).any() and not (blob != sliced)[~mask].any()
    assert not sliced[mask].any()


# ------------------------------------------------------------------------------------------
# GaussianActor.emulate

def _policy(rng, hidden=(32,), in_dim=19, seed=0):
    from ctr_reach_amd.policy import GaussianActor
    dims = [in_dim] + list(hidden) + [12]
    layers = [((rng.uniform(-1, 1, (o, i)) / np.sqrt(i)).astype(np.float32), rng.uniform(-.1, .1, o).astype(np.float32))
              for i, o in zip(dims[:-1], dims[1:])]
    return GaussianActor(layers, np.array([0.001, 0.002, 0.003, 0.087, 0.05, 3.0], dtype=np.float32), seed=seed)


def test_emulate_deterministic_is_the_mean():
    rng = np.random.default_rng(0)
    pi = _policy(rng)
    rows = rng.uniform(-1, 1, (40, 19)).astype(np.float32)
    out = pi.emulate(rows, counter=3, deterministic=True)
    y = out["logits"]
    assert y.shape == (40, 12)
    assert np.array_equal(out["unit"], np.tanh(y[:, :6]))
    assert np.array_equal(out["action"], pi.scale.astype(np.float64) * np.tanh(y[:, :6]))
    s = np.clip(y[:, 6:], -20, 2)
    want = (-s - 0.5 * np.log(2 * np.pi)).sum(axis=1) - np.log1p(-np.tanh(y[:, :6]) ** 2).sum(axis=1)
    assert np.abs(out["logp"] - want).max() < 1e-12
    # and another counter changes nothing here, while it changes every sampled row
    assert np.array_equal(pi.emulate(rows, counter=4, deterministic=True)["logp"], out["logp"])
    a, b = pi.emulate(rows, counter=3)["unit"], pi.emulate(rows, counter=4)["unit"]
    assert (a != b).any(axis=1).all()
    # a row's noise is keyed by row_base + its index
    assert np.array_equal(pi.emulate(rows[10:], counter=3, row_base=10)["unit"], a[10:])


def test_emulate_logp_agrees_with_torch_distributions():
    import torch
    from ctr_reach_amd.policy import gauss_head
    rng = np.random.default_rng(1)
    y = np.concatenate((rng.uniform(-1, 1, (200, 6)), rng.uniform(-3, -0.5, (200, 6))), axis=1)
    eps = rng.standard_normal((200, 6))
    out = gauss_head(y, eps, np.ones(6))
    mu, std = torch.from_numpy(y[:, :6]), torch.from_numpy(np.exp(y[:, 6:]))
    u = mu + std * torch.from_numpy(eps)
    base = torch.distributions.Normal(mu, std)
    want = (base.log_prob(u) - torch.log1p(-torch.tanh(u) ** 2)).sum(dim=1).numpy()
    assert 1 < np.abs(out["u"]).max() < 4              # moderate: torch's log1p(-tanh^2) is the one that loses digits beyond
    assert np.abs(out["logp"] - want).max() < 1e-12 * max(1.0, np.abs(want).max())
    assert np.array_equal(out["unit"], np.tanh(out["u"]))


def test_emulate_logp_is_finite_where_tanh_saturates():
    from ctr_reach_amd.policy import gauss_head
    y = np.zeros((2, 12))
    y[0, :6], y[1, :6] = 50.0, -50.0
    for dtype in (np.float64, np.float32):
        out = gauss_head(y, np.zeros((2, 6)), np.ones(6), dtype)
        assert np.isfinite(out["logp"]).all() and (np.abs(out["unit"]) == 1).all()
        # log(1 - tanh^2 u) -> 2 (log 2 - |u|): logp = -6 * 0.5 log(2 pi) - 12 (log 2 - 50)
        want = -3 * np.log(2 * np.pi) - 12 * (np.log(2) - 50)
        assert np.abs(out["logp"] - want).max() < (1e-9 if dtype == np.float64 else 1e-3)
    clipped = gauss_head(np.concatenate((np.zeros((1, 6)), [[5, 5, -25, -25, 1, -19]]), axis=1), np.ones((1, 6)), np.ones(6))
    assert np.array_equal(clipped["s"], [[2, 2, -20, -20, 1, -19]])


def test_gaussian_actor_constructor_and_mean_layers():
    from ctr_reach_amd.policy import GaussianActor, polyak_
    rng = np.random.default_rng(2)
    pi = _policy(rng, (64, 32), 20)
    assert pi.in_dim == 20 and pi.hidden == [64, 32] and pi.OUT == 12
    six = [(rng.standard_normal((32, 19)).astype(np.float32), np.zeros(32, np.float32)),
           (rng.standard_normal((6, 32)).astype(np.float32), np.zeros(6, np.float32))]
    with pytest.raises(ValueError, match="12 rows"):
        GaussianActor(six, np.ones(6))
    with pytest.raises(ValueError, match="scale"):
        GaussianActor(list(zip(pi.weights, pi.biases)), np.ones(5))
    with pytest.raises(RuntimeError, match="on the host"):
        pi.mean_actor()
    with pytest.raises(ValueError, match="MlpActor or an MlpCritic"):
        polyak_([(pi, [], [])], 0.5)
    import torch
    seq = R.mlp(19, (32,), 12, False)
    assert GaussianActor.from_torch(seq, np.ones(6)).hidden == [32]
    with pytest.raises(ValueError):
        GaussianActor.from_torch(R.mlp(19, (32,), 12, True), np.ones(6))
    cut = pi.mean_layers(seq)
    assert tuple(cut[-1][0].shape) == (6, 32) and cut[-1][0].is_contiguous() and cut[-1][1].is_contiguous()
    assert cut[-1][0].data_ptr() == seq[-1].weight.data_ptr() and isinstance(cut[0][0], torch.Tensor)


# ------------------------------------------------------------------------------------------
# sac_ref

def test_reference_gradient_against_central_differences():
    import torch
    policy, c1, c2, rows = S.make(0, (32,), (32,), (32,), 19, 5)
    eps = S.eps_for(5)
    ref = S.autograd(policy, c1, c2, rows, eps, S.ALPHA, torch.float64)
    assert S.clear(ref)
    pol64 = policy.double()
    rng = np.random.default_rng(0)
    h = 1e-6
    for l, (W, b) in enumerate(R.params(pol64)):
        for which, t in enumerate((W, b)):
            flat = t.view(-1)
            for idx in rng.choice(flat.numel(), size=min(6, flat.numel()), replace=False):
                old = float(flat[idx])
                vals = []
                for d in (h, -h):
                    with torch.no_grad():
                        flat[idx] = old + d
                    vals.append(S.autograd(pol64, c1, c2, rows, eps, S.ALPHA, torch.float64)["loss"])
                with torch.no_grad():
                    flat[idx] = old
                fd = (vals[0] - vals[1]) / (2 * h)
                g = ref["grads"][l][which].reshape(-1)[idx]
                assert abs(fd - g) <= 1e-6 * max(1.0, abs(g)), (l, which, idx, fd, g)
    assert ref["alpha_grad"] == -(ref["logp_mean"] + S.TARGET_ENTROPY)


def test_reference_noise_is_the_policy_draw():
    from ctr_reach_amd.policy import GaussianActor, TargetSmoothing
    eps = S.eps_for(7, seed=5, counter=(3 << 32) | 9)
    pi = GaussianActor.__new__(GaussianActor)
    pi.seed = 5
    u = pi.uniforms((3 << 32) | 9, np.arange(7))
    assert u.dtype == np.float32 and ((u >= 0) & (u < 1)).all()
    # stream 8: not TD3's smoothing noise (stream 7) of the same key
    assert not np.array_equal(u, TargetSmoothing().uniforms(5, (3 << 32) | 9, np.arange(7)))
    r = np.sqrt(-2 * np.log(1 - u[:, 0::2].astype(np.float64)))
    ang = float(np.float32(6.2831855)) * u[:, 1::2].astype(np.float64)
    assert np.array_equal(eps[:, 0::2], r * np.cos(ang)) and np.array_equal(eps[:, 1::2], r * np.sin(ang))
    eps32 = S.eps_for(7, seed=5, counter=(3 << 32) | 9, dtype=np.float32)
    assert eps32.dtype == np.float32 and np.abs(eps32 - eps).max() < 1e-5


# ------------------------------------------------------------------------------------------
# ctr_sac_actor_step

WS, WS_BYTES, ROWS = H.WS, H.WS_BYTES, H.ROWS
LOG_ALPHA, STATE, GRAD, LOSS, LPM = 90 << 24, 91 << 24, 92 << 24, 93 << 24, 94 << 24


def _critic_layers(which, holes=()):
    return _ptrs((40 + 2 * which) << 24, holes), _ptrs((41 + 2 * which) << 24, holes)


def _sac(actor=NOARG, critics=NOARG, net=NOARG, adam=NOARG, cW=NOARG, cb=NOARG, rows=ROWS, B=64, log_alpha=LOG_ALPHA,
         alpha=NOARG, state=STATE, grad=GRAD, lr=3e-4, learn=1, target_entropy=-6.0, loss=LOSS, lpm=LPM, ws=WS,
         ws_bytes=WS_BYTES):
    from ctr_reach_amd import _abi_sac, _abi_td3
    _abi, lib = _lib()
    keep = []
    actor = _actor((32,)) if actor is NOARG else actor
    critics = (_critic(), _critic((32,))) if critics is NOARG else critics
    pair = None
    if critics is not None:
        pair = _abi_td3.CriticPair()
        for i, c in enumerate(critics):
            if c is not None:
                keep.append(c)
                pair[i] = ctypes.pointer(c)
    layer_pairs = []
    for given, idx in ((cW, 0), (cb, 1)):
        if given is NOARG:
            given = (_critic_layers(0)[idx], _critic_layers(1)[idx])
        arr = None
        if given is not None:
            arr = _abi_sac.LayersPair()
            for i, a in enumerate(given):
                if a is not None:
                    keep.append(a)
                    arr[i] = ctypes.cast(a, ctypes.POINTER(ctypes.c_void_p))
        layer_pairs.append(arr)
    net = _net(0) if net is NOARG else net
    adam = _adam() if adam is NOARG else adam
    if alpha is NOARG:
        alpha = _abi_sac.CtrSacAlpha(state, grad, lr, learn)
    rc = lib.ctr_sac_actor_step(actor, net, adam, pair, layer_pairs[0], layer_pairs[1], rows, B, 1, 2, log_alpha, alpha,
                                target_entropy, loss, lpm, ws, ws_bytes, None)
    return rc, lib.ctr_last_error()


def _sac_refused(word, **kw):
    rc, msg = _sac(**kw)
    assert rc == -1 and b"ctr_sac_actor_step" in msg and word in msg, (word, kw, rc, msg)


def test_a_good_sac_step_gets_to_b_zero():
    assert _sac(B=0)[0] == 0, _sac(B=0)
    assert _sac(B=0, rows=None, loss=None, lpm=None, grad=None, learn=0)[0] == 0
    assert _sac(B=0, actor=_actor((256, 128, 32)), critics=(_critic((256, 128, 32)), _critic((256, 128, 32))))[0] == 0
    assert _sac(B=0, actor=_actor((32,), 20), critics=(_critic((32,), 26), _critic((64, 96), 26)))[0] == 0


def test_sac_step_refuses_nulls_shapes_and_constants():
    _sac_refused(b"is NULL", critics=None)
    _sac_refused(b"is NULL", cW=None)
    _sac_refused(b"is NULL", cb=None)
    _sac_refused(b"actor is NULL", actor=None)
    _sac_refused(b"is NULL", critics=(_critic(), None))
    _sac_refused(b"is NULL", critics=(None, _critic()))
    _sac_refused(b"NULL entry", cW=(_critic_layers(0)[0], None))
    _sac_refused(b"NULL entry", cb=(None, _critic_layers(1)[1]))
    _sac_refused(b"NULL layer", cW=(_critic_layers(0, holes=(2,))[0], _critic_layers(1)[0]))    # critic 1 reads layers 0..2
    assert _sac(B=0, cW=(_critic_layers(0)[0], _critic_layers(1, holes=(2,))[0]))[0] == 0         # critic 2 layers 0..1
    _sac_refused(b"net is NULL", net=None)
    _sac_refused(b"adam is NULL", adam=None)
    for name in H.FIELDS:
        _sac_refused(b"NULL pointer array", net=_net(0, **{name: None}))
        _sac_refused(b"NULL layer", net=_net(0, **{name: _ptrs(50 << 24, holes=(1,))}))
    _sac_refused(b"pow", net=_net(0, pow=None))
    same = _ptrs(60 << 24)
    _sac_refused(b"is a parameter tensor", net=_net(0, gW=same, W=same))
    good = _critic()
    for bad, word in ((_critic(in_dim=24), b"in_dim"), (_critic(()), b"n_hidden"), (_critic((64, 48)), b"width"),
                      (_critic((256, 256)), b"CTR_ACTOR_MAX_BYTES"), (_critic(in_dim=26), b"in_dim + 6")):
        _sac_refused(word, critics=(bad, good))
        _sac_refused(word, critics=(good, bad))
    for bad, word in ((_actor(()), b"n_hidden"), (_actor((64, 48)), b"width"), (_actor((32,), 25), b"in_dim"),
                      (_actor((256, 256, 256)), b"CTR_ACTOR_MAX_BYTES"), (_actor((32,), 20), b"in_dim + 6")):
        _sac_refused(word, actor=bad)
    nan, inf = float("nan"), float("inf")
    for kw in ({"lr": nan}, {"beta1": inf}, {"eps": nan}):
        _sac_refused(b"must be finite", adam=_adam(**kw))
    _sac_refused(b"[0, 1)", adam=_adam(beta1=1.0))
    _sac_refused(b"eps must be positive", adam=_adam(eps=0.0))
    for bad in (nan, inf, -inf):
        _sac_refused(b"must be finite", target_entropy=bad)
        _sac_refused(b"must be finite", lr=bad)
    for B in (-1, 65537, 1 << 40):
        _sac_refused(b"B must be", B=B)
    _sac_refused(b"rows is NULL", rows=None)
    _sac_refused(b"log_alpha or alpha_state is NULL", log_alpha=None)
    _sac_refused(b"log_alpha or alpha_state is NULL", alpha=None)
    _sac_refused(b"state is NULL", state=None)


def test_sac_step_refuses_shared_tensors():
    net = _net(0)
    w1 = ctypes.cast(net.W, ctypes.POINTER(ctypes.c_void_p))[1]
    m0 = ctypes.cast(net.mb, ctypes.POINTER(ctypes.c_void_p))[0]
    # a critic tensor that the step writes
    for other in (w1, m0, net.pow, LOG_ALPHA, STATE, GRAD, LOSS, LPM):
        arr = _critic_layers(1)[0]
        arr[1] = other
        _sac_refused(b"a critic tensor", net=net, cW=(_critic_layers(0)[0], arr))
        arr = _critic_layers(0)[1]
        arr[0] = other
        _sac_refused(b"a critic tensor", net=net, cb=(arr, _critic_layers(1)[1]))
    # the temperature and the outputs among the policy's tensors, among each other, or the batch
    for name in ("log_alpha", "state", "grad", "loss", "lpm"):
        _sac_refused(b"tensor of the policy", net=net, **{name: w1})
        _sac_refused(b"tensor of the policy", net=net, **{name: m0})
        _sac_refused(b"distinct", net=net, **{name: net.pow})
        _sac_refused(b"rows is one of", net=net, **{name: ROWS})
    _sac_refused(b"distinct", state=LOG_ALPHA)
    _sac_refused(b"distinct", grad=STATE)
    _sac_refused(b"distinct", loss=LPM)
    _sac_refused(b"distinct", lpm=LOG_ALPHA)
    # the two critics may be one and the same (they are only read)
    c = _critic()
    assert _sac(B=0, critics=(c, c), cW=(_critic_layers(0)[0],) * 2, cb=(_critic_layers(0)[1],) * 2)[0] == 0


def test_sac_workspace_and_lds_limit():
    _abi, lib = _lib()
    _sac_refused(b"workspace is NULL", ws=None)
    _sac_refused(b"16-B aligned", ws=WS + 8)
    a, c1, c2 = _actor((32,)), _critic(), _critic((32,))
    need = lib.ctr_sac_workspace_bytes(a, c1, c2, 64)
    twin = lib.ctr_td3_workspace_bytes(a, c1, c2, 64)
    assert need >= twin > 0
    # the policy's own region: 16 B + 64 loss partials, 4 slots of the 12-row network, 64 logp partials
    params = 32 * 19 + 32 + 12 * 32 + 12
    own = 16 + 64 * 8 + 4 * (params * 4 + 2 * (32 + 12) * 4) + 64 * 8
    wide_a = _actor((256, 128))
    assert lib.ctr_sac_workspace_bytes(wide_a, _critic((32,)), _critic((32,)), 64) == \
        16 + 64 * 8 + 4 * ((256 * 20 + 128 * 257 + 12 * 129) * 4 + 2 * (256 + 128 + 12) * 4) + 64 * 8
    _sac_refused(b"workspace too small", ws_bytes=own - 1)
    assert _sac(B=64, ws_bytes=own, rows=None)[1].find(b"rows is NULL") >= 0          # past the workspace checks
    _sac_refused(b"workspace too small", ws_bytes=own, B=65)
    assert lib.ctr_sac_workspace_bytes(None, c1, c2, 64) == -1 and b"ctr_sac_workspace_bytes" in lib.ctr_last_error()
    assert lib.ctr_sac_workspace_bytes(a, None, c2, 64) == -1 and lib.ctr_sac_workspace_bytes(a, c1, None, 64) == -1
    assert lib.ctr_sac_workspace_bytes(a, c1, _critic(in_dim=26), 64) == -1
    for bad in (0, -1, 65537):
        assert lib.ctr_sac_workspace_bytes(a, c1, c2, bad) == -1 and b"max_B" in lib.ctr_last_error()
    # three tile images: every network whose blob fits CTR_ACTOR_MAX_BYTES has a tile image of at most 38.25 KB, so every
    # trio the entry points accept fits the 160 KB of LDS (the refusal is a guard behind the shape checks)
    widths = range(32, 257, 32)
    shapes = [(a,) for a in widths] + [(a, b) for a in widths for b in widths] + \
        [(a, b, c) for a in widths for b in widths for c in widths]
    fits = [h for h in shapes if lib.ctr_critic_blob_bytes(_critic(h, 26)) > 0]
    assert (256, 128, 32) in fits and (256, 256) not in fits
    image = max(16 * ((32 + 4) + sum(w + 4 for w in h) + (16 + 4)) * 4 for h in fits)
    worst = max(fits, key=lambda h: sum(w + 4 for w in h))
    assert worst == (224, 64, 256) and image == 39168 and 3 * image + 4096 + 16 <= 160 * 1024
    assert _sac(B=0, actor=_actor(worst), critics=(_critic(worst), _critic(worst)))[0] == 0


# ------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_sac_grads.py exist, and SacLearner's constructor

def test_the_gpu_cases_have_their_seeds():
    """``sac_ref.case`` on the CPU for every case tests/test_gpu_sac_grads.py runs, the one past T * SLOTS
    rows included: a seed below 50 qualifies, and on the mixed shapes both critics give the minimum."""
    for shape in S.SHAPES:
        for B in (1, 70, 3 * S.T + 5):
            mixed = shape in S.MIXED and B > 1
            seed, made, eps, ref64, ref32 = S.case(*shape, B, mixed=mixed)
            assert S.clear(ref64) and eps.shape == (B, 6)
            assert not mixed or 0.1 <= ref64["share"] <= 0.9
            worst = max(S.err(g32, g64) for p32, p64 in zip(ref32["grads"], ref64["grads"]) for g32, g64 in zip(p32, p64))
            assert 0 < worst < 2e-6, (shape, B, worst)
    seed, made, eps, ref64, _ = S.case(*S.SHAPES[0], S.T * S.SLOTS + 5)
    assert S.clear(ref64) and 0.1 <= ref64["share"] <= 0.9
    assert S.clear(S.case(*S.SHAPES[1], 70, log_std=(5.0, 5.0, -25.0, None, None, None))[3])


def test_sac_learner_constructor_errors():
    import torch
    from ctr_reach_amd.learner import SacLearner
    policy, c1, c2, _ = S.make(0, (32,), (32,), (64,), 19, 4)
    six = R.mlp(19, (32,), 6, True).requires_grad_(False)
    with pytest.raises(ValueError, match=exact("policy layer 1: W must be [12, 32], not [6, 32]")):
        SacLearner(six[:-1], c1, c2)
    with pytest.raises(ValueError, match=exact("the policy ends with its output nn.Linear (no activation after it)")):
        SacLearner(six, c1, c2)
    with pytest.raises(ValueError, match=exact("the critic2 takes [row, action]: 19 + 6 inputs, not 26")):
        SacLearner(policy, c1, R.mlp(26, (32,), 1, False).requires_grad_(False))
    with pytest.raises(ValueError, match=exact("policy layer 0: W" + WRITES_IN_PLACE)):
        SacLearner(copy_with_grad(policy), c1, c2)
    with pytest.raises(ValueError, match=exact("critic1 and critic2 share a tensor: the twin step updates them side by side")):
        SacLearner(policy, c1, c1)
    for kw, word in (({"alpha_lr": float("nan")}, "alpha_lr must be finite"),
                     ({"target_entropy": float("inf")}, "target_entropy must be finite"),
                     ({"init_alpha": 0.0}, "init_alpha must be positive and finite"),
                     ({"init_alpha": float("inf")}, "init_alpha must be positive and finite"),
                     ({"betas": (0.9, 1.0)}, "betas must be in [0, 1)"), ({"eps": 0.0}, "eps must be positive"),
                     ({"max_batch": 0}, "max_batch must be in 1..65536"), ({"max_batch": 65537}, "max_batch must be in 1..65536"),
                     ({"scale": [1, 2, 3]}, "scale is six finite, non-zero floats"),
                     ({"scale": [1, 2, 3, 0, 1, 1]}, "scale is six finite, non-zero floats")):
        with pytest.raises(ValueError, match=exact(word)):
            SacLearner(policy, c1, c2, **kw)
    with pytest.raises(ValueError, match=exact("the networks are on cpu: the learner's networks are on a GPU")):
        SacLearner(policy, c1, c2)
    assert all(not p.requires_grad for p in policy.parameters()) and isinstance(policy[0].weight, torch.Tensor)


def copy_with_grad(net):
    import copy
    return copy.deepcopy(net).requires_grad_(True)
