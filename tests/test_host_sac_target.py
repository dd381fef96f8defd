"""SAC's soft target inside the sampler, on the host (no GPU): ctr_her_sample_sac is declared, listed
and exported within ABI 17; the ctypes mirror of ctr_her_sac_t matches the header; every refusal the
header lists returns CTR_EINVAL (-1) with a ctr_last_error that starts with the function's name,
before any HIP call (the device pointers are fake and never dereferenced); an empty draw is a
checked no-op; HerReplayBuffer.sample_sac refuses what it would have to convert or copy."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FN = "ctr_her_sample_sac"


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


def _her(obs_dim=13, n=8):
    from ctr_reach_amd import _abi
    h = _abi.CtrHer()
    h.obs_dim, h.t_max, h.n_sampled_goal, h.strategy = obs_dim, 5, 4, _abi.CTR_HER_FUTURE
    h.n, h.env_base, h.slots, h.seed = n, 0, 3, 1
    for name in ("state", "step", "dg", "tol", "len", "epoch", "cur_t", "cur_epoch", "cdf"):
        setattr(h, name, 1 << 12)
    return h


def test_declared_listed_and_exported():
    _abi, lib = _lib()
    header = open(os.path.join(ROOT, "include", "ctr_reach_amd.h")).read()
    assert re.search(r"^int ctr_her_sample_sac\(const ctr_her_t \*her, int64_t batch_size, uint64_t seed, uint64_t counter,\n"
                     r" +const ctr_her_batch_t \*out, const ctr_her_sac_t \*td, void \*stream\);", header, re.M)
    assert re.search(r"^#define CTR_ABI_VERSION 17$", header, re.M)
    assert FN in _abi.EXPORTED and hasattr(lib, FN)
    assert lib.ctr_abi_version() == _abi.CTR_ABI_VERSION == 17
    nm = subprocess.check_output(["nm", "-D", "--defined-only", lib._name]).decode()
    assert re.search(r" T ctr_her_sample_sac$", nm, re.M)
    import ctr_reach_amd
    assert hasattr(ctr_reach_amd.HerReplayBuffer, "sample_sac")


def test_struct_layout_matches_header(tmp_path):
    from ctr_reach_amd import _abi_sac
    cls = _abi_sac.CtrHerSac
    lines = ['  printf("%zu\\n", sizeof(ctr_her_sac_t));']
    want = [ctypes.sizeof(cls)]
    for fname, _ in cls._fields_:
        lines.append('  printf("%%zu\\n", offsetof(ctr_her_sac_t, %s));' % fname)
        want.append(getattr(cls, fname).offset)
    lines.append('  printf("%d\\n", CTR_ABI_VERSION);')
    want.append(17)
    prog = tmp_path / "sac_target_layout.c"
    prog.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"ctr_reach_amd.h\"\nint main(void) {\n"
                    + "\n".join(lines) + "\n  return 0; }\n")
    exe = tmp_path / "sac_target_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(prog), "-o", str(exe)])
    assert list(map(int, subprocess.check_output([str(exe)]).split())) == want
    assert [f for f, _ in cls._fields_] == ["actor", "critic1", "critic2", "log_alpha", "gamma", "pad", "target",
                                            "q1_next", "q2_next", "next_action", "next_logp"]


NOARG = object()


def _call(her=None, B=8, out="default", td="default", actor=NOARG, critic1=NOARG, critic2=NOARG, gamma=0.99,
          log_alpha=1 << 15, target=1 << 14):
    from ctr_reach_amd import _abi_sac
    _abi, lib = _lib()
    her = her if her is not None else _her()
    if out == "default":
        out = _abi.CtrHerBatch()
        out.obs = out.action = out.reward = out.next_obs = out.done = 1 << 13
    if td == "default":
        td = _abi_sac.CtrHerSac()
        actor = _actor() if actor is NOARG else actor
        critic1 = _critic() if critic1 is NOARG else critic1
        critic2 = _critic((32,), blob=3 << 20) if critic2 is NOARG else critic2
        for name, net in (("actor", actor), ("critic1", critic1), ("critic2", critic2)):
            if net is not None:
                setattr(td, name, ctypes.pointer(net))
        td.gamma, td.log_alpha, td.target = gamma, log_alpha, target
    return lib.ctr_her_sample_sac(her, B, 1, 0, out, td, None), lib.ctr_last_error()


def test_refusals():
    _abi, lib = _lib()

    def refused(word, **kw):
        rc, msg = _call(**kw)
        assert rc == -1 and msg.startswith(b"ctr_her_sample_sac: ") and word in msg, (word, kw, rc, msg)

    # what ctr_her_sample refuses
    assert lib.ctr_her_sample_sac(None, 8, 1, 0, None, None, None) == -1
    assert lib.ctr_last_error().startswith(b"ctr_her_sample_sac: ") and b"her is NULL" in lib.ctr_last_error()
    bad = _her()
    bad.obs_dim = 15
    refused(b"obs_dim", her=bad)
    bad = _her()
    bad.slots = 1
    refused(b"slots", her=bad)
    refused(b"bad batch", out=None)
    refused(b"bad batch", B=-1)
    refused(b"bad batch", B=(1 << 32) + 1)                 # the row index is the noise key's 32-bit word
    refused(b"bad batch", B=1 << 31)
    refused(b"empty store", her=_her(n=0))
    out = _abi.CtrHerBatch()
    out.obs = out.action = out.reward = out.next_obs = 1 << 13
    refused(b"output missing", out=out)
    out.done = 1 << 13
    out.next_obs = (1 << 13) + 4
    refused(b"16-byte aligned", out=out)
    # the struct's pointers
    refused(b"td is NULL", td=None)
    refused(b"actor is NULL", actor=None)
    refused(b"critic1 or critic2 is NULL", critic1=None)
    refused(b"critic1 or critic2 is NULL", critic2=None)
    refused(b"log_alpha is NULL", log_alpha=None)
    refused(b"target is NULL", target=None)
    # a shape gauss_layout / critic_check refuse, a NULL or misaligned blob
    refused(b"actor: n_hidden", actor=_actor(()))
    deep = _actor((32, 32, 32))
    deep.n_hidden = 4
    refused(b"actor: n_hidden", actor=deep)
    refused(b"actor: every hidden width", actor=_actor((64, 48)))
    refused(b"CTR_ACTOR_MAX_BYTES", actor=_actor((256, 256)))
    refused(b"actor: in_dim", actor=_actor(in_dim=18))
    refused(b"actor: blob is NULL", actor=_actor(blob=None))
    refused(b"actor: blob must be 16-B aligned", actor=_actor(blob=(1 << 21) + 8))
    for which in ("critic1", "critic2"):
        refused(b"critic: n_hidden", **{which: _critic(())})
        refused(b"critic: every hidden width", **{which: _critic((64, 48))})
        refused(b"CTR_ACTOR_MAX_BYTES", **{which: _critic((256, 256))})
        refused(b"critic: in_dim", **{which: _critic(in_dim=24)})
        refused(b"critic: blob is NULL", **{which: _critic(blob=None)})
        refused(b"critic: blob must be 16-B aligned", **{which: _critic(blob=(1 << 20) + 4)})
        # the row lengths against the store's
        refused(b"in_dim must be her->obs_dim + 12", **{which: _critic(in_dim=26)})
    refused(b"actor->in_dim must be her->obs_dim + 6", actor=_actor(in_dim=20))
    refused(b"actor->in_dim must be her->obs_dim + 6", her=_her(obs_dim=14))
    refused(b"in_dim must be her->obs_dim + 12", her=_her(obs_dim=14), actor=_actor(in_dim=20))
    nan, inf = float("nan"), float("inf")
    for g in (nan, inf, -inf):
        refused(b"gamma", gamma=g)
    # an empty draw is still a checked call
    refused(b"td is NULL", B=0, td=None)
    refused(b"log_alpha is NULL", B=0, log_alpha=None)


def test_an_empty_draw_is_a_no_op():
    nan = float("nan")
    assert _call(B=0)[0] == 0
    assert _call(B=0, gamma=0.0)[0] == 0
    c = _critic()
    assert _call(B=0, critic1=c, critic2=c)[0] == 0        # the two critics may be one
    a = _actor()
    a.scale[2] = nan
    assert _call(B=0, actor=a)[0] == 0                     # the policy's scale is not read
    assert _call(B=0, her=_her(n=0))[0] == 0
    assert _call(B=0, actor=_actor((32,)), critic1=_critic((256, 128)), critic2=_critic((128, 128, 128)))[0] == 0
    assert _call(B=0, her=_her(obs_dim=14), actor=_actor(in_dim=20), critic1=_critic(in_dim=26),
                 critic2=_critic((32,), 26, 3 << 20))[0] == 0


def test_sample_sac_refuses_what_it_would_have_to_convert():
    """The checks come before anything is allocated or the library is called: a buffer that has only
    its device is enough to see them."""
    import torch
    from ctr_reach_amd.her import HerReplayBuffer
    from ctr_reach_amd.policy import GaussianActor, MlpActor, MlpCritic
    rng = np.random.default_rng(3)

    def layers(dims):
        return [(rng.uniform(-1, 1, (dims[l + 1], dims[l])).astype(np.float32),
                 rng.uniform(-1, 1, dims[l + 1]).astype(np.float32)) for l in range(len(dims) - 1)]

    buf = HerReplayBuffer.__new__(HerReplayBuffer)
    buf.venv = types.SimpleNamespace(device=torch.device("cpu"))
    scale = np.full(6, 0.5, np.float32)
    host_pi = GaussianActor(layers([19, 64, 12]), scale, device=None)
    pi = GaussianActor(layers([19, 64, 12]), scale, device="cpu")
    actor = MlpActor(layers([19, 64, 6]), scale, device="cpu")
    host_critic = MlpCritic(layers([25, 32, 1]), device=None)
    critic = MlpCritic(layers([25, 32, 1]), device="cpu")
    la = torch.zeros((), dtype=torch.float32)
    # the temperature: a float32 tensor of one element on the buffer's device, nothing else
    for bad, word in ((0.0, "torch tensor"), (np.zeros((), np.float32), "torch tensor"),
                      (torch.zeros((), dtype=torch.float64), "float32"), (torch.zeros(2), "0-d or 1-element"),
                      (torch.zeros((1, 1)), "0-d or 1-element"), (torch.zeros(0), "0-d or 1-element")):
        with pytest.raises(ValueError, match="sample_sac: log_alpha must be a? ?" + word):
            buf.sample_sac(8, pi, critic, critic, 0.99, bad)
    # the networks
    with pytest.raises(ValueError, match="sample_sac: the policy must be a GaussianActor"):
        buf.sample_sac(8, actor, critic, critic, 0.99, la)
    with pytest.raises(ValueError, match="sample_sac: the critic1 must be an MlpCritic"):
        buf.sample_sac(8, pi, actor, critic, 0.99, la)
    with pytest.raises(ValueError, match="sample_sac: the critic2 must be an MlpCritic"):
        buf.sample_sac(8, pi, critic, pi, 0.99, la)
    with pytest.raises(ValueError, match="sample_sac: the policy must be on the device"):
        buf.sample_sac(8, host_pi, critic, critic, 0.99, la)
    with pytest.raises(ValueError, match="sample_sac: the critic1 must be on the device"):
        buf.sample_sac(8, pi, host_critic, critic, 0.99, la)
    with pytest.raises(ValueError, match="sample_sac: the critic2 must be on the device"):
        buf.sample_sac(8, pi, critic, host_critic, 0.99, la.reshape(1))
    for g in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sample_sac: gamma must be finite"):
            buf.sample_sac(8, pi, critic, critic, g, la)
    # a buffer on a GPU: a host temperature would have to be copied, host networks too
    buf.venv.device = torch.device("cuda", 0)
    with pytest.raises(ValueError, match="sample_sac: log_alpha is on cpu, the buffer on cuda:0"):
        buf.sample_sac(8, pi, critic, critic, 0.99, la)
