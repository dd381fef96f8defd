"""A run of SAC updates from one call, on the host (no GPU): ctr_sac_update is declared, listed and
exported within ABI 17; the ctypes mirror of ctr_sac_update_t matches the header; every refusal the
header lists returns CTR_EINVAL (-1) with a ctr_last_error whose whole text is pinned here, before
any launch (the device pointers are fake and never dereferenced); updates == 0 and batch_size == 0 are
checked no-ops; SacLearner.update refuses what it would have to convert or copy, on stub objects."""
import ctypes
import itertools
import os
import re
import subprocess
import types

import numpy as np
import pytest

from test_host_ddpg import exact
from test_host_sac_target import _actor, _critic, _her

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FN = "ctr_sac_update"


def _lib():
    from ctr_reach_amd import _abi
    return _abi, _abi.load()


def test_declared_listed_and_exported():
    _abi, lib = _lib()
    header = open(os.path.join(ROOT, "include", "ctr_reach_amd.h")).read()
    assert re.search(r"^int ctr_sac_update\(const ctr_sac_update_t \*u, int32_t updates, void \*stream\);", header, re.M)
    assert re.search(r"^#define CTR_ABI_VERSION 17$", header, re.M)
    assert FN in _abi.EXPORTED and hasattr(lib, FN)
    assert lib.ctr_abi_version() == _abi.CTR_ABI_VERSION == 17
    nm = subprocess.check_output(["nm", "-D", "--defined-only", lib._name]).decode()
    assert re.search(r" T ctr_sac_update$", nm, re.M)
    from ctr_reach_amd.learner import SacLearner
    assert hasattr(SacLearner, "update")
    makefile = open(os.path.join(ROOT, "gym-ctr-reach_amd", "Makefile")).read()
    assert "csrc/ctr_sac_update.inc" in re.search(r"^DEPS := (.*)$", makefile, re.M).group(1)


def test_struct_layout_matches_header(tmp_path):
    from ctr_reach_amd import _abi_sac
    cls = _abi_sac.CtrSacUpdate
    lines = ['  printf("%zu\\n", sizeof(ctr_sac_update_t));']
    want = [ctypes.sizeof(cls)]
    for fname, _ in cls._fields_:
        lines.append('  printf("%%zu\\n", offsetof(ctr_sac_update_t, %s));' % fname)
        want.append(getattr(cls, fname).offset)
    lines.append('  printf("%d\\n", CTR_ABI_VERSION);')
    want.append(17)
    prog = tmp_path / "sac_update_layout.c"
    prog.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"ctr_reach_amd.h\"\nint main(void) {\n"
                    + "\n".join(lines) + "\n  return 0; }\n")
    exe = tmp_path / "sac_update_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(prog), "-o", str(exe)])
    assert list(map(int, subprocess.check_output([str(exe)]).split())) == want
    assert [f for f, _ in cls._fields_] == [
        "her", "batch_size", "draw_seed", "draw_counter", "batch", "target", "q1_next", "q2_next", "next_action",
        "next_logp", "gamma", "tau", "policy", "policy_net", "policy_adam", "critic", "critic_net", "critic_adam", "scale",
        "critic_targ", "W_targ", "b_targ", "seed", "step_counter", "log_alpha", "alpha", "target_entropy", "pad",
        "critic_loss", "actor_loss", "logp_mean", "workspace", "workspace_bytes", "history"]


class _Call(object):
    """A whole, valid ctr_sac_update_t on fake device pointers (distinct multiples of 4 096), with everything
    it points to kept alive; a test changes one thing and calls."""

    def __init__(self, policy=(64, 64), critics=((64, 64), (32,)), obs_dim=13, B=8):
        from ctr_reach_amd import _abi, _abi_ddpg, _abi_sac
        self._abi = _abi
        self._next = itertools.count(16)
        self.keep = []
        self.u = u = _abi_sac.CtrSacUpdate()
        self.her = _her(obs_dim)
        self.batch = _abi.CtrHerBatch()
        for name in ("obs", "action", "reward", "next_obs", "done"):
            setattr(self.batch, name, self.ptr())
        u.her, u.batch, u.batch_size = ctypes.pointer(self.her), ctypes.pointer(self.batch), B
        u.draw_seed, u.draw_counter, u.seed, u.step_counter = 1, 2, 3, 4
        u.target = self.ptr()
        u.gamma, u.tau = 0.99, 0.005
        self.policy = _actor(policy, obs_dim + 6, blob=self.ptr())
        self.policy_net = self.net(policy, obs_dim + 6, 12)
        self.policy_adam = _abi_ddpg.CtrDdpgAdam(3e-4, 0.9, 0.999, 1e-8)
        self.critic_adam = _abi_ddpg.CtrDdpgAdam(3e-4, 0.9, 0.999, 1e-8)
        u.policy, u.policy_net = ctypes.pointer(self.policy), ctypes.pointer(self.policy_net)
        u.policy_adam, u.critic_adam = ctypes.pointer(self.policy_adam), ctypes.pointer(self.critic_adam)
        self.critic, self.critic_net, self.targ, self.targ_arrays = [], [], [], []
        for y, hidden in enumerate(critics):
            self.critic.append(_critic(hidden, obs_dim + 12, blob=None))       # the online critics' blobs are not read
            self.critic_net.append(self.net(hidden, obs_dim + 12, 1))
            self.targ.append(_critic(hidden, obs_dim + 12, blob=self.ptr()))
            W, b = self.layers(len(hidden) + 1), self.layers(len(hidden) + 1)
            self.targ_arrays.append((W, b))
            u.critic[y], u.critic_net[y] = ctypes.pointer(self.critic[y]), ctypes.pointer(self.critic_net[y])
            u.critic_targ[y], u.W_targ[y], u.b_targ[y] = ctypes.pointer(self.targ[y]), W, b
        u.log_alpha = self.ptr()
        self.alpha = _abi_sac.CtrSacAlpha(self.ptr(), self.ptr(), 3e-4, 1)
        u.alpha, u.target_entropy = ctypes.pointer(self.alpha), -6.0
        u.critic_loss, u.actor_loss, u.logp_mean = self.ptr(), self.ptr(), self.ptr()
        u.workspace, u.workspace_bytes = self.ptr(), self.workspace_bytes(256)

    def ptr(self):
        return next(self._next) << 12

    def layers(self, n):
        arr = (self._abi._P * n)(*[self.ptr() for _ in range(n)])
        self.keep.append(arr)
        return arr

    def net(self, hidden, in_dim, out):
        from ctr_reach_amd import _abi_ddpg
        s = _abi_ddpg.CtrDdpgNet()
        for field in ("W", "b", "gW", "gb", "mW", "mb", "vW", "vb"):
            setattr(s, field, self.layers(len(hidden) + 1))
        s.pow = self.ptr()
        return s

    def workspace_bytes(self, B):
        _, lib = _lib()
        n = int(lib.ctr_sac_workspace_bytes(self.policy, self.critic[0], self.critic[1], B))
        assert n > 0
        return n

    def __call__(self, updates=2):
        _, lib = _lib()
        return lib.ctr_sac_update(self.u, updates, None), lib.ctr_last_error()


def _refused(word, change, updates=2, **kw):
    c = _Call(**kw)
    change(c)
    rc, msg = c(updates)
    assert rc == -1 and msg == word, (word, rc, msg)


def _set(path, value):
    """change(c): c.<path> = value, path like "u.target" or "policy.blob"."""
    def change(c):
        obj = c
        names = path.split(".")
        for name in names[:-1]:
            obj = getattr(obj, name)
        setattr(obj, names[-1], value)
    return change


def _layer(path, l, value):
    def change(c):
        obj = c
        for name in path.split("."):
            obj = obj[int(name)] if name.isdigit() else getattr(obj, name)
        obj[l] = value
    return change


def test_a_valid_call_passes_the_checks_only_as_a_no_op():
    """(with updates > 0 and B > 0 the call would launch on the fake pointers: not made here)"""
    assert _Call()(0)[0] == 0
    assert _Call(B=0)(3)[0] == 0
    assert _Call(B=0, obs_dim=14)(3)[0] == 0
    assert _Call(policy=(32,), critics=((256, 128), (128, 128, 128)))(0)[0] == 0
    c = _Call()
    c.u.history = c.ptr()
    assert c(0)[0] == 0
    c = _Call(B=0)
    c.u.scale = c.ptr()
    c.alpha.learn = 0
    c.alpha.grad = None
    c.u.critic_loss = c.u.actor_loss = c.u.logp_mean = None
    assert c(5)[0] == 0
    c = _Call(B=0)
    c.u.tau = 1.0
    assert c(1)[0] == 0
    c.u.tau = 0.0
    assert c(1)[0] == 0


def test_the_no_ops_are_still_checked():
    _refused(b"ctr_sac_update: log_alpha is NULL", _set("u.log_alpha", None), updates=0)
    _refused(b"ctr_sac_update: target is NULL", _set("u.target", None), B=0)
    _refused(b"ctr_sac_update: tau must be in [0, 1]", _set("u.tau", 1.5), updates=0)


def test_refusals_of_the_call_itself():
    _, lib = _lib()
    assert lib.ctr_sac_update(None, 1, None) == -1
    assert lib.ctr_last_error() == b"ctr_sac_update: u is NULL"
    _refused(b"ctr_sac_update: updates must be >= 0", lambda c: None, updates=-1)


def test_refusals_of_the_draw():
    _refused(b"ctr_sac_update: her is NULL", _set("u.her", None))
    _refused(b"ctr_sac_update: bad batch", _set("u.batch", None))
    _refused(b"ctr_sac_update: bad batch", _set("u.batch_size", -1))
    _refused(b"ctr_sac_update: her: obs_dim must be 13 or 14", _set("her.obs_dim", 15))
    _refused(b"ctr_sac_update: her: slots must be >= 2", _set("her.slots", 1))
    _refused(b"ctr_sac_update: empty store", _set("her.n", 0))
    _refused(b"ctr_sac_update: output missing", _set("batch.done", None))
    _refused(b"ctr_sac_update: obs / next_obs / action must be 16-byte aligned", _set("batch.next_obs", (1 << 13) + 4))
    _refused(b"ctr_sac_update: actor is NULL", _set("u.policy", None))
    _refused(b"ctr_sac_update: actor: n_hidden must be in 1..CTR_ACTOR_MAX_HIDDEN (3)", _set("policy.n_hidden", 4))
    _refused(b"ctr_sac_update: actor: every hidden width must be a multiple of 32 in 32..CTR_ACTOR_MAX_WIDTH (256)",
             lambda c: c.policy.width.__setitem__(1, 48))
    _refused(b"ctr_sac_update: actor: in_dim must be obs_dim + 6 = 19 or 20", _set("policy.in_dim", 18))
    _refused(b"ctr_sac_update: actor: blob is NULL", _set("policy.blob", None))
    _refused(b"ctr_sac_update: actor: blob must be 16-B aligned", _set("policy.blob", (1 << 21) + 8))
    for y in (0, 1):
        _refused(b"ctr_sac_update: critic_targ[0] or critic_targ[1] is NULL", _layer("u.critic_targ", y, None))
        _refused(b"ctr_sac_update: critic: n_hidden must be in 1..CTR_ACTOR_MAX_HIDDEN (3)",
                 lambda c: setattr(c.targ[y], "n_hidden", 0))
        _refused(b"ctr_sac_update: critic: every hidden width must be a multiple of 32 in 32..CTR_ACTOR_MAX_WIDTH (256)",
                 lambda c: c.targ[y].width.__setitem__(0, 48))
        _refused(b"ctr_sac_update: critic: blob is NULL", lambda c: setattr(c.targ[y], "blob", None))
        _refused(b"ctr_sac_update: critic: blob must be 16-B aligned", lambda c: setattr(c.targ[y], "blob", (1 << 20) + 4))
        _refused(b"ctr_sac_update: critic_targ[0]->in_dim and critic_targ[1]->in_dim must be her->obs_dim + 12",
                 lambda c: setattr(c.targ[y], "in_dim", 26))
    _refused(b"ctr_sac_update: policy->in_dim must be her->obs_dim + 6", _set("her.obs_dim", 14))
    for g in (float("nan"), float("inf"), -float("inf")):
        _refused(b"ctr_sac_update: gamma must be finite", _set("u.gamma", g))
    _refused(b"ctr_sac_update: log_alpha is NULL", _set("u.log_alpha", None))
    _refused(b"ctr_sac_update: target is NULL", _set("u.target", None))


def test_refusals_of_the_critics_step():
    for y in (0, 1):
        _refused(b"ctr_sac_update: NULL entry in critic[2] or critic_net[2]", _layer("u.critic", y, None))
        _refused(b"ctr_sac_update: NULL entry in critic[2] or critic_net[2]", _layer("u.critic_net", y, None))
        _refused(b"ctr_sac_update: critic: n_hidden must be in 1..CTR_ACTOR_MAX_HIDDEN (3)",
                 lambda c: setattr(c.critic[y], "n_hidden", 4))
        _refused(b"ctr_sac_update: critic: in_dim must be obs_dim + 12 = 25 or 26", lambda c: setattr(c.critic[y], "in_dim", 24))
        _refused(b"ctr_sac_update: the two critics must have the same in_dim", lambda c: setattr(c.critic[y], "in_dim", 26))
        for field in ("W", "b", "gW", "gb", "mW", "mb", "vW", "vb", "pow"):
            _refused(b"ctr_sac_update: NULL pointer array or pow in net", lambda c: setattr(c.critic_net[y], field, None))
        _refused(b"ctr_sac_update: NULL layer among W, b, gW, gb, mW, mb, vW, vb [0..n_hidden]",
                 lambda c: c.critic_net[y].mW.__setitem__(1, None))
        _refused(b"ctr_sac_update: a gradient or state tensor is a parameter tensor",
                 lambda c: c.critic_net[y].vb.__setitem__(0, c.critic_net[y].W[1]))
    _refused(b"ctr_sac_update: adam is NULL", _set("u.critic_adam", None))
    finite = b"ctr_sac_update: lr, beta1, beta2 and eps must be finite"
    betas, eps = b"ctr_sac_update: beta1 and beta2 must be in [0, 1)", b"ctr_sac_update: eps must be positive"
    for field, bad, word in (("lr", float("nan"), finite), ("lr", float("inf"), finite), ("beta1", float("nan"), finite),
                             ("beta1", 1.0, betas), ("beta2", -0.1, betas), ("eps", 0.0, eps), ("eps", -1e-8, eps),
                             ("eps", float("nan"), finite)):
        _refused(word, _set("critic_adam." + field, bad))
        _refused(word, _set("policy_adam." + field, bad))
    _refused(b"ctr_sac_update: B must be in 0..65536", _set("u.batch_size", 65537))
    _refused(b"ctr_sac_update: workspace is NULL", _set("u.workspace", None))
    _refused(b"ctr_sac_update: workspace must be 16-B aligned", _set("u.workspace", (1 << 30) + 8))
    _refused(b"ctr_sac_update: workspace too small (ctr_sac_workspace_bytes)",
             lambda c: setattr(c.u, "workspace_bytes", c.workspace_bytes(8) - 16))
    _refused(b"ctr_sac_update: workspace too small (ctr_ddpg_workspace_bytes)", _set("u.workspace_bytes", 1024))
    # the workspace is sized for the call's B: one for 8 rows does not serve 300
    _refused(b"ctr_sac_update: workspace too small (ctr_ddpg_workspace_bytes)",
             lambda c: (setattr(c.u, "workspace_bytes", c.workspace_bytes(8)),
                                                setattr(c.u, "batch_size", 300)))


def test_refusals_of_the_policys_step_and_the_temperature():
    _refused(b"ctr_sac_update: net is NULL", _set("u.policy_net", None))
    _refused(b"ctr_sac_update: adam is NULL", _set("u.policy_adam", None))
    _refused(b"ctr_sac_update: NULL layer among W, b, gW, gb, mW, mb, vW, vb [0..n_hidden]",
             lambda c: c.policy_net.gb.__setitem__(2, None))
    _refused(b"ctr_sac_update: actor->in_dim + 6 must be critic->in_dim of both critics",
             lambda c: (setattr(c.critic[0], "in_dim", 25), setattr(c.critic[1], "in_dim", 25)), obs_dim=14)
    _refused(b"ctr_sac_update: alpha is NULL", _set("u.alpha", None))
    _refused(b"ctr_sac_update: alpha->state is NULL", _set("alpha.state", None))
    for bad in (float("nan"), float("inf")):
        _refused(b"ctr_sac_update: target_entropy and alpha->lr must be finite", _set("u.target_entropy", bad))
        _refused(b"ctr_sac_update: target_entropy and alpha->lr must be finite", _set("alpha.lr", bad))


def test_refusals_of_the_soft_update_and_the_targets():
    for tau in (float("nan"), -0.001, 1.001, float("inf")):
        _refused(b"ctr_sac_update: tau must be in [0, 1]", _set("u.tau", tau))
    for y in (0, 1):
        _refused(b"ctr_sac_update: NULL entry in W_targ[2] or b_targ[2]", _layer("u.W_targ", y, None))
        _refused(b"ctr_sac_update: NULL entry in W_targ[2] or b_targ[2]", _layer("u.b_targ", y, None))
        _refused(b"ctr_sac_update: NULL layer among W_targ, b_targ [0..n_hidden]",
                 lambda c: c.targ_arrays[y][0].__setitem__(0, None))
        _refused(b"ctr_sac_update: NULL layer among W_targ, b_targ [0..n_hidden]",
                 lambda c: c.targ_arrays[y][1].__setitem__(1, None))
    # a target critic has its online critic's shape
    _refused(b"ctr_sac_update: a target critic's shape differs from its online critic's",
             lambda c: c.targ[0].width.__setitem__(1, 32))
    _refused(b"ctr_sac_update: a target critic's shape differs from its online critic's",
             lambda c: (setattr(c.targ[1], "n_hidden", 2), c.targ[1].width.__setitem__(1, 32)))
    _refused(b"ctr_sac_update: a target critic's shape differs from its online critic's",
             lambda c: c.targ[1].width.__setitem__(0, 64))


def test_refusals_of_shared_memory():
    def same(a, b):
        return b"ctr_sac_update: " + a + b" and " + b + b" are the same memory"
    param, grad, targ, blob = b"a parameter tensor", b"a gradient tensor", b"a target tensor", b"a target critic's blob"
    # a target tensor shared with an online one, between the two targets, with the policy
    _refused(same(param, targ), lambda c: c.targ_arrays[0][0].__setitem__(0, c.critic_net[0].W[0]))
    _refused(same(targ, param), lambda c: c.targ_arrays[1][1].__setitem__(0, c.critic_net[1].b[0]))
    _refused(same(targ, targ), lambda c: c.targ_arrays[1][0].__setitem__(1, c.targ_arrays[0][0][1]))
    _refused(same(param, targ), lambda c: c.targ_arrays[0][1].__setitem__(0, c.policy_net.b[0]))
    _refused(same(targ, b"a first-moment tensor"), lambda c: c.targ_arrays[0][1].__setitem__(0, c.critic_net[1].mb[0]))
    # the blobs
    _refused(same(blob, blob), lambda c: setattr(c.targ[1], "blob", c.targ[0].blob))
    _refused(same(blob, b"the policy's blob"), lambda c: setattr(c.targ[0], "blob", c.policy.blob))
    _refused(same(b"the policy's blob", param), lambda c: setattr(c.policy, "blob", c.critic_net[0].W[0]))
    # ctr_td3_critic_step's: the two nets share a tensor; ctr_sac_actor_step's: a critic tensor is the policy's
    _refused(same(grad, grad), lambda c: c.critic_net[1].gW.__setitem__(0, c.critic_net[0].gW[0]))
    _refused(same(b"a net's pow", b"a net's pow"), lambda c: setattr(c.critic_net[1], "pow", c.critic_net[0].pow))
    _refused(same(param, param), lambda c: c.critic_net[0].W.__setitem__(0, c.policy_net.W[0]))
    _refused(same(b"log_alpha", b"alpha->state"), lambda c: setattr(c.u, "log_alpha", c.alpha.state))
    _refused(same(b"actor_loss", b"logp_mean"), lambda c: setattr(c.u, "logp_mean", c.u.actor_loss))
    _refused(same(b"actor_loss", b"a net's pow"), lambda c: setattr(c.u, "actor_loss", c.policy_net.pow))
    _refused(same(b"batch->reward", b"target"), lambda c: setattr(c.u, "target", c.batch.reward))
    _refused(same(b"scale", param), lambda c: setattr(c.u, "scale", c.critic_net[0].W[0]))
    _refused(same(b"the workspace", blob), lambda c: setattr(c.u, "workspace", c.targ[0].blob))
    # history against every kind of output, at its first float and inside its rows
    hist = b"history"
    for other, word in ((lambda c: c.u.target, same(hist, b"target")), (lambda c: c.u.critic_loss, same(b"critic_loss", hist)),
                        (lambda c: c.batch.obs, same(hist, b"batch->obs")), (lambda c: c.policy_net.W[0], same(param, hist)),
                        (lambda c: c.targ_arrays[1][0][0], same(hist, targ)), (lambda c: c.targ[0].blob, same(hist, blob)),
                        (lambda c: c.u.log_alpha, same(hist, b"log_alpha")), (lambda c: c.alpha.state, same(hist, b"alpha->state")),
                        (lambda c: c.u.workspace, same(b"the workspace", hist))):
        _refused(word, lambda c: setattr(c.u, "history", other(c)))
    _refused(b"ctr_sac_update: history and logp_mean are the same memory",
             lambda c: (setattr(c.u, "history", c.ptr()), setattr(c.u, "logp_mean", c.u.history + 5 * 4)),
             updates=2)
    _refused(b"ctr_sac_update: history and actor_loss are the same memory",
             lambda c: (setattr(c.u, "history", c.ptr()), setattr(c.u, "actor_loss", c.u.history + 39)),
             updates=2)
    # ... and what lies behind its rows is not its memory
    c = _Call(B=0)
    c.u.history = c.ptr()
    c.u.logp_mean = c.u.history + 40
    assert c(2)[0] == 0


# --- SacLearner.update's own refusals, on stub objects --------------------------------------------------

def _layers(rng, dims):
    import torch
    return [(torch.from_numpy(rng.uniform(-1, 1, (dims[l + 1], dims[l])).astype(np.float32)),
             torch.from_numpy(rng.uniform(-1, 1, dims[l + 1]).astype(np.float32))) for l in range(len(dims) - 1)]


def _stubs():
    """A learner, a buffer, a policy and two targets that have only what the checks read, on the CPU."""
    import torch
    from ctr_reach_amd.learner import SacLearner
    from ctr_reach_amd.policy import GaussianActor, MlpCritic
    rng = np.random.default_rng(5)
    cpu = torch.device("cpu")
    scale = np.full(6, 0.5, np.float32)
    masters = _layers(rng, [19, 64, 12])
    critics = [_layers(rng, [25, 32, 1]), _layers(rng, [25, 64, 64, 1])]
    learner = SacLearner.__new__(SacLearner)
    learner.device, learner.max_batch, learner.in_dim = cpu, 256, 19
    learner._actor = types.SimpleNamespace(params=masters)
    learner._critics = [types.SimpleNamespace(params=c) for c in critics]
    her = types.SimpleNamespace(venv=types.SimpleNamespace(device=cpu), obs_dim=13)
    pi = GaussianActor(masters, scale, device="cpu")
    owners = [_layers(rng, [25, 32, 1]), _layers(rng, [25, 64, 64, 1])]
    targets = [(MlpCritic(o, device="cpu"), o) for o in owners]
    return learner, her, pi, targets


def test_update_refuses_before_anything_is_converted_or_written():
    import torch
    from ctr_reach_amd.policy import GaussianActor, MlpActor, MlpCritic
    learner, her, pi, targets = _stubs()
    rng = np.random.default_rng(6)
    scale = np.full(6, 0.5, np.float32)

    def bad(match, her=her, pi=pi, targets=targets, B=8, gamma=0.99, tau=0.005, **kw):
        with pytest.raises(ValueError, match=exact(match)):
            learner.update(her, pi, targets, B, gamma, tau, **kw)

    # the checks pass on the stubs as they are: the call then needs what a stub lacks
    with pytest.raises(AttributeError):
        learner.update(her, pi, targets, 8, 0.99, 0.005)
    bad("update: pi must be a GaussianActor (the 12-row head), not MlpActor",
        pi=MlpActor(_layers(rng, [19, 64, 6]), scale, device="cpu"))
    bad("update: the policy must be on the device", pi=GaussianActor(_layers(rng, [19, 64, 12]), scale, device=None))
    bad("update: targets is [(critic1_targ_dev, critic1_targ), (critic2_targ_dev, critic2_targ)]", targets=targets[:1])
    bad("update: targets is [(critic1_targ_dev, critic1_targ), (critic2_targ_dev, critic2_targ)]",
        targets=[targets[0], (targets[1][0],)])
    bad("update: target 2 must be an MlpCritic, not GaussianActor", targets=[targets[0], (pi, targets[1][1])])
    bad("update: the target 1 must be on the device", targets=[(MlpCritic(targets[0][1], device=None), targets[0][1]), targets[1]])
    bad("update: the two targets are one MlpCritic: each has its own blob", targets=[targets[0], targets[0]])
    for g in (float("nan"), float("inf")):
        bad("update: gamma must be finite", gamma=g)
    for t in (float("nan"), -0.1, 1.5):
        bad("update: tau must be in [0, 1]", tau=t)
    bad("update: batch_size = 257, the learner was built for max_batch = 256", B=257)
    bad("update: batch_size = -1, the learner was built for max_batch = 256", B=-1)
    bad("update: updates must be >= 0", updates=-1)
    bad("update: the buffer's rows are 20 floats, the policy's 19", her=types.SimpleNamespace(venv=her.venv, obs_dim=14))
    bad("update: the buffer is on cuda:0, the learner on cpu",
        her=types.SimpleNamespace(venv=types.SimpleNamespace(device=torch.device("cuda", 0)), obs_dim=13))
    # load_'s and polyak_'s checks of the tensors: shapes, dtype, contiguity, requires_grad
    bad("update: the policy's layer 0: W must be [32, 19], not [64, 19]",
        pi=GaussianActor(_layers(rng, [19, 32, 12]), scale, device="cpu"))
    deep = _layers(rng, [25, 64, 64, 1])
    bad("update: target 1: online the critic has 3 layers of (W, b)",targets=[(MlpCritic(deep, device="cpu"), deep), targets[1]])
    wide = _layers(rng, [25, 64, 1])
    bad("update: target 1: online layer 0: W must be [64, 25], not [32, 25]",
        targets=[(MlpCritic(wide, device="cpu"), wide), targets[1]])
    wrong = [(W.double(), b) for W, b in targets[0][1]]
    bad("update: target 1: target layer 0: W must be float32, not torch.float64", targets=[(targets[0][0], wrong), targets[1]])
    wrong = [(W.t().contiguous().t(), b) for W, b in targets[1][1]]
    bad("update: target 2: target layer 0: W must be contiguous", targets=[targets[0], (targets[1][0], wrong)])
    wrong = [(W.clone().requires_grad_(True), b) for W, b in targets[1][1]]
    bad("update: target 2: target layer 0: W requires grad: a target is written in place, outside autograd",
        targets=[targets[0], (targets[1][0], wrong)])
    # history: float32, [updates, 5], contiguous, on the device
    for h in (np.zeros((2, 5), np.float32), torch.zeros((2, 5), dtype=torch.float64), torch.zeros((3, 5)), torch.zeros(10),
              torch.zeros((5, 2)).t()):
        bad("update: history must be a contiguous float32 [updates, 5] = [2, 5] tensor on cpu", updates=2, history=h)
    # nothing was dropped or set by a refused call
    assert pi.weights is not None and pi._sources is None
    assert all(net.weights is not None and net._sources is None for net, _ in targets)
    assert not hasattr(her, "_counter") and not hasattr(learner, "counter")
