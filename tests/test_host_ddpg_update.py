"""A run of DDPG / TD3 updates from one call, on the host (no GPU): ctr_ddpg_update is declared, listed
and exported within ABI 17; the ctypes mirror of ctr_ddpg_update_t matches the header; every refusal the
header lists returns CTR_EINVAL (-1) with a ctr_last_error whose whole text is pinned here, before
any launch (the device pointers are fake and never dereferenced); updates == 0 and batch_size == 0 are
checked no-ops; DdpgLearner.update and Td3Learner.update refuse what they would have to convert or copy,
on stub objects; SacLearner keeps its own update."""
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
from test_host_sac_update import _layer, _layers, _set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FN = "ctr_ddpg_update"
FIELDS = ["her", "batch_size", "draw_seed", "draw_counter", "batch", "target", "q1_next", "q2_next", "next_action", "gamma",
          "tau", "n_critics", "sigma", "clip", "policy_delay", "update_index", "policy", "policy_net", "policy_adam", "critic",
          "critic_net", "critic_adam", "scale", "actor_targ", "W_targ_actor", "b_targ_actor", "critic_targ", "W_targ",
          "b_targ", "actor", "critic_loss", "actor_loss", "workspace", "workspace_bytes", "history"]


def _lib():
    from ctr_reach_amd import _abi
    return _abi, _abi.load()


def test_declared_listed_and_exported():
    _abi, lib = _lib()
    header = open(os.path.join(ROOT, "include", "ctr_reach_amd.h")).read()
    assert re.search(r"^int ctr_ddpg_update\(const ctr_ddpg_update_t \*u, int32_t updates, void \*stream\);", header, re.M)
    assert re.search(r"^#define CTR_ABI_VERSION 17$", header, re.M)
    assert "A run of DDPG / TD3 updates" in header
    assert FN in _abi.EXPORTED and hasattr(lib, FN)
    assert lib.ctr_abi_version() == _abi.CTR_ABI_VERSION == 17
    assert lib.ctr_ddpg_update.argtypes is not None and len(lib.ctr_ddpg_update.argtypes) == 3
    nm = subprocess.check_output(["nm", "-D", "--defined-only", lib._name]).decode()
    assert re.search(r" T ctr_ddpg_update$", nm, re.M)
    makefile = open(os.path.join(ROOT, "gym-ctr-reach_amd", "Makefile")).read()
    assert "csrc/ctr_ddpg_update.inc" in re.search(r"^DEPS := (.*)$", makefile, re.M).group(1)
    kernels = open(os.path.join(ROOT, "gym-ctr-reach_amd", "csrc", "ctr_kernels.hip")).read()
    assert kernels.rstrip().endswith('#include "ctr_sac_update.inc"\n#include "ctr_ddpg_update.inc"')


def test_the_learners_have_their_own_update():
    from ctr_reach_amd.learner import DdpgLearner, SacLearner, Td3Learner
    assert hasattr(DdpgLearner, "update") and hasattr(Td3Learner, "update")
    # SacLearner borrows methods from both: its update stays ctr_sac_update's
    assert len({DdpgLearner.update, Td3Learner.update, SacLearner.update}) == 3
    assert "ctr_sac_update" in SacLearner.update.__doc__
    assert not issubclass(SacLearner, (DdpgLearner, Td3Learner))


def test_struct_layout_matches_header(tmp_path):
    from ctr_reach_amd import _abi_ddpg
    cls = _abi_ddpg.CtrDdpgUpdate
    lines = ['  printf("%zu\\n", sizeof(ctr_ddpg_update_t));']
    want = [ctypes.sizeof(cls)]
    for fname, _ in cls._fields_:
        lines.append('  printf("%%zu\\n", offsetof(ctr_ddpg_update_t, %s));' % fname)
        want.append(getattr(cls, fname).offset)
    lines.append('  printf("%d\\n", CTR_ABI_VERSION);')
    want.append(17)
    prog = tmp_path / "ddpg_update_layout.c"
    prog.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"ctr_reach_amd.h\"\nint main(void) {\n"
                    + "\n".join(lines) + "\n  return 0; }\n")
    exe = tmp_path / "ddpg_update_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(prog), "-o", str(exe)])
    assert list(map(int, subprocess.check_output([str(exe)]).split())) == want
    assert [f for f, _ in cls._fields_] == FIELDS


class _Call(object):
    """A whole, valid ctr_ddpg_update_t on fake device pointers (distinct multiples of 4 096), with everything
    it points to kept alive; a test changes one thing and calls."""

    def __init__(self, nc=2, policy=(64, 64), critics=((64, 64), (32,)), obs_dim=13, B=8, actor=True):
        from ctr_reach_amd import _abi, _abi_ddpg
        self._abi = _abi
        self._next = itertools.count(16)
        self.keep = []
        self.nc = nc
        self.u = u = _abi_ddpg.CtrDdpgUpdate()
        self.her = _her(obs_dim)
        self.batch = _abi.CtrHerBatch()
        for name in ("obs", "action", "reward", "next_obs", "done"):
            setattr(self.batch, name, self.ptr())
        u.her, u.batch, u.batch_size = ctypes.pointer(self.her), ctypes.pointer(self.batch), B
        u.draw_seed, u.draw_counter = 1, 2
        u.target = self.ptr()
        u.gamma, u.tau, u.n_critics, u.sigma, u.clip, u.policy_delay, u.update_index = 0.99, 0.005, nc, 0.2, 0.5, 2, 0
        self.policy = _actor(policy, obs_dim + 6, blob=None)                    # the policy's blob is not read
        self.policy_net = self.net(policy)
        self.policy_adam = _abi_ddpg.CtrDdpgAdam(1e-4, 0.9, 0.999, 1e-8)
        self.critic_adam = _abi_ddpg.CtrDdpgAdam(1e-3, 0.9, 0.999, 1e-8)
        u.policy, u.policy_net = ctypes.pointer(self.policy), ctypes.pointer(self.policy_net)
        u.policy_adam, u.critic_adam = ctypes.pointer(self.policy_adam), ctypes.pointer(self.critic_adam)
        self.actor_targ = _actor(policy, obs_dim + 6, blob=self.ptr())
        self.actor_targ_arrays = (self.layers(len(policy) + 1), self.layers(len(policy) + 1))
        u.actor_targ = ctypes.pointer(self.actor_targ)
        u.W_targ_actor, u.b_targ_actor = self.actor_targ_arrays
        self.actor = _actor(policy, obs_dim + 6, blob=self.ptr())
        if actor:
            u.actor = ctypes.pointer(self.actor)
        self.critic, self.critic_net, self.targ, self.targ_arrays = [], [], [], []
        for y, hidden in enumerate(critics[:nc]):
            self.critic.append(_critic(hidden, obs_dim + 12, blob=None))       # the online critics' blobs are not read
            self.critic_net.append(self.net(hidden))
            self.targ.append(_critic(hidden, obs_dim + 12, blob=self.ptr()))
            W, b = self.layers(len(hidden) + 1), self.layers(len(hidden) + 1)
            self.targ_arrays.append((W, b))
            u.critic[y], u.critic_net[y] = ctypes.pointer(self.critic[y]), ctypes.pointer(self.critic_net[y])
            u.critic_targ[y], u.W_targ[y], u.b_targ[y] = ctypes.pointer(self.targ[y]), W, b
        u.critic_loss, u.actor_loss = self.ptr(), self.ptr()
        u.workspace, u.workspace_bytes = self.ptr(), self.workspace_bytes(256)

    def ptr(self):
        return next(self._next) << 12

    def layers(self, n):
        arr = (self._abi._P * n)(*[self.ptr() for _ in range(n)])
        self.keep.append(arr)
        return arr

    def net(self, hidden):
        from ctr_reach_amd import _abi_ddpg
        s = _abi_ddpg.CtrDdpgNet()
        for field in ("W", "b", "gW", "gb", "mW", "mb", "vW", "vb"):
            setattr(s, field, self.layers(len(hidden) + 1))
        s.pow = self.ptr()
        return s

    def workspace_bytes(self, B):
        _, lib = _lib()
        if self.nc == 1:
            n = int(lib.ctr_ddpg_workspace_bytes(self.policy, self.critic[0], B))
        else:
            n = int(lib.ctr_td3_workspace_bytes(self.policy, self.critic[0], self.critic[1], B))
        assert n > 0
        return n

    def __call__(self, updates=2):
        _, lib = _lib()
        return lib.ctr_ddpg_update(self.u, updates, None), lib.ctr_last_error()


def _refused(word, change, updates=2, **kw):
    c = _Call(**kw)
    change(c)
    rc, msg = c(updates)
    assert rc == -1 and msg == word, (word, rc, msg)


def test_a_valid_call_passes_the_checks_only_as_a_no_op():
    """(with updates > 0 and B > 0 the call would launch on the fake pointers: not made here)"""
    for nc in (1, 2):
        assert _Call(nc=nc)(0)[0] == 0
        assert _Call(nc=nc, B=0)(3)[0] == 0
        assert _Call(nc=nc, B=0, obs_dim=14)(3)[0] == 0
        assert _Call(nc=nc, actor=False, B=0)(3)[0] == 0
        assert _Call(nc=nc, policy=(32,), critics=((256, 128), (128, 128, 128)))(0)[0] == 0
        assert _Call(nc=nc, policy=(64, 32), critics=((32, 64, 32), (96, 64)))(0)[0] == 0
        c = _Call(nc=nc)
        c.u.history = c.ptr()
        assert c(0)[0] == 0
        c = _Call(nc=nc, B=0)
        c.u.scale = c.ptr()
        c.u.critic_loss = c.u.actor_loss = None
        c.u.q1_next, c.u.next_action = c.ptr(), c.ptr()
        assert c(5)[0] == 0
        for tau in (0.0, 1.0):
            c = _Call(nc=nc, B=0)
            c.u.tau = tau
            assert c(1)[0] == 0
    # one critic: the second critic's fields, sigma and clip are not read
    c = _Call(nc=1, B=0)
    c.u.sigma, c.u.clip = float("nan"), -1.0
    c.u.q2_next = c.u.target
    assert c(1)[0] == 0
    c = _Call(nc=2, B=0)
    c.u.sigma, c.u.clip, c.u.policy_delay, c.u.update_index = 0.0, float("inf"), 1, 2 ** 64 - 1
    assert c(1)[0] == 0


def test_the_no_ops_are_still_checked():
    _refused(b"ctr_ddpg_update: target is NULL", _set("u.target", None), updates=0)
    _refused(b"ctr_ddpg_update: target is NULL", _set("u.target", None), B=0)
    _refused(b"ctr_ddpg_update: tau must be in [0, 1]", _set("u.tau", 1.5), updates=0)
    _refused(b"ctr_ddpg_update: policy_delay must be >= 1", _set("u.policy_delay", 0), B=0)


def test_refusals_of_the_call_itself():
    _, lib = _lib()
    assert lib.ctr_ddpg_update(None, 1, None) == -1
    assert lib.ctr_last_error() == b"ctr_ddpg_update: u is NULL"
    _refused(b"ctr_ddpg_update: updates must be >= 0", lambda c: None, updates=-1)
    for n in (0, 3, -1):
        _refused(b"ctr_ddpg_update: n_critics must be 1 (DDPG) or 2 (TD3)", _set("u.n_critics", n))
    for d in (0, -2):
        _refused(b"ctr_ddpg_update: policy_delay must be >= 1", _set("u.policy_delay", d))
        _refused(b"ctr_ddpg_update: policy_delay must be >= 1", _set("u.policy_delay", d), nc=1)


@pytest.mark.parametrize("nc", [1, 2])
def test_refusals_of_the_draw(nc):
    def refused(word, change):
        _refused(word, change, nc=nc)
    refused(b"ctr_ddpg_update: her is NULL", _set("u.her", None))
    refused(b"ctr_ddpg_update: bad batch", _set("u.batch", None))
    refused(b"ctr_ddpg_update: bad batch", _set("u.batch_size", -1))
    refused(b"ctr_ddpg_update: her: obs_dim must be 13 or 14", _set("her.obs_dim", 15))
    refused(b"ctr_ddpg_update: her: slots must be >= 2", _set("her.slots", 1))
    refused(b"ctr_ddpg_update: empty store", _set("her.n", 0))
    refused(b"ctr_ddpg_update: output missing", _set("batch.done", None))
    refused(b"ctr_ddpg_update: obs / next_obs / action must be 16-byte aligned", _set("batch.next_obs", (1 << 13) + 4))
    refused(b"ctr_ddpg_update: actor is NULL", _set("u.actor_targ", None))
    refused(b"ctr_ddpg_update: actor: n_hidden must be in 1..CTR_ACTOR_MAX_HIDDEN (3)", _set("actor_targ.n_hidden", 4))
    refused(b"ctr_ddpg_update: actor: every hidden width must be a multiple of 32 in 32..CTR_ACTOR_MAX_WIDTH (256)",
            lambda c: c.actor_targ.width.__setitem__(1, 48))
    refused(b"ctr_ddpg_update: actor: in_dim must be obs_dim + 6 = 19 or 20", _set("actor_targ.in_dim", 18))
    refused(b"ctr_ddpg_update: actor: blob is NULL", _set("actor_targ.blob", None))
    refused(b"ctr_ddpg_update: actor: blob must be 16-B aligned", _set("actor_targ.blob", (1 << 21) + 8))
    for y in range(nc):
        refused(b"ctr_ddpg_update: NULL entry in critic_targ[n_critics]", _layer("u.critic_targ", y, None))
        refused(b"ctr_ddpg_update: critic: n_hidden must be in 1..CTR_ACTOR_MAX_HIDDEN (3)",
                lambda c: setattr(c.targ[y], "n_hidden", 0))
        refused(b"ctr_ddpg_update: critic: every hidden width must be a multiple of 32 in 32..CTR_ACTOR_MAX_WIDTH (256)",
                lambda c: c.targ[y].width.__setitem__(0, 48))
        refused(b"ctr_ddpg_update: critic: blob is NULL", lambda c: setattr(c.targ[y], "blob", None))
        refused(b"ctr_ddpg_update: critic: blob must be 16-B aligned", lambda c: setattr(c.targ[y], "blob", (1 << 20) + 4))
        refused(b"ctr_ddpg_update: a critic_targ's in_dim must be her->obs_dim + 12", lambda c: setattr(c.targ[y], "in_dim", 26))
    refused(b"ctr_ddpg_update: actor_targ->in_dim must be her->obs_dim + 6", _set("her.obs_dim", 14))
    for g in (float("nan"), float("inf"), -float("inf")):
        refused(b"ctr_ddpg_update: gamma must be finite", _set("u.gamma", g))
    refused(b"ctr_ddpg_update: target is NULL", _set("u.target", None))


def test_refusals_of_the_smoothing():
    for s in (float("nan"), float("inf"), -0.1):
        _refused(b"ctr_ddpg_update: sigma must be finite and >= 0", _set("u.sigma", s))
    for cl in (float("nan"), -0.5):
        _refused(b"ctr_ddpg_update: clip must be >= 0 (INFINITY: no clip)", _set("u.clip", cl))


@pytest.mark.parametrize("nc", [1, 2])
def test_refusals_of_the_critics_step(nc):
    def refused(word, change):
        _refused(word, change, nc=nc)
    for y in range(nc):
        refused(b"ctr_ddpg_update: NULL entry in critic[n_critics] or critic_net[n_critics]", _layer("u.critic", y, None))
        refused(b"ctr_ddpg_update: NULL entry in critic[n_critics] or critic_net[n_critics]", _layer("u.critic_net", y, None))
        refused(b"ctr_ddpg_update: critic: n_hidden must be in 1..CTR_ACTOR_MAX_HIDDEN (3)",
                lambda c: setattr(c.critic[y], "n_hidden", 4))
        refused(b"ctr_ddpg_update: critic: in_dim must be obs_dim + 12 = 25 or 26", lambda c: setattr(c.critic[y], "in_dim", 24))
        for field in ("W", "b", "gW", "gb", "mW", "mb", "vW", "vb", "pow"):
            refused(b"ctr_ddpg_update: NULL pointer array or pow in net", lambda c: setattr(c.critic_net[y], field, None))
        refused(b"ctr_ddpg_update: NULL layer among W, b, gW, gb, mW, mb, vW, vb [0..n_hidden]",
                lambda c: c.critic_net[y].mW.__setitem__(1, None))
        refused(b"ctr_ddpg_update: a gradient or state tensor is a parameter tensor",
                lambda c: c.critic_net[y].vb.__setitem__(0, c.critic_net[y].W[1]))
    if nc == 2:
        refused(b"ctr_ddpg_update: the two critics must have the same in_dim", lambda c: setattr(c.critic[1], "in_dim", 26))
    refused(b"ctr_ddpg_update: adam is NULL", _set("u.critic_adam", None))
    finite = b"ctr_ddpg_update: lr, beta1, beta2 and eps must be finite"
    betas, eps = b"ctr_ddpg_update: beta1 and beta2 must be in [0, 1)", b"ctr_ddpg_update: eps must be positive"
    for field, bad, word in (("lr", float("nan"), finite), ("lr", float("inf"), finite), ("beta1", float("nan"), finite),
                             ("beta1", 1.0, betas), ("beta2", -0.1, betas), ("eps", 0.0, eps), ("eps", -1e-8, eps),
                             ("eps", float("nan"), finite)):
        refused(word, _set("critic_adam." + field, bad))
        refused(word, _set("policy_adam." + field, bad))
    refused(b"ctr_ddpg_update: B must be in 0..65536", _set("u.batch_size", 65537))
    refused(b"ctr_ddpg_update: workspace is NULL", _set("u.workspace", None))
    refused(b"ctr_ddpg_update: workspace must be 16-B aligned", _set("u.workspace", (1 << 30) + 8))
    # (one critic: the region's own check; two: the check of the two regions' sum)
    refused(b"ctr_ddpg_update: workspace too small (%s)" % (b"ctr_ddpg_workspace_bytes", b"ctr_td3_workspace_bytes")[nc - 1],
            lambda c: setattr(c.u, "workspace_bytes", c.workspace_bytes(8) - 16))
    refused(b"ctr_ddpg_update: workspace too small (ctr_ddpg_workspace_bytes)", _set("u.workspace_bytes", 1024))
    # the workspace is sized for the call's B: one for 8 rows does not serve 300
    refused(b"ctr_ddpg_update: workspace too small (ctr_ddpg_workspace_bytes)",
            lambda c: (setattr(c.u, "workspace_bytes", c.workspace_bytes(8)),
                                               setattr(c.u, "batch_size", 300)))


@pytest.mark.parametrize("nc", [1, 2])
def test_refusals_of_the_policys_step(nc):
    def refused(word, change, **kw):
        _refused(word, change, nc=nc, **kw)
    refused(b"ctr_ddpg_update: actor is NULL", _set("u.policy", None))
    refused(b"ctr_ddpg_update: actor: n_hidden must be in 1..CTR_ACTOR_MAX_HIDDEN (3)", _set("policy.n_hidden", 0))
    refused(b"ctr_ddpg_update: net is NULL", _set("u.policy_net", None))
    refused(b"ctr_ddpg_update: adam is NULL", _set("u.policy_adam", None))
    refused(b"ctr_ddpg_update: NULL layer among W, b, gW, gb, mW, mb, vW, vb [0..n_hidden]",
            lambda c: c.policy_net.gb.__setitem__(2, None))
    refused(b"ctr_ddpg_update: actor->in_dim + 6 must be critic->in_dim", _set("policy.in_dim", 20))


@pytest.mark.parametrize("nc", [1, 2])
def test_refusals_of_the_soft_update_the_targets_and_the_actor(nc):
    def refused(word, change, **kw):
        _refused(word, change, nc=nc, **kw)
    for tau in (float("nan"), -0.001, 1.001, float("inf")):
        refused(b"ctr_ddpg_update: tau must be in [0, 1]", _set("u.tau", tau))
    refused(b"ctr_ddpg_update: W_targ_actor or b_targ_actor is NULL", _set("u.W_targ_actor", None))
    refused(b"ctr_ddpg_update: W_targ_actor or b_targ_actor is NULL", _set("u.b_targ_actor", None))
    refused(b"ctr_ddpg_update: NULL layer among W_targ_actor, b_targ_actor [0..n_hidden]",
            lambda c: c.actor_targ_arrays[0].__setitem__(2, None))
    refused(b"ctr_ddpg_update: NULL layer among W_targ_actor, b_targ_actor [0..n_hidden]",
            lambda c: c.actor_targ_arrays[1].__setitem__(0, None))
    for y in range(nc):
        refused(b"ctr_ddpg_update: NULL entry in W_targ[n_critics] or b_targ[n_critics]", _layer("u.W_targ", y, None))
        refused(b"ctr_ddpg_update: NULL entry in W_targ[n_critics] or b_targ[n_critics]", _layer("u.b_targ", y, None))
        refused(b"ctr_ddpg_update: NULL layer among W_targ, b_targ [0..n_hidden]",
                lambda c: c.targ_arrays[y][0].__setitem__(0, None))
        refused(b"ctr_ddpg_update: NULL layer among W_targ, b_targ [0..n_hidden]",
                lambda c: c.targ_arrays[y][1].__setitem__(1, None))
    # a target has its online network's shape; so has the online actor
    refused(b"ctr_ddpg_update: a target critic's shape differs from its online critic's",
            lambda c: c.targ[0].width.__setitem__(1, 32))
    refused(b"ctr_ddpg_update: a target critic's shape differs from its online critic's",
            lambda c: c.targ[nc - 1].width.__setitem__(0, 128))
    refused(b"ctr_ddpg_update: the target policy's shape differs from the policy's",
            lambda c: c.actor_targ.width.__setitem__(0, 32))
    refused(b"ctr_ddpg_update: the target policy's shape differs from the policy's",
            lambda c: (setattr(c.actor_targ, "n_hidden", 1)))
    refused(b"ctr_ddpg_update: the online actor's shape differs from the policy's", lambda c: c.actor.width.__setitem__(1, 128))
    refused(b"ctr_ddpg_update: the online actor's shape differs from the policy's",
            lambda c: setattr(c.actor, "n_hidden", 3) or c.actor.width.__setitem__(2, 32))
    refused(b"ctr_ddpg_update: actor: blob is NULL", _set("actor.blob", None))
    refused(b"ctr_ddpg_update: actor: blob must be 16-B aligned", _set("actor.blob", (1 << 22) + 4))
    refused(b"ctr_ddpg_update: actor: in_dim must be obs_dim + 6 = 19 or 20", _set("actor.in_dim", 21))


@pytest.mark.parametrize("nc", [1, 2])
def test_refusals_of_shared_memory(nc):
    last = nc - 1

    def same(a, b, swap=False):
        """swap: with two critics the sort leaves the pair in the other order."""
        if swap and nc == 2:
            a, b = b, a
        return b"ctr_ddpg_update: " + a + b" and " + b + b" are the same memory"
    param, grad, targ, blob = b"a parameter tensor", b"a gradient tensor", b"a target tensor", b"a target critic's blob"
    pblob, ablob, ws, hist = b"the target policy's blob", b"the online actor's blob", b"the workspace", b"history"

    def refused(word, change, **kw):
        _refused(word, change, nc=nc, **kw)
    # a target tensor shared with an online one, between targets, with the policy
    refused(same(param, targ, True), lambda c: c.targ_arrays[0][0].__setitem__(0, c.critic_net[0].W[0]))
    refused(same(targ, param, True), lambda c: c.targ_arrays[last][1].__setitem__(0, c.critic_net[last].b[0]))
    refused(same(param, targ), lambda c: c.actor_targ_arrays[0].__setitem__(1, c.policy_net.W[1]))
    refused(same(targ, targ), lambda c: c.actor_targ_arrays[1].__setitem__(0, c.targ_arrays[last][1][0]))
    refused(same(param, targ), lambda c: c.targ_arrays[0][1].__setitem__(0, c.policy_net.b[0]))
    refused(same(b"a first-moment tensor", targ, True), lambda c: c.targ_arrays[0][1].__setitem__(0, c.critic_net[last].mb[0]))
    # the blobs
    refused(same(blob, pblob), lambda c: setattr(c.targ[0], "blob", c.actor_targ.blob))
    refused(same(ablob, pblob), lambda c: setattr(c.actor, "blob", c.actor_targ.blob))
    refused(same(blob, ablob), lambda c: setattr(c.actor, "blob", c.targ[last].blob))
    refused(same(param, pblob, True), lambda c: setattr(c.actor_targ, "blob", c.critic_net[0].W[0]))
    refused(same(b"a second-moment tensor", ablob), lambda c: setattr(c.actor, "blob", c.policy_net.vW[0]))
    # the steps' own: a critic tensor is the policy's, an output is a tensor
    refused(same(param, param), lambda c: c.critic_net[0].W.__setitem__(0, c.policy_net.W[0]))
    refused(same(b"critic_loss", b"actor_loss"), lambda c: setattr(c.u, "actor_loss", c.u.critic_loss))
    refused(same(b"a net's pow", b"actor_loss"), lambda c: setattr(c.u, "actor_loss", c.policy_net.pow))
    refused(same(b"batch->reward", b"target"), lambda c: setattr(c.u, "target", c.batch.reward))
    refused(same(b"q1_next", b"target"), lambda c: setattr(c.u, "q1_next", c.u.target))
    refused(same(b"batch->action", b"next_action"), lambda c: setattr(c.u, "next_action", c.batch.action))
    refused(same(b"scale", param), lambda c: setattr(c.u, "scale", c.critic_net[0].W[0]))
    refused(same(blob, ws, True), lambda c: setattr(c.u, "workspace", c.targ[0].blob))
    if nc == 2:
        refused(same(blob, blob), lambda c: setattr(c.targ[1], "blob", c.targ[0].blob))
        refused(same(targ, targ), lambda c: c.targ_arrays[1][0].__setitem__(1, c.targ_arrays[0][0][1]))
        refused(same(grad, grad), lambda c: c.critic_net[1].gW.__setitem__(0, c.critic_net[0].gW[0]))
        refused(same(b"a net's pow", b"a net's pow"), lambda c: setattr(c.critic_net[1], "pow", c.critic_net[0].pow))
        refused(same(b"q2_next", b"target"), lambda c: setattr(c.u, "q2_next", c.u.target))
    # history against every kind of output, at its first float and inside its rows
    for other, word in ((lambda c: c.u.target, same(hist, b"target")), (lambda c: c.u.critic_loss, same(b"critic_loss", hist)),
                        (lambda c: c.batch.obs, same(hist, b"batch->obs")), (lambda c: c.policy_net.W[0], same(param, hist)),
                        (lambda c: c.targ_arrays[last][0][0], same(hist, targ)),
                        (lambda c: c.actor_targ_arrays[1][0], same(hist, targ)), (lambda c: c.targ[0].blob, same(hist, blob, True)),
                        (lambda c: c.actor.blob, same(hist, ablob)), (lambda c: c.u.workspace, same(ws, hist))):
        refused(word, lambda c: setattr(c.u, "history", other(c)))
    row = 4 * (1 + nc)
    refused(same(hist, b"actor_loss"), lambda c: (setattr(c.u, "history", c.ptr()), setattr(c.u, "actor_loss", c.u.history + row)),
            updates=2)
    refused(same(hist, b"actor_loss"),
            lambda c: (setattr(c.u, "history", c.ptr()), setattr(c.u, "actor_loss", c.u.history + 2 * row - 1)), updates=2)
    # ... and what lies behind its rows is not its memory
    c = _Call(nc=nc, B=0)
    c.u.history = c.ptr()
    c.u.actor_loss = c.u.history + 2 * row
    assert c(2)[0] == 0


# --- the two update methods' own refusals, on stub objects ---------------------------------------------

def _stubs(nc):
    """A learner, a buffer, the nets and the targets that have only what the checks read, on the CPU."""
    import torch
    from ctr_reach_amd.learner import DdpgLearner, Td3Learner
    from ctr_reach_amd.policy import MlpActor, MlpCritic
    rng = np.random.default_rng(5)
    cpu = torch.device("cpu")
    scale = np.full(6, 0.5, np.float32)
    masters = _layers(rng, [19, 64, 6])
    critics = [_layers(rng, [25, 32, 1]), _layers(rng, [25, 64, 64, 1])][:nc]
    cls = DdpgLearner if nc == 1 else Td3Learner
    learner = cls.__new__(cls)
    learner.device, learner.max_batch, learner.in_dim = cpu, 256, 19
    learner._actor = types.SimpleNamespace(params=masters)
    nets = [types.SimpleNamespace(params=c) for c in critics]
    if nc == 1:
        learner._critic, learner._critic_struct = nets[0], None
    else:
        learner._critics, learner._critic_structs, learner.update_count = nets, (None, None), 0
    her = types.SimpleNamespace(venv=types.SimpleNamespace(device=cpu), obs_dim=13)
    owner = _layers(rng, [19, 64, 6])
    actor_targ = MlpActor(owner, scale, device="cpu")
    actor = MlpActor(masters, scale, device="cpu")
    owners = [_layers(rng, [25, 32, 1]), _layers(rng, [25, 64, 64, 1])][:nc]
    targets = [(actor_targ, owner)] + [(MlpCritic(o, device="cpu"), o) for o in owners]
    return learner, her, actor_targ, actor, targets


@pytest.mark.parametrize("nc", [1, 2])
def test_update_refuses_before_anything_is_converted_or_written(nc):
    import torch
    from ctr_reach_amd.policy import GaussianActor, MlpActor, MlpCritic
    learner, her, actor_targ, actor, targets = _stubs(nc)
    rng = np.random.default_rng(6)
    scale = np.full(6, 0.5, np.float32)

    def bad(match, her=her, actor_targ=actor_targ, targets=targets, B=8, gamma=0.99, tau=0.005, actor=actor, **kw):
        with pytest.raises(ValueError, match=exact(match)):
            learner.update(her, actor_targ, targets, B, gamma, tau, actor=actor, **kw)

    # the checks pass on the stubs as they are: the call then needs what a stub lacks
    with pytest.raises(AttributeError):
        learner.update(her, actor_targ, targets, 8, 0.99, 0.005, actor=actor)
    with pytest.raises(AttributeError):
        learner.update(her, actor_targ, targets, 8, 0.99, 0.005)
    bad("update: actor_targ must be an MlpActor, not GaussianActor",
        actor_targ=GaussianActor(_layers(rng, [19, 64, 12]), scale, device="cpu"))
    bad("update: actor must be an MlpActor or None, not MlpCritic", actor=targets[1][0])
    bad("update: actor and actor_targ are one MlpActor: each has its own blob", actor=actor_targ)
    shape = "update: targets is [(actor_targ, policy_targ), " + (
        "(critic_targ_dev, critic_targ)]" if nc == 1 else "(critic1_targ_dev, critic1_targ), (critic2_targ_dev, critic2_targ)]")
    bad(shape, targets=targets[:-1])
    bad(shape, targets=targets + [targets[-1]])
    bad(shape, targets=targets[:-1] + [(targets[-1][0],)])
    other = MlpActor(targets[0][1], scale, device="cpu")
    bad("update: targets[0] is (actor_targ, policy_targ): its net is not actor_targ",
        targets=[(other, targets[0][1])] + targets[1:])
    bad("update: target %d must be an MlpCritic, not MlpActor" % nc, targets=targets[:-1] + [(actor, targets[-1][1])])
    host = MlpActor(targets[0][1], scale, device=None)
    bad("update: the target policy must be on the device", actor_targ=host, targets=[(host, targets[0][1])] + targets[1:])
    bad("update: the target 1 must be on the device",
        targets=[targets[0], (MlpCritic(targets[1][1], device=None), targets[1][1])] + targets[2:])
    bad("update: the actor must be on the device", actor=MlpActor(learner._actor.params, scale, device=None))
    if nc == 2:
        bad("update: the two critic targets are one MlpCritic: each has its own blob", targets=[targets[0], targets[1], targets[1]])
        for s in (float("nan"), float("inf"), -0.1):
            bad("update: sigma must be finite and >= 0", sigma=s)
        for cl in (float("nan"), -0.5):
            bad("update: clip must be >= 0 (inf: the noise is not clipped)", clip=cl)
        for d in (0, -1):
            bad("update: policy_delay must be >= 1", policy_delay=d)
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
    # polyak_'s and load_'s checks of the tensors: shapes, dtype, contiguity, requires_grad
    narrow = _layers(rng, [19, 32, 6])
    narrow_targ = MlpActor(narrow, scale, device="cpu")
    bad("update: target policy: online layer 0: W must be [32, 19], not [64, 19]",
        actor_targ=narrow_targ, targets=[(narrow_targ, narrow)] + targets[1:])
    bad("update: the actor's layer 0: W must be [32, 19], not [64, 19]", actor=MlpActor(narrow, scale, device="cpu"))
    deep = _layers(rng, [25, 64, 64, 64, 1])
    bad("update: target 1: online the critic has 4 layers of (W, b)",
        targets=[targets[0], (MlpCritic(deep, device="cpu"), deep)] + targets[2:])
    wide = _layers(rng, [25, 64, 1])
    bad("update: target 1: online layer 0: W must be [64, 25], not [32, 25]",
        targets=[targets[0], (MlpCritic(wide, device="cpu"), wide)] + targets[2:])
    wrong = [(W.double(), b) for W, b in targets[0][1]]
    bad("update: target policy: target layer 0: W must be float32, not torch.float64", targets=[(actor_targ, wrong)] + targets[1:])
    wrong = [(W.t().contiguous().t(), b) for W, b in targets[-1][1]]
    bad("update: target %d: target layer 0: W must be contiguous" % nc, targets=targets[:-1] + [(targets[-1][0], wrong)])
    wrong = [(W.clone().requires_grad_(True), b) for W, b in targets[-1][1]]
    bad("update: target %d: target layer 0: W requires grad: a target is written in place, outside autograd" % nc,
        targets=targets[:-1] + [(targets[-1][0], wrong)])
    # history: float32, [updates, 1 + n_critics], contiguous, on the device
    cols = 1 + nc
    for h in (np.zeros((2, cols), np.float32), torch.zeros((2, cols), dtype=torch.float64), torch.zeros((3, cols)),
              torch.zeros(2 * cols), torch.zeros((cols, 2)).t(), torch.zeros((2, cols + 1))):
        bad("update: history must be a contiguous float32 [updates, %d] = [2, %d] tensor on cpu" % (cols, cols), updates=2,
            history=h)
    # nothing was dropped or set by a refused call
    for net in [actor] + [t[0] for t in targets]:
        assert net.weights is not None and net._sources is None
    assert not hasattr(her, "_counter")
    if nc == 2:
        assert learner.update_count == 0
