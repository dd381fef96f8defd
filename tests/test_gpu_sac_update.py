"""SacLearner.update (ctr_sac_update: a run of SAC updates from one call) against the five-call eager
sequence it replaces,

    her.sample_sac -> learner.critic_step -> learner.actor_step -> pi.load_ -> polyak_

made on a second, identically built and identically seeded set of objects (never by the call under
test).  Everything those calls write is compared as bits: the policy's and both critics' parameters,
gradients, m, v and pow; log_alpha, its state and gradient; the target critics' float32 tensors; the
three blobs; the batch and target tensors and the four loss scalars of the last update; the two
counters; and the history rows against the eager scalars cloned after each eager update."""
import types

import numpy as np
import pytest

from test_gpu_collect import HER_KEYS

pytestmark = pytest.mark.gpu

GAMMA = 0.98
HIDDEN = dict(policy=(64, 32), critic1=(32,), critic2=(64, 64))      # the critics differ: the tail's planes too
BATCH_KEYS = ("obs", "action", "reward", "next_obs", "done", "target")
NEXT_KEYS = ("q1_next", "q2_next", "next_action", "next_logp")


def _mlp(n_in, hidden, n_out):
    import torch.nn as nn
    dims = [n_in] + list(hidden)
    mods = []
    for a, b in zip(dims[:-1], dims[1:]):
        mods += [nn.Linear(a, b), nn.ReLU()]
    mods.append(nn.Linear(dims[-1], n_out))
    return nn.Sequential(*mods)


def _world(cuda, systems=(0,), collect=12, scale=True, **learner_kw):
    """A 300-env store of 10-step episodes in 4 slots (1 200 entries: two scan tiles, one partial), filled by
    one short collect_gauss, and a SAC learner with its device networks; the same arguments give the same
    world, bit for bit."""
    import torch
    from ctr_reach_amd import CtrReachVecEnv
    from ctr_reach_amd.learner import SacLearner
    from ctr_reach_amd.policy import GaussianActor, MlpCritic
    torch.manual_seed(11)
    venv = CtrReachVecEnv(300, device=cuda, seed=7, select_systems=list(systems), max_steps_per_episode=10, refill_interval=4)
    venv.goal_tolerance.current_tol = 0.03
    her = venv.enable_her(slots=4)
    venv.reset()
    g = torch.Generator(device="cpu")
    g.manual_seed(3)
    venv.t.copy_(torch.randint(0, 10, (300,), generator=g, dtype=torch.int32))       # episodes close from the first steps on
    d = venv.obs_dim + 6
    policy = _mlp(d, HIDDEN["policy"], 12).to(cuda).requires_grad_(False)
    critics = [_mlp(d + 6, HIDDEN[k], 1).to(cuda).requires_grad_(False) for k in ("critic1", "critic2")]
    targets = [_mlp(d + 6, HIDDEN[k], 1).to(cuda).requires_grad_(False) for k in ("critic1", "critic2")]
    for c, t in zip(critics, targets):
        t.load_state_dict(c.state_dict())
        for p in t.parameters():                       # targets that differ from their critics: the lerp has work
            p.mul_(0.75)
    learner = SacLearner(policy, critics[0], critics[1], scale=venv.action_space.high if scale else None, max_batch=1040,
                         seed=5, **learner_kw)
    pi = GaussianActor.from_torch(policy, venv.action_space.high, cuda, seed=5)
    targ_dev = [MlpCritic.from_torch(t, cuda) for t in targets]
    w = types.SimpleNamespace(venv=venv, her=her, policy=policy, critics=critics, targets=targets, learner=learner, pi=pi,
                              targ_dev=targ_dev, step=0)
    if collect:
        _collect(w, collect)
    return w


def _collect(w, steps):
    w.venv.collect_gauss(w.pi, steps, counter=w.step)
    w.step += steps


def _scalars(learner):
    import torch
    return torch.stack([learner.critic_loss[0], learner.critic_loss[1], learner.actor_loss, learner.logp_mean,
                        learner.log_alpha]).clone()


def _eager(w, B, updates, tau, return_next=False):
    """The five calls, ``updates`` times -> (the last batch, the scalars after each update [updates, 5])."""
    import torch
    from ctr_reach_amd.policy import polyak_
    rows, batch = [], None
    for _ in range(updates):
        batch = w.her.sample_sac(B, w.pi, w.targ_dev[0], w.targ_dev[1], GAMMA, w.learner.log_alpha, return_next=return_next)
        w.learner.critic_step(batch["obs"], batch["action"], batch["target"])
        w.learner.actor_step(batch["obs"])
        w.pi.load_(w.policy)
        polyak_([(w.targ_dev[0], w.critics[0], w.targets[0]), (w.targ_dev[1], w.critics[1], w.targets[1])], tau)
        rows.append(_scalars(w.learner))
    return batch, torch.stack(rows)


def _update(w, B, updates, tau, return_next=False, history=True):
    import torch
    hist = torch.full((updates, 5), float("nan"), dtype=torch.float32, device=w.learner.device) if history else None
    out = w.learner.update(w.her, w.pi, list(zip(w.targ_dev, w.targets)), B, GAMMA, tau, updates=updates, history=hist,
                           return_next=return_next)
    return out, hist


def _tensors(w, batch):
    """name -> tensor, for everything the contract names."""
    L = w.learner
    out = {}
    for name, net in (("policy", L._actor), ("critic1", L._critics[0]), ("critic2", L._critics[1])):
        for kind, layers in (("p", net.params), ("g", net.grads), ("m", net.m), ("v", net.v)):
            for l, (W, b) in enumerate(layers):
                out["%s.%s.W%d" % (name, kind, l)], out["%s.%s.b%d" % (name, kind, l)] = W, b
        out[name + ".pow"] = net.pow
    for name in ("log_alpha", "alpha_state", "alpha_grad", "critic_loss", "actor_loss", "logp_mean"):
        out[name] = getattr(L, name)
    for y, t in enumerate(w.targets):
        for i, p in enumerate(t.parameters()):
            out["target%d.%d" % (y + 1, i)] = p
        out["target%d.blob" % (y + 1)] = w.targ_dev[y].blob
    out["policy.blob"] = w.pi.blob
    for k, v in batch.items():
        if k != "history":
            out["batch." + k] = v
    return out


def _same(a, b, batch_a, batch_b, where):
    """a: the eager world, b: the world under test.  -> the number of tensors compared."""
    import torch
    torch.cuda.synchronize()
    ta, tb = _tensors(a, batch_a), _tensors(b, batch_b)
    assert sorted(ta) == sorted(tb), where
    for name in ta:
        x, y = ta[name].detach(), tb[name].detach()
        assert x.shape == y.shape and x.dtype == y.dtype, (where, name)
        if x.dtype == torch.float32:
            x, y = x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)
        bad = int((x != y).sum().item())
        assert bad == 0, (where, name, "%d of %d words differ" % (bad, x.numel()))
    assert a.her._counter == b.her._counter and a.learner.counter == b.learner.counter, where
    return len(ta)


def _same_history(rows, hist, where):
    import torch
    assert torch.equal(rows.view(torch.int32), hist.view(torch.int32)), (where, rows, hist)


def _check(a, b, B, updates, tau=0.005, return_next=False, where=""):
    batch_a, rows = _eager(a, B, updates, tau, return_next)
    batch_b, hist = _update(b, B, updates, tau, return_next)
    keys = BATCH_KEYS + (NEXT_KEYS if return_next else ())
    assert sorted(batch_b) == sorted(keys + ("history",)) and sorted(batch_a) == sorted(keys), where
    _same(a, b, batch_a, batch_b, where)
    _same_history(rows, hist, where)
    return rows


# --- 1, 2: the base cases ----------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [17, 1040], ids=["one_tile_and_a_row", "64_slots_and_a_tile"])
def test_three_updates_are_the_five_calls_three_times(cuda, B):
    import torch
    a, b = _world(cuda), _world(cuda)
    assert a.pi.in_dim == 19 and a.her.len.numel() == 1200 and len(a.her) > 0
    before = a.policy[0].weight.clone()
    rows = _check(a, b, B, 3, where="B %d" % B)
    # the updates were updates: the draws and the losses differ from one to the next, everything learned
    assert len({tuple(r.tolist()) for r in rows}) == 3 and bool(torch.isfinite(rows).all())
    assert not torch.equal(before, b.policy[0].weight)
    assert b.learner._critics[1].pow.tolist() == a.learner._actor.pow.tolist() and b.learner._actor.pow[0].item() < 0.75
    assert b.pi._sources is not None and b.pi.weights is None
    assert all(net._sources is not None and net.weights is None for net in b.targ_dev)
    assert b.her._log_alpha is b.learner.log_alpha
    # the returned tensors are reused: the next call writes the same memory
    first = b.learner.update(b.her, b.pi, list(zip(b.targ_dev, b.targets)), B, GAMMA, 0.005)
    allocated = torch.cuda.memory_allocated()
    again = b.learner.update(b.her, b.pi, list(zip(b.targ_dev, b.targets)), B, GAMMA, 0.005)
    assert torch.cuda.memory_allocated() == allocated
    assert all(first[k].data_ptr() == again[k].data_ptr() for k in BATCH_KEYS) and "history" not in again
    _eager(a, B, 2, 0.005)
    _same(a, b, {}, {}, "two single-update calls without history")


def test_the_20_float_row(cuda):
    a, b = _world(cuda, systems=(0, 1, 2, 3)), _world(cuda, systems=(0, 1, 2, 3))
    assert a.pi.in_dim == 20
    _check(a, b, 16, 2, where="multi-system")


# --- 3: the counters -----------------------------------------------------------------------------------------

def test_both_counters_are_64_bit_sums_that_wrap(cuda):
    a, b = _world(cuda), _world(cuda)
    for w in (a, b):
        w.her._counter = 2 ** 32 - 1                     # the low word wraps inside the call
        w.learner.counter = 2 ** 64 - 2                  # the sum wraps to 0 for the last update
    _check(a, b, 17, 3, where="counters")
    assert b.her._counter == 2 ** 32 + 2 and b.learner.counter == 2 ** 64 + 1


# --- 4: the store changes between two calls ----------------------------------------------------------------

def test_the_scans_are_made_by_every_call(cuda):
    import torch
    a, b = _world(cuda), _world(cuda)
    _check(a, b, 17, 2, where="first call")
    rows_before = len(b.her)
    epoch = b.her.epoch.clone()
    for w in (a, b):
        _collect(w, 12)                                  # episodes close and enter the store, slots are reused
    assert len(b.her) != rows_before and bool((b.her.epoch != epoch).any())
    for k in HER_KEYS:
        assert torch.equal(getattr(a.her, k).view(torch.uint8), getattr(b.her, k).view(torch.uint8)), k
    _check(a, b, 17, 2, where="second call, after 12 more steps")


# --- 5: the switches ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw,tau,return_next", [
    (dict(learn_alpha=False), 0.005, False), (dict(scale=False), 0.005, False), ({}, 0.0, False), ({}, 0.6, False),
    ({}, 1.0, False), ({}, 0.005, True)], ids=["learn_alpha_off", "no_scale", "tau_0", "tau_0.6", "tau_1", "return_next"])
def test_the_switches(cuda, kw, tau, return_next):
    import torch
    a, b = _world(cuda, **kw), _world(cuda, **kw)
    la = b.learner.log_alpha.clone()
    rows = _check(a, b, 17, 2, tau=tau, return_next=return_next, where=str((kw, tau, return_next)))
    if kw.get("learn_alpha") is False:
        assert torch.equal(b.learner.log_alpha, la) and b.learner.alpha_state.tolist() == [0.0, 0.0, 1.0, 1.0]
        assert rows[:, 4].tolist() == [la.item()] * 2
    else:
        assert not torch.equal(b.learner.log_alpha, la)
    if tau == 1.0:
        for c, t in zip(b.critics, b.targets):
            assert all(torch.equal(p, q) for p, q in zip(c.parameters(), t.parameters()))


def test_the_seed_and_the_target_entropy_are_read_on_every_call(cuda):
    """actor_step reads learner.seed and learner.target_entropy per call; the cached struct must too."""
    import torch
    a, b = _world(cuda), _world(cuda)
    _check(a, b, 17, 1, where="as built")
    grad = b.learner.alpha_grad.clone()
    for w in (a, b):
        w.learner.seed = 12345
        w.learner.target_entropy = -3.0
    _check(a, b, 17, 2, where="another seed and target entropy")
    assert not torch.equal(grad, b.learner.alpha_grad)


# --- 6: the call only reads the store -----------------------------------------------------------------------

def test_the_call_only_reads_the_store(cuda):
    import torch
    b = _world(cuda)
    before = {k: getattr(b.her, k).clone() for k in HER_KEYS}
    _update(b, 1040, 2, 0.005)
    torch.cuda.synchronize()
    for k in HER_KEYS:
        assert torch.equal(before[k].view(torch.uint8), getattr(b.her, k).view(torch.uint8)), k


# --- 7: the empty store -------------------------------------------------------------------------------------

def test_an_empty_store(cuda):
    import torch
    a, b = _world(cuda, collect=0), _world(cuda, collect=0)
    assert len(b.her) == 0
    _check(a, b, 17, 2, where="empty store")
    torch.cuda.synchronize()
    assert not b.learner.update(b.her, b.pi, list(zip(b.targ_dev, b.targets)), 17, GAMMA, 0.005, updates=0)["obs"].any()


# --- 8: a captured call -------------------------------------------------------------------------------------

def test_a_captured_call_replays_as_an_eager_call_with_its_counters(cuda):
    """The counters are arguments of the captured call: a replay repeats its draws (and its noise), on
    whatever the networks hold then.  One replay after the capture is the eager updates with the counters
    the call was captured with."""
    import torch
    a, b = _world(cuda), _world(cuda)
    _eager(a, 17, 2, 0.005)
    _update(b, 17, 2, 0.005)                                           # (the kernels' first launch is not the captured one)
    torch.cuda.synchronize()
    hist = torch.zeros((2, 5), dtype=torch.float32, device=cuda)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                      # a synchronisation or an allocation in here raises
        out = b.learner.update(b.her, b.pi, list(zip(b.targ_dev, b.targets)), 17, GAMMA, 0.005, updates=2, history=hist)
    assert b.her._counter == 4 and b.learner.counter == 4
    graph.replay()
    torch.cuda.synchronize()
    batch, rows = _eager(a, 17, 2, 0.005)
    _same(a, b, batch, out, "replayed")
    _same_history(rows, hist, "replayed")
