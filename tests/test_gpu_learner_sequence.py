"""DdpgLearner, Td3Learner and SacLearner as a training run keeps them: ONE learner, built for max_batch =
1 040, stepped at 1 040, 1, 17, 16, 300, 1 024, 15 and 1 040 rows, so that every step finds the workspace
as a step of another size left it (other slot counts, loss partials and advanced powers, and TD3's and
SAC's second region at another offset), or, before every other step, filled with the byte 0xFF, which
is a NaN as float32 and as float64.  tests/seq_ref.py makes the inputs and
tests/test_host_learner_sequence.py checks their conditions without a GPU.

A1: with real learning rates, every step of the long-lived learner is, bit for bit, the step of a fresh
learner built for exactly that size from copies of the networks and the state: the slots, the grid and
the order of summation are functions of B alone, so neither the history nor max_batch may show.

A2: with every learning rate 0, the gradients and losses at every size against float64 autograd of the
same prefix, under the bars of tests/test_gpu_ddpg_edges.py and tests/test_gpu_sac_edges.py (imported,
not restated): per tensor max|g - g64| / max|g64| at most 8 times torch float32's, the 2^-23 floor for
the losses, SAC's scalars and 1-element tensors only."""
import copy
import re
import types

import numpy as np
import pytest

import ddpg_ref as R
import sac_ref as S
import seq_ref as Q
import test_gpu_ddpg_edges as DE
import test_gpu_sac_adam as SA
import test_gpu_sac_edges as SE

pytestmark = pytest.mark.gpu

CASES = [(kind, i) for kind in ("ddpg", "td3", "sac") for i in (0, 1)]
IDS = ["%s-%d" % case for case in CASES]
SAC_SEED = 3                  # of the learners' noise in A1


def _poison(learner):
    learner.workspace.fill_(0xFF)


def _nets(learner):
    if hasattr(learner, "_critic"):
        return {"actor": learner._actor, "critic": learner._critic}
    return {"actor": learner._actor, "critic1": learner._critics[0], "critic2": learner._critics[1]}


def _snapshot(learner):
    """Everything a step writes, on the host: per network p, g, m, v, pow; the losses; SAC's scalars."""
    import torch
    torch.cuda.synchronize()
    out = {name: dict(p=R.host(net.params), g=R.host(net.grads), m=R.host(net.m), v=R.host(net.v), pow=net.pow.cpu().numpy().copy())
           for name, net in _nets(learner).items()}
    names = ["critic_loss", "actor_loss"] + (["logp_mean", "log_alpha", "alpha_state", "alpha_grad"] if hasattr(learner, "log_alpha") else [])
    out["scalars"] = {name: getattr(learner, name).cpu().numpy().copy() for name in names}
    return out


def _assert_same_and_finite(a, b, tag):
    """-> the number of float32 words compared."""
    words = 0
    assert set(a) == set(b)
    for name in a:
        if name == "scalars":
            continue
        for key in ("p", "g", "m", "v"):
            for l, (x, y) in enumerate(zip(a[name][key], b[name][key])):
                for which, s, t in zip("Wb", x, y):
                    assert np.isfinite(s).all() and np.isfinite(t).all(), (tag, name, key, which, l, "not finite")
                    bad = int((R.bits(s) != R.bits(t)).sum())
                    assert bad == 0, (tag, name, key, which, l, "%d of %d words differ" % (bad, s.size))
                    words += s.size
        assert np.isfinite(a[name]["pow"]).all()
        assert np.array_equal(R.bits(a[name]["pow"]), R.bits(b[name]["pow"])), (tag, name, "pow", a[name]["pow"], b[name]["pow"])
    for name, x in a["scalars"].items():
        y = b["scalars"][name]
        assert np.isfinite(x).all() and np.isfinite(y).all(), (tag, name, x, y)
        assert np.array_equal(R.bits(x), R.bits(y)), (tag, name, x, y)
        words += x.size
    return words


def _a1_inputs(kind, i, cuda):
    """(the three or two networks on the device, (rows, actions, target) on the device)."""
    if kind == "sac":
        policy, c1, c2, rows = Q.sac_case(i).made
        nets, batch = (policy, c1, c2), (rows,) + Q.sac_regression(i)
    elif kind == "td3":
        policy, c1, c2, rows, actions, target, _ = Q.td3_case(i)
        nets, batch = (policy, c1, c2), (rows, actions, target)
    else:
        policy, critic, rows, actions, target = Q.ddpg_case(i).made
        nets, batch = (policy, critic), (rows, actions, target)
    return tuple(R.to_device(n, cuda) for n in nets), tuple(t.to(cuda) for t in batch)


def _build(kind, nets, max_batch):
    from ctr_reach_amd.learner import DdpgLearner, SacLearner, Td3Learner
    rates = dict(actor_lr=SA.RATES["actor_lr"], critic_lr=SA.RATES["critic_lr"])
    if kind == "sac":
        return SacLearner(*nets, init_alpha=S.ALPHA, alpha_lr=SA.RATES["alpha_lr"], seed=SAC_SEED, max_batch=max_batch, **rates)
    return (Td3Learner if kind == "td3" else DdpgLearner)(*nets, max_batch=max_batch, **rates)


def _step(kind, learner, batch, B, k):
    rows, actions, target = (t[:B] for t in batch)
    learner.critic_step(rows, actions, target)
    if kind == "sac":
        learner.actor_step(rows, counter=k)
    else:
        learner.actor_step(rows)


# --- A1 ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,i", CASES, ids=IDS)
def test_a_step_does_not_depend_on_the_learners_history_or_max_batch(cuda, capsys, kind, i):
    nets, batch = _a1_inputs(kind, i, cuda)
    long = _build(kind, nets, Q.MAX_BATCH)
    assert long.workspace.numel() > _build(kind, tuple(copy.deepcopy(n) for n in nets), 1).workspace.numel()
    words, before = 0, _snapshot(long)
    for k, B in enumerate(Q.SIZES):
        fresh = _build(kind, tuple(copy.deepcopy(n) for n in nets), B)
        fresh.load_state_dict(long.state_dict())
        assert fresh.max_batch == B and fresh.workspace.data_ptr() != long.workspace.data_ptr()
        if k % 2:
            _poison(long)
        _step(kind, long, batch, B, k)
        _step(kind, fresh, batch, B, k)
        after = _snapshot(long)
        words += _assert_same_and_finite(after, _snapshot(fresh), (kind, i, "step", k, "B", B))
        # the step was one: every network learned, and Adam's powers advanced
        for name in after:
            if name != "scalars":
                assert not np.array_equal(after[name]["p"][0][0], before[name]["p"][0][0]), (k, name)
                assert after[name]["pow"][0] < before[name]["pow"][0], (k, name)
        before = after
    assert np.array_equal(R.bits(after["actor"]["pow"]), R.bits(Q.pow_after(len(Q.SIZES))))
    with capsys.disabled():
        print("\nA1 %s %d: %d steps, %d float32 words bit-equal to a fresh learner of max_batch = B" % (kind, i, len(Q.SIZES), words))


# --- A2 ----------------------------------------------------------------------------------------------------

_FIGURES = re.compile(r"^(.*) ([0-9.eE+-]+|nan|inf) \(torch f32 ([0-9.eE+-]+)\)$")


def _worst(report, failed):
    """(the largest kernel / torch-float32 ratio of a ``test_gpu_ddpg_edges._compare`` report, its name, how many
    entries passed by the 2^-23 floor: a loss or a 1-element tensor more than 8 times torch's error away, which
    that module's bar admits and which the ratio leaves out)."""
    worst, floored = (0.0, ""), 0
    for line in report:
        name, ours, theirs = _FIGURES.match(line).groups()
        ours, theirs = float(ours), float(theirs)
        if line not in failed and ours > 8 * theirs:
            floored += 1
        elif theirs > 0:
            worst = max(worst, (ours / theirs, name))
    return worst + (floored,)


def _walk_ddpg(kind, i, cuda, capsys):
    import torch
    from ctr_reach_amd.learner import DdpgLearner, Td3Learner
    if kind == "td3":
        policy, critic1, critic2, rows, actions, target, _ = Q.td3_case(i)
        learner = Td3Learner(*(R.to_device(n, cuda) for n in (policy, critic1, critic2)), actor_lr=0.0, critic_lr=0.0,
                             max_batch=Q.MAX_BATCH)
    else:
        policy, critic1, rows, actions, target = Q.ddpg_case(i).made
        learner = DdpgLearner(R.to_device(policy, cuda), R.to_device(critic1, cuda), actor_lr=0.0, critic_lr=0.0,
                              max_batch=Q.MAX_BATCH)
    d_rows, d_actions, d_target = (t.to(cuda) for t in (rows, actions, target))
    failed = []
    for k, B in enumerate(Q.SIZES):
        if k % 2:
            _poison(learner)
        learner.critic_step(d_rows[:B], d_actions[:B], d_target[:B])
        learner.actor_step(d_rows[:B])
        torch.cuda.synchronize()
        if kind == "td3":
            (one64, one32), (two64, two32) = Q.td3_refs(i, B)
            planes = [types.SimpleNamespace(critic_loss=learner.critic_loss[y], critic_grads=learner.critic_grads[y],
                                            actor_loss=learner.actor_loss, actor_grads=learner.actor_grads) for y in (0, 1)]
            report, bad = DE._compare(planes[0], one64, one32, ("critic", "actor"))
            report2, bad2 = DE._compare(planes[1], two64, two32, ("critic",))
            report, bad = report + ["critic 2's " + line for line in report2], bad + ["critic 2's " + line for line in bad2]
        else:
            report, bad = DE._compare(learner, *Q.ddpg_refs(i, B), ("critic", "actor"))
        ratio, name, floored = _worst(report, bad)
        with capsys.disabled():
            print("\nA2 %s %d, step %d, B %d%s: %s; worst ratio %.2f (%s), %d by the floor"
                  % (kind, i, k, B, ", poisoned" if k % 2 else "", "; ".join(report), ratio, name, floored))
        failed += [(k, B, line) for line in bad]
    assert not failed, failed
    if kind == "td3":
        DE._assert_unmoved(types.SimpleNamespace(_actor=learner._actor, _critic=learner._critics[0]), policy, critic1)
        DE._assert_unmoved(types.SimpleNamespace(_actor=learner._actor, _critic=learner._critics[1]), policy, critic2)
    else:
        DE._assert_unmoved(learner, policy, critic1)
    return learner


def _walk_sac(i, cuda, capsys):
    clear = Q.sac_case(i)
    learner = SE._learner(clear.made, cuda, Q.MAX_BATCH)
    rows = clear.made[3].to(cuda)
    failed = []
    for k, B in enumerate(Q.SIZES):
        if k % 2:
            _poison(learner)
        learner.actor_step(rows[:B], counter=0)
        ref64, ref32 = Q.sac_refs(i, B)
        bad = SE._compare(SE._snapshot(learner), ref64, ref32, "A2 sac %d, step %d, B %d%s" % (i, k, B, ", poisoned" if k % 2 else ""),
                          capsys)
        failed += [(k, B, line) for line in bad]
    assert not failed, failed
    SE._frozen(learner, clear.made)
    return learner


@pytest.mark.parametrize("kind,i", CASES, ids=IDS)
def test_the_gradients_at_every_size_against_float64_autograd(cuda, capsys, kind, i):
    learner = _walk_sac(i, cuda, capsys) if kind == "sac" else _walk_ddpg(kind, i, cuda, capsys)
    # the rates are 0 and Adam's state still advanced, once per step and network
    want = Q.pow_after(len(Q.SIZES))
    stepped = {name: net for name, net in _nets(learner).items() if kind != "sac" or name == "actor"}
    for name, net in stepped.items():
        assert np.array_equal(R.bits(net.pow.cpu().numpy()), R.bits(want)), (name, net.pow.cpu().numpy(), want)
        assert all(np.isfinite(t.cpu().numpy()).all() and t.any() for pair in net.m + net.v for t in pair), name
    if kind == "sac":
        state = learner.alpha_state.cpu().numpy()
        assert np.array_equal(R.bits(state[2:]), R.bits(want)) and np.isfinite(state).all() and state[:2].all()
        for net in learner._critics:                      # the policy's step only reads them
            assert net.pow.cpu().tolist() == [1.0, 1.0]
