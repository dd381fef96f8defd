"""DdpgLearner's and Td3Learner's gradients where training takes the kernels and
tests/test_gpu_ddpg_grads.py does not: several tiles per workspace slot on every shape, a saturated
policy, and exact gradients for both steps, every shape and TD3's two planes.  tests/ddpg_ref.py makes
the inputs and tests/test_host_ddpg_ref.py checks their conditions without a GPU.

Against float64 autograd the rule is test_gpu_ddpg_grads.py's: per tensor err = max|g - g64| /
max|g64|, the bar 8 times the same quantity of torch's float32 CPU autograd, lr = 0.  For the two
losses and for 1-element tensors the bar is max(8 x torch's, 2^-23): float32's spacing is between
2^-24 and 2^-23 of the value, so a neighbour of the correctly rounded float passes even where torch
happens to hit the float64 value.  The matrices get no floor.

On small integers (``ddpg_ref.integer_case``) every product and partial sum of either step is an
integer multiple of 1 / B far below 2^24 of them, so the kernels' order of summation gives float64's
result exactly, and an element in the wrong place, counted twice or left out does not."""
import numpy as np
import pytest

import ddpg_ref as R

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -23


def _learner(policy, critic, cuda, max_batch):
    from ctr_reach_amd.learner import DdpgLearner
    return DdpgLearner(R.to_device(policy, cuda), R.to_device(critic, cuda), actor_lr=0.0, critic_lr=0.0, max_batch=max_batch)


def _err(g, g64):
    return float(np.abs(g.astype(np.float64) - g64).max() / np.abs(g64).max())


def _compare(learner, ref64, ref32, names):
    """(report, failed) of the losses and gradients of ``names`` (of "critic", "actor") under the bars."""
    report, failed = [], []
    for name in names:
        want = ref64[name + "_loss"]
        ours = abs(float(getattr(learner, name + "_loss")) - want) / abs(want)
        theirs = abs(ref32[name + "_loss"] - want) / abs(want)
        report.append("%s loss %.3g (torch f32 %.3g)" % (name, ours, theirs))
        if not ours <= max(8 * theirs, FLOOR):
            failed.append(report[-1])
        got = R.host(getattr(learner, name + "_grads"))
        assert len(got) == len(ref64[name + "_grads"])
        for l, (pair, pair64, pair32) in enumerate(zip(got, ref64[name + "_grads"], ref32[name + "_grads"])):
            for which, g, g64, g32 in zip("Wb", pair, pair64, pair32):
                assert g.shape == g64.shape and np.isfinite(g).all()
                ours, theirs = _err(g, g64), _err(g32, g64)
                report.append("%s g%s[%d] %.3g (torch f32 %.3g)" % (name, which, l, ours, theirs))
                if not ours <= (max(8 * theirs, FLOOR) if g.size == 1 else 8 * theirs):
                    failed.append(report[-1])
    return report, failed


def _assert_unmoved(learner, policy, critic):
    for net, start in ((learner._actor, policy), (learner._critic, critic)):
        for (W, b), (W0, b0) in zip(R.host(net.params), R.host(R.params(start))):
            assert np.array_equal(R.bits(W), R.bits(W0)) and np.array_equal(R.bits(b), R.bits(b0))


@pytest.mark.parametrize("a_hidden,c_hidden,in_dim,B", R.CLEAR_CASES)
def test_several_tiles_per_slot_against_float64_autograd(cuda, capsys, a_hidden, c_hidden, in_dim, B):
    import torch
    clear = R.case_clear(a_hidden, c_hidden, in_dim, B)
    policy, critic, rows, actions, target = clear.made
    assert clear.ref64["kink"] >= 1e-5 and clear.redrawn <= 0.15 * B and clear.passes <= 20
    learner = _learner(policy, critic, cuda, B)
    d_rows, d_actions, d_target = (t.to(cuda) for t in (rows, actions, target))
    learner.critic_step(d_rows, d_actions, d_target)
    learner.actor_step(d_rows)
    torch.cuda.synchronize()
    report, failed = _compare(learner, clear.ref64, clear.ref32, ("critic", "actor"))
    with capsys.disabled():
        print("\nclear %s / %s, in_dim %d, B %d, redrawn %d in %d passes, kink %.3g: %s"
              % (list(a_hidden), list(c_hidden), in_dim, B, clear.redrawn, clear.passes, clear.ref64["kink"], "; ".join(report)))
    assert not failed, failed
    _assert_unmoved(learner, policy, critic)


@pytest.mark.parametrize("a_hidden,c_hidden,in_dim,B", R.SATURATED_CASES)
def test_a_saturated_policy_against_float64_autograd(cuda, capsys, a_hidden, c_hidden, in_dim, B):
    """The policy's output layer times 100: the actions that round to +-1.0f have 1 - a * a exactly
    zero in the kernel and about 1e-8 or less in float64, those near it are a cancellation."""
    import torch
    clear = R.case_clear(a_hidden, c_hidden, in_dim, B, R.GAIN)
    policy, critic, rows, actions, target = clear.made
    assert clear.ref64["kink"] >= 1e-5 and clear.redrawn <= 0.15 * B and clear.passes <= 20
    pi = R.actions64(policy, rows)
    one, low = float((np.abs(pi.astype(np.float32)) == 1).mean()), float((np.abs(pi) < 0.9).mean())
    assert one >= 0.05 and low >= 0.05
    assert all(np.abs(g).max() > 0 for pair in clear.ref64["actor_grads"] for g in pair)
    learner = _learner(policy, critic, cuda, B)
    learner.actor_step(rows.to(cuda))
    torch.cuda.synchronize()
    report, failed = _compare(learner, clear.ref64, clear.ref32, ("actor",))
    with capsys.disabled():
        print("\nsaturated %s / %s, in_dim %d, B %d, redrawn %d in %d passes, +-1.0f %.3f, below 0.9 %.3f: %s"
              % (list(a_hidden), list(c_hidden), in_dim, B, clear.redrawn, clear.passes, one, low, "; ".join(report)))
    assert not failed, failed
    _assert_unmoved(learner, policy, critic)


def _assert_integer_conditions(one, names):
    assert one.report["integral"] and one.report["bound"] < 2 ** 24
    for name in names:
        assert one.ref64[name + "_loss"] != 0
        assert all(np.count_nonzero(g) >= 0.01 * g.size for pair in one.ref64[name + "_grads"] for g in pair)
    if "actor" in names:
        pi = one.report["pi"]
        assert (pi == 0).mean() >= 0.02 and (np.abs(pi) == 1).mean() >= 0.02


def _assert_exact(loss, grads, ref64, name, tag):
    assert np.array_equal(np.float64(loss), np.float64(ref64[name + "_loss"])), (tag, name, "loss", float(loss))
    assert len(grads) == len(ref64[name + "_grads"])
    for l, (pair, pair64) in enumerate(zip(grads, ref64[name + "_grads"])):
        for which, g, g64 in zip("Wb", pair, pair64):
            assert g.shape == g64.shape
            assert np.array_equal(g.astype(np.float64), g64), (tag, name, which, l, int((g.astype(np.float64) != g64).sum()))


@pytest.mark.parametrize("case", R.INTEGER_CASES, ids=lambda c: "%s-%s-%d-%d" % ("x".join(map(str, c[0])), "x".join(map(str, c[1])), c[2], c[3]))
def test_integer_data_makes_both_steps_exact(cuda, case):
    """The critic's and the policy's step on every shape (B = 2 048 and 4 096: two and four tiles in
    every slot), at B = 1 024, the last batch with one tile in every slot, and at B = 65 536, the
    largest, with 64.  The policy's output layer is multiplied by 20, so that every action is exactly
    0 (which carries gradient) or +-1 (which carries none)."""
    import torch
    one = R.integer_case(*case)
    policy, critic, rows, actions, target = one.made
    B = case[3]
    _assert_integer_conditions(one, ("critic", "actor"))
    learner = _learner(policy, critic, cuda, B)
    d_rows = rows.to(cuda)
    learner.critic_step(d_rows, actions.to(cuda), target.to(cuda))
    learner.actor_step(d_rows)
    torch.cuda.synchronize()
    _assert_exact(learner.critic_loss.cpu().numpy(), R.host(learner.critic_grads), one.ref64, "critic", B)
    _assert_exact(learner.actor_loss.cpu().numpy(), R.host(learner.actor_grads), one.ref64, "actor", B)
    _assert_unmoved(learner, policy, critic)


def test_one_whole_extra_tile_in_slot_0_against_float64_autograd(cuda, capsys):
    """B = 1 040: slot 0 alone gets a second tile, a whole one.  1 040 is no power of two, so 2 / B and
    1 / B are rounded and this is NOT an exact comparison: the integer rows (the B = 1 024 case and its
    first tile again) are held to float64 autograd under the bars of the float cases.  The exact
    statement near this size is tests/test_gpu_td3_step.py's bit comparison at B = 1 029."""
    import torch
    (policy, critic, rows, actions, target), ref64, ref32 = R.integer_tail_case(*R.TAIL_CASE)
    B = R.T * R.SLOTS + R.T
    assert len(rows) == B
    learner = _learner(policy, critic, cuda, B)
    d_rows = rows.to(cuda)
    learner.critic_step(d_rows, actions.to(cuda), target.to(cuda))
    learner.actor_step(d_rows)
    torch.cuda.synchronize()
    report, failed = _compare(learner, ref64, ref32, ("critic", "actor"))
    with capsys.disabled():
        print("\ninteger rows, B %d: %s" % (B, "; ".join(report)))
    assert not failed, failed
    _assert_unmoved(learner, policy, critic)


@pytest.mark.parametrize("case", R.TWIN_CASES, ids=lambda c: "%s-%s-%d" % ("x".join(map(str, c[0])), "x".join(map(str, c[1])), c[2]))
def test_integer_data_makes_both_planes_of_the_twin_step_exact(cuda, case):
    """Td3Learner.critic_step on two differently drawn integer critics: each plane's loss and gradients
    are its own float64 reference's, exactly (no DdpgLearner in between)."""
    import torch
    from ctr_reach_amd.learner import Td3Learner
    one, two = R.integer_twin(*case)
    policy, critic1, rows, actions, target = one.made
    critic2 = two.made[1]
    B = case[3]
    _assert_integer_conditions(one, ("critic",))
    _assert_integer_conditions(two, ("critic",))
    assert one.ref64["critic_loss"] != two.ref64["critic_loss"]
    td3 = Td3Learner(R.to_device(policy, cuda), R.to_device(critic1, cuda), R.to_device(critic2, cuda), actor_lr=0.0,
                     critic_lr=0.0, max_batch=B)
    td3.critic_step(rows.to(cuda), actions.to(cuda), target.to(cuda))
    torch.cuda.synchronize()
    losses = td3.critic_loss.cpu().numpy()
    for plane, ref in enumerate((one, two)):
        _assert_exact(losses[plane], R.host(td3.critic_grads[plane]), ref.ref64, "critic", ("plane", plane))
    for net, start in zip(td3._critics, (critic1, critic2)):
        for (W, b), (W0, b0) in zip(R.host(net.params), R.host(R.params(start))):
            assert np.array_equal(R.bits(W), R.bits(W0)) and np.array_equal(R.bits(b), R.bits(b0))
