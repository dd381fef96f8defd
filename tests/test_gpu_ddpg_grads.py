"""DdpgLearner's gradients and losses (ctr_ddpg_critic_step / ctr_ddpg_actor_step, both with lr = 0
so that the two steps see the same parameters) against the example's two loss expressions under
float64 autograd on the CPU.  Per parameter tensor err = max|g - g64| / max|g64|, and the bar is 8
times the same quantity of torch's own float32 CPU autograd, computed here (the kernel's order of
summation -- MFMA k-chains, tiles, slots -- differs from torch's); the losses under the same rule.
The float64 reference keeps every hidden pre-activation at least 1e-5 from the relu's kink (the first
seed from 0 for which that holds), since a flipped mask is another function and not a rounding.

Also: with ``scale`` the gradients are those of a call on pre-divided actions, bit for bit; and on
small integers, where every product and sum is exact, the critic's gradients are exactly float64's."""
import numpy as np
import pytest

import ddpg_ref as R

pytestmark = pytest.mark.gpu

# B = 1; several tiles and a ragged tail; 3 T + 5: several workgroups, a ragged tail, the slots' sum
BATCHES = [1, 70, 3 * R.T + 5]
CASES = [(a, c, d, B) for a, c, d in R.SHAPES for B in BATCHES]
# ... and past T * SLOTS rows a workgroup adds a second tile to its slot, here a ragged one (the smallest
# shape: 100 000 pre-activations leave few seeds that keep away from the kink, and a wider one none)
CASES += [((32,), (32,), 19, R.T * R.SLOTS + 5)]


def _learner(policy, critic, cuda, max_batch, **kw):
    from ctr_reach_amd.learner import DdpgLearner
    kw.setdefault("actor_lr", 0.0)
    kw.setdefault("critic_lr", 0.0)
    return DdpgLearner(R.to_device(policy, cuda), R.to_device(critic, cuda), max_batch=max_batch, **kw)


def _err(g, g64):
    return float(np.abs(g.astype(np.float64) - g64).max() / np.abs(g64).max())


@pytest.mark.parametrize("a_hidden,c_hidden,in_dim,B", CASES)
def test_gradients_and_losses_against_float64_autograd(cuda, capsys, a_hidden, c_hidden, in_dim, B):
    import torch
    seed, (policy, critic, rows, actions, target), ref64, ref32 = R.case(a_hidden, c_hidden, in_dim, B)
    assert ref64["kink"] >= 1e-5
    learner = _learner(policy, critic, cuda, B)
    d_rows, d_actions, d_target = (t.to(cuda) for t in (rows, actions, target))
    learner.critic_step(d_rows, d_actions, d_target)
    learner.actor_step(d_rows)
    torch.cuda.synchronize()
    report, failed = [], []
    for name, loss in (("critic", learner.critic_loss), ("actor", learner.actor_loss)):
        want = ref64[name + "_loss"]
        ours, theirs = abs(float(loss) - want) / abs(want), abs(ref32[name + "_loss"] - want) / abs(want)
        report.append("%s loss %.3g (torch f32 %.3g)" % (name, ours, theirs))
        if not ours <= 8 * theirs:
            failed.append(report[-1])
    for name, got in (("critic", learner.critic_grads), ("actor", learner.actor_grads)):
        for l, (pair, pair64, pair32) in enumerate(zip(R.host(got), ref64[name + "_grads"], ref32[name + "_grads"])):
            for which, g, g64, g32 in zip("Wb", pair, pair64, pair32):
                assert g.shape == g64.shape and np.isfinite(g).all()
                ours, theirs = _err(g, g64), _err(g32, g64)
                report.append("%s g%s[%d] %.3g (torch f32 %.3g)" % (name, which, l, ours, theirs))
                if not ours <= 8 * theirs:
                    failed.append(report[-1])
    with capsys.disabled():
        print("\n%s / %s, in_dim %d, B %d, seed %d, kink %.3g: %s" % (list(a_hidden), list(c_hidden), in_dim, B, seed,
                                                                     ref64["kink"], "; ".join(report)))
    assert not failed, failed
    # lr = 0: nothing moved
    for net, start in ((learner._actor, policy), (learner._critic, critic)):
        for (W, b), (W0, b0) in zip(R.host(net.params), R.host(R.params(start))):
            assert np.array_equal(R.bits(W), R.bits(W0)) and np.array_equal(R.bits(b), R.bits(b0))


@pytest.mark.parametrize("in_dim", [19, 20])
def test_scale_is_one_division(cuda, in_dim):
    import torch
    policy, critic, rows, actions, target = R.make(3, (64, 96), (32, 64), in_dim, 70)
    scale = np.array([0.001, 0.002, 0.003, 0.087, 0.05, 3.0], dtype=np.float32)
    actions = actions * torch.from_numpy(scale) * 1.7                     # (not normalised, and not only in the box)
    with_scale, without = _learner(policy, critic, cuda, 70, scale=scale), _learner(policy, critic, cuda, 70)
    d_rows, d_actions, d_target = (t.to(cuda) for t in (rows, actions, target))
    with_scale.critic_step(d_rows, d_actions, d_target)
    divided = actions.numpy() / scale                                      # numpy's float32 division: correctly rounded
    assert divided.dtype == np.float32
    without.critic_step(d_rows, torch.from_numpy(divided).to(cuda), d_target)
    torch.cuda.synchronize()
    assert R.bits(with_scale.critic_loss.cpu().numpy()) == R.bits(without.critic_loss.cpu().numpy())
    for (W, b), (W1, b1) in zip(R.host(with_scale.critic_grads), R.host(without.critic_grads)):
        assert np.abs(W).max() > 0
        assert np.array_equal(R.bits(W), R.bits(W1)) and np.array_equal(R.bits(b), R.bits(b1))
    # ... and the scale matters: other actions give other gradients
    without.critic_step(d_rows, d_actions, d_target)
    torch.cuda.synchronize()
    assert not np.array_equal(R.host(without.critic_grads)[0][0], R.host(with_scale.critic_grads)[0][0])


@pytest.mark.parametrize("in_dim,B", [(25, 64), (26, 128), (25, 2048)])      # 2048: two tiles in every slot
def test_integer_data_makes_the_critic_gradients_exact(cuda, in_dim, B):
    """Weights, rows, actions and targets are small integers, one hidden layer, B a power of two (2 / B
    is exact): every product and every partial sum is an integer multiple of 2 / B far below 2^24
    of them, so any order of summation gives float64's result exactly.  An element in the wrong
    place, counted twice or left out does not."""
    import torch
    from ctr_reach_amd.learner import DdpgLearner
    rng = np.random.default_rng(in_dim)
    critic = R.mlp(in_dim, (32,), 1, False).requires_grad_(False)
    policy = R.mlp(in_dim - 6, (32,), 6, True).requires_grad_(False)
    for m in R.params(critic):
        for t in m:
            t.copy_(torch.from_numpy(rng.integers(-2, 3, tuple(t.shape)).astype(np.float32)))
    rows = torch.from_numpy(rng.integers(-2, 3, (B, in_dim - 6)).astype(np.float32))
    actions = torch.from_numpy(rng.integers(-1, 2, (B, 6)).astype(np.float32))
    target = torch.from_numpy(rng.integers(-8, 9, (B,)).astype(np.float32))
    ref = R.autograd(policy, critic, rows, actions, target, torch.float64)
    learner = DdpgLearner(R.to_device(policy, cuda), R.to_device(critic, cuda), actor_lr=0.0, critic_lr=0.0, max_batch=B)
    learner.critic_step(rows.to(cuda), actions.to(cuda), target.to(cuda))
    torch.cuda.synchronize()
    for (W, b), (W64, b64) in zip(R.host(learner.critic_grads), ref["critic_grads"]):
        assert np.abs(W64).max() > 0 and np.abs(W64 * B / 2).max() < 2 ** 24
        assert np.array_equal(W.astype(np.float64), W64) and np.array_equal(b.astype(np.float64), b64)
