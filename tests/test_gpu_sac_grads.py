"""SacLearner.actor_step's gradients, loss, mean log-probability and temperature gradient
(ctr_sac_actor_step, every learning rate 0) against SAC's policy loss under float64 autograd on the
CPU (tests/sac_ref.py), with the noise of GaussianActor's Python restatement of the draw.  Per tensor
err = max|g - g64| / max|g64|, the scalars by their relative error, and the bar is 8 times the same
quantity of torch's own float32 CPU autograd, computed here and printed: the project's rule
(tests/test_gpu_ddpg_grads.py).  The float64 reference keeps clear of the relu's kink, of Q1 = Q2
and of the clip's two ends (``sac_ref.case``), where a rounding would make another function.

That the restatement's noise is the kernels' is checked against ctr_gauss_act's own outputs; both
kernels call one device function for the draw."""
import numpy as np
import pytest

import ddpg_ref as R
import sac_ref as S

pytestmark = pytest.mark.gpu

BATCHES = [1, 70, 3 * S.T + 5]
CASES = [(shape, B) for shape in S.SHAPES for B in BATCHES]
# past T * SLOTS rows a workgroup adds a second tile to its slot, here a ragged one (the smallest shape, as
# tests/test_gpu_ddpg_grads.py; tests/test_host_sac.py finds its seed without a GPU)
CASES += [(S.SHAPES[0], S.T * S.SLOTS + 5)]


def _learner(made, cuda, B, alpha=S.ALPHA, **kw):
    from ctr_reach_amd.learner import SacLearner
    policy, c1, c2, _ = made
    for name in ("actor_lr", "critic_lr", "alpha_lr"):
        kw.setdefault(name, 0.0)
    return SacLearner(R.to_device(policy, cuda), R.to_device(c1, cuda), R.to_device(c2, cuda), init_alpha=alpha,
                      target_entropy=S.TARGET_ENTROPY, max_batch=B, seed=0, **kw)


def _step(made, cuda, B, **kw):
    import torch
    learner = _learner(made, cuda, B, **kw)
    learner.actor_step(made[3].to(cuda), counter=0)
    torch.cuda.synchronize()
    return learner


def _compare(learner, ref64, ref32, tag, capsys):
    """The report and the list of what misses the bar."""
    report, failed = [], []
    for name, got in (("loss", learner.actor_loss), ("logp_mean", learner.logp_mean), ("alpha_grad", learner.alpha_grad)):
        want = ref64[name]
        ours, theirs = abs(float(got) - want) / abs(want), abs(ref32[name] - want) / abs(want)
        report.append("%s %.3g (torch f32 %.3g)" % (name, ours, theirs))
        if not ours <= 8 * theirs:
            failed.append(report[-1])
    for l, (pair, pair64, pair32) in enumerate(zip(R.host(learner.actor_grads), ref64["grads"], ref32["grads"])):
        for which, g, g64, g32 in zip("Wb", pair, pair64, pair32):
            assert g.shape == g64.shape and np.isfinite(g).all()
            ours, theirs = S.err(g, g64), S.err(g32, g64)
            report.append("g%s[%d] %.3g (torch f32 %.3g)" % (which, l, ours, theirs))
            if not ours <= 8 * theirs:
                failed.append(report[-1])
    with capsys.disabled():
        print("\n%s: %s" % (tag, "; ".join(report)))
    return failed


def _unmoved(learner, made):
    for net, start in zip((learner._actor,) + learner._critics, made[:3]):
        for (W, b), (W0, b0) in zip(R.host(net.params), R.host(R.params(start))):
            assert np.array_equal(R.bits(W), R.bits(W0)) and np.array_equal(R.bits(b), R.bits(b0))


@pytest.mark.parametrize("shape,B", CASES)
def test_gradients_against_float64_autograd(cuda, capsys, shape, B):
    mixed = shape in S.MIXED and B > 1
    seed, made, eps, ref64, ref32 = S.case(*shape, B, mixed=mixed)
    assert S.clear(ref64)
    if mixed:
        assert 0.1 <= ref64["share"] <= 0.9
    learner = _step(made, cuda, B)
    failed = _compare(learner, ref64, ref32, "%s, B %d, seed %d, kink %.3g, gap %.3g, critic 1's share %.2f"
                      % (shape, B, seed, ref64["kink"], ref64["gap"], ref64["share"]), capsys)
    assert not failed, failed
    # every learning rate 0: nothing moved, the critics' parameters and the temperature included
    _unmoved(learner, made)
    assert R.bits(learner.log_alpha.cpu().numpy()) == R.bits(np.float32(np.log(S.ALPHA)))
    assert float(learner.alpha) == pytest.approx(S.ALPHA, rel=1e-6)


def test_the_restated_noise_is_the_kernels(cuda, capsys):
    """sac_ref.eps_for against ctr_gauss_act: unit and logp recomputed in float64 from the kernel's
    logits and eps_for's noise, under tests/test_gpu_gauss_actor.py's rule (4 times the numpy float32
    restatement's error)."""
    import torch
    from ctr_reach_amd.policy import GaussianActor, gauss_head
    B = 70
    _, (policy, _, _, rows), eps, _, _ = S.case(*S.SHAPES[1], B, mixed=True)
    pi = GaussianActor.from_torch(policy, np.ones(6, dtype=np.float32), cuda, seed=0)
    out = pi.sample(rows.to(cuda), 0, logits=True)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    want = gauss_head(out["logits"].astype(np.float64), eps, np.ones(6))
    f32 = gauss_head(out["logits"], S.eps_for(B, dtype=np.float32), np.ones(6), np.float32)
    for name in ("unit", "logp"):
        ours = float(np.abs(out[name] - want[name]).max())
        theirs = float(np.abs(f32[name].astype(np.float64) - want[name]).max())
        with capsys.disabled():
            print("\n%s %.3g (numpy f32 %.3g)" % (name, ours, theirs))
        assert ours <= 4 * theirs, name
    # and with another draw's noise it is not
    other = gauss_head(out["logits"].astype(np.float64), S.eps_for(B, counter=1), np.ones(6))
    assert np.abs(out["unit"] - other["unit"]).max() > 1e-2


@pytest.mark.parametrize("shape", S.MIXED)
def test_both_critics_count(cuda, capsys, shape):
    """The critics in the other order are the same loss, and the gradients match the reference that
    swaps too.  With critic 1 in both places every row is a tie, which goes to critic 1, and critic 2's
    path carries nothing: other gradients, which match their own reference."""
    import torch
    B = 70
    seed, made, eps, ref64, ref32 = S.case(*shape, B, mixed=True)
    plain = _step(made, cuda, B)
    _, swapped_made, _, sref64, sref32 = S.case(*shape, B, mixed=True, swap=True)
    assert sref64["share"] == pytest.approx(1 - ref64["share"]) and swapped_made[1] is not made[1]
    swapped = _step(swapped_made, cuda, B)
    failed = _compare(swapped, sref64, sref32, "%s swapped" % (shape,), capsys)
    assert not failed, failed
    policy, c1, c2, rows = made
    same = (policy, c1, c1, rows)
    one64, one32 = (S.autograd(*same, eps, S.ALPHA, d) for d in (torch.float64, torch.float32))
    assert one64["kink"] >= 1e-5 and one64["clip"] >= 1e-3 and one64["gap"] == 0 and one64["share"] == 1
    only = _step(same, cuda, B)
    failed = _compare(only, one64, one32, "%s critic 1 twice" % (shape,), capsys)
    assert not failed, failed
    for (W, b), (W1, b1) in zip(R.host(plain.actor_grads), R.host(only.actor_grads)):
        assert S.err(W1, W.astype(np.float64)) > 1e-3 and S.err(b1, b.astype(np.float64)) > 1e-3


def test_the_clip_stops_the_gradient(cuda, capsys):
    log_std = (5.0, 5.0, -25.0, None, None, None)
    shape, B = S.SHAPES[1], 70
    seed, made, eps, ref64, ref32 = S.case(*shape, B, log_std=log_std)
    learner = _step(made, cuda, B)
    gW, gb = R.host(learner.actor_grads)[-1]
    for i in (0, 1, 2):
        assert not gW[6 + i].any() and gb[6 + i] == 0 and not ref64["grads"][-1][0][6 + i].any()
    for i in (3, 4, 5):
        assert gW[6 + i].any() and gb[6 + i] != 0
    failed = _compare(learner, ref64, ref32, "log std biases %s" % (log_std,), capsys)
    assert not failed, failed


def test_alpha_matters(cuda, capsys):
    import torch
    shape, B = S.SHAPES[0], 70
    seed, made, eps, ref64, ref32 = S.case(*shape, B, mixed=True)
    got = {}
    for alpha in (S.ALPHA, 1.0):
        r64, r32 = (S.autograd(*made, eps, alpha, d) for d in (torch.float64, torch.float32))
        assert S.clear(r64)
        learner = _step(made, cuda, B, alpha=alpha)
        failed = _compare(learner, r64, r32, "alpha %g" % alpha, capsys)
        assert not failed, failed
        got[alpha] = R.host(learner.actor_grads)
    for (W, b), (W1, b1) in zip(got[S.ALPHA], got[1.0]):
        assert S.err(W1, W.astype(np.float64)) > 1e-2 and S.err(b1, b.astype(np.float64)) > 1e-2
