"""examples/train_ddpg_her.py with sac=True at a tiny size: collection is the GaussianActor's sample
and the step with its HER feed, an update is her.sample, the target in torch from the policy's next
sample and the two target critics, the SacLearner's two steps, the policy blob's refresh and one
polyak_ of the two target critics; none of it is autograd.  The losses and alpha are finite, every
tensor of the policy and of both critics moved, the three blobs are the host packs of the final
parameters, the store is not empty, and the policy's mean runs a rollout."""
import numpy as np
import pytest

import test_gpu_train_example_td3 as T3

pytestmark = pytest.mark.gpu


def test_two_iterations_of_sac(cuda):
    import torch
    from ctr_reach_amd import _abi
    from ctr_reach_amd.learner import SacLearner
    from ctr_reach_amd.policy import GaussianActor, MlpActor
    ex = T3._example()
    assert (ex.SAC_LR, ex.SAC_TAU, ex.INIT_ALPHA, ex.TARGET_ENTROPY) == (3e-4, 0.005, 1.0, -6.0)
    with pytest.raises(ValueError, match="--sac and --td3"):
        ex.main(num_envs=256, iterations=1, td3=True, sac=True)
    # main_sac builds the policy, the two critics, then their two targets
    start, plain_mlp = [], ex.mlp

    def recording_mlp(*args):
        net = plain_mlp(*args)
        start.append([p.detach().clone() for p in net.parameters()])
        return net

    ex.mlp = recording_mlp
    iterations, updates_per_iter = 2, 4
    out = ex.main(num_envs=256, iterations=iterations, steps_per_iter=8, batch_size=64, updates_per_iter=updates_per_iter,
                  hidden=(32, 32), sac=True)
    torch.cuda.synchronize()
    assert len(start) == 5
    losses = np.array(out["losses"])
    assert losses.shape == (2, 2) and np.isfinite(losses).all(), losses
    learner = out["learner"]
    assert isinstance(learner, SacLearner) and isinstance(out["pi_dev"], GaussianActor)
    alpha = float(out["alpha"])
    assert np.isfinite(alpha) and alpha > 0 and alpha != ex.INIT_ALPHA          # the temperature learned
    assert torch.isfinite(learner.critic_loss).all() and torch.isfinite(learner.logp_mean)
    assert learner.counter == iterations * updates_per_iter
    assert len(out["her"]) > 0
    assert list(out["policy"].parameters())[-1].shape == (12,)
    for net, first in ((out["policy"], start[0]), (out["critic"], start[1]), (out["critic2"], start[2])):
        for p, p0 in zip(net.parameters(), first):
            assert not p.requires_grad and p.grad is None and torch.isfinite(p).all()
            assert not torch.equal(p.cpu(), p0)
    lib = _abi.load()
    for net, bytes_fn, pack_fn, module in (
            (out["pi_dev"], lib.ctr_gauss_blob_bytes, lib.ctr_gauss_pack, out["policy"]),
            (out["critic_targ_dev"], lib.ctr_critic_blob_bytes, lib.ctr_critic_pack, out["critic_targ"]),
            (out["critic2_targ_dev"], lib.ctr_critic_blob_bytes, lib.ctr_critic_pack, out["critic2_targ"])):
        want = T3._host_pack(lib, net, bytes_fn, pack_fn, list(module.parameters()))
        assert np.array_equal(net.blob.cpu().numpy(), want)
    for net, targ, first in ((out["critic"], out["critic_targ"], start[1]), (out["critic2"], out["critic2_targ"], start[2])):
        for p, pt, p0 in zip(net.parameters(), targ.parameters(), first):
            assert not torch.equal(pt, p) and not torch.equal(pt.cpu(), p0)
    # the trained policy's deterministic mean through the period kernels
    mean = out["pi_dev"].mean_actor()
    assert isinstance(mean, MlpActor)
    from ctr_reach_amd import CtrReachVecEnv
    venv = CtrReachVecEnv(256, device=cuda, seed=1)                          # (an evaluation env: rollout is not for the HER feed)
    venv.reset()
    applied = venv.rollout(mean, 8, record_actions=True)
    torch.cuda.synchronize()
    assert applied.shape == (8, 256, 6) and torch.isfinite(applied).all() and (venv.t > 0).any()
    rows = venv.actor_rows()
    det = out["pi_dev"].sample(rows, 0, deterministic=True)["action"]
    assert torch.equal(det, mean(rows))
