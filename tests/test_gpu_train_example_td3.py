"""examples/train_ddpg_her.py with td3=True at a tiny size: an update is her.sample_td3 and the
Td3Learner's twin critic_step, and every second one also actor_step and one polyak_ of the three
targets; none of it is autograd.  The losses are finite, no online parameter requires grad, every
tensor of the policy and of both critics moved from its start (the policy within Adam's bound for
its delayed steps), the two critics differ, the four blobs are the host packs of the final torch
parameters, and the targets differ from the online networks."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _example():
    spec = importlib.util.spec_from_file_location("train_ddpg_her", os.path.join(ROOT, "examples", "train_ddpg_her.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _host_pack(lib, net, bytes_fn, pack_fn, params):
    host = [p.detach().cpu().numpy() for p in params]
    want = np.full(bytes_fn(net._struct), 0xAB, dtype=np.uint8)
    n = len(host) // 2
    W = (ctypes.c_void_p * n)(*[w.ctypes.data for w in host[0::2]])
    b = (ctypes.c_void_p * n)(*[v.ctypes.data for v in host[1::2]])
    assert pack_fn(net._struct, W, b, want.ctypes.data) == 0
    return want


def test_two_iterations_of_td3(cuda):
    import torch
    from ctr_reach_amd import _abi
    from ctr_reach_amd.learner import Td3Learner
    ex = _example()
    assert (ex.TARGET_NOISE, ex.NOISE_CLIP, ex.POLICY_DELAY) == (0.2, 0.5, 2)
    # main builds policy, critic, their targets, then the second critic and its target
    start, plain_mlp = [], ex.mlp

    def recording_mlp(*args):
        net = plain_mlp(*args)
        start.append([p.detach().clone() for p in net.parameters()])
        return net

    ex.mlp = recording_mlp
    iterations, updates_per_iter = 2, 4
    out = ex.main(num_envs=256, iterations=iterations, steps_per_iter=8, batch_size=64, updates_per_iter=updates_per_iter,
                  hidden=(32, 32), td3=True)
    torch.cuda.synchronize()
    assert len(start) == 6
    losses = np.array(out["losses"])
    assert losses.shape == (2, 2) and np.isfinite(losses).all(), losses
    assert len(out["her"]) > 0
    assert isinstance(out["learner"], Td3Learner)
    assert torch.isfinite(out["learner"].critic_loss).all() and out["learner"].critic_loss.shape == (2,)
    for key in ("actor_targ", "critic_targ_dev", "critic2", "critic2_targ", "critic2_targ_dev"):
        assert out[key] is not None, key                                   # the flag implies device_update
    updates = iterations * updates_per_iter
    policy_steps = updates // ex.POLICY_DELAY
    assert policy_steps == 4
    for net, first, lr, steps in ((out["policy"], start[0], ex.ACTOR_LR, policy_steps),
                                  (out["critic"], start[1], ex.CRITIC_LR, updates),
                                  (out["critic2"], start[4], ex.CRITIC_LR, updates)):
        for p, p0 in zip(net.parameters(), first):
            assert not p.requires_grad and p.grad is None and torch.isfinite(p).all()
            assert not torch.equal(p.cpu(), p0)                            # it moved from its start ...
            assert (p.cpu() - p0).abs().max() < 4 * steps * lr              # ... within Adam's step bound
    assert all(not torch.equal(p, q) for p, q in zip(out["critic"].parameters(), out["critic2"].parameters()))
    lib = _abi.load()
    for net, bytes_fn, pack_fn, module in (
            (out["actor"], lib.ctr_actor_blob_bytes, lib.ctr_actor_pack, out["policy"]),
            (out["actor_targ"], lib.ctr_actor_blob_bytes, lib.ctr_actor_pack, out["policy_targ"]),
            (out["critic_targ_dev"], lib.ctr_critic_blob_bytes, lib.ctr_critic_pack, out["critic_targ"]),
            (out["critic2_targ_dev"], lib.ctr_critic_blob_bytes, lib.ctr_critic_pack, out["critic2_targ"])):
        want = _host_pack(lib, net, bytes_fn, pack_fn, list(module.parameters()))
        assert np.array_equal(net.blob.cpu().numpy(), want)
    # the targets followed the online networks, and are not them
    for net, targ, first in ((out["policy"], out["policy_targ"], start[0]), (out["critic"], out["critic_targ"], start[1]),
                             (out["critic2"], out["critic2_targ"], start[4])):
        for p, pt, p0 in zip(net.parameters(), targ.parameters(), first):
            assert not torch.equal(pt, p) and not torch.equal(pt.cpu(), p0)
