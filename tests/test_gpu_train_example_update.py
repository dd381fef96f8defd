"""examples/train_ddpg_her.py with device_update=True at a tiny size: an update is her.sample_td, the
learner's critic_step and actor_step and polyak_, and none of it is autograd.  The losses are finite,
no online parameter requires grad, every online parameter tensor moved from its start and by less
than Adam's step bound, and the three blobs are the host packs of the final torch parameters."""
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


def test_two_iterations_with_device_update(cuda):
    import torch
    from ctr_reach_amd import _abi
    from ctr_reach_amd.learner import DdpgLearner
    ex = _example()
    # the online networks are the first two that main builds
    start, plain_mlp = [], ex.mlp

    def recording_mlp(*args):
        net = plain_mlp(*args)
        start.append([p.detach().clone() for p in net.parameters()])
        return net

    ex.mlp = recording_mlp
    iterations, updates_per_iter = 2, 2
    out = ex.main(num_envs=256, iterations=iterations, steps_per_iter=8, batch_size=64, updates_per_iter=updates_per_iter,
                  hidden=(32, 32), device_update=True)
    torch.cuda.synchronize()
    losses = np.array(out["losses"])
    assert losses.shape == (2, 2) and np.isfinite(losses).all(), losses
    assert len(out["her"]) > 0
    assert isinstance(out["learner"], DdpgLearner)
    assert out["actor_targ"] is not None and out["critic_targ_dev"] is not None     # the flag implies device_polyak
    updates = iterations * updates_per_iter
    for net, first, lr in ((out["policy"], start[0], ex.ACTOR_LR), (out["critic"], start[1], ex.CRITIC_LR)):
        for p, p0 in zip(net.parameters(), first):
            assert not p.requires_grad and p.grad is None and torch.isfinite(p).all()
            assert not torch.equal(p.cpu(), p0)                            # it moved from its start ...
            assert (p.cpu() - p0).abs().max() < 4 * updates * lr            # ... within Adam's step bound
    lib = _abi.load()
    for net, bytes_fn, pack_fn, module in (
            (out["actor"], lib.ctr_actor_blob_bytes, lib.ctr_actor_pack, out["policy"]),
            (out["actor_targ"], lib.ctr_actor_blob_bytes, lib.ctr_actor_pack, out["policy_targ"]),
            (out["critic_targ_dev"], lib.ctr_critic_blob_bytes, lib.ctr_critic_pack, out["critic_targ"])):
        want = _host_pack(lib, net, bytes_fn, pack_fn, list(module.parameters()))
        assert np.array_equal(net.blob.cpu().numpy(), want)
    # the targets followed the online networks
    for net, targ in ((out["policy"], out["policy_targ"]), (out["critic"], out["critic_targ"])):
        for p, pt in zip(net.parameters(), targ.parameters()):
            assert not torch.equal(pt, p)
