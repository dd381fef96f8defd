"""examples/train_ddpg_her.py with device_polyak=True at a tiny size: the DDPG target comes from
her.sample_td, and after every update one polyak_ launch moves both target networks and repacks both
blobs.  The losses are finite, the two blobs are the host packs of the final torch target parameters
(which the launch wrote in place), and those parameters moved away from their start without becoming
the online ones: the update ran, and it was not a copy."""
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


def test_two_iterations_with_device_polyak(cuda):
    import torch
    from ctr_reach_amd import _abi
    ex = _example()
    # the targets start as copies of the freshly initialised online networks, the first two that main builds
    start, plain_mlp = [], ex.mlp

    def recording_mlp(*args):
        net = plain_mlp(*args)
        start.append([p.detach().clone() for p in net.parameters()])
        return net

    ex.mlp = recording_mlp
    out = ex.main(num_envs=256, iterations=2, steps_per_iter=8, batch_size=64, updates_per_iter=2, hidden=(32, 32),
                  device_polyak=True)
    torch.cuda.synchronize()
    losses = np.array(out["losses"])
    assert losses.shape == (2, 2) and np.isfinite(losses).all(), losses
    assert len(out["her"]) > 0
    lib = _abi.load()
    actor_targ, critic_targ = out["actor_targ"], out["critic_targ_dev"]
    assert actor_targ is not None and critic_targ is not None              # the flag implies the device targets
    assert actor_targ.hidden == [32, 32] and actor_targ.in_dim == 19
    assert critic_targ.hidden == [32, 32] and critic_targ.in_dim == 25
    want = _host_pack(lib, actor_targ, lib.ctr_actor_blob_bytes, lib.ctr_actor_pack, list(out["policy_targ"].parameters()))
    assert np.array_equal(actor_targ.blob.cpu().numpy(), want)
    want = _host_pack(lib, critic_targ, lib.ctr_critic_blob_bytes, lib.ctr_critic_pack,
                      list(out["critic_targ"].parameters()))
    assert np.array_equal(critic_targ.blob.cpu().numpy(), want)
    # (the learner's own actor, as without the flag)
    want = _host_pack(lib, out["actor"], lib.ctr_actor_blob_bytes, lib.ctr_actor_pack, list(out["policy"].parameters()))
    assert np.array_equal(out["actor"].blob.cpu().numpy(), want)
    # the torch modules still own the masters: their parameters are what the launch wrote
    for net, targ, first in ((out["policy"], out["policy_targ"], start[0]), (out["critic"], out["critic_targ"], start[1])):
        assert set(targ.state_dict()) == set(net.state_dict())
        for p, pt, p0 in zip(net.parameters(), targ.parameters(), first):
            assert not pt.requires_grad and torch.isfinite(pt).all()
            assert not torch.equal(pt, p)                                  # not a copy of the online network
            assert not torch.equal(pt.cpu(), p0)                           # and it moved from its start
            # by tau per update towards parameters that Adam moves by about its learning rate
            assert (pt.cpu() - p0).abs().max() < 1e-3
