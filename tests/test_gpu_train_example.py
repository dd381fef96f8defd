"""examples/train_ddpg_her.py end to end at a tiny size: collect, sample, the DDPG updates and
MlpActor.load_ in a loop.  The losses are finite, the HER store holds rows, the policy moved, and
the actor's device blob is the host pack of the policy's final parameters (the last load_ landed)."""
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


def test_two_iterations(cuda):
    import torch
    from ctr_reach_amd import _abi
    ex = _example()
    made, mlp = [], ex.mlp

    def recording_mlp(*args):                            # the networks as main builds them, before any update
        net = mlp(*args)
        made.append((net, [p.detach().clone() for p in net.parameters()]))
        return net

    ex.mlp = recording_mlp
    out = ex.main(num_envs=256, iterations=2, steps_per_iter=8, batch_size=64, updates_per_iter=2, hidden=(32, 32), seed=0)
    torch.cuda.synchronize()
    first = [q.to(cuda) for net, init in made if net is out["policy"] for q in init]
    losses = np.array(out["losses"])
    assert losses.shape == (2, 2) and np.isfinite(losses).all(), losses
    assert len(out["her"]) > 0
    assert set(out["rollout_stats"]) == {"episodes", "successes", "error_sum", "length_sum"}
    assert int(out["rollout_stats"]["episodes"].sum()) > 0
    params = list(out["policy"].parameters())
    assert len(params) == len(first) == 6
    assert all(p.shape == q.shape and not torch.equal(p.detach(), q) for p, q in zip(params, first))
    # the blob is ctr_actor_pack of the final parameters
    actor = out["actor"]
    assert actor.hidden == [32, 32] and actor.in_dim == 19
    host = [p.detach().cpu().numpy() for p in params]
    lib = _abi.load()
    want = np.full(lib.ctr_actor_blob_bytes(actor._struct), 0xAB, dtype=np.uint8)
    W = (ctypes.c_void_p * 3)(*[w.ctypes.data for w in host[0::2]])
    b = (ctypes.c_void_p * 3)(*[v.ctypes.data for v in host[1::2]])
    assert lib.ctr_actor_pack(actor._struct, W, b, want.ctypes.data) == 0
    assert np.array_equal(actor.blob.cpu().numpy(), want)
