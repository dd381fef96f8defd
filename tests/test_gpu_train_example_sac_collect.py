"""examples/train_ddpg_her.py with sac=True, device_targets=True, device_collect=True at a tiny size:
the collection of an iteration is one venv.collect_gauss call (the policy's samples inside the fused
period kernel, one launch per refill period) and never GaussianActor.sample on the envs' rows; with
the policy held fixed the envs and the HER store are what the per-step loop leaves, bit for bit."""
import numpy as np
import pytest

import test_gpu_train_example_td3 as T3
from test_gpu_collect import HER_KEYS
from test_gpu_rollout import KEYS

pytestmark = pytest.mark.gpu

SIZE = dict(num_envs=256, iterations=2, steps_per_iter=8, batch_size=64, hidden=(32, 32), sac=True, device_targets=True)


def test_two_iterations_of_sac_with_the_collection_in_the_period_kernel(cuda, monkeypatch):
    import torch
    from ctr_reach_amd.policy import GaussianActor
    ex = T3._example()
    calls = {"pi": 0}
    plain_pi = GaussianActor.sample

    def counting_pi(self, *args, **kw):
        calls["pi"] += 1
        return plain_pi(self, *args, **kw)

    monkeypatch.setattr(GaussianActor, "sample", counting_pi)
    out = ex.main(updates_per_iter=4, device_collect=True, **SIZE)
    torch.cuda.synchronize()
    assert calls["pi"] == 0                       # neither the collection nor the target calls ctr_gauss_act
    losses = np.array(out["losses"])
    assert losses.shape == (2, 2) and np.isfinite(losses).all(), losses
    alpha = float(out["alpha"])
    assert np.isfinite(alpha) and alpha > 0
    assert len(out["her"]) > 0
    venv = out["venv"]
    assert 0 < venv.fused_launches < 16           # period launches, fewer than the 16 steps they ran
    assert int(venv.t.max().item()) > 0 and out["learner"].counter == 8


def test_the_collection_does_not_depend_on_where_the_policy_is_sampled(cuda):
    """No updates: the policy never changes, so collect_gauss and the per-step loop must collect the same."""
    import torch
    ex = T3._example()
    fused = ex.main(updates_per_iter=0, device_collect=True, **SIZE)
    eager = ex.main(updates_per_iter=0, device_collect=False, **SIZE)
    torch.cuda.synchronize()
    a, b = eager["venv"], fused["venv"]
    assert b.fused_launches > 0 and a.fused_launches == 0
    for k in KEYS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    bits = {torch.float32: torch.int32, torch.float64: torch.int64}
    for k in HER_KEYS:
        x, y = getattr(a._her, k), getattr(b._her, k)
        assert torch.equal(x.view(bits.get(x.dtype, x.dtype)), y.view(bits.get(y.dtype, y.dtype))), "her." + k
    assert len(eager["her"]) == len(fused["her"]) > 0
    assert a.refills == b.refills


def test_device_collect_is_sacs(cuda):
    ex = T3._example()
    with pytest.raises(ValueError, match="--sac"):
        ex.main(num_envs=256, iterations=1, steps_per_iter=4, batch_size=64, updates_per_iter=0, hidden=(32, 32),
                device_collect=True)
    with pytest.raises(ValueError, match="--sac"):
        ex.main(num_envs=256, iterations=1, steps_per_iter=4, batch_size=64, updates_per_iter=0, hidden=(32, 32),
                td3=True, device_collect=True)
