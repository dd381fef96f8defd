"""examples/train_ddpg_her.py with sac=True, update_call=True at a tiny size: an iteration's updates are one
SacLearner.update call (ctr_sac_update) and leave what the five-call loop of device_targets=True leaves,
bit for bit: the networks, the blobs, the temperature, the HER store and the envs; GaussianActor.load_ and
polyak_ are never called; the reported losses are the same sums made in another order."""
import numpy as np
import pytest

import test_gpu_train_example_td3 as T3
from test_gpu_collect import HER_KEYS
from test_gpu_rollout import KEYS
from test_gpu_train_example_sac_collect import SIZE

pytestmark = pytest.mark.gpu


def test_the_update_call_trains_what_the_five_call_loop_trains(cuda, monkeypatch):
    import torch
    from ctr_reach_amd import policy as P
    ex = T3._example()
    calls = {"load_": 0, "polyak_": 0}
    plain_load, plain_polyak = P.GaussianActor.load_, ex.polyak_

    def counting_load(self, *args, **kw):
        calls["load_"] += 1
        return plain_load(self, *args, **kw)

    def counting_polyak(*args, **kw):
        calls["polyak_"] += 1
        return plain_polyak(*args, **kw)

    monkeypatch.setattr(P.GaussianActor, "load_", counting_load)
    monkeypatch.setattr(ex, "polyak_", counting_polyak)
    monkeypatch.setattr(P, "polyak_", counting_polyak)
    fused = ex.main(updates_per_iter=4, device_collect=True, update_call=True, **SIZE)
    assert calls == {"load_": 0, "polyak_": 0}
    eager = ex.main(updates_per_iter=4, device_collect=True, **SIZE)
    assert calls == {"load_": 8, "polyak_": 8}
    torch.cuda.synchronize()
    for name in ("policy", "critic", "critic2", "critic_targ", "critic2_targ"):
        for (k, p), (_, q) in zip(eager[name].named_parameters(), fused[name].named_parameters()):
            assert torch.equal(p.view(torch.int32), q.view(torch.int32)), (name, k)
    for name in ("pi_dev", "critic_targ_dev", "critic2_targ_dev"):
        assert torch.equal(eager[name].blob, fused[name].blob), name
    assert torch.equal(eager["alpha"].view(torch.int32), fused["alpha"].view(torch.int32))
    a, b = eager["venv"], fused["venv"]
    for k in KEYS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    bits = {torch.float32: torch.int32, torch.float64: torch.int64}
    for k in HER_KEYS:
        x, y = getattr(a._her, k), getattr(b._her, k)
        assert torch.equal(x.view(bits.get(x.dtype, x.dtype)), y.view(bits.get(y.dtype, y.dtype))), "her." + k
    assert eager["her"]._counter == fused["her"]._counter == 8 and eager["learner"].counter == fused["learner"].counter == 8
    want, got = np.array(eager["losses"]), np.array(fused["losses"])
    assert want.shape == got.shape == (2, 2) and np.isfinite(got).all()
    # the same float32 losses, summed in another order
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)


def test_update_call_is_sacs(cuda):
    ex = T3._example()
    with pytest.raises(ValueError, match="--sac"):
        ex.main(num_envs=256, iterations=1, steps_per_iter=4, batch_size=64, updates_per_iter=1, hidden=(32, 32),
                update_call=True)
    with pytest.raises(ValueError, match="--sac"):
        ex.main(num_envs=256, iterations=1, steps_per_iter=4, batch_size=64, updates_per_iter=1, hidden=(32, 32),
                td3=True, update_call=True)
