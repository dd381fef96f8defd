"""examples/train_ddpg_her.py with update_run=True at a tiny size, for DDPG and for TD3: an iteration's
updates are one DdpgLearner.update / Td3Learner.update call (ctr_ddpg_update) and leave what the eager
device_update / td3 loops leave, bit for bit: the networks, the targets, the four or five blobs, the HER
store and the envs; polyak_ and MlpActor.load_ are never called inside the updates; the reported losses are
the same float32 values summed in another order."""
import numpy as np
import pytest

import test_gpu_train_example_td3 as T3
from test_gpu_collect import HER_KEYS
from test_gpu_rollout import KEYS

pytestmark = pytest.mark.gpu

SIZE = dict(num_envs=256, iterations=2, steps_per_iter=8, batch_size=64, hidden=(32, 32))


@pytest.mark.parametrize("td3,updates_per_iter", [(False, 4), (True, 4), (True, 3)], ids=["ddpg", "td3", "td3_odd"])
def test_the_update_run_trains_what_the_eager_loop_trains(cuda, monkeypatch, td3, updates_per_iter):
    import torch
    from ctr_reach_amd import policy as P
    ex = T3._example()
    calls = {"load_": 0, "polyak_": 0}
    plain_load, plain_polyak = P.MlpActor.load_, ex.polyak_

    def counting_load(self, *args, **kw):
        calls["load_"] += 1
        return plain_load(self, *args, **kw)

    def counting_polyak(*args, **kw):
        calls["polyak_"] += 1
        return plain_polyak(*args, **kw)

    monkeypatch.setattr(P.MlpActor, "load_", counting_load)
    monkeypatch.setattr(ex, "polyak_", counting_polyak)
    monkeypatch.setattr(P, "polyak_", counting_polyak)
    fused = ex.main(updates_per_iter=updates_per_iter, td3=td3, update_run=True, **SIZE)
    assert calls == {"load_": 0, "polyak_": 0}
    eager = ex.main(updates_per_iter=updates_per_iter, td3=td3, device_update=True, **SIZE)
    total = 2 * updates_per_iter
    # the eager loop: one load_ per iteration, one polyak_ per update with a policy step
    assert calls == {"load_": 2, "polyak_": total // ex.POLICY_DELAY if td3 else total}
    torch.cuda.synchronize()
    nets = ("policy", "critic", "policy_targ", "critic_targ") + (("critic2", "critic2_targ") if td3 else ())
    for name in nets:
        for (k, p), (_, q) in zip(eager[name].named_parameters(), fused[name].named_parameters()):
            assert torch.equal(p.view(torch.int32), q.view(torch.int32)), (name, k)
    for name in ("actor", "actor_targ", "critic_targ_dev") + (("critic2_targ_dev",) if td3 else ()):
        assert torch.equal(eager[name].blob, fused[name].blob), name
    a, b = eager["venv"], fused["venv"]
    for k in KEYS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    bits = {torch.float32: torch.int32, torch.float64: torch.int64}
    for k in HER_KEYS:
        x, y = getattr(a._her, k), getattr(b._her, k)
        assert torch.equal(x.view(bits.get(x.dtype, x.dtype)), y.view(bits.get(y.dtype, y.dtype))), "her." + k
    assert eager["her"]._counter == fused["her"]._counter == total
    if td3:
        assert fused["learner"].update_count == total and eager["learner"].update_count == 0
    for name in ("actor", "critic") + (("critic1", "critic2") if td3 else ()):
        sa, sb = eager["learner"].state_dict().get(name), fused["learner"].state_dict().get(name)
        if sa is not None:
            assert torch.equal(sa["pow"], sb["pow"]), name
    want, got = np.array(eager["losses"]), np.array(fused["losses"])
    assert want.shape == got.shape == (2, 2) and np.isfinite(got).all()
    # the same float32 losses, summed in another order
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)


def test_update_run_is_not_sacs(cuda):
    ex = T3._example()
    with pytest.raises(ValueError, match="--update-call"):
        ex.main(num_envs=256, iterations=1, steps_per_iter=4, batch_size=64, updates_per_iter=1, hidden=(32, 32),
                sac=True, update_run=True)
