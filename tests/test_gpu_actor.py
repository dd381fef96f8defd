"""ctr_actor (the MLP actor as a kernel of its own) against MlpActor.emulate, the CPU reference of its
arithmetic: exactly on data where every value of the specification is a small integer (the
fragment-layout test), within the measured f32-accumulation difference on random data; an env's
action depends on its own row only."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(32,), (64, 96), (128, 128, 128)]
SCALE = np.array([0.001, 0.001, 0.001, 0.087, 0.087, 0.087])


def _integer_actor(rng, hidden, in_dim, device):
    """Sparse asymmetric weights: at most 4 non-zeros of +-1 per row; integer biases."""
    from ctr_reach_amd.policy import MlpActor
    dims = [in_dim] + list(hidden) + [6]
    layers = []
    for l in range(len(dims) - 1):
        W = np.zeros((dims[l + 1], dims[l]), dtype=np.float32)
        for i in range(dims[l + 1]):
            cols = rng.choice(dims[l], size=rng.integers(1, 5), replace=False)
            W[i, cols] = rng.choice([-1.0, 1.0], size=cols.size)
        # later layers: a row sums at most 4 activations; keep them <= 256 by pulling each layer
        # back with a negative bias
        b = rng.integers(-2, 3, dims[l + 1]).astype(np.float32) if l == 0 else rng.integers(-6, 2, dims[l + 1]).astype(np.float32)
        layers.append((W, b))
    return MlpActor(layers, SCALE, device=device)


@pytest.mark.parametrize("in_dim", [19, 20])
@pytest.mark.parametrize("hidden", SHAPES)
def test_logits_are_exact_on_integer_data(cuda, hidden, in_dim):
    import torch
    rng = np.random.default_rng(100 * len(hidden) + in_dim)
    act = _integer_actor(rng, hidden, in_dim, cuda)
    for n in (1, 65, 300):
        rows = rng.integers(-2, 3, (n, in_dim)).astype(np.float32)
        a_ref, y_ref = act.emulate(rows)
        # the condition under which the specification is exact in every format it uses
        assert np.abs(rows @ act.weights[0].T + act.biases[0]).max() <= 10
        for h in act.last_hidden:
            assert np.abs(h).max() <= 256 and np.array_equal(h, np.round(h))
        assert np.array_equal(y_ref, np.round(y_ref)) and np.abs(y_ref).max() < 2 ** 20
        assert len(np.unique(y_ref)) > 3                     # (not a degenerate network)
        a, y = act(torch.tensor(rows, device=cuda), logits=True)
        torch.cuda.synchronize()
        assert np.array_equal(y.cpu().numpy().astype(np.float64), y_ref), (hidden, in_dim, n)
        assert np.allclose(a.cpu().numpy(), a_ref, rtol=0, atol=2e-7)


def _uniform_actor(rng, hidden, in_dim, device):
    from ctr_reach_amd.policy import MlpActor
    dims = [in_dim] + list(hidden) + [6]
    layers = []
    for l in range(len(dims) - 1):
        s = 1.0 / np.sqrt(dims[l])
        layers.append((rng.uniform(-s, s, (dims[l + 1], dims[l])).astype(np.float32),
                       rng.uniform(-s, s, dims[l + 1]).astype(np.float32)))
    return MlpActor(layers, SCALE, device=device)


@pytest.fixture(scope="module")
def reset_rows(cuda):
    """The flat rows of a reset 300-env four-system batch (computed once, not modified)."""
    from ctr_reach_amd import CtrReachVecEnv
    env = CtrReachVecEnv(300, device=cuda, seed=5, select_systems=[0, 1, 2, 3])
    env.reset()
    rows = env.actor_rows().clone()
    assert rows.shape == (300, 20)
    return rows


# max |actions / scale - emulate| measured on an MI355X over these inputs; the
# bound is 4x that: the two differ by f32 accumulation order and the rare bf16 rounding flip that
# follows from it, and flips are discrete (these inputs hold none for [32] and [64, 96]; other
# weight seeds on the same rows gave up to 1.6e-4 for [32], one flipped activation)
MEASURED = {(32,): 3.961e-08, (64, 96): 2.111e-08, (128, 128, 128): 3.217e-07}


@pytest.mark.parametrize("hidden", SHAPES)
def test_random_data_matches_the_emulation(cuda, reset_rows, hidden):
    import torch
    rng = np.random.default_rng(17)
    act = _uniform_actor(rng, hidden, 20, cuda)
    a = act(reset_rows)
    torch.cuda.synchronize()
    a_ref, _ = act.emulate(reset_rows.cpu().numpy())
    err = np.abs(a.cpu().numpy().astype(np.float64) / SCALE - a_ref / SCALE).max()
    print("ctr_actor vs emulate, hidden %s: max |d action / scale| = %.3g" % (list(hidden), err))
    assert err <= 4 * MEASURED[hidden]


def test_a_bad_row_stays_in_its_env(cuda, reset_rows):
    import torch
    act = _uniform_actor(np.random.default_rng(3), (64, 96), 20, cuda)
    rows = reset_rows[:130].clone()
    a0, y0 = act(rows, logits=True)
    rows[7, 4] = float("nan")
    rows[100, 15] = 1e30
    a1, y1 = act(rows, logits=True)
    torch.cuda.synchronize()
    keep = torch.ones(130, dtype=torch.bool, device=cuda)
    keep[7] = keep[100] = False
    assert torch.equal(a0[keep], a1[keep]) and torch.equal(y0[keep], y1[keep])
    for i in (7, 100):
        assert not torch.equal(y0[i], y1[i])


def test_actions_do_not_depend_on_the_order_or_the_batch(cuda, reset_rows):
    import torch
    act = _uniform_actor(np.random.default_rng(4), (128, 128, 128), 20, cuda)
    a = act(reset_rows)
    perm = torch.tensor(np.random.default_rng(5).permutation(300), device=cuda)
    b = act(reset_rows[perm])
    c = act(reset_rows[:65])
    torch.cuda.synchronize()
    assert torch.equal(a[perm], b)
    assert torch.equal(a[:65], c)


def test_from_torch_and_act(cuda, reset_rows):
    import torch
    import torch.nn as nn
    from ctr_reach_amd import CtrReachVecEnv
    from ctr_reach_amd.policy import MlpActor
    torch.manual_seed(0)
    seq = nn.Sequential(nn.Linear(20, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, 6), nn.Tanh())
    act = MlpActor.from_torch(seq, SCALE, cuda)
    env = CtrReachVecEnv(300, device=cuda, seed=5, select_systems=[0, 1, 2, 3])
    env.reset()
    a = env.act(act)
    torch.cuda.synchronize()
    with torch.no_grad():
        ref = seq(env.actor_rows().cpu()).numpy() * SCALE
    assert a.shape == (300, 6) and a.dtype == torch.float32
    assert np.abs(a.cpu().numpy() / SCALE - ref / SCALE).max() < 0.02      # bf16 against f32: the same policy
    one = CtrReachVecEnv(8, device=cuda, seed=5)
    one.reset()
    with pytest.raises(ValueError):
        one.act(act)                                                       # 19 inputs wanted there
