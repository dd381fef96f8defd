"""ctr_actor (the MLP actor as a kernel of its own) against MlpActor.emulate, the CPU reference of its
arithmetic: exactly on data where every value of the specification is a small integer (the
fragment-layout test: its logits depend on every input feature and on most units of every k-step
fragment), within the measured f32-accumulation difference on random data, over both halves of
the width range; an env's action depends on its own row only; large logits saturate."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(32,), (64, 96), (128, 128, 128)]
# the upper half of the width range: 8; 8 -> 4; 7 -> 5; 5 -> 6 -> 1; 1 -> 8 -> 1 row tiles (the blobs are
# 33 920, 91 776, 97 920, 87 680 and 38 272 B of the 98 304 B an actor may take)
WIDE = [(256,), (256, 128), (224, 160), (160, 192, 32), (32, 256, 32)]
SCALE = np.array([0.001, 0.001, 0.001, 0.087, 0.087, 0.087])


def _integer_actor(rng, hidden, in_dim, device):
    """Small integers everywhere, and every input column of every layer read by some row: row i of a
    hidden layer reads columns i, i + fout, ... (column i mod fin where the layer widens) and 0..3
    further ones, all with +-1; first-layer biases in -2..2, later ones in 0..3 (units are not stuck
    at zero).  The output layer is dense, weights in -8..8, with an integer bias."""
    from ctr_reach_amd.policy import MlpActor
    dims = [in_dim] + list(hidden) + [6]
    layers = []
    for l in range(len(hidden)):
        fin, fout = dims[l], dims[l + 1]
        W = np.zeros((fout, fin), dtype=np.float32)
        for i in range(fout):
            cols = np.arange(i % fin, fin, fout) if fout < fin else np.array([i % fin])
            if l == 0:                                   # |pre-activation| <= 2 * 4 + 2
                cols = np.union1d(cols, rng.choice(fin, size=rng.integers(0, 4), replace=False))
            W[i, cols] = rng.choice([-1.0, 1.0], size=cols.size)
            if l:
                extra = rng.choice(fin, size=rng.integers(0, 4), replace=False)
                W[i, extra] = rng.choice([-1.0, 1.0], size=extra.size)
        b = rng.integers(-2, 3, fout) if l == 0 else rng.integers(0, 4, fout)
        layers.append((W, b.astype(np.float32)))
    layers.append((rng.integers(-8, 9, (6, dims[-2])).astype(np.float32), rng.integers(-8, 9, 6).astype(np.float32)))
    return MlpActor(layers, SCALE, device=device)


def _observable(act, rows):
    """From the reference alone: which input features, and how many units of every 16-unit group
    (one k-step fragment) of every hidden layer, change some logit of `rows` when their outgoing
    weights are zeroed.  -> (bool [in_dim], [int [width / 16] per hidden layer])"""
    y0 = act.emulate(rows)[1]
    hidden = [h.astype(np.float64) for h in act.last_hidden]
    W = [w.astype(np.float64) for w in act.weights]
    b = [v.astype(np.float64) for v in act.biases]

    def logits_from(l, h):
        # the layers after hidden layer l, on integers (where float64 is emulate's arithmetic)
        for m in range(l + 1, len(W) - 1):
            h = np.maximum(h @ W[m].T + b[m], 0.0)
        return h @ W[-1].T + b[-1]

    def without(a, u):
        a = a.copy()
        a[:, u] = 0
        return a

    assert all(np.array_equal(logits_from(l, h), y0) for l, h in enumerate(hidden))
    # (zeroing a feature's weights is zeroing the feature)
    feats = np.array([not np.array_equal(act.emulate(without(rows, f))[1], y0) for f in range(act.in_dim)])
    groups = [np.array([not np.array_equal(logits_from(l, without(h, u)), y0) for u in range(h.shape[1])])
              .reshape(-1, 16).sum(axis=1) for l, h in enumerate(hidden)]
    return feats, groups


@pytest.mark.parametrize("in_dim", [19, 20])
@pytest.mark.parametrize("hidden", SHAPES + WIDE)
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
        if n == 300:
            # ... and under which a wrong fragment anywhere shows: the logits of these rows depend on
            # every input feature and on at least half of every k-step fragment's units
            feats, groups = _observable(act, rows)
            assert feats.all(), np.flatnonzero(~feats)
            assert all(g.min() >= 8 for g in groups), [g.tolist() for g in groups]
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
# the wide shapes, measured the same way (against emulate, on these rows)
MEASURED.update({(256,): 9.047e-08, (256, 128): 2.479e-08, (224, 160): 3.637e-08, (160, 192, 32): 1.886e-08,
                 (32, 256, 32): 2.810e-07})
# the weight seed: 17, or the next one whose network has no flipped bf16 rounding on these rows (a
# flip shows as a difference above 1e-5, is not accumulation order and is not what is pinned):
# [224, 160] gave 1.72e-5 with seed 17
SEED = {(224, 160): 18}


@pytest.mark.parametrize("hidden", SHAPES + WIDE)
def test_random_data_matches_the_emulation(cuda, reset_rows, hidden):
    import torch
    rng = np.random.default_rng(SEED.get(hidden, 17))
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
    for hidden in ((128, 128, 128), (224, 160)):
        act = _uniform_actor(np.random.default_rng(4), hidden, 20, cuda)
        a = act(reset_rows)
        perm = torch.tensor(np.random.default_rng(5).permutation(300), device=cuda)
        b = act(reset_rows[perm])
        c = act(reset_rows[:65])
        torch.cuda.synchronize()
        assert torch.equal(a[perm], b), hidden
        assert torch.equal(a[:65], c), hidden


def test_large_logits_saturate_to_the_scale(cuda, reset_rows):
    """Output biases of +-30, +-100 and +-1e4 over zero hidden weights: the actions are +-scale (the
    reference is scale * tanh(y) in float64, rounded to float32), finite and inside the box."""
    import torch
    from ctr_reach_amd.policy import MlpActor
    bias = np.array([30.0, -30.0, 100.0, -100.0, 1e4, -1e4], dtype=np.float32)
    layers = [(np.zeros((32, 20), dtype=np.float32), np.zeros(32, dtype=np.float32)),
              (np.zeros((6, 32), dtype=np.float32), bias)]
    act = MlpActor(layers, SCALE, device=cuda)
    a, y = act(reset_rows[:65], logits=True)
    torch.cuda.synchronize()
    a, y = a.cpu().numpy(), y.cpu().numpy()
    ref = (SCALE * np.tanh(bias.astype(np.float64))).astype(np.float32)
    assert np.array_equal(ref, (np.sign(bias) * SCALE).astype(np.float32))
    assert np.array_equal(y, np.tile(bias, (65, 1)))
    assert np.isfinite(a).all() and (np.abs(a) <= SCALE.astype(np.float32)).all()
    assert np.allclose(a, np.tile(ref, (65, 1)), rtol=0, atol=2e-7)


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
