"""GaussianActor.sample (ctr_gauss_act) on the GPU.

The 12 rows of the head and their bias are pinned on integer data, on which every product, sum and
bf16 rounding is exact; rows 0..5 are the 6-row actor's logits bit for bit.  On random data ``unit``,
``action`` and ``logp`` are recomputed in float64 from the kernel's own logits and the exact
uniforms; the bar is 4 times the error that the numpy float32 restatement of the same formulas
(policy.gauss_head, GaussianActor.gaussians in float32) shows against that float64 result on the
same inputs -- computed here and printed (the device's expf, tanhf, log1pf, logf and sincosf are
within a few ulp of numpy's).  The noise is a pure function of (seed, counter, row_base + row)."""
import numpy as np
import pytest

import ddpg_ref as R

pytestmark = pytest.mark.gpu

SCALE = np.array([0.001, 0.002, 0.003, 0.087, 0.05, 3.0], dtype=np.float32)
SHAPES = [((32,), 19), ((64, 96), 20), ((128, 128, 128), 19)]
NS = [1, 65, 300]                        # a ragged wave; two waves; several workgroups
CASES = [(h, d, n) for h, d in SHAPES for n in NS]


def _random_layers(rng, hidden, in_dim):
    dims = [in_dim] + list(hidden) + [12]
    return [((rng.uniform(-1, 1, (o, i)) * np.sqrt(3.0 / i)).astype(np.float32), rng.uniform(-.2, .2, o).astype(np.float32))
            for i, o in zip(dims[:-1], dims[1:])]


def _policy(cuda, layers, seed=7):
    from ctr_reach_amd.policy import GaussianActor
    return GaussianActor(layers, SCALE, cuda, seed=seed)


def _rows(rng, n, in_dim, cuda):
    import torch
    return torch.from_numpy(rng.uniform(-1, 1, (n, in_dim)).astype(np.float32)).to(cuda)


def _host(out):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


# --- integer data: the placement of the 12 rows and of their bias --------------------------------

def _integer_layers(rng, hidden, in_dim, only_row=None):
    """Weights, biases and (below) rows of small integers with every hidden pre-activation a positive
    integer of at most 256: the relu passes it and bf16 holds it exactly."""
    layers = [(rng.integers(-1, 2, (hidden[0], in_dim)).astype(np.float32), rng.integers(20, 24, hidden[0]).astype(np.float32))]
    for a, b in zip(hidden[:-1], hidden[1:]):
        W = np.zeros((b, a), dtype=np.float32)
        for r in range(b):
            W[r, rng.choice(a, 2, replace=False)] = 1
        layers.append((W, rng.integers(1, 4, b).astype(np.float32)))
    W = np.zeros((12, hidden[-1]), dtype=np.float32)
    for r in range(12):
        W[r, rng.choice(hidden[-1], 3, replace=False)] = rng.choice([-1.0, 1.0], 3)
    bias = (np.arange(12) - 5).astype(np.float32)                # a different one per row
    if only_row is not None:
        keep = W[only_row].copy()
        W[:] = 0
        W[only_row] = keep
    layers.append((W, bias))
    return layers


def _forward64(layers, x):
    z = x.astype(np.float64)
    for l, (W, b) in enumerate(layers):
        z = z @ W.astype(np.float64).T + b
        if l < len(layers) - 1:
            assert z.min() >= 1 and z.max() <= 256 and np.array_equal(z, np.rint(z))
    return z


@pytest.mark.parametrize("hidden,in_dim,n", CASES)
def test_integer_data_gives_all_12_logits_exactly(cuda, hidden, in_dim, n):
    import torch
    rng = np.random.default_rng([n, in_dim])
    layers = _integer_layers(rng, hidden, in_dim)
    rows = rng.integers(-1, 2, (n, in_dim)).astype(np.float32)
    want = _forward64(layers, rows)
    assert np.abs(want).max() > 6 and all(np.ptp(want[:, i]) > 0 or n == 1 for i in range(12))
    out = _host(_policy(cuda, layers).sample(torch.from_numpy(rows).to(cuda), 0, deterministic=True, logits=True))
    assert out["logits"].shape == (n, 12)
    assert np.array_equal(out["logits"].astype(np.float64), want)


def test_integer_weights_in_one_row_of_the_log_std_at_a_time(cuda):
    import torch
    for only in range(6, 12):
        rng = np.random.default_rng(only)
        layers = _integer_layers(rng, (64, 32), 20, only_row=only)
        rows = rng.integers(-1, 2, (65, 20)).astype(np.float32)
        want = _forward64(layers, rows)
        others = [i for i in range(12) if i != only]
        assert np.ptp(want[:, only]) > 0 and np.array_equal(want[:, others], np.tile((np.arange(12) - 5.0)[others], (65, 1)))
        out = _host(_policy(cuda, layers).sample(torch.from_numpy(rows).to(cuda), 0, deterministic=True, logits=True))
        assert np.array_equal(out["logits"].astype(np.float64), want), only


# --- the 6-row actor --------------------------------------------------------------------------------

@pytest.mark.parametrize("hidden,in_dim,n", CASES)
def test_mean_rows_are_the_six_row_actor_bit_for_bit(cuda, hidden, in_dim, n):
    rng = np.random.default_rng([1, n, in_dim])
    pi = _policy(cuda, _random_layers(rng, hidden, in_dim))
    rows = _rows(rng, n, in_dim, cuda)
    out = pi.sample(rows, 5, deterministic=True, logits=True)
    act, lg = pi.mean_actor()(rows, logits=True)
    out, act, lg = _host(out), act.cpu().numpy(), lg.cpu().numpy()
    assert np.abs(lg).max() > 0
    assert np.array_equal(R.bits(out["logits"][:, :6]), R.bits(lg))
    assert np.array_equal(R.bits(out["action"]), R.bits(act))


# --- random data: the head's formulas -----------------------------------------------------------------

def _check_head(pi, out, counter, row_base, deterministic, capsys, tag):
    """The device's unit, action and logp against the float64 formulas on its own logits; returns the
    report's figures {name: (device error, numpy float32 error)}."""
    from ctr_reach_amd.policy import gauss_head
    y = out["logits"]
    n = len(y)
    index = row_base + np.arange(n)
    zero = np.zeros((n, 6))
    want = gauss_head(y.astype(np.float64), zero if deterministic else pi.gaussians(counter, index), SCALE)
    f32 = gauss_head(y, zero if deterministic else pi.gaussians(counter, index, np.float32), SCALE, np.float32)
    figures = {}
    for name in ("unit", "action", "logp"):
        assert out[name].dtype == np.float32 and np.isfinite(out[name]).all(), name
        figures[name] = (float(np.abs(out[name].astype(np.float64) - want[name]).max()),
                         float(np.abs(f32[name].astype(np.float64) - want[name]).max()))
    with capsys.disabled():
        print("\n%s: " % tag + "; ".join("%s %.3g (numpy f32 %.3g)" % ((k,) + v) for k, v in figures.items()))
    bad = {k: v for k, v in figures.items() if not v[0] <= 4 * v[1]}
    assert not bad, bad
    return want


@pytest.mark.parametrize("hidden,in_dim,n", [c for c in CASES if c[2] > 1])
def test_random_data_against_the_float64_formulas(cuda, capsys, hidden, in_dim, n):
    rng = np.random.default_rng([2, n, in_dim])
    pi = _policy(cuda, _random_layers(rng, hidden, in_dim))
    rows = _rows(rng, n, in_dim, cuda)
    counter = (9 << 32) | 1234
    out = _host(pi.sample(rows, counter, row_base=1000, logits=True))
    want = _check_head(pi, out, counter, 1000, False, capsys, "%s, in_dim %d, n %d" % (list(hidden), in_dim, n))
    assert np.abs(want["unit"]).max() > 0.5 and np.ptp(want["logp"]) > 1


def test_one_row(cuda):
    """n = 1: a single lane of a ragged wave; its results are row 0's of a larger call, bit for bit."""
    rng = np.random.default_rng(3)
    pi = _policy(cuda, _random_layers(rng, (64, 96), 20))
    rows = _rows(rng, 65, 20, cuda)
    one, many = _host(pi.sample(rows[:1], 3, logits=True)), _host(pi.sample(rows, 3, logits=True))
    for k in one:
        assert np.array_equal(R.bits(one[k]), R.bits(many[k][:1])), k


# --- a pure function of (seed, counter, row_base + row) ---------------------------------------------

def test_noise_is_a_pure_function_of_seed_counter_and_row(cuda):
    import torch
    rng = np.random.default_rng(4)
    pi = _policy(cuda, _random_layers(rng, (64, 96), 19))
    rows = _rows(rng, 300, 19, cuda)
    whole = _host(pi.sample(rows, 11, logits=True))
    first, second = _host(pi.sample(rows[:130], 11, logits=True)), _host(pi.sample(rows[130:], 11, row_base=130, logits=True))
    for k in whole:
        assert np.array_equal(R.bits(whole[k]), R.bits(np.concatenate((first[k], second[k])))), k
    other = _host(pi.sample(rows, 12))
    assert (other["action"] != whole["action"]).any(axis=1).all()
    assert (_host(pi.sample(rows[130:], 11))["action"] != second["action"]).any(axis=1).all()      # row_base matters
    # another seed: another draw
    layers = [(torch.from_numpy(W), torch.from_numpy(b)) for W, b in zip(pi.weights, pi.biases)]
    assert (_host(_policy(cuda, layers, seed=8).sample(rows, 11))["action"] != whole["action"]).any(axis=1).all()
    # deterministic: nothing is drawn
    det = [_host(pi.sample(rows, c, row_base=b, deterministic=True, logits=True)) for c, b in ((11, 0), (12, 7))]
    for k in det[0]:
        assert np.array_equal(R.bits(det[0][k]), R.bits(det[1][k])), k
    assert np.array_equal(R.bits(det[0]["logits"]), R.bits(whole["logits"]))


def test_deterministic_head(cuda, capsys):
    rng = np.random.default_rng(5)
    pi = _policy(cuda, _random_layers(rng, (32,), 20))
    out = _host(pi.sample(_rows(rng, 300, 20, cuda), 1, deterministic=True, logits=True))
    _check_head(pi, out, 1, 0, True, capsys, "deterministic")


# --- saturation and the clip ------------------------------------------------------------------------

def test_saturated_means(cuda, capsys):
    rng = np.random.default_rng(6)
    layers = _random_layers(rng, (64, 96), 19)
    layers[-1][0][:6] = 0
    layers[-1][1][:6] = [40, -40, 40, -40, 40, -40]
    pi = _policy(cuda, layers)
    out = _host(pi.sample(_rows(rng, 300, 19, cuda), 2, logits=True))
    sign = np.array([1, -1, 1, -1, 1, -1], dtype=np.float32)
    assert np.array_equal(out["logits"][:, :6], np.tile(40 * sign, (300, 1)))
    assert np.array_equal(out["unit"], np.tile(sign, (300, 1)))
    assert np.array_equal(out["action"], np.tile(sign * SCALE, (300, 1)))
    assert np.isfinite(out["logp"]).all() and out["logp"].max() > 400
    _check_head(pi, out, 2, 0, False, capsys, "means of +-40")


def test_clipped_log_std(cuda, capsys):
    rng = np.random.default_rng(7)
    layers = _random_layers(rng, (64, 96), 20)
    layers[-1][0][6:10] = 0
    layers[-1][1][6:10] = [5, -25, 5, -25]
    pi = _policy(cuda, layers)
    out = _host(pi.sample(_rows(rng, 300, 20, cuda), 3, logits=True))
    assert np.array_equal(out["logits"][:, 6:10], np.tile(np.float32([5, -25, 5, -25]), (300, 1)))
    want = _check_head(pi, out, 3, 0, False, capsys, "log std of +5 and -25")
    assert np.array_equal(want["s"][:, :4], np.tile([2.0, -20.0, 2.0, -20.0], (300, 1)))
    # s = 2 and -20 and nothing else: the unclipped values are far outside the bar
    unclipped = out["logits"].astype(np.float64)
    eps = pi.gaussians(3, np.arange(300))
    raw = np.tanh(unclipped[:, :6] + np.exp(unclipped[:, 6:]) * eps)
    assert np.abs(raw[:, 0] - out["unit"][:, 0]).max() > 1e-2
    # where s = -20 the noise is gone: the action is the mean's, to the last bits of exp(-20) eps
    assert np.abs(out["unit"][:, 1] - np.tanh(unclipped[:, 1])).max() < 1e-6


# --- load_ --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hidden,in_dim", SHAPES)
def test_load_gives_the_host_pack_of_the_new_parameters(cuda, hidden, in_dim):
    import torch
    from ctr_reach_amd.policy import GaussianActor
    torch.manual_seed(in_dim)
    seq = R.mlp(in_dim, hidden, 12, False).requires_grad_(False)
    dev = R.to_device(seq, cuda)
    pi = GaussianActor.from_torch(seq, SCALE, cuda)
    mean = pi.mean_actor()
    with torch.no_grad():
        for p in dev.parameters():
            p.mul_(1.5).add_(0.01)
    pi.load_(dev)
    torch.cuda.synchronize()
    want = GaussianActor.from_torch(R.to_device(dev, "cpu"), SCALE)._pack_host()
    assert np.array_equal(pi.blob.cpu().numpy(), want)
    assert pi.weights is None
    # the mean actor follows on its next use, from the same device tensors
    rows = _rows(np.random.default_rng(0), 65, in_dim, cuda)
    again = pi.mean_actor()
    assert again is mean
    got = pi.sample(rows, 0, deterministic=True)["action"]
    assert np.array_equal(R.bits(got.cpu().numpy()), R.bits(again(rows).cpu().numpy()))
