"""What the DdpgLearner tests share (not a test module): the networks with torch's default init, the
U(-1, 1) batch, and the example's two loss expressions with autograd on the CPU in a chosen
precision; a batch kept clear of the relu's kink row by row (``make_clear``), also under a saturated
policy; networks and batches of small integers on which both steps are exact (``integer_case``); and
the cases of tests/test_gpu_ddpg_edges.py."""
import collections
import copy
import functools

import numpy as np

T = 16                  # rows of a tile of k_ddpg_grad (csrc/ctr_ddpg.inc: DDPG_T)
SLOTS = 64              # workgroups of a launch at most: from T * SLOTS rows on, a workgroup sums several tiles

# (actor hidden, critic hidden, the actor's in_dim)
SHAPES = [((32,), (32,), 19), ((64, 96), (64, 96), 20), ((128, 128, 128), (256, 128), 19), ((32, 256, 32), (32,), 20)]


def mlp(n_in, hidden, n_out, tanh):
    import torch.nn as nn
    dims = [n_in] + list(hidden)
    mods = []
    for a, b in zip(dims[:-1], dims[1:]):
        mods += [nn.Linear(a, b), nn.ReLU()]
    mods.append(nn.Linear(dims[-1], n_out))
    if tanh:
        mods.append(nn.Tanh())
    return nn.Sequential(*mods)


def make(seed, a_hidden, c_hidden, in_dim, B):
    """(policy, critic, rows, actions, target) on the CPU in float32: torch's default init, U(-1, 1)
    data.  The data come from a generator of their own, seeded 1000 + seed.  (With the data seeded
    like the networks, no seed below 50 met ``case``'s condition for the widest shape at B = 70: the
    best was 8.4e-6.  That shape has some 80 000 pre-activations per batch and a seed qualifies about
    one time in sixteen, so fifty seeds come up empty one time in twenty-five, and did.  The condition
    looks at the float64 reference only.)"""
    import torch
    g = torch.Generator().manual_seed(1000 + seed)
    state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    policy, critic = mlp(in_dim, a_hidden, 6, True), mlp(in_dim + 6, c_hidden, 1, False)
    torch.random.set_rng_state(state)
    rows, actions, target = (torch.rand(shape, generator=g) * 2 - 1 for shape in ((B, in_dim), (B, 6), (B,)))
    return policy.requires_grad_(False), critic.requires_grad_(False), rows, actions, target


def autograd(policy, critic, rows, actions, target, dtype):
    """The example's critic loss and policy loss from the same parameters, with their gradients, in
    ``dtype`` on the CPU: dict(critic_loss, critic_grads, actor_loss, actor_grads, kink) with the
    gradients as [(gW, gb), ...] numpy arrays and kink the smallest |hidden pre-activation| met."""
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    policy, critic = (copy.deepcopy(n).to(dtype).requires_grad_(True) for n in (policy, critic))
    rows, actions, target = (t.to(dtype) for t in (rows, actions, target))
    kinks = []

    def hook(mod, inp, out):
        kinks.append(float(inp[0].detach().abs().min()))

    for net in (policy, critic):
        for m in net:
            if isinstance(m, nn.ReLU):
                m.register_forward_hook(hook)

    def grads(net):
        lin = [m for m in net if isinstance(m, nn.Linear)]
        out = [(m.weight.grad.detach().numpy().copy(), m.bias.grad.detach().numpy().copy()) for m in lin]
        net.zero_grad(set_to_none=True)
        return out

    critic_loss = F.mse_loss(critic(torch.cat((rows, actions), dim=1)).squeeze(1), target)
    critic_loss.backward()
    critic_grads = grads(critic)
    actor_loss = -critic(torch.cat((rows, policy(rows)), dim=1)).mean()
    actor_loss.backward()
    return dict(critic_loss=float(critic_loss.detach()), critic_grads=critic_grads, actor_loss=float(actor_loss.detach()),
                actor_grads=grads(policy), kink=min(kinks))


@functools.lru_cache(maxsize=None)
def case(a_hidden, c_hidden, in_dim, B, min_kink=1e-5, max_seeds=50):
    """The first seed from 0 upward whose float64 reference keeps every hidden pre-activation at least
    ``min_kink`` from the relu's kink (a flipped mask is another function, not a rounding):
    (seed, the make() tuple, the float64 reference, the float32 reference).  Computed once."""
    for seed in range(max_seeds):
        made = make(seed, a_hidden, c_hidden, in_dim, B)
        import torch
        ref64 = autograd(*made, dtype=torch.float64)
        if ref64["kink"] >= min_kink:
            return seed, made, ref64, autograd(*made, dtype=torch.float32)
    raise AssertionError("no seed below %d keeps the pre-activations %g from the kink" % (max_seeds, min_kink))


def to_device(net, device):
    return copy.deepcopy(net).to(device).requires_grad_(False)


def host(pairs):
    return [(a.detach().cpu().numpy().copy(), b.detach().cpu().numpy().copy()) for a, b in pairs]


def params(net):
    import torch.nn as nn
    return [(m.weight, m.bias) for m in net if isinstance(m, nn.Linear)]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# --- a batch clear of the relu's kink row by row -------------------------------------------------

Clear = collections.namedtuple("Clear", "made redrawn passes ref64 ref32")


def _np64(net):
    return [(W.detach().double().numpy(), b.detach().double().numpy()) for W, b in params(net)]


def _forward64(layers, x, tanh):
    """A network's pass in float64 numpy: (output, [hidden pre-activation, ...], [layer input, ...])."""
    pre, inputs = [], []
    for W, b in layers[:-1]:
        inputs.append(x)
        pre.append(x @ W.T + b)
        x = np.maximum(pre[-1], 0.0)
    inputs.append(x)
    y = x @ layers[-1][0].T + layers[-1][1]
    return (np.tanh(y) if tanh else y), pre, inputs


def actions64(policy, rows):
    """policy(rows) in float64 numpy."""
    return _forward64(_np64(policy), rows.double().numpy(), True)[0]


def row_kinks(policy, critic, rows, actions):
    """Per row, the smallest |hidden pre-activation| the float64 networks meet in policy(row),
    critic(row, action) and critic(row, policy(row)).  Each row's value depends on that row alone."""
    P, C = _np64(policy), _np64(critic)
    x, a = rows.double().numpy(), actions.double().numpy()
    pi, pre, _ = _forward64(P, x, True)
    for xa in (np.concatenate((x, a), axis=1), np.concatenate((x, pi), axis=1)):
        pre = pre + _forward64(C, xa, False)[1]
    return np.min([np.abs(z).min(axis=1) for z in pre], axis=0)


def make_clear(seed, a_hidden, c_hidden, in_dim, B, gain=1.0, min_kink=1e-5, max_passes=20):
    """``make``'s networks and batch, the policy's output layer (W and b) multiplied by ``gain``, and
    every row (rows[i], actions[i]) whose ``row_kinks`` value is below ``min_kink`` drawn again, pass
    after pass, until none is left: Clear(made, redrawn, passes, ref64, ref32) with redrawn the number of
    draws made again and ref64, ref32 ``autograd``'s references.  The new rows come from a generator
    of their own (seeded 5000 + seed), a row's passes do not see the other rows, and the targets stay.
    With gain 1 and nothing to draw again the batch is ``make``'s, bit for bit."""
    import torch
    policy, critic, rows, actions, target = make(seed, a_hidden, c_hidden, in_dim, B)
    W, b = params(policy)[-1]
    W.mul_(gain)
    b.mul_(gain)
    g = torch.Generator().manual_seed(5000 + seed)
    redrawn = passes = 0
    while True:
        bad = np.flatnonzero(row_kinks(policy, critic, rows, actions) < min_kink)
        if not len(bad):
            break
        assert passes < max_passes, "%d rows within %g of the kink after %d passes" % (len(bad), min_kink, passes)
        passes += 1
        redrawn += len(bad)
        idx = torch.from_numpy(bad)
        rows[idx] = torch.rand((len(bad), in_dim), generator=g) * 2 - 1
        actions[idx] = torch.rand((len(bad), 6), generator=g) * 2 - 1
    made = (policy, critic, rows, actions, target)
    return Clear(made, redrawn, passes, autograd(*made, dtype=torch.float64), autograd(*made, dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def case_clear(a_hidden, c_hidden, in_dim, B, gain=1.0, seed=0):
    """``make_clear`` computed once per case."""
    return make_clear(seed, a_hidden, c_hidden, in_dim, B, gain=gain)


# --- small integers: every product and every sum exact -------------------------------------------

Integer = collections.namedtuple("Integer", "made ref64 ref32 report")


def _thinned(rng, low, high, shape, density):
    return (rng.integers(low, high + 1, shape) * (rng.random(shape) < density)).astype(np.float32)


def integer_net(n_in, hidden, n_out, tanh, densities, seed, out_mult=1):
    """An ``mlp`` whose weights and biases are drawn from {-1, 0, 1} and kept with probability
    densities[l] (zero otherwise); the output layer is multiplied by ``out_mult``."""
    import torch
    assert len(densities) == len(hidden) + 1
    rng = np.random.default_rng(seed)
    net = mlp(n_in, hidden, n_out, tanh).requires_grad_(False)
    for l, ((W, b), density) in enumerate(zip(params(net), densities)):
        mult = out_mult if l == len(hidden) else 1
        for t in (W, b):
            t.copy_(torch.from_numpy(mult * _thinned(rng, -1, 1, tuple(t.shape), density)))
    return net


def _backward64(layers, pre, inputs, dz):
    """From dZ of the output layer down: ([(dW, db), ...], dX, the largest sum of absolute values
    among the products |dZ| |W|, |dZ|^T |H| and the column sums of |dZ|)."""
    grads, bound = [], 0.0
    for l in range(len(layers) - 1, -1, -1):
        W, h = layers[l][0], inputs[l]
        grads.append((dz.T @ h, dz.sum(axis=0)))
        bound = max(bound, (np.abs(dz).T @ np.abs(h)).max(), np.abs(dz).sum(axis=0).max(), (np.abs(dz) @ np.abs(W)).max())
        dz = dz @ W
        if l > 0:
            dz = dz * (pre[l - 1] > 0)
    return grads[::-1], dz, bound


def _forward_bound(layers, inputs):
    return max((np.abs(x) @ np.abs(W).T + np.abs(b)).max() for (W, b), x in zip(layers, inputs))


def integer_report(policy, critic, rows, actions, target):
    """The two steps on integer data restated in float64 numpy, with what decides whether any order of
    summation is exact: dict(bound: the largest sum of absolute values of any product either step
    forms (|X| |W|^T + |b| forward, |dZ| |W| and |dZ|^T |H| backward, the bias sums, the two losses'
    row sums), the backward ones in units of 1 / B; integral: every input, activation and B * dZ is an
    integer; critic_loss, critic_grads, actor_loss, actor_grads as ``autograd`` gives them; pi: the
    policy's actions)."""
    P, C = _np64(policy), _np64(critic)
    x, a, t = (v.double().numpy() for v in (rows, actions, target))
    B = len(x)
    out = {}
    # the critic's regression
    xa = np.concatenate((x, a), axis=1)
    q, pre, inputs = _forward64(C, xa, False)
    d = q[:, 0] - t
    out["critic_loss"] = float((d * d).sum() / B)
    dz = (2.0 / B * d)[:, None]
    out["critic_grads"], _, back = _backward64(C, pre, inputs, dz)
    bound = max(_forward_bound(C, inputs), B * back, (d * d).sum())
    integral = all(np.array_equal(v, np.rint(v)) for v in inputs + [q, B * dz])
    # the policy's ascent
    pi, ppre, pinputs = _forward64(P, x, True)
    q, pre, inputs = _forward64(C, np.concatenate((x, pi), axis=1), False)
    out["actor_loss"] = float(-q.sum() / B)
    _, dx, back = _backward64(C, pre, inputs, np.full((B, 1), -1.0 / B))
    da = dx[:, -6:] * (1.0 - pi * pi)
    out["actor_grads"], _, pback = _backward64(P, ppre, pinputs, da)
    bound = max(bound, _forward_bound(P, pinputs), _forward_bound(C, inputs), B * back, B * pback, np.abs(q).sum())
    integral = integral and all(np.array_equal(v, np.rint(v)) for v in pinputs + inputs + [pi, q, B * da])
    out.update(bound=float(bound), integral=bool(integral), pi=pi)
    return out


def integer_data(in_dim, B, seed):
    """(rows from {-2..2}, actions from {-1, 0, 1}, targets from {-8..8}) as float32 tensors."""
    import torch
    rng = np.random.default_rng([seed, 1])
    return tuple(torch.from_numpy(rng.integers(-k, k + 1, shape).astype(np.float32))
                 for k, shape in ((2, (B, in_dim)), (1, (B, 6)), (8, (B,))))


def integer_critic(c_hidden, c_in, densities, seed):
    return integer_net(c_in, c_hidden, 1, False, densities, [seed, 2])


def integer_check(made):
    """Integer(made, float64 autograd, float32 autograd, ``integer_report``) of a (policy, critic,
    rows, actions, target) on integer data."""
    import torch
    return Integer(made, autograd(*made, dtype=torch.float64), autograd(*made, dtype=torch.float32), integer_report(*made))


@functools.lru_cache(maxsize=None)
def integer_case(a_hidden, c_hidden, in_dim, B, densities, seed):
    """Networks and a batch of small integers on which both steps are exact in any order of summation
    (``integer_report``'s bound below 2^24 is the condition, the caller's to assert): densities =
    (the policy's per layer, the critic's per layer); the policy's output layer is multiplied by 20,
    so that every tanh is exactly 0 or +-1 in float32 and in float64 and 1 - a * a exactly 1 or 0.
    B a power of two.  Computed once."""
    assert B & (B - 1) == 0
    policy = integer_net(in_dim, a_hidden, 6, True, densities[0], [seed, 0], out_mult=20)
    critic = integer_critic(c_hidden, in_dim + 6, densities[1], seed)
    return integer_check((policy, critic) + integer_data(in_dim, B, seed))


@functools.lru_cache(maxsize=None)
def integer_twin(h1, h2, in_dim, B, densities1, densities2, seed):
    """TD3's critic step on integer data: one batch, a [32] policy and two critics drawn from different
    seeds, each with its own references: (Integer of critic 1, Integer of critic 2)."""
    one = integer_case((32,), h1, in_dim, B, ((.5, .5), densities1), seed)
    policy, _, rows, actions, target = one.made
    return one, integer_check((policy, integer_critic(h2, in_dim + 6, densities2, seed + 1), rows, actions, target))


@functools.lru_cache(maxsize=None)
def integer_tail_case(a_hidden, c_hidden, in_dim, densities, seed):
    """B = T * SLOTS + T = 1 040, which is no power of two: ``integer_case`` at B = 1 024 with its rows
    0..15 once more behind it, so that slot 0 alone gets a second, whole tile.  The forward passes stay
    exact; 2 / B and 1 / B are rounded, so the gradients are not.  (made, ref64, ref32)."""
    import torch
    policy, critic, rows, actions, target = integer_case(a_hidden, c_hidden, in_dim, T * SLOTS, densities, seed).made
    made = (policy, critic) + tuple(torch.cat((t, t[:T])) for t in (rows, actions, target))
    return made, autograd(*made, dtype=torch.float64), autograd(*made, dtype=torch.float32)


# The cases of tests/test_gpu_ddpg_edges.py, whose conditions tests/test_host_ddpg_ref.py checks without a GPU.
# (actor hidden, critic hidden, in_dim, B): past T * SLOTS rows with a ragged tile; 2 101 = 2 * 1 024 + 3 * 16 + 5:
# two tiles in every slot, a third in three of them, the last one ragged
CLEAR_CASES = [(a, c, d, T * SLOTS + 5) for a, c, d in SHAPES]
CLEAR_CASES += [(a, c, d, 2 * T * SLOTS + 3 * T + 5) for a, c, d in (SHAPES[2], SHAPES[1])]
GAIN = 100.0            # of the saturated policy's output layer
SATURATED_CASES = [((64, 96), (64, 96), 20, 70), ((64, 96), (64, 96), 20, T * SLOTS + 5), ((128, 128, 128), (256, 128), 19, 70)]
# (actor hidden, critic hidden, in_dim, B, (the policy's densities, the critic's), seed); the last two: the
# last B with one tile in every slot, and DDPG_MAX_B with 64 tiles in every slot
INTEGER_CASES = [((32,), (32,), 19, 2048, ((.5, .5), (.5, .5)), 0),
                 ((64, 96), (64, 96), 20, 2048, ((.3, .15, .15), (.3, .15, .15)), 0),
                 ((128, 128, 128), (256, 128), 19, 4096, ((.3, .08, .06, .06), (.3, .06, .08)), 0),
                 ((32, 256, 32), (32,), 20, 4096, ((.3, .15, .1, .15), (.5, .5)), 0),
                 ((32,), (32,), 20, T * SLOTS, ((.5, .5), (.5, .5)), 0),
                 ((32,), (32,), 19, 65536, ((.5, .5), (.5, .5)), 0)]
TAIL_CASE = ((32,), (32,), 20, ((.5, .5), (.5, .5)), 0)
# (critic 1's hidden, critic 2's, in_dim, B, critic 1's densities, critic 2's, seed)
TWIN_CASES = [((64, 96), (256, 128), 20, 2048, (.3, .15, .15), (.3, .06, .08), 0),
              ((32,), (32,), 19, 2048, (.5, .5), (.5, .5), 0)]
