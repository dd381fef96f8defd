"""What the DdpgLearner tests share (not a test module): the networks with torch's default init, the
U(-1, 1) batch, and the example's two loss expressions with autograd on the CPU in a chosen
precision."""
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
