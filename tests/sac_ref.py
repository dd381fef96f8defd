"""What the SacLearner / GaussianActor tests share (not a test module; ``ddpg_ref`` has the networks
and the small helpers): SAC's policy loss under CPU autograd in a chosen precision with the noise
passed in, and ``case``: networks with torch's default init and a U(-1, 1) batch whose float64
reference stays clear of the three places where a rounding would change the function -- a relu's
kink, the minimum of the two critics, the clip of the log standard deviation."""
import copy
import functools

import numpy as np

import ddpg_ref as R

T, SLOTS = R.T, R.SLOTS
ALPHA = 0.2
TARGET_ENTROPY = -6.0
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0

# (policy hidden, critic 1 hidden, critic 2 hidden, the policy's in_dim)
SHAPES = [((32,), (32,), (32,), 19), ((64, 96), (64, 96), (96, 32), 20), ((128, 128, 128), (128, 64), (64, 128), 19),
          ((32, 256, 32), (32,), (64,), 20)]
MIXED = [SHAPES[0], SHAPES[1], SHAPES[3]]            # shapes on which both critics give the minimum on some rows


def make(seed, p_hidden, c1_hidden, c2_hidden, in_dim, B):
    """(policy with a 12-row head, critic1, critic2, rows) on the CPU in float32: torch's default init,
    U(-1, 1) rows from a generator of their own (seeded 1000 + seed, as ``ddpg_ref.make``)."""
    import torch
    g = torch.Generator().manual_seed(1000 + seed)
    state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    policy = R.mlp(in_dim, p_hidden, 12, False)
    critic1, critic2 = R.mlp(in_dim + 6, c1_hidden, 1, False), R.mlp(in_dim + 6, c2_hidden, 1, False)
    torch.random.set_rng_state(state)
    rows = torch.rand((B, in_dim), generator=g) * 2 - 1
    return policy.requires_grad_(False), critic1.requires_grad_(False), critic2.requires_grad_(False), rows


def eps_for(B, seed=0, counter=0, dtype=np.float64):
    """The learner's noise for rows 0..B-1 of draw (seed, counter): GaussianActor's Python restatement
    (exact uniforms, Box-Muller in ``dtype``)."""
    from ctr_reach_amd.policy import GaussianActor
    draw = GaussianActor.__new__(GaussianActor)
    draw.seed = seed
    return draw.gaussians(counter, np.arange(B), dtype)


def autograd(policy, critic1, critic2, rows, eps, alpha, dtype, target_entropy=TARGET_ENTROPY):
    """SAC's policy loss mean(alpha * logp - min(Q1, Q2)) from ``eps`` [B, 6] (float64 numpy), with its
    gradients, in ``dtype`` on the CPU: dict(loss, grads [(gW, gb), ...], logp_mean, alpha_grad, kink,
    gap: the smallest |Q1 - Q2|, clip: the smallest distance of a y[6+i] from -20 and 2, share: the
    fraction of rows on which critic 1 is the minimum)."""
    import torch
    import torch.nn as nn
    policy, critic1, critic2 = (copy.deepcopy(n).to(dtype) for n in (policy, critic1, critic2))
    policy.requires_grad_(True)
    rows = rows.to(dtype)
    eps = torch.from_numpy(np.asarray(eps, dtype=np.float64)).to(dtype)
    kinks = []

    def hook(mod, inp, out):
        kinks.append(float(inp[0].detach().abs().min()))

    for net in (policy, critic1, critic2):
        for m in net:
            if isinstance(m, nn.ReLU):
                m.register_forward_hook(hook)
    y = policy(rows)
    mu, raw = y[:, :6], y[:, 6:]
    s = torch.clamp(raw, LOG_STD_MIN, LOG_STD_MAX)
    u = mu + torch.exp(s) * eps
    t = torch.tanh(u)
    logp = (-0.5 * eps * eps - s - 0.5 * np.log(2 * np.pi)).sum(dim=1) \
        - (2.0 * (np.log(2.0) - u - nn.functional.softplus(-2.0 * u))).sum(dim=1)
    xa = torch.cat((rows, t), dim=1)
    q1, q2 = critic1(xa).squeeze(1), critic2(xa).squeeze(1)
    loss = (alpha * logp - torch.minimum(q1, q2)).mean()
    loss.backward()
    grads = [(m.weight.grad.detach().numpy().copy(), m.bias.grad.detach().numpy().copy())
             for m in policy if isinstance(m, nn.Linear)]
    logp_mean = logp.detach().mean()
    alpha_grad = float(-(logp_mean + target_entropy))        # in ``dtype`` too: the gradient of -log_alpha (logp_mean + target)
    logp_mean = float(logp_mean)
    raw = raw.detach()
    return dict(loss=float(loss.detach()), grads=grads, logp_mean=logp_mean, alpha_grad=alpha_grad,
                kink=min(kinks), gap=float((q1 - q2).detach().abs().min()),
                clip=float(torch.minimum((raw - LOG_STD_MIN).abs(), (raw - LOG_STD_MAX).abs()).min()),
                share=float((q1 <= q2).double().mean()))


def clear(ref64, min_kink=1e-5, min_gap=1e-4, min_clip=1e-3):
    return ref64["kink"] >= min_kink and ref64["gap"] >= min_gap and ref64["clip"] >= min_clip


@functools.lru_cache(maxsize=None)
def case(p_hidden, c1_hidden, c2_hidden, in_dim, B, alpha=ALPHA, swap=False, mixed=False, log_std=None, max_seeds=50):
    """The first seed from 0 upward whose float64 reference keeps every hidden pre-activation of the
    three networks 1e-5 from the relu's kink, every row's |Q1 - Q2| at least 1e-4 and every y[6+i] 1e-3
    from -20 and 2 (a flipped mask, minimum or clip is another function, not a rounding): (seed, the
    make() tuple, eps float64, the float64 reference, the float32 reference).  ``mixed``: the seed must
    also give critic 1 the minimum on 0.1 .. 0.9 of the rows, so that the selection is exercised (this,
    too, looks at the float64 reference only).  ``swap``: the two critics change places after ``make``
    (the same networks, the other one first).  ``log_std``: ``set_log_std_bias``'s values.  None of
    the conditions depends on alpha.  Computed once."""
    import torch
    for seed in range(max_seeds):
        policy, c1, c2, rows = make(seed, p_hidden, c1_hidden, c2_hidden, in_dim, B)
        if log_std is not None:
            set_log_std_bias(policy, log_std)
        if swap:
            c1, c2 = c2, c1
        made = (policy, c1, c2, rows)
        eps = eps_for(B)
        ref64 = autograd(*made, eps, alpha, torch.float64)
        if clear(ref64) and (not mixed or 0.1 <= ref64["share"] <= 0.9):
            return seed, made, eps, ref64, autograd(*made, eps, alpha, torch.float32)
    raise AssertionError("no seed below %d keeps clear of the kink, the minimum and the clip" % max_seeds)


def err(g, g64):
    return float(np.abs(np.asarray(g, dtype=np.float64) - g64).max() / np.abs(g64).max())


def set_log_std_bias(policy, values):
    """The policy's log-standard-deviation rows made constant: W_out[6 + i] = 0, b_out[6 + i] = values[i]
    for every i whose value is not None."""
    import torch
    W, b = R.params(policy)[-1]
    with torch.no_grad():
        for i, v in enumerate(values):
            if v is not None:
                W[6 + i].zero_()
                b[6 + i] = float(v)
