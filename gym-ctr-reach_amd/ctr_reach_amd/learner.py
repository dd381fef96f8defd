"""DDPG's two updates on the device (ctr_ddpg_critic_step / ctr_ddpg_actor_step,
include/ctr_reach_amd.h): forward, loss, backward and Adam of the critic's regression on the target
and of the policy's ascent on Q(s, pi(s)), two launches each, in float32 on the learner's own
parameters.  No autograd and no torch optimiser:

    learner = DdpgLearner(policy, critic, scale=venv.action_space.high)
    batch = buf.sample_td(256, actor_targ, critic_targ, gamma)
    learner.critic_step(batch["obs"], batch["action"], batch["target"])
    learner.actor_step(batch["obs"])
    polyak_([(actor_targ, policy, policy_targ), (critic_targ_dev, critic, critic_targ)], 0.001)

``Td3Learner`` is the same learner with TD3's two critics, both regressed by one call
(ctr_td3_critic_step).  ``SacLearner`` is SAC: the same twin critic step, and the stochastic policy's
step under both critics with the learned temperature (ctr_sac_actor_step).  Each learner's ``update``
makes a run of whole updates from one C call (ctr_ddpg_update for DDPG and TD3, ctr_sac_update for SAC),
bit for bit what the calls above leave.  ``adam_reference`` is the
numpy float32 restatement of the Adam step (the kernel gives its bits).
"""
import ctypes

import numpy as np

from . import _abi, _abi_critic


def adam_reference(p, g, m, v, pow, lr, betas=(0.9, 0.999), eps=1e-8):
    """One Adam step as the header states it, every operation a float32 numpy operation (one rounding
    each): (p', m', v', pow') from float32 arrays p, g, m, v and pow = [beta1^t, beta2^t]."""
    f = np.float32
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    b1, b2, lr, eps, one = f(betas[0]), f(betas[1]), f(lr), f(eps), f(1)
    pw = np.asarray(pow, dtype=f)
    pw1, pw2 = pw[0] * b1, pw[1] * b2
    m1 = (b1 * m) + ((one - b1) * g)
    v1 = (b2 * v) + (((one - b2) * g) * g)
    with np.errstate(all="ignore"):
        p1 = p - lr * ((m1 / (one - pw1)) / (np.sqrt(v1 / (one - pw2)) + eps))
    assert p1.dtype == m1.dtype == v1.dtype == f
    return p1, m1, v1, np.array([pw1, pw2], dtype=f)


def _layers_of(net, tanh, name):
    """[(W, b), ...] of an ``nn.Sequential`` (the parameters themselves) or of such a list."""
    import torch
    from .policy import _sequential_layers
    if isinstance(net, torch.nn.Module):
        return _sequential_layers(net, tanh, name, detach=False)
    layers = [tuple(pair) for pair in net]
    if any(len(pair) != 2 for pair in layers):
        raise ValueError("the %s is an nn.Sequential or a list of (W, b)" % name)
    return layers


def _masters(net, tanh, name, in_dims, out, in_msg):
    """The checks of ``_Mlp._device_layers`` on a learning network: every tensor a float32, contiguous
    torch tensor of its shape on one device that does not require grad (it is written in place, outside
    autograd); nothing is converted.  -> ([(W, b), ...] detached, in_dim, hidden)."""
    import torch
    layers = _layers_of(net, tanh, name)
    if not 2 <= len(layers) <= _abi.CTR_ACTOR_MAX_HIDDEN + 1:
        raise ValueError("the %s has 1..%d hidden layers and an output layer" % (name, _abi.CTR_ACTOR_MAX_HIDDEN))
    for l, (W, b) in enumerate(layers):
        for what, t in (("W", W), ("b", b)):
            if not isinstance(t, torch.Tensor):
                raise ValueError("%s layer %d: %s must be a torch tensor" % (name, l, what))
    W0 = layers[0][0]
    if W0.dim() != 2 or W0.shape[1] not in in_dims:
        raise ValueError(in_msg)
    in_dim = int(W0.shape[1])
    hidden = [int(W.shape[0]) for W, _ in layers[:-1]]
    for w in hidden:
        if w % 32 or not 32 <= w <= _abi.CTR_ACTOR_MAX_WIDTH:
            raise ValueError("%s: hidden widths must be multiples of 32 in 32..%d" % (name, _abi.CTR_ACTOR_MAX_WIDTH))
    dims = [in_dim] + hidden + [out]
    src, device = [], None
    for l, (W, b) in enumerate(layers):
        pair = []
        for what, t, shape in (("W", W, (dims[l + 1], dims[l])), ("b", b, (dims[l + 1],))):
            what = "%s layer %d: %s" % (name, l, what)
            if t.dtype != torch.float32:
                raise ValueError("%s must be float32, not %s" % (what, t.dtype))
            if tuple(t.shape) != shape:
                raise ValueError("%s must be %s, not %s" % (what, list(shape), list(t.shape)))
            if not t.is_contiguous():
                raise ValueError(what + " must be contiguous")
            if t.requires_grad:
                raise ValueError(what + " requires grad: the learner writes it in place, outside autograd")
            if device is not None and t.device != device:
                raise ValueError("%s is on %s, the rest of the %s on %s" % (what, t.device, name, device))
            device = t.device
            pair.append(t.detach())
        src.append(tuple(pair))
    return src, in_dim, hidden


class _Net(object):
    """One learning network: its masters, gradients, Adam state and their ctr_ddpg_net_t."""

    def __init__(self, params, alloc, lr, betas, eps):
        import torch
        from . import _abi_ddpg
        self.params = params
        self.grads = [(alloc(tuple(W.shape)), alloc(tuple(b.shape))) for W, b in params]
        self.m = [(alloc(tuple(W.shape)), alloc(tuple(b.shape))) for W, b in params]
        self.v = [(alloc(tuple(W.shape)), alloc(tuple(b.shape))) for W, b in params]
        self.pow = torch.ones(2, dtype=torch.float32, device=params[0][0].device)
        n = len(params)
        self.arrays = {}
        self.struct = s = _abi_ddpg.CtrDdpgNet()
        for field, src, which in (("W", params, 0), ("b", params, 1), ("gW", self.grads, 0), ("gb", self.grads, 1),
                                  ("mW", self.m, 0), ("mb", self.m, 1), ("vW", self.v, 0), ("vb", self.v, 1)):
            for pair in src:
                t = pair[which]
                if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.is_contiguous()
                        and t.device == params[0][0].device):
                    raise ValueError("alloc must return contiguous float32 tensors on the networks' device")
            self.arrays[field] = arr = (_abi._P * n)(*[pair[which].data_ptr() for pair in src])
            setattr(s, field, arr)
        s.pow = self.pow.data_ptr()
        self.adam = _abi_ddpg.CtrDdpgAdam(float(lr), float(betas[0]), float(betas[1]), float(eps))

    def state(self):
        return {"m": [(a.clone(), b.clone()) for a, b in self.m], "v": [(a.clone(), b.clone()) for a, b in self.v],
                "pow": self.pow.clone()}

    def load_state(self, state):
        for name, mine in (("m", self.m), ("v", self.v)):
            theirs = state[name]
            if len(theirs) != len(mine):
                raise ValueError("state: %s has %d layers, the network %d" % (name, len(theirs), len(mine)))
            for (a, b), (a1, b1) in zip(mine, theirs):
                if tuple(a1.shape) != tuple(a.shape) or tuple(b1.shape) != tuple(b.shape):
                    raise ValueError("state: a tensor of %s has another shape" % name)
        if tuple(state["pow"].shape) != (2,):
            raise ValueError("state: pow must have 2 elements")
        for name, mine in (("m", self.m), ("v", self.v)):
            for (a, b), (a1, b1) in zip(mine, state[name]):
                a.copy_(a1)
                b.copy_(b1)
        self.pow.copy_(state["pow"])


def _update_check(self, critics, her, policy, targets, batch_size, gamma, tau, updates, history, *, policy_cls, policy_msg,
                  policy_name, paired, shape, two, cols, actor=None, noise=None):
    """The three ``update`` methods' checks (the sampler's, ``critic_step``'s, ``polyak_``'s and ``load_``'s), before
    anything is allocated, converted or written.  ``critics``: the learner's critic ``_Net``s; ``policy``: the net
    the draw acts with, a ``policy_cls`` (``policy_msg``, ``policy_name``: its words in the messages); ``paired``:
    it is a target, ``targets[0]``'s net (DDPG, TD3), else the online policy (SAC: its blob is refreshed from
    the masters); ``shape``: what ``targets`` is; ``two``: the two critic targets' words; ``cols``: ``history``'s
    width; ``actor``: DDPG's and TD3's online actor; ``noise``: their (sigma, clip, policy_delay).
    -> (B, updates, gamma, tau, noise, [(net, target layers), ...])."""
    import torch
    from .policy import MlpActor, MlpCritic
    dev = self.device
    nc = len(critics)

    def elsewhere(d):
        return d.type != dev.type or (None not in (d.index, dev.index) and d.index != dev.index)

    hdev = her.venv.device
    if elsewhere(hdev):
        raise ValueError("update: the buffer is on %s, the learner on %s" % (hdev, dev))
    if not paired and not isinstance(policy, policy_cls):
        raise ValueError(policy_msg % type(policy).__name__)
    targets = [tuple(t) for t in targets]
    first = 1 if paired else 0
    if len(targets) != first + nc or any(len(t) != 2 for t in targets):
        raise ValueError("update: targets is " + shape)
    if paired:
        if not isinstance(policy, policy_cls):
            raise ValueError(policy_msg % type(policy).__name__)
        if targets[0][0] is not policy:
            raise ValueError("update: targets[0] is (actor_targ, policy_targ): its net is not actor_targ")
    critic_targets = targets[first:]
    for m, (net, _) in enumerate(critic_targets):
        if not isinstance(net, MlpCritic):
            raise ValueError("update: target %d must be an MlpCritic, not %s" % (m + 1, type(net).__name__))
    if actor is not None and not isinstance(actor, MlpActor):
        raise ValueError("update: actor must be an MlpActor or None, not %s" % type(actor).__name__)
    if actor is policy:
        raise ValueError("update: actor and actor_targ are one MlpActor: each has its own blob")
    named = [(policy, policy_name)] + [(net, "target %d" % (m + 1)) for m, (net, _) in enumerate(critic_targets)]
    if actor is not None:
        named.append((actor, "actor"))
    for net, name in named:
        if getattr(net, "blob", None) is None:
            raise ValueError("update: the %s must be on the device" % name)
        if elsewhere(net.device):
            raise ValueError("update: the %s is on %s, the learner on %s" % (name, net.device, dev))
    if nc == 2 and critic_targets[0][0] is critic_targets[1][0]:
        raise ValueError("update: the two %s are one MlpCritic: each has its own blob" % two)
    gamma, tau = float(gamma), float(tau)
    if not np.isfinite(gamma):
        raise ValueError("update: gamma must be finite")
    if not 0.0 <= tau <= 1.0:
        raise ValueError("update: tau must be in [0, 1]")
    if noise is not None:
        sigma, clip = float(noise[0]), float(noise[1])
        if nc == 2:
            if not (np.isfinite(sigma) and sigma >= 0.0):
                raise ValueError("update: sigma must be finite and >= 0")
            if not clip >= 0.0:
                raise ValueError("update: clip must be >= 0 (inf: the noise is not clipped)")
        policy_delay = int(noise[2])
        if policy_delay < 1:
            raise ValueError("update: policy_delay must be >= 1")
        noise = (sigma, clip, policy_delay)
    B, updates = int(batch_size), int(updates)
    if not 0 <= B <= self.max_batch:
        raise ValueError("update: batch_size = %d, the learner was built for max_batch = %d" % (B, self.max_batch))
    if updates < 0:
        raise ValueError("update: updates must be >= 0")
    if her.obs_dim + 6 != self.in_dim:
        raise ValueError("update: the buffer's rows are %d floats, the policy's %d" % (her.obs_dim + 6, self.in_dim))
    done = []
    if paired:
        policy._device_layers(self._actor.params, "update: target policy: online ")
        done.append((policy, policy._device_layers(targets[0][1], "update: target policy: target ", target=True)))
    else:
        policy._device_layers(self._actor.params, "update: the policy's ")        # load_'s: it has the masters' shape
    for m, (net, target) in enumerate(critic_targets):
        net._device_layers(critics[m].params, "update: target %d: online " % (m + 1))
        done.append((net, net._device_layers(target, "update: target %d: target " % (m + 1), target=True)))
    if actor is not None:
        actor._device_layers(self._actor.params, "update: the actor's ")          # load_'s
    if history is not None:
        if not (isinstance(history, torch.Tensor) and history.dtype == torch.float32 and not elsewhere(history.device)
                and tuple(history.shape) == (updates, cols) and history.is_contiguous()):
            raise ValueError("update: history must be a contiguous float32 [updates, %d] = [%d, %d] tensor on %s"
                             % (cols, updates, cols, dev))
    return B, updates, gamma, tau, noise, done


def _cache_slot(self, key):
    """-> (the learner's cache of update structs, its entry for ``key`` or None: eight entries, emptied
    before a ninth)."""
    cache = self.__dict__.setdefault("_update_cache", {})
    entry = cache.get(key)
    if entry is None and len(cache) >= 8:
        cache.clear()
    return cache, entry


def _update_struct(self, u, her, B, extra):
    """What a new ``ctr_sac_update_t`` or ``ctr_ddpg_update_t`` ``u`` takes from the buffer and the learner:
    the batch's output tensors (with the target and those named in ``extra``), the policy's and the
    critics' learning state, the scale, the losses, the workspace -> (the batch dict, its ctr_her_batch_t)."""
    import torch
    _, out, hb = her._batch(B, False)
    for name in ("target",) + tuple(extra):
        out[name] = torch.empty((B, 6) if name == "next_action" else B, dtype=torch.float32, device=self.device)
    u.her, u.batch_size, u.draw_seed, u.batch = ctypes.pointer(her._h), B, her._draw_seed(None), ctypes.pointer(hb)
    u.target, u.next_action = _abi.ptr(out["target"]), _abi.ptr(out.get("next_action"))
    u.policy_net, u.policy_adam = ctypes.pointer(self._actor.struct), ctypes.pointer(self._actor.adam)
    u.scale = self._scale_p
    u.critic_loss, u.actor_loss = self._closs, self._aloss
    u.workspace, u.workspace_bytes = self._ws, self._ws_bytes
    return out, hb


def _update_critic(u, y, struct, critic, net, tg):
    """Critic ``y`` of an update struct: its shape, its ``_Net``, its target ``net`` and the target's layers
    ``tg`` -> the two pointer arrays, which the caller keeps alive."""
    W = (_abi._P * len(tg))(*[w.data_ptr() for w, _ in tg])
    b = (_abi._P * len(tg))(*[v.data_ptr() for _, v in tg])
    u.critic[y], u.critic_net[y] = ctypes.pointer(struct), ctypes.pointer(critic.struct)
    u.critic_targ[y], u.W_targ[y], u.b_targ[y] = ctypes.pointer(net._struct), W, b
    if y == 0:
        u.critic_adam = ctypes.pointer(critic.adam)
    return [W, b]


def _update_call(self, fn, name, u, updates, history, stream):
    """The C call ``fn`` (``name``) of ``updates`` updates on the current stream (or ``stream``)."""
    u.history = None if history is None else history.data_ptr()
    s = stream.cuda_stream if stream is not None else self._raw_stream(self._index)
    rc = fn(u, updates, s)
    if rc:
        _abi.check(rc, name)


def _refreshed(net, sources):
    """A net as ``load_`` / ``polyak_`` leave it: sources set, host copies dropped."""
    net._sources = sources
    net.weights = net.biases = net.packed = None


def _run_update(self, critic_structs, critics, her, actor_targ, targets, batch_size, gamma, tau, updates, actor, history,
                return_next, stream, sigma=0.0, clip=0.0, policy_delay=1, update_index=0):
    """The work of ``DdpgLearner.update`` and ``Td3Learner.update`` (ctr_ddpg_update) -> (the batch dict,
    updates)."""
    from . import _abi_ddpg
    from .policy import MlpActor
    nc = len(critics)
    B, updates, gamma, tau, (sigma, clip, policy_delay), done = _update_check(
        self, critics, her, actor_targ, targets, batch_size, gamma, tau, updates, history,
        policy_cls=MlpActor, policy_msg="update: actor_targ must be an MlpActor, not %s", policy_name="target policy",
        paired=True, two="critic targets", cols=1 + nc, actor=actor, noise=(sigma, clip, policy_delay),
        shape="[(actor_targ, policy_targ), (critic_targ_dev, critic_targ)]" if nc == 1 else
        "[(actor_targ, policy_targ), (critic1_targ_dev, critic1_targ), (critic2_targ_dev, critic2_targ)]")
    key = (id(her), B, bool(return_next), id(actor), None if actor is None else actor.blob.data_ptr()) + tuple(
        (id(net), net.blob.data_ptr()) + tuple(t.data_ptr() for pair in tg for t in pair) for net, tg in done)
    cache, entry = _cache_slot(self, key)
    if entry is None:
        u = _abi_ddpg.CtrDdpgUpdate()
        q_next = ("q_next",) if nc == 1 else ("q1_next", "q2_next")
        out, hb = _update_struct(self, u, her, B, q_next + ("next_action",) if return_next else ())
        u.q1_next, u.q2_next = _abi.ptr(out.get(q_next[0])), _abi.ptr(out.get("q2_next"))
        u.n_critics = nc
        u.policy = ctypes.pointer(self._actor_struct)
        tg = done[0][1]
        arrays = [(_abi._P * len(tg))(*[w.data_ptr() for w, _ in tg]), (_abi._P * len(tg))(*[v.data_ptr() for _, v in tg])]
        u.actor_targ, u.W_targ_actor, u.b_targ_actor = ctypes.pointer(actor_targ._struct), arrays[0], arrays[1]
        for y, (net, tg) in enumerate(done[1:]):
            arrays += _update_critic(u, y, critic_structs[y], critics[y], net, tg)
        if actor is not None:
            u.actor = ctypes.pointer(actor._struct)
        # (the entry keeps alive what the struct points into, and the objects whose ids are the key)
        entry = cache[key] = (u, out, hb, arrays, her, actor, done)
    u, out = entry[0], entry[1]
    u.gamma, u.tau, u.sigma, u.clip = gamma, tau, sigma, clip
    u.policy_delay, u.update_index = policy_delay, int(update_index) & 0xFFFFFFFFFFFFFFFF
    u.draw_counter = her._counter & 0xFFFFFFFFFFFFFFFF
    _update_call(self, self._lib.ctr_ddpg_update, "ctr_ddpg_update", u, updates, history, stream)
    her._counter += updates
    if B and (int(update_index) + updates) // policy_delay > int(update_index) // policy_delay:
        # a policy step was made: the nets are as polyak_ and load_ leave them
        for net, tg in done:
            _refreshed(net, tg)
        if actor is not None:
            _refreshed(actor, list(self._actor.params))
    out = dict(out)
    if history is not None:
        out["history"] = history
    return out, updates


def _setup(self, policy, tanh, out_rows, critics, scale, rates, betas, eps, max_batch, alloc, workspace_fn):
    """The three constructors' work: the checks, the ``_Net`` of the policy and of each critic, the
    workspace (``workspace_fn``'s bytes) and everything ``critic_step`` takes.  ``tanh``, ``out_rows``: the
    policy's head; ``critics``: ((network, its name), ...), one (``_critic``, ``_critic_struct``,
    ``critic_loss`` 0-d) or two (``_critics``, ``_critic_structs``, ``critic_loss`` [2], the twin step's
    pairs); ``rates``: ((name, value), ...), every value finite, the first two the policy's and the
    critics' learning rates."""
    import torch
    from . import _abi_ddpg, _abi_td3
    a_params, a_in, a_hidden = _masters(policy, tanh, "policy", (19, 20), out_rows,
                                        "the policy's rows are obs_dim + 6 = 19 or 20 floats")
    c_nets = []
    for critic, name in critics:
        c_params, c_in, c_hidden = _masters(critic, False, name, (25, 26), 1,
                                            "the %s's rows are obs_dim + 12 = 25 or 26 floats" % name)
        if a_in + 6 != c_in:
            raise ValueError("the %s takes [row, action]: %d + 6 inputs, not %d" % (name, a_in, c_in))
        c_nets.append((c_params, c_in, c_hidden))
    self.device = device = a_params[0][0].device
    for (c_params, _, _), (_, name) in zip(c_nets, critics):
        if c_params[0][0].device != device:
            raise ValueError("the %s is on %s, the policy on %s" % (name, c_params[0][0].device, device))
    if len(c_nets) == 2 and any(t1 is t2 or (t1.numel() and t1.data_ptr() == t2.data_ptr())
                                for p1 in c_nets[0][0] for t1 in p1 for p2 in c_nets[1][0] for t2 in p2):
        raise ValueError("critic1 and critic2 share a tensor: the twin step updates them side by side")
    betas = (float(betas[0]), float(betas[1]))
    for name, val in tuple(rates) + (("eps", eps),):
        if not np.isfinite(float(val)):
            raise ValueError(name + " must be finite")
    if not all(0.0 <= b < 1.0 for b in betas):
        raise ValueError("betas must be in [0, 1)")
    if not float(eps) > 0.0:
        raise ValueError("eps must be positive")
    max_batch = int(max_batch)
    if not 1 <= max_batch <= _abi_ddpg.CTR_DDPG_MAX_B:
        raise ValueError("max_batch must be in 1..%d" % _abi_ddpg.CTR_DDPG_MAX_B)
    if scale is not None:
        scale = np.asarray(scale, dtype=np.float32).reshape(-1)
        if scale.shape != (6,) or not np.isfinite(scale).all() or (scale == 0).any():
            raise ValueError("scale is six finite, non-zero floats")
    if device.type != "cuda":
        raise ValueError("the networks are on %s: the learner's networks are on a GPU" % (device,))
    if alloc is None:
        def alloc(shape):
            return torch.zeros(shape, dtype=torch.float32, device=device)
    self._lib = lib = _abi.load()
    self.max_batch = max_batch
    self.in_dim = a_in
    self._actor_struct = sa = _abi.CtrActor()
    sc = tuple(_abi_critic.CtrCritic() for _ in c_nets)
    for s, in_dim, hidden in [(sa, a_in, a_hidden)] + [(c,) + net[1:] for c, net in zip(sc, c_nets)]:
        s.in_dim, s.n_hidden = in_dim, len(hidden)
        for l, w in enumerate(hidden):
            s.width[l] = w
    actor_lr, critic_lr = rates[0][1], rates[1][1]
    self._actor = _Net(a_params, alloc, actor_lr, betas, eps)
    nets = tuple(_Net(net[0], alloc, critic_lr, betas, eps) for net in c_nets)
    self.actor_grads = self._actor.grads
    nbytes = int(getattr(lib, workspace_fn)(sa, *sc, max_batch))
    if nbytes < 0:
        raise _abi.CtrError(workspace_fn + ": " + lib.ctr_last_error().decode())
    self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=device)
    if self.workspace.data_ptr() % 16:
        raise RuntimeError("workspace not 16-B aligned")
    self.scale = None if scale is None else torch.from_numpy(scale).to(device)
    self.critic_loss = torch.zeros(() if len(nets) == 1 else 2, dtype=torch.float32, device=device)
    self.actor_loss = torch.zeros((), dtype=torch.float32, device=device)
    # everything the steps take but the batch and the stream, once
    P = ctypes.c_void_p
    if len(nets) == 1:
        self._critic, self._critic_struct, self.critic_grads = nets[0], sc[0], nets[0].grads
        self._critic_step = lib.ctr_ddpg_critic_step
    else:
        self._critics, self._critic_structs, self.critic_grads = nets, sc, (nets[0].grads, nets[1].grads)
        self._critic_pair = _abi_td3.CriticPair(ctypes.pointer(sc[0]), ctypes.pointer(sc[1]))
        self._net_pair = _abi_td3.NetPair(ctypes.pointer(nets[0].struct), ctypes.pointer(nets[1].struct))
        self._critic_step = lib.ctr_td3_critic_step
    self._ws, self._ws_bytes = P(self.workspace.data_ptr()), nbytes
    self._scale_p = P(None if self.scale is None else self.scale.data_ptr())
    self._closs, self._aloss = P(self.critic_loss.data_ptr()), P(self.actor_loss.data_ptr())
    self._f32, self._index = torch.float32, device.index
    self._raw_stream = torch._C._cuda_getCurrentRawStream


class DdpgLearner(object):
    """``policy``: an ``nn.Sequential`` (Linear, ReLU, ..., Linear, Tanh) and ``critic`` one without
    the Tanh, as ``MlpActor.from_torch`` / ``MlpCritic.from_torch`` take them (or lists of
    ``(W, b)`` tensors), on a GPU.  Their parameters are the float32 masters and are written in
    place, so none may require grad (ValueError, as ``polyak_`` refuses such a target).

    ``scale``: six floats; ``critic_step`` then feeds the critic ``actions / scale`` (one float32
    division); None: the actions are normalised already.  ``max_batch``: the largest B of a step
    (1..65 536); the workspace is sized for it once.  ``alloc(shape)``: the allocator of the
    gradient and state tensors (default: ``torch.zeros`` on the networks' device; zeros are
    required).

    The constructor allocates ``actor_grads`` / ``critic_grads`` ([(gW, gb), ...], written whole by
    every step), the Adam state and the workspace and builds every struct of the two C calls once; a
    step checks its batch tensors and makes one call: two launches on the current stream (or
    ``stream``), nothing allocated or read back, so both steps can be captured into a graph.  The
    losses stay on the device (``critic_loss``, ``actor_loss``: 0-d tensors)."""

    def __init__(self, policy, critic, scale=None, actor_lr=1e-4, critic_lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 max_batch=256, alloc=None):
        _setup(self, policy, True, 6, ((critic, "critic"),), scale, (("actor_lr", actor_lr), ("critic_lr", critic_lr)), betas,
               eps, max_batch, alloc, "ctr_ddpg_workspace_bytes")
        self._actor_step = self._lib.ctr_ddpg_actor_step

    def _rows(self, t, cols, name):
        if t.dtype is not self._f32 or t.device != self.device or t.dim() != 2 or t.shape[1] != cols \
                or not t.is_contiguous():
            raise ValueError("%s must be a contiguous float32 [B, %d] tensor on %s" % (name, cols, self.device))
        B = t.shape[0]
        if B > self.max_batch:
            raise ValueError("B = %d rows, the learner was built for max_batch = %d" % (B, self.max_batch))
        return B

    def _critic_batch(self, rows, actions, target):
        """``critic_step``'s checks of its batch -> B."""
        B = self._rows(rows, self.in_dim, "rows")
        if self._rows(actions, 6, "actions") != B:
            raise ValueError("actions has another B than rows")
        if target.dtype is not self._f32 or target.device != self.device or tuple(target.shape) != (B,) \
                or not target.is_contiguous():
            raise ValueError("target must be a contiguous float32 [B] tensor on %s" % (self.device,))
        return B

    def critic_step(self, rows, actions, target, stream=None):
        """One regression step of the critic on ``target`` ([B] float32): rows [B, in_dim] as the
        policy takes them, actions [B, 6] (divided by ``scale`` in the kernel when the learner has
        one).  The loss goes to ``critic_loss``, the gradients to ``critic_grads``."""
        B = self._critic_batch(rows, actions, target)
        s = stream.cuda_stream if stream is not None else self._raw_stream(self._index)
        c = self._critic
        rc = self._critic_step(self._critic_struct, c.struct, c.adam, rows.data_ptr(), actions.data_ptr(), self._scale_p,
                               target.data_ptr(), B, self._closs, self._ws, self._ws_bytes, s)
        if rc:
            _abi.check(rc, "ctr_ddpg_critic_step")

    def actor_step(self, rows, stream=None):
        """One step of the policy up Q(row, pi(row)) under the critic's current parameters, which
        are only read.  The loss (-mean Q) goes to ``actor_loss``, the gradients to ``actor_grads``."""
        B = self._rows(rows, self.in_dim, "rows")
        s = stream.cuda_stream if stream is not None else self._raw_stream(self._index)
        a, c = self._actor, self._critic
        rc = self._actor_step(self._actor_struct, a.struct, a.adam, self._critic_struct, c.arrays["W"], c.arrays["b"],
                              rows.data_ptr(), B, self._aloss, self._ws, self._ws_bytes, s)
        if rc:
            _abi.check(rc, "ctr_ddpg_actor_step")

    def update(self, her, actor_targ, targets, batch_size, gamma, tau, updates=1, actor=None, history=None, return_next=False,
               stream=None):
        """``updates`` whole DDPG updates from one call (ctr_ddpg_update): each is what

            batch = her.sample_td(batch_size, actor_targ, critic_targ_dev, gamma)
            learner.critic_step(batch["obs"], batch["action"], batch["target"])
            learner.actor_step(batch["obs"])
            polyak_([(actor_targ, policy, policy_targ), (critic_targ_dev, critic, critic_targ)], tau)
            actor.load_(policy)                                      # with ``actor``

        leaves, bit for bit, in five launches and without the host work of four or five calls; the
        sampler's two scans run once per call.  ``her``: the ``HerReplayBuffer``; ``actor_targ``: the
        target policy's ``MlpActor``; ``targets``: [(actor_targ, policy_targ), (critic_targ_dev,
        critic_targ)], each a target's device net and the owner of its float32 parameters
        (``nn.Sequential`` or [(W, b), ...]) as ``polyak_`` takes them; ``actor``: None, or the online
        policy's ``MlpActor``, whose blob is then repacked from the learner's policy masters by every
        update.

        Returns ``sample_td``'s dict (with ``return_next`` also q_next and next_action), holding the LAST
        update's draw.  Its tensors are allocated on the first call for a ``batch_size`` and reused: THE
        NEXT ``update`` CALL OVERWRITES THEM.  ``history``: None, or a contiguous float32 [updates, 2]
        tensor on the device; row i gets update i's critic loss and actor loss, and the dict returns it
        under "history".  ``critic_loss`` and ``actor_loss`` hold the last update's values.

        Every check of the calls is made first (ValueError, nothing converted, nothing written).
        Afterwards ``her``'s draw counter has advanced by ``updates`` and the target nets and ``actor``
        are as ``polyak_`` / ``load_`` leave them (sources set, host copies dropped).  Asynchronous: no
        allocation after the first call, no host read; a captured call repeats its draws on replay.  The
        call's struct is built once per (her, nets, batch_size) and cached."""
        return _run_update(self, (self._critic_struct,), (self._critic,), her, actor_targ, targets, batch_size, gamma, tau,
                           updates, actor, history, return_next, stream)[0]

    def state_dict(self):
        """Adam's state of both networks, cloned: {"actor": {"m", "v", "pow"}, "critic": {...}} with
        ``m`` and ``v`` as [(W-shaped, b-shaped), ...] and ``pow`` = [beta1^t, beta2^t]."""
        return {"actor": self._actor.state(), "critic": self._critic.state()}

    def load_state_dict(self, state):
        """Copies a ``state_dict()`` into the learner's own tensors (the device pointers stay)."""
        self._actor.load_state(state["actor"])
        self._critic.load_state(state["critic"])


class Td3Learner(object):
    """``DdpgLearner`` with TD3's twin critics (ctr_td3_critic_step): ``policy`` and two critics
    ``critic1``, ``critic2`` of one input width (their hidden layers may differ), given as
    ``DdpgLearner`` takes its networks.  The two critics may share no tensor.

        learner = Td3Learner(policy, critic1, critic2, scale=venv.action_space.high)
        batch = buf.sample_td3(256, actor_targ, critic1_targ, critic2_targ, gamma, sigma=0.2, clip=0.5)
        learner.critic_step(batch["obs"], batch["action"], batch["target"])
        if update % 2 == 0:                                  # TD3's delayed policy and target updates
            learner.actor_step(batch["obs"])
            polyak_([(actor_targ, policy, policy_targ), (critic1_targ_dev, critic1, critic1_targ),
                     (critic2_targ_dev, critic2, critic2_targ)], 0.005)

    ``critic_step`` regresses both critics on the one target in one call: two launches, whose second
    grid dimension is the critic, each critic's bits those of ``DdpgLearner.critic_step`` on it.
    ``actor_step`` is ``DdpgLearner``'s under critic 1 (TD3 ascends Q1).  ``critic_lr`` serves both
    critics.  The constructor builds every struct of the two C calls once; ``critic_grads`` is the
    pair of the critics' gradient lists, ``critic_loss`` a device tensor [2], ``actor_loss`` 0-d."""

    def __init__(self, policy, critic1, critic2, scale=None, actor_lr=1e-4, critic_lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 max_batch=256, alloc=None):
        _setup(self, policy, True, 6, ((critic1, "critic1"), (critic2, "critic2")), scale,
               (("actor_lr", actor_lr), ("critic_lr", critic_lr)), betas, eps, max_batch, alloc, "ctr_td3_workspace_bytes")
        self._actor_step = self._lib.ctr_ddpg_actor_step
        self.update_count = 0           # the updates made through ``update``: where TD3's delayed steps fall

    _rows, _critic_batch = DdpgLearner._rows, DdpgLearner._critic_batch

    def critic_step(self, rows, actions, target, stream=None):
        """One regression step of both critics on ``target`` ([B] float32), as
        ``DdpgLearner.critic_step`` makes it for one.  The losses go to ``critic_loss`` [2], the
        gradients to ``critic_grads``."""
        B = self._critic_batch(rows, actions, target)
        s = stream.cuda_stream if stream is not None else self._raw_stream(self._index)
        rc = self._critic_step(self._critic_pair, self._net_pair, self._critics[0].adam, rows.data_ptr(),
                               actions.data_ptr(), self._scale_p, target.data_ptr(), B, self._closs, self._ws,
                               self._ws_bytes, s)
        if rc:
            _abi.check(rc, "ctr_td3_critic_step")

    def actor_step(self, rows, stream=None):
        """One step of the policy up Q1(row, pi(row)) under critic 1's current parameters, which are
        only read; critic 2 takes no part.  The loss (-mean Q1) goes to ``actor_loss``, the gradients
        to ``actor_grads``."""
        B = self._rows(rows, self.in_dim, "rows")
        s = stream.cuda_stream if stream is not None else self._raw_stream(self._index)
        a, c = self._actor, self._critics[0]
        rc = self._actor_step(self._actor_struct, a.struct, a.adam, self._critic_structs[0], c.arrays["W"], c.arrays["b"],
                              rows.data_ptr(), B, self._aloss, self._ws, self._ws_bytes, s)
        if rc:
            _abi.check(rc, "ctr_ddpg_actor_step")

    def update(self, her, actor_targ, targets, batch_size, gamma, tau, sigma=0.2, clip=0.5, policy_delay=2, updates=1,
               actor=None, history=None, return_next=False, stream=None):
        """``updates`` whole TD3 updates from one call (ctr_ddpg_update with two critics): each is what

            batch = her.sample_td3(batch_size, actor_targ, critic1_targ_dev, critic2_targ_dev, gamma, sigma, clip)
            learner.critic_step(batch["obs"], batch["action"], batch["target"])
            learner.update_count += 1
            if learner.update_count % policy_delay == 0:
                learner.actor_step(batch["obs"])
                polyak_([(actor_targ, policy, policy_targ), (critic1_targ_dev, critic1, critic1_targ),
                         (critic2_targ_dev, critic2, critic2_targ)], tau)
                actor.load_(policy)                                  # with ``actor``

        leaves, bit for bit: five launches for an update with a policy step, three for one without.
        ``targets`` has three pairs; everything else is ``DdpgLearner.update``'s.  ``update_count`` (a
        plain attribute, 0 at construction, not part of ``state_dict``) counts the updates made through
        this method and decides where the delayed steps fall; it advances by ``updates``.  ``history``:
        [updates, 3]: the two critic losses, then the actor loss, whose entry an update without a
        policy step leaves untouched.  ``return_next``: q1_next, q2_next and next_action."""
        out, made = _run_update(self, self._critic_structs, self._critics, her, actor_targ, targets, batch_size, gamma, tau,
                                updates, actor, history, return_next, stream, sigma, clip, policy_delay, self.update_count)
        self.update_count += made
        return out

    def state_dict(self):
        """Adam's state of the three networks, cloned: {"actor": {"m", "v", "pow"}, "critic1": {...},
        "critic2": {...}}, each as in ``DdpgLearner.state_dict``."""
        return {"actor": self._actor.state(), "critic1": self._critics[0].state(), "critic2": self._critics[1].state()}

    def load_state_dict(self, state):
        """Copies a ``state_dict()`` into the learner's own tensors (the device pointers stay)."""
        self._actor.load_state(state["actor"])
        self._critics[0].load_state(state["critic1"])
        self._critics[1].load_state(state["critic2"])


class SacLearner(object):
    """SAC (Haarnoja et al. 2018, with the learned temperature) on the device: ``policy`` an
    ``nn.Sequential(Linear, ReLU, ..., Linear(h, 12))`` as ``GaussianActor.from_torch`` takes it (six
    means, six log standard deviations, no Tanh), ``critic1`` and ``critic2`` as ``Td3Learner`` takes
    them; all given as ``DdpgLearner`` takes its networks.

        learner = SacLearner(policy, critic1, critic2, scale=venv.action_space.high)
        batch = her.sample_sac(256, pi, critic1_targ_dev, critic2_targ_dev, gamma, learner.log_alpha)
        learner.critic_step(batch["obs"], batch["action"], batch["target"])
        learner.actor_step(batch["obs"])
        pi.load_(policy)
        polyak_([(critic1_targ_dev, critic1, critic1_targ), (critic2_targ_dev, critic2, critic2_targ)], 0.005)

    ``sample_sac`` (ctr_her_sample_sac) draws the batch and makes target = r + gamma (1 - done) (min(Q1',
    Q2')(s', a') - alpha logp(a')) with a' from the current policy ``pi``, in the sampler's launch; it
    reads ``log_alpha`` on the device.  ``critic_step`` is ``Td3Learner.critic_step`` (the same C call).  ``actor_step`` (ctr_sac_actor_step,
    two launches) samples an action per row from the policy with the noise of (``seed``, ``counter``,
    the row's index), and descends mean(alpha * logp - min(Q1, Q2)) through both critics, the tanh and
    the reparametrisation; with ``learn_alpha`` the temperature's ``log_alpha`` then takes its own Adam
    step on -log_alpha * (logp_mean + target_entropy).  The learning rates, ``init_alpha`` and
    ``target_entropy`` = -dim(A) are stable-baselines SAC's defaults with ``ent_coef='auto'``.
    ``actor_loss``, ``logp_mean``, ``log_alpha``, ``alpha_grad`` (0-d) and ``alpha_state`` ([4]: m, v,
    beta1^t, beta2^t) stay on the device; ``alpha`` is exp(log_alpha) as a device tensor."""

    def __init__(self, policy, critic1, critic2, scale=None, actor_lr=3e-4, critic_lr=3e-4, alpha_lr=3e-4, init_alpha=1.0,
                 target_entropy=-6.0, learn_alpha=True, betas=(0.9, 0.999), eps=1e-8, max_batch=256, alloc=None, seed=0):
        import torch
        from . import _abi_sac
        if not (np.isfinite(float(init_alpha)) and float(init_alpha) > 0.0):
            raise ValueError("init_alpha must be positive and finite")
        _setup(self, policy, False, 12, ((critic1, "critic1"), (critic2, "critic2")), scale,
               (("actor_lr", actor_lr), ("critic_lr", critic_lr), ("alpha_lr", alpha_lr), ("target_entropy", target_entropy)),
               betas, eps, max_batch, alloc, "ctr_sac_workspace_bytes")
        device = self.device
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.counter = 0
        self.target_entropy, self.learn_alpha = float(target_entropy), bool(learn_alpha)
        self.logp_mean = torch.zeros((), dtype=torch.float32, device=device)
        self.log_alpha = torch.tensor(float(np.log(np.float64(init_alpha))), dtype=torch.float32, device=device)
        self.alpha_state = torch.tensor([0.0, 0.0, 1.0, 1.0], dtype=torch.float32, device=device)
        self.alpha_grad = torch.zeros((), dtype=torch.float32, device=device)
        # what ctr_sac_actor_step takes beyond the twin step's arguments, once
        P = ctypes.c_void_p
        self._cW = _abi_sac.LayersPair(self._critics[0].arrays["W"], self._critics[1].arrays["W"])
        self._cb = _abi_sac.LayersPair(self._critics[0].arrays["b"], self._critics[1].arrays["b"])
        self._alpha_struct = _abi_sac.CtrSacAlpha(self.alpha_state.data_ptr(), self.alpha_grad.data_ptr(), float(alpha_lr),
                                                  int(self.learn_alpha))
        self._lpm, self._la = P(self.logp_mean.data_ptr()), P(self.log_alpha.data_ptr())
        self._actor_step = self._lib.ctr_sac_actor_step

    _rows, _critic_batch = DdpgLearner._rows, DdpgLearner._critic_batch
    critic_step = Td3Learner.critic_step

    @property
    def alpha(self):
        """exp(log_alpha): a 0-d device tensor (no host read)."""
        return self.log_alpha.exp()

    def actor_step(self, rows, counter=None, stream=None):
        """One step of the policy down mean(alpha * logp - min(Q1, Q2)) on actions sampled with the
        noise of (seed, ``counter``, row), under both critics' current parameters, which are only
        read; then the temperature's step (``learn_alpha``).  ``counter`` None: a count the learner
        keeps, advanced by every such call.  The loss goes to ``actor_loss``, the mean log-probability
        to ``logp_mean``, the gradients to ``actor_grads`` and ``alpha_grad``."""
        B = self._rows(rows, self.in_dim, "rows")
        if counter is None:
            counter = self.counter
            self.counter += 1
        s = stream.cuda_stream if stream is not None else self._raw_stream(self._index)
        a = self._actor
        rc = self._actor_step(self._actor_struct, a.struct, a.adam, self._critic_pair, self._cW, self._cb, rows.data_ptr(), B,
                              self.seed, int(counter) & 0xFFFFFFFFFFFFFFFF, self._la, self._alpha_struct, self.target_entropy,
                              self._aloss, self._lpm, self._ws, self._ws_bytes, s)
        if rc:
            _abi.check(rc, "ctr_sac_actor_step")

    def update(self, her, pi, targets, batch_size, gamma, tau, updates=1, history=None, return_next=False, stream=None):
        """``updates`` whole SAC updates from one call (ctr_sac_update): each is what

            batch = her.sample_sac(batch_size, pi, critic1_targ_dev, critic2_targ_dev, gamma, learner.log_alpha)
            learner.critic_step(batch["obs"], batch["action"], batch["target"])
            learner.actor_step(batch["obs"])
            pi.load_(policy)
            polyak_([(critic1_targ_dev, critic1, critic1_targ), (critic2_targ_dev, critic2, critic2_targ)], tau)

        leaves, bit for bit, in five launches instead of nine and without the host work of five calls;
        the sampler's two scans run once per call.  ``her``: the ``HerReplayBuffer``; ``pi``: the
        ``GaussianActor`` whose blob is refreshed from the learner's own policy masters; ``targets``:
        [(critic1_targ_dev, critic1_targ), (critic2_targ_dev, critic2_targ)], each the target's
        ``MlpCritic`` and the owner of its float32 parameters (``nn.Sequential`` or [(W, b), ...]) as
        ``polyak_`` takes them.  The draws run under the buffer's draw seed and counter, the policy's
        noise under the learner's seed and counter, as the five calls' would.

        Returns ``sample_sac``'s dict (with ``return_next`` also q1_next, q2_next, next_action,
        next_logp), holding the LAST update's draw.  Its tensors are allocated on the first call for a
        ``batch_size`` and reused: THE NEXT ``update`` CALL OVERWRITES THEM.  ``history``: None, or a
        contiguous float32 [updates, 5] tensor on the device; row i gets update i's critic 1 loss,
        critic 2 loss, actor loss, logp_mean and log_alpha after its step, and the dict returns it under
        "history".  ``critic_loss``, ``actor_loss`` and ``logp_mean`` hold the last update's values.

        Every check of the five calls is made first (ValueError, nothing converted, nothing written).
        Afterwards ``her``'s draw counter and the learner's ``counter`` have advanced by ``updates``,
        ``pi`` and the target nets are as ``load_`` / ``polyak_`` leave them (sources set, host copies
        dropped) and the buffer keeps ``log_alpha`` referenced as ``sample_sac`` does.  Asynchronous:
        no allocation after the first call, no host read; a captured call repeats its draws on replay
        (the counters are arguments).  The call's struct is built once per (her, pi, targets,
        batch_size) and cached."""
        from . import _abi_sac
        from .policy import GaussianActor
        B, updates, gamma, tau, _, done = _update_check(
            self, self._critics, her, pi, targets, batch_size, gamma, tau, updates, history,
            policy_cls=GaussianActor, policy_msg="update: pi must be a GaussianActor (the 12-row head), not %s",
            policy_name="policy", paired=False, two="targets", cols=5,
            shape="[(critic1_targ_dev, critic1_targ), (critic2_targ_dev, critic2_targ)]")
        key = (id(her), id(pi), B, bool(return_next), pi.blob.data_ptr()) + tuple(
            (id(net), net.blob.data_ptr()) + tuple(t.data_ptr() for pair in tg for t in pair) for net, tg in done)
        cache, entry = _cache_slot(self, key)
        if entry is None:
            u = _abi_sac.CtrSacUpdate()
            out, hb = _update_struct(self, u, her, B, ("q1_next", "q2_next", "next_action", "next_logp") if return_next else ())
            u.q1_next, u.q2_next = _abi.ptr(out.get("q1_next")), _abi.ptr(out.get("q2_next"))
            u.next_logp = _abi.ptr(out.get("next_logp"))
            u.policy = ctypes.pointer(pi._struct)
            arrays = []
            for y, (net, tg) in enumerate(done):
                arrays += _update_critic(u, y, self._critic_structs[y], self._critics[y], net, tg)
            u.log_alpha, u.alpha, u.logp_mean = self._la, ctypes.pointer(self._alpha_struct), self._lpm
            # (the entry keeps alive what the struct points into, and the objects whose ids are the key)
            entry = cache[key] = (u, out, hb, arrays, her, pi, done)
        u, out = entry[0], entry[1]
        u.gamma, u.tau = gamma, tau
        u.seed, u.target_entropy = self.seed, self.target_entropy        # read on every call, as actor_step reads them
        u.draw_counter = her._counter & 0xFFFFFFFFFFFFFFFF
        u.step_counter = self.counter & 0xFFFFFFFFFFFFFFFF
        _update_call(self, self._lib.ctr_sac_update, "ctr_sac_update", u, updates, history, stream)
        her._log_alpha = self.log_alpha    # stays referenced until the next draw: the launches read it
        her._counter += updates
        self.counter += updates
        _refreshed(pi, list(self._actor.params))
        for net, tg in done:
            _refreshed(net, tg)
        out = dict(out)
        if history is not None:
            out["history"] = history
        return out

    def state_dict(self):
        """Adam's state of the three networks as ``Td3Learner.state_dict`` gives it, with the
        temperature (``log_alpha``, ``alpha_state``: cloned) and the noise ``counter``."""
        return {"actor": self._actor.state(), "critic1": self._critics[0].state(), "critic2": self._critics[1].state(),
                "log_alpha": self.log_alpha.clone(), "alpha_state": self.alpha_state.clone(), "counter": self.counter}

    def load_state_dict(self, state):
        """Copies a ``state_dict()`` into the learner's own tensors (the device pointers stay)."""
        if tuple(state["alpha_state"].shape) != (4,) or tuple(state["log_alpha"].shape) != ():
            raise ValueError("state: log_alpha is 0-d and alpha_state has 4 elements")
        self._actor.load_state(state["actor"])
        self._critics[0].load_state(state["critic1"])
        self._critics[1].load_state(state["critic2"])
        self.log_alpha.copy_(state["log_alpha"])
        self.alpha_state.copy_(state["alpha_state"])
        self.counter = int(state["counter"])
