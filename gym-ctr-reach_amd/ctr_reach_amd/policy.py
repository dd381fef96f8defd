"""A deterministic MLP actor on the device (ctr_actor / ctr_rollout, include/ctr_reach_amd.h): the
reference's stable-baselines DDPG ``MlpPolicy`` actor on HERGoalEnvWrapper's flat row
``[observation, achieved_goal, desired_goal]``.

    actor = MlpActor([(W1, b1), (W2, b2), (Wout, bout)], scale=venv.action_space.high, device="cuda")
    actions = venv.act(actor)                 # one ctr_actor launch
    venv.rollout(actor, 20)                   # 20 closed-loop steps, one launch per refill period
    actor.load_(policy_net)                   # new weights from device parameters, one ctr_actor_load launch

``MlpActor.emulate`` is the CPU reference of the actor's arithmetic (numpy, no GPU, no library).

``MlpCritic`` is the Q-network on the same kernels (ctr_critic; ``HerReplayBuffer.sample_td`` runs a
target policy and a target critic on every sampled row and returns the DDPG target with the batch).
``polyak_`` is the soft update of such target networks' float32 parameters together with the
refresh of their blobs, one launch for all of them (ctr_polyak).

``GaussianActor`` is SAC's tanh-Gaussian policy on the actor's kernels (ctr_gauss_act): a 12-row head,
an action sampled with its log-probability in one launch, and its deterministic mean as an ``MlpActor``.

``ExploreNoise`` is the exploration noise of the reference's DDPG + HER training on such an actor's
actions (ctr_explore / ctr_collect), with its own numpy restatement.
"""
import ctypes

import numpy as np

from . import _abi, _abi_critic


def bf16_round(x):
    """float32 values rounded to bfloat16 (nearest even), as float32.  NaN stays NaN."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(np.float32)
    return np.where(np.isnan(x), np.float32(np.nan), r).astype(np.float32)


class _Mlp(object):
    """What the actor and the critic share: the shape checks, the packed device blob and its two
    packers (host: ctr_*_pack, device: ctr_*_load), and the hidden layers of the emulation."""

    NAME = None                 # "actor" / "critic": the messages, and ctr_<NAME>_pack / _load / _blob_bytes
    IN_DIMS = None              # the two row lengths
    OUT = None                  # rows of the output layer
    TANH = None                 # whether the nn.Sequential ends with nn.Tanh

    def _init_layers(self, layers, struct):
        ws, bs = [], []
        for W, b in layers:
            ws.append(np.ascontiguousarray(_to_numpy(W), dtype=np.float32))
            bs.append(np.ascontiguousarray(_to_numpy(b), dtype=np.float32).reshape(-1))
        if not 2 <= len(ws) <= _abi.CTR_ACTOR_MAX_HIDDEN + 1:
            raise ValueError("%s has 1..%d hidden layers and an output layer"
                             % ("an actor" if self.NAME == "actor" else "a critic", _abi.CTR_ACTOR_MAX_HIDDEN))
        for l, (W, b) in enumerate(zip(ws, bs)):
            if W.ndim != 2 or b.shape != (W.shape[0],):
                raise ValueError("layer %d: W must be [out, in] and b [out]" % l)
            if l and W.shape[1] != ws[l - 1].shape[0]:
                raise ValueError("layer %d takes %d inputs, layer %d gives %d" % (l, W.shape[1], l - 1, ws[l - 1].shape[0]))
        if ws[0].shape[1] not in self.IN_DIMS:
            raise ValueError(self._IN_MSG)
        if ws[-1].shape[0] != self.OUT:
            raise ValueError(self._OUT_MSG)
        for W in ws[:-1]:
            if W.shape[0] % 32 or not 32 <= W.shape[0] <= _abi.CTR_ACTOR_MAX_WIDTH:
                raise ValueError("hidden widths must be multiples of 32 in 32..%d" % _abi.CTR_ACTOR_MAX_WIDTH)
        self.weights, self.biases = ws, bs
        self.in_dim = ws[0].shape[1]
        self.hidden = [W.shape[0] for W in ws[:-1]]
        self.device = None
        self.blob = None
        self._sources = None            # load_'s device tensors (the blob was packed from them)
        self._struct = s = struct
        s.in_dim, s.n_hidden = self.in_dim, len(self.hidden)
        for l, w in enumerate(self.hidden):
            s.width[l] = w

    @property
    def _A(self):
        return "the " + self.NAME

    def _fn(self, what):
        return "ctr_%s_%s" % (self.NAME, what)

    def _device_layers(self, layers, role="", target=False):
        """The checks of ``load_`` and ``polyak_`` on one list of device parameters: ``layers`` as
        ``load_`` takes them -> [(W, b), ...] detached.  Every tensor on the network's device,
        float32, of its shape and contiguous, or ValueError (``role`` names the list in the
        messages); nothing is converted.  ``target``: the tensors will be written, so none may
        require grad."""
        import torch
        if self.blob is None:
            raise RuntimeError("%s is on the host (%s(..., device=None)): nothing to load into"
                               % (self._A, type(self).__name__))
        if isinstance(layers, torch.nn.Module):
            layers = _sequential_layers(layers, self.TANH, self.NAME, detach=False)
        layers = [tuple(pair) for pair in layers]
        dims = [self.in_dim] + self.hidden + [self.OUT]
        if len(layers) != len(dims) - 1 or any(len(pair) != 2 for pair in layers):
            raise ValueError("%s%s has %d layers of (W, b)" % (role, self._A, len(dims) - 1))
        src = []
        for l, (W, b) in enumerate(layers):
            pair = []
            for name, t, shape in (("W", W, (dims[l + 1], dims[l])), ("b", b, (dims[l + 1],))):
                what = "%slayer %d: %s" % (role, l, name)
                if not isinstance(t, torch.Tensor):
                    raise ValueError(what + " must be a torch tensor")
                if t.device.type != self.device.type or (self.device.index is not None
                                                         and t.device.index != self.device.index):
                    raise ValueError("%s is on %s, %s on %s" % (what, t.device, self._A, self.device))
                if t.dtype != torch.float32:
                    raise ValueError("%s must be float32, not %s" % (what, t.dtype))
                if tuple(t.shape) != shape:
                    raise ValueError("%s must be %s, not %s" % (what, list(shape), list(t.shape)))
                if not t.is_contiguous():
                    raise ValueError(what + " must be contiguous")
                if target and t.requires_grad:
                    raise ValueError(what + " requires grad: a target is written in place, outside autograd")
                pair.append(t.detach())
            src.append(tuple(pair))
        return src

    def polyak_(self, online, target, tau, stream=None):
        """The one-net case of the module's ``polyak_``: ``target`` moves towards ``online`` by
        ``tau`` in place and this network's blob becomes the pack of the new ``target``, in one
        launch.  Returns self."""
        polyak_([(self, online, target)], tau, stream)
        return self

    def load_(self, layers, stream=None, keep_host=False):
        """Refresh the device blob in place from device-resident parameters (ctr_actor_load /
        ctr_critic_load): one launch on ``stream`` (default: the current stream), ordered like any
        other launch there; no allocation, no copy to the host and no synchronisation, so it can be
        captured into a graph (a replay packs whatever the parameters hold then).  ``layers``:
        [(W, b), ...] torch tensors or an ``nn.Sequential`` as ``from_torch`` takes; every tensor on
        the network's device, float32, contiguous and of its shapes, or ValueError is raised and the
        blob stays (nothing is converted: a hidden copy would be a temporary the launch outlives).
        The tensors stay referenced until the next ``load_``.

        The host copies (``weights``, ``biases``, ``packed``) would go stale: they are dropped, and
        ``emulate`` / ``reference`` raise until a load with ``keep_host=True``, which copies the
        sources back to the host and therefore SYNCHRONISES (not for a captured graph).  Returns
        self."""
        src = self._device_layers(layers)
        n = len(src)
        W = (_abi._P * n)(*[w.data_ptr() for w, _ in src])
        b = (_abi._P * n)(*[v.data_ptr() for _, v in src])
        rc = getattr(_abi.load(), self._fn("load"))(self._struct, W, b, _abi.stream_ptr(stream, self.device.index))
        _abi.check(rc, self._fn("load"))
        self._sources = src
        self.weights = self.biases = self.packed = None
        if keep_host:
            if stream is not None:
                stream.synchronize()
            self.weights = [np.ascontiguousarray(_to_numpy(w), dtype=np.float32) for w, _ in src]
            self.biases = [np.ascontiguousarray(_to_numpy(v), dtype=np.float32) for _, v in src]
            self.packed = self._pack_host()
        return self

    def _pack_host(self):
        """ctr_actor_pack / ctr_critic_pack of the host copies -> the blob's bytes (numpy uint8)."""
        lib = _abi.load()
        nb = int(getattr(lib, self._fn("blob_bytes"))(self._struct))
        if nb < 0:
            raise _abi.CtrError(self._fn("blob_bytes") + ": " + lib.ctr_last_error().decode())
        host = np.zeros(nb, dtype=np.uint8)
        n = len(self.weights)
        W = (_abi._P * n)(*[w.ctypes.data for w in self.weights])
        b = (_abi._P * n)(*[v.ctypes.data for v in self.biases])
        _abi.check(getattr(lib, self._fn("pack"))(self._struct, W, b, host.ctypes.data), self._fn("pack"))
        return host

    def _upload(self, device):
        import torch
        self.packed = host = self._pack_host()
        self.device = torch.device(device)
        self.blob = torch.from_numpy(host).to(self.device)
        if self.blob.data_ptr() % 16:
            raise RuntimeError(self.NAME + " blob not 16-B aligned")
        self._struct.blob = self.blob.data_ptr()

    def _emulate_output(self, x):
        """The shared arithmetic (include/ctr_reach_amd.h) in numpy float64 with the kernel's bf16
        roundings: x [n, in_dim] float32 -> the output layer's result [n, OUT] float64; the bf16
        activations of every hidden layer in ``self.last_hidden``."""
        hi = bf16_round(x)
        lo = bf16_round(x - hi)
        Wq = [bf16_round(W).astype(np.float64) for W in self.weights]
        z = hi.astype(np.float64) @ Wq[0].T + lo.astype(np.float64) @ Wq[0].T
        self.last_hidden = []
        for l in range(len(self.hidden)):
            z = (z.astype(np.float32) + self.biases[l]).astype(np.float32)      # f32 result + f32 bias
            h = bf16_round(np.where(z > 0, z, np.float32(0)))
            self.last_hidden.append(h)
            z = h.astype(np.float64) @ Wq[l + 1].T
        return z + self.biases[-1].astype(np.float64)

    def _reference_output(self, x):
        """The plain float64 MLP (no bf16 anywhere) up to the output layer's result."""
        z = x
        for l, (W, b) in enumerate(zip(self.weights, self.biases)):
            z = z @ W.astype(np.float64).T + b.astype(np.float64)
            if l < len(self.hidden):
                z = np.maximum(z, 0.0)
        return z

    def _need_host(self):
        if self.weights is None:
            raise RuntimeError("the host copy of the weights was dropped by load_; load with keep_host=True")


class MlpActor(_Mlp):
    """``layers``: [(W, b), ...] numpy arrays or torch tensors in torch's [out, in] convention, 1..3
    hidden layers (widths multiples of 32, at most 256) and the 6-row output layer; the first
    layer takes the flat row of obs_dim + 6 = 19 or 20 floats.  ``scale``: the action space's high
    (6 floats): action = scale * tanh(output).  ``device`` None keeps the actor on the host
    (``emulate`` only).

    Training: build the actor once from the learner's initial weights, then refresh it on the
    device after every optimiser step with ``load_``: one launch on the learner's stream, no copy
    to the host, no allocation (it can sit in a captured graph next to the update).

        actor = MlpActor.from_torch(policy, venv.action_space.high, "cuda")
        for it in range(iterations):
            venv.collect(actor, steps, noise)
            ...                                   # the learner's update of ``policy`` on her.sample(...)
            optimiser.step()
            actor.load_(policy)                   # ctr_actor_load: the blob now holds the new weights"""

    NAME, IN_DIMS, OUT, TANH = "actor", (19, 20), 6, True
    _IN_MSG = "the first layer takes the flat row of obs_dim + 6 = 19 or 20 floats"
    _OUT_MSG = "the output layer has 6 rows (the actions)"

    def __init__(self, layers, scale, device=None):
        self._init_layers(layers, _abi.CtrActor())
        self.scale = np.ascontiguousarray(scale, dtype=np.float32).reshape(-1)
        if self.scale.shape != (6,) or not np.isfinite(self.scale).all():
            raise ValueError("scale must be 6 finite floats")
        for i in range(6):
            self._struct.scale[i] = float(self.scale[i])
        if device is not None:
            self._upload(device)

    @classmethod
    def from_torch(cls, seq, scale, device=None):
        """From an ``nn.Sequential`` of Linear, ReLU, ..., Linear, Tanh."""
        return cls(_sequential_layers(seq), scale, device)

    def emulate(self, rows):
        """The actor's arithmetic (include/ctr_reach_amd.h) in numpy float64 with the kernel's bf16
        roundings: rows [n, in_dim] -> (actions [n, 6], logits [n, 6]) float64.  Also returns the
        intermediates in ``self.last_hidden`` (the bf16 activations of every hidden layer)."""
        self._need_host()
        x = np.asarray(rows, dtype=np.float32).reshape(-1, self.in_dim)
        with np.errstate(invalid="ignore", over="ignore"):
            y = self._emulate_output(x)
            return self.scale.astype(np.float64) * np.tanh(y), y

    def reference(self, rows):
        """The plain float64 MLP (no bf16 anywhere): actions [n, 6]."""
        self._need_host()
        z = self._reference_output(np.asarray(rows, dtype=np.float64).reshape(-1, self.in_dim))
        return self.scale.astype(np.float64) * np.tanh(z)

    def __call__(self, rows, logits=False, stream=None):
        """ctr_actor: rows [n, in_dim] float32 device tensor -> actions [n, 6] (and the pre-tanh
        outputs with ``logits``)."""
        import torch
        if self.blob is None:
            raise RuntimeError("the actor is on the host (MlpActor(..., device=None))")
        rows = rows.to(device=self.device, dtype=torch.float32).contiguous()
        if rows.dim() != 2 or rows.shape[1] != self.in_dim:
            raise ValueError("rows must be [n, %d]" % self.in_dim)
        n = rows.shape[0]
        act = torch.empty((n, 6), dtype=torch.float32, device=self.device)
        lg = torch.empty((n, 6), dtype=torch.float32, device=self.device) if logits else None
        rc = _abi.load().ctr_actor(self._struct, _abi.ptr(rows), n, _abi.ptr(act), _abi.ptr(lg),
                                   _abi.stream_ptr(stream, self.device.index))
        _abi.check(rc, "ctr_actor")
        return (act, lg) if logits else act


class MlpCritic(_Mlp):
    """The Q-network of the reference's DDPG on the device (ctr_critic / ctr_her_sample_td).
    ``layers``: [(W, b), ...] as ``MlpActor`` takes them, 1..3 hidden layers (widths multiples of
    32, at most 256) and the 1-row output layer; the first layer takes [row, action]: the flat row
    and the six actions in the normalised box [-1, 1], obs_dim + 12 = 25 or 26 floats.  ``device``
    None keeps the critic on the host (``emulate`` only).

        critic_targ = MlpCritic.from_torch(critic_targ_net, "cuda")
        q = critic_targ(rows, actions / scale)                  # one ctr_critic launch
        batch = her.sample_td(256, actor_targ, critic_targ, 0.98)   # the batch and its DDPG target
        critic_targ.load_(critic_targ_net)                      # after the Polyak update: ctr_critic_load

    ``emulate`` is the CPU reference of the arithmetic (numpy, no GPU, no library)."""

    NAME, IN_DIMS, OUT, TANH = "critic", (25, 26), 1, False
    _IN_MSG = "the first layer takes [row, action]: obs_dim + 12 = 25 or 26 floats"
    _OUT_MSG = "the output layer has 1 row (Q)"

    def __init__(self, layers, device=None):
        self._init_layers(layers, _abi_critic.CtrCritic())
        if device is not None:
            self._upload(device)

    @classmethod
    def from_torch(cls, seq, device=None):
        """From an ``nn.Sequential`` of Linear, ReLU, ..., Linear (no Tanh, one output)."""
        return cls(_sequential_layers(seq, False, "critic"), device)

    def _input(self, rows, actions, dtype):
        r = np.asarray(rows, dtype=dtype).reshape(-1, self.in_dim - 6)
        a = np.asarray(actions, dtype=dtype).reshape(-1, 6)
        if r.shape[0] != a.shape[0]:
            raise ValueError("rows and actions differ in length")
        return np.concatenate([r, a], axis=1)

    def emulate(self, rows, actions):
        """The critic's arithmetic (include/ctr_reach_amd.h) in numpy float64 with the kernel's bf16
        roundings: rows [n, in_dim - 6], actions [n, 6] -> q [n] float64.  The bf16 activations of
        every hidden layer are left in ``self.last_hidden``."""
        self._need_host()
        with np.errstate(invalid="ignore", over="ignore"):
            return self._emulate_output(self._input(rows, actions, np.float32))[:, 0]

    def reference(self, rows, actions):
        """The plain float64 MLP (no bf16 anywhere): q [n]."""
        self._need_host()
        return self._reference_output(self._input(rows, actions, np.float64))[:, 0]

    def __call__(self, rows, actions, stream=None):
        """ctr_critic: rows [n, in_dim - 6] and actions [n, 6] float32 device tensors -> q [n]."""
        import torch
        if self.blob is None:
            raise RuntimeError("the critic is on the host (MlpCritic(..., device=None))")
        rows = rows.to(device=self.device, dtype=torch.float32).contiguous()
        actions = actions.to(device=self.device, dtype=torch.float32).contiguous()
        if rows.dim() != 2 or rows.shape[1] != self.in_dim - 6:
            raise ValueError("rows must be [n, %d]" % (self.in_dim - 6))
        n = rows.shape[0]
        if tuple(actions.shape) != (n, 6):
            raise ValueError("actions must be [%d, 6]" % n)
        q = torch.empty(n, dtype=torch.float32, device=self.device)
        rc = _abi.load().ctr_critic(self._struct, _abi.ptr(rows), _abi.ptr(actions), n, _abi.ptr(q),
                                    _abi.stream_ptr(stream, self.device.index))
        _abi.check(rc, "ctr_critic")
        return q


def philox4x32(counter, key):
    """Philox4x32-10 in numpy: counter [..., 4] and key [..., 2] uint32 (broadcast against each other)
    -> the block's four words [..., 4] uint32."""
    c = np.asarray(counter, dtype=np.uint32)
    k = np.asarray(key, dtype=np.uint32)
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape).astype(np.uint64) for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape).astype(np.uint64) for i in range(2))
    m32 = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2     # 32 x 32 -> 64 bits
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack((c0, c1, c2, c3), axis=-1).astype(np.uint32)


class ExploreNoise(object):
    """The exploration of the reference's DDPG + HER training (ctr_explore / ctr_collect,
    include/ctr_reach_amd.h "Exploration noise"): Gaussian action noise of std ``sigma`` (a scalar
    or 6 values, in units of the action box), clipped to the box, and with probability
    ``random_eps`` a uniformly random action of the box instead.  The noise of a step is a pure
    function of (seed, global env id, reset number, the env's clock before the step).

        noise = ExploreNoise(0.3, random_eps=0.3, seed=1)
        venv.step(venv.explore(venv.act(actor), noise))      # one launch each
        venv.collect(actor, 20, noise)                       # the same 20 times, one launch per period

    ``emulate`` is the numpy restatement (no GPU, no library)."""

    STREAM = 6

    def __init__(self, sigma, random_eps=0.0, seed=0):
        s = np.asarray(sigma, dtype=np.float32).reshape(-1)
        if s.shape == (1,):
            s = np.repeat(s, 6)
        if s.shape != (6,) or not np.isfinite(s).all() or (s < 0).any():
            raise ValueError("sigma must be a scalar or 6 values, finite and >= 0")
        eps = np.float32(random_eps)
        if not 0.0 <= eps <= 1.0:
            raise ValueError("random_eps must be in [0, 1]")
        self.sigma, self.random_eps = np.ascontiguousarray(s), eps
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        x = self._struct = _abi.CtrExplore()
        x.seed, x.random_eps = self.seed, float(eps)
        for i in range(6):
            x.sigma[i] = float(s[i])

    def uniforms(self, genv, epoch, t):
        """The step's seven uniforms [n, 7] float32 (exact: 24 bits each)."""
        genv, epoch, t = np.broadcast_arrays(np.asarray(genv, dtype=np.uint64), np.asarray(epoch, dtype=np.uint64),
                                             np.asarray(t, dtype=np.uint64))
        m32 = np.uint64(0xFFFFFFFF)
        key = np.array([self.seed & 0xFFFFFFFF, self.seed >> 32], dtype=np.uint32)
        w = []
        for blk in range(2):
            ctr = np.stack(((t & m32) | np.uint64(blk << 16), epoch & m32, genv & m32,
                            (genv >> np.uint64(32)) ^ np.uint64(self.STREAM << 24)), axis=-1).astype(np.uint32)
            w.append(philox4x32(ctr, key))
        w = np.concatenate(w, axis=-1)[..., :7]
        return (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)

    def emulate(self, genv, epoch, t, actions, scale):
        """The noise of envs ``genv`` (global ids) in episode ``epoch`` at clock ``t`` on ``actions``
        [n, 6] in the box ``scale`` (6 values): the perturbed actions [n, 6] float64.  The uniforms,
        the random branch and the choice between the branches are float32 and exact (equal to the
        device's bits); the Gaussian branch is plain float64 on them.  ``self.last_random`` marks
        the rows that took the random action."""
        a32 = np.asarray(actions, dtype=np.float32).reshape(-1, 6)
        sc = np.asarray(scale, dtype=np.float32).reshape(6)
        n = a32.shape[0]
        self.last_random = np.zeros(n, dtype=bool)
        if not self.sigma.any() and self.random_eps == 0:
            return a32.astype(np.float64)                      # the no-op case: the bits stay
        u = self.uniforms(np.broadcast_to(genv, (n,)), np.broadcast_to(epoch, (n,)), np.broadcast_to(t, (n,)))
        rnd = u[:, 6] < self.random_eps
        self.last_random = rnd
        uniform = sc * (np.float32(2) * u[:, :6] - np.float32(1))            # float32, one rounding
        u64 = u.astype(np.float64)
        r = np.sqrt(-2.0 * np.log(1.0 - u64[:, 0:6:2]))
        ang = float(np.float32(6.2831855)) * u64[:, 1:6:2]
        z = np.stack((r * np.cos(ang), r * np.sin(ang)), axis=-1).reshape(n, 6)
        box = np.abs(sc)
        s = (self.sigma * box).astype(np.float64)                            # the float32 product
        gauss = np.clip(a32.astype(np.float64) + s * z, -box.astype(np.float64), box.astype(np.float64))
        return np.where(rnd[:, None], uniform.astype(np.float64), gauss)


class TargetSmoothing(object):
    """TD3's target policy smoothing as ctr_her_sample_td3 applies it (include/ctr_reach_amd.h,
    "TD3"): Gaussian noise of std ``sigma`` clipped to +-``clip`` on the target action, the sum
    clipped to the normalised box [-1, 1].  The noise of a row is a pure function of (seed, counter,
    the row's index in the batch).

        batch = buf.sample_td3(256, actor_targ, critic1_targ, critic2_targ, gamma, sigma=0.2, clip=0.5)

    ``emulate`` is the numpy restatement (no GPU, no library)."""

    STREAM = 7

    def __init__(self, sigma=0.2, clip=0.5):
        sigma, clip = np.float32(sigma), np.float32(clip)
        if not (np.isfinite(sigma) and sigma >= 0):
            raise ValueError("sigma must be finite and >= 0")
        if not clip >= 0:
            raise ValueError("clip must be >= 0 (inf: the noise is not clipped)")
        self.sigma, self.clip = sigma, clip

    def uniforms(self, seed, counter, index):
        """The six uniforms [n, 6] float32 of rows ``index`` (exact: 24 bits each)."""
        seed, counter = int(seed) & 0xFFFFFFFFFFFFFFFF, int(counter) & 0xFFFFFFFFFFFFFFFF
        i = np.asarray(index, dtype=np.uint64).reshape(-1) & np.uint64(0xFFFFFFFF)
        key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
        w = []
        for blk in range(2):
            ctr = np.stack((np.full_like(i, blk), np.full_like(i, counter & 0xFFFFFFFF), i,
                            np.full_like(i, (counter >> 32) ^ (self.STREAM << 24))), axis=-1).astype(np.uint32)
            w.append(philox4x32(ctr, key))
        w = np.concatenate(w, axis=-1)[..., :6]
        return (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)

    def gaussians(self, seed, counter, index):
        """The six standard Gaussians [n, 6] float64 of rows ``index``: Box-Muller in plain float64
        on the exact uniforms."""
        u64 = self.uniforms(seed, counter, index).astype(np.float64)
        r = np.sqrt(-2.0 * np.log(1.0 - u64[:, 0:6:2]))
        ang = float(np.float32(6.2831855)) * u64[:, 1:6:2]
        return np.stack((r * np.cos(ang), r * np.sin(ang)), axis=-1).reshape(-1, 6)

    def emulate(self, seed, counter, index, actions):
        """The smoothed actions [n, 6] float64 of the rows ``index`` (their places in the batch) of
        draw (seed, counter) on the target actions ``actions`` [n, 6] in [-1, 1].  The uniforms are
        float32 and exact (equal to the device's bits); the Gaussian, the clip and the sum are plain
        float64 on them.  sigma == 0: the actions' bits."""
        a32 = np.asarray(actions, dtype=np.float32).reshape(-1, 6)
        if self.sigma == 0:
            return a32.astype(np.float64)                      # the no-op case: the bits stay
        index = np.broadcast_to(np.asarray(index, dtype=np.uint64).reshape(-1), (a32.shape[0],))
        z = self.gaussians(seed, counter, index)
        e = np.clip(float(self.sigma) * z, -float(self.clip), float(self.clip))
        return np.clip(a32.astype(np.float64) + e, -1.0, 1.0)


def gauss_head(y, eps, scale, dtype=np.float64):
    """The tanh-Gaussian head (include/ctr_reach_amd.h, "SAC") on the head's outputs ``y`` [n, 12] and
    the standard normals ``eps`` [n, 6], every operation in ``dtype`` and in the header's order:
    dict(action, unit, logp, s, u).  float64 is the reference; float32 restates the kernel's roundings
    (numpy's exp, tanh and log1p in place of the device's)."""
    f = np.dtype(dtype).type
    y, eps, scale = np.asarray(y, dtype=f), np.asarray(eps, dtype=f), np.asarray(scale, dtype=f).reshape(6)
    with np.errstate(over="ignore", under="ignore"):
        s = np.minimum(np.maximum(y[:, 6:], f(-20)), f(2))
        u = (np.exp(s) * eps + y[:, :6]) if dtype == np.float64 else \
            (np.exp(s).astype(np.float64) * eps.astype(np.float64) + y[:, :6].astype(np.float64)).astype(f)   # fmaf
        t = np.tanh(u)
        x = f(-2) * u
        softplus = np.maximum(x, f(0)) + np.log1p(np.exp(-np.abs(x)))
        a = (f(-0.5) * (eps * eps) - s) - f(0.9189385332046727)
        c = f(2) * ((f(0.6931471805599453) - u) - softplus)
        term = a - c
        logp = np.zeros(len(y), dtype=f)
        for i in range(6):
            logp = logp + term[:, i]
    return dict(action=scale * t, unit=t, logp=logp, s=s, u=u)


class GaussianActor(_Mlp):
    """SAC's tanh-Gaussian policy on the device (ctr_gauss_act, include/ctr_reach_amd.h "SAC"):
    ``MlpActor``'s network with a 12-row output layer and no Tanh behind it, rows 0..5 the mean and
    rows 6..11 the log standard deviation (clipped to [-20, 2]).  ``layers`` / ``from_torch`` as
    ``MlpActor`` takes them (``nn.Sequential(Linear, ReLU, ..., Linear(h, 12))``), ``scale`` the
    action space's high, ``seed`` the key of the noise.

        pi = GaussianActor.from_torch(policy, venv.action_space.high, "cuda")
        out = pi.sample(venv.actor_rows(), counter=step, row_base=venv.env_base)
        venv.step(out["action"])                  # out["unit"] is what a critic takes, out["logp"] its log-probability
        pi.load_(policy)                          # after the learner's step: ctr_gauss_load
        venv.rollout(pi.mean_actor(), 20)         # the deterministic mean through the period kernels

    The noise of a row is a pure function of (seed, counter, row_base + the row's index).
    ``emulate`` is the numpy restatement (no GPU, no library)."""

    NAME, IN_DIMS, OUT, TANH = "actor", (19, 20), 12, False
    STREAM = 8
    _IN_MSG = "the first layer takes the flat row of obs_dim + 6 = 19 or 20 floats"
    _OUT_MSG = "the output layer has 12 rows (six means, six log standard deviations)"

    def __init__(self, layers, scale, device=None, seed=0):
        self._init_layers(layers, _abi.CtrActor())
        self.scale = np.ascontiguousarray(scale, dtype=np.float32).reshape(-1)
        if self.scale.shape != (6,) or not np.isfinite(self.scale).all():
            raise ValueError("scale must be 6 finite floats")
        for i in range(6):
            self._struct.scale[i] = float(self.scale[i])
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._mean = self._mean_sources = None
        if device is not None:
            self._upload(device)

    @classmethod
    def from_torch(cls, seq, scale, device=None, seed=0):
        """From an ``nn.Sequential`` of Linear, ReLU, ..., Linear(h, 12)."""
        return cls(_sequential_layers(seq, False, "policy"), scale, device, seed)

    def _fn(self, what):
        return "ctr_gauss_" + what

    def uniforms(self, counter, index):
        """The six uniforms [n, 6] float32 of rows ``index`` (row_base + the row) of draw ``counter``
        (exact: 24 bits each)."""
        return TargetSmoothing.uniforms(self, self.seed, counter, index)

    def gaussians(self, counter, index, dtype=np.float64):
        """The six standard normals [n, 6] of rows ``index``: Box-Muller in ``dtype`` on the exact
        uniforms (float64: the reference; float32: numpy's restatement of the kernel's roundings)."""
        f = np.dtype(dtype).type
        u = self.uniforms(counter, index).astype(f)
        r = np.sqrt(f(-2) * np.log(f(1) - u[:, 0:6:2]))
        ang = f(np.float32(6.2831855)) * u[:, 1:6:2]
        return np.stack((r * np.cos(ang), r * np.sin(ang)), axis=-1).reshape(-1, 6)

    def emulate(self, rows, counter, row_base=0, deterministic=False):
        """The policy's arithmetic in numpy: the bf16 head as the kernel makes it, then the header's
        formulas in float64 on the exact uniforms: dict(action, unit, logp [n], logits [n, 12], s, u)."""
        self._need_host()
        x = np.asarray(rows, dtype=np.float32).reshape(-1, self.in_dim)
        with np.errstate(invalid="ignore", over="ignore"):
            y = self._emulate_output(x)
        n = len(x)
        eps = np.zeros((n, 6)) if deterministic else self.gaussians(counter, int(row_base) + np.arange(n))
        out = gauss_head(y, eps, self.scale)
        out["logits"] = y
        return out

    def mean_layers(self, layers):
        """``layers`` as ``load_`` takes them with the output layer cut to its first six rows (the
        mean; contiguous views, nothing copied): what the mean actor's ``load_`` takes."""
        import torch
        if isinstance(layers, torch.nn.Module):
            layers = _sequential_layers(layers, False, "policy", detach=False)
        layers = [tuple(pair) for pair in layers]
        W, b = layers[-1]
        return layers[:-1] + [(W[:6], b[:6])]

    def mean_actor(self):
        """The policy's deterministic mean as an ``MlpActor`` on the same device (action = scale *
        tanh(mu)), for ``venv.rollout`` / ``follow`` / ``collect`` and the path comparisons.  Built
        once; after a ``load_`` the next call refreshes it from the same device parameters."""
        if self.blob is None:
            raise RuntimeError("the policy is on the host (GaussianActor(..., device=None))")
        if self._mean is None:
            if self.weights is not None:
                layers = list(zip(self.weights[:-1], self.biases[:-1])) + [(self.weights[-1][:6], self.biases[-1][:6])]
            else:
                layers = self.mean_layers(self._sources)
            self._mean = MlpActor(layers, self.scale, self.device)
            self._mean_sources = self._sources
        elif self._sources is not None and self._mean_sources is not self._sources:
            self._mean.load_(self.mean_layers(self._sources))
            self._mean_sources = self._sources
        return self._mean

    def sample(self, rows, counter, row_base=0, deterministic=False, logits=False, stream=None):
        """ctr_gauss_act: rows [n, in_dim] float32 device tensor -> dict(action [n, 6], unit [n, 6],
        logp [n]) and with ``logits`` the head's outputs [n, 12].  One launch."""
        import torch
        if self.blob is None:
            raise RuntimeError("the policy is on the host (GaussianActor(..., device=None))")
        rows = rows.to(device=self.device, dtype=torch.float32).contiguous()
        if rows.dim() != 2 or rows.shape[1] != self.in_dim:
            raise ValueError("rows must be [n, %d]" % self.in_dim)
        n = rows.shape[0]
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device)  # noqa: E731
        out = dict(action=new(n, 6), unit=new(n, 6), logp=new(n))
        if logits:
            out["logits"] = new(n, 12)
        rc = _abi.load().ctr_gauss_act(self._struct, _abi.ptr(rows), n, self.seed, int(counter) & 0xFFFFFFFFFFFFFFFF,
                                       int(row_base), int(bool(deterministic)), _abi.ptr(out["action"]),
                                       _abi.ptr(out["unit"]), _abi.ptr(out["logp"]), _abi.ptr(out.get("logits")),
                                       _abi.stream_ptr(stream, self.device.index))
        _abi.check(rc, "ctr_gauss_act")
        return out


def polyak_(nets, tau, stream=None):
    """The soft (Polyak) update of 1..4 target networks and the refresh of their device blobs in one
    launch (ctr_polyak).  ``nets``: a list of triples ``(net, online, target)``: ``net`` the device
    ``MlpActor`` / ``MlpCritic`` that holds the TARGET network's blob, ``online`` and ``target`` the
    learner's and the target's float32 parameters as ``load_`` takes them ([(W, b), ...] or an
    ``nn.Sequential``).  For every element, torch's ``lerp`` in float32 without fused multiply-add
    (include/ctr_reach_amd.h):

        target <- target + tau * (online - target)              (tau < 0.5)
        target <- online - (online - target) * (1 - tau)        (otherwise)

    stored over ``target``, and each net's blob becomes what ``net.load_(target)`` would make of the
    result.  It replaces the trainer's ``lerp_`` loop and the ``load_`` of each target:

        polyak_([(actor_targ, policy, policy_targ), (critic_targ_dev, critic, critic_targ)], 0.001)

    One launch on ``stream`` (default: the current stream); no allocation, no copy to the host and
    no synchronisation, so it can be captured into a graph.  Every tensor is checked as ``load_``
    checks it (ValueError, nothing converted, nothing written); a target tensor must not require
    grad, since it is written behind autograd's back; a host-only net raises RuntimeError.
    Afterwards each net's sources are its target tensors and its host copies (``weights``,
    ``biases``, ``packed``) are dropped, as ``load_`` drops them; ``net.load_(target,
    keep_host=True)`` brings them back."""
    from . import _abi_polyak
    nets = [tuple(n) for n in nets]
    if not 1 <= len(nets) <= _abi_polyak.CTR_POLYAK_MAX_NETS or any(len(n) != 3 for n in nets):
        raise ValueError("nets is a list of 1..%d triples (net, online, target)" % _abi_polyak.CTR_POLYAK_MAX_NETS)
    tau = float(tau)
    if not 0.0 <= tau <= 1.0:
        raise ValueError("tau must be in [0, 1]")
    arr = (_abi_polyak.CtrPolyakNet * len(nets))()
    device, done = None, []
    for m, (net, online, target) in enumerate(nets):
        if not isinstance(net, _Mlp) or isinstance(net, GaussianActor):
            raise ValueError("net %d must be an MlpActor or an MlpCritic" % m)
        on = net._device_layers(online, "net %d: online " % m)
        tg = net._device_layers(target, "net %d: target " % m, target=True)
        if device is not None and net.device != device:
            raise ValueError("net %d is on %s, net 0 on %s" % (m, net.device, device))
        device = net.device
        n = len(on)
        a = arr[m]
        setattr(a, net.NAME, ctypes.pointer(net._struct))
        a.W = (_abi._P * n)(*[w.data_ptr() for w, _ in on])
        a.b = (_abi._P * n)(*[v.data_ptr() for _, v in on])
        a.W_targ = (_abi._P * n)(*[w.data_ptr() for w, _ in tg])
        a.b_targ = (_abi._P * n)(*[v.data_ptr() for _, v in tg])
        done.append((net, tg))
    rc = _abi.load().ctr_polyak(arr, len(nets), tau, _abi.stream_ptr(stream, device.index))
    _abi.check(rc, "ctr_polyak")
    for net, tg in done:
        net._sources = tg
        net.weights = net.biases = net.packed = None


def _sequential_layers(seq, tanh=True, name="actor", detach=True):
    """[(W, b), ...] (detached, or with ``detach`` False the parameters themselves) of an
    ``nn.Sequential`` of Linear, ReLU, ..., Linear, then Tanh (the actor) or nothing (the critic)."""
    import torch.nn as nn
    mods = list(seq)
    if tanh:
        if not mods or not isinstance(mods[-1], nn.Tanh):
            raise ValueError("the actor ends with nn.Tanh")
        mods = mods[:-1]
    elif not mods or not isinstance(mods[-1], nn.Linear):
        raise ValueError("the %s ends with its output nn.Linear (no activation after it)" % name)
    layers = []
    for i, m in enumerate(mods):
        if i % 2 == 0:
            if not isinstance(m, nn.Linear) or m.bias is None:
                raise ValueError("module %d must be an nn.Linear with a bias" % i)
            layers.append((m.weight.detach(), m.bias.detach()) if detach else (m.weight, m.bias))
        elif not isinstance(m, nn.ReLU):
            raise ValueError("module %d must be an nn.ReLU" % i)
    if len(mods) % 2 == 0:
        raise ValueError("expected Linear, ReLU, ..., Linear" + (", Tanh" if tanh else ""))
    return layers


def _to_numpy(t):
    if hasattr(t, "detach"):
        return t.detach().cpu().numpy()
    return np.asarray(t)
