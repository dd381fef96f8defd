"""HerReplayBuffer -- the replay side of the reference's training pipeline, on the device.

The reference trains CTR-Reach with stable-baselines 2 HER + DDPG (goal_selection_strategy
'future', n_sampled_goal 4, batch_size 256, buffer_size 500000: saved_policies/**/her/
CTR-Generic-Reach-v0_1/CTR-Generic-Reach-v0/config.yml).  That wrapper keeps each episode's
transitions, and when the episode ends stores every transition plus, for all but the last one,
k copies whose desired goal is the achieved goal of a later observation of the same episode,
with the reward recomputed by ``env.compute_reward`` (envs/ctr_reach_env.py:160-170).
``ReplayBuffer.sample`` then draws rows uniformly.

Here the episodes are recorded where the environments run (``ctr_her_record`` after every
``ctr_step``; ``ctr_her_open`` after every ``ctr_reset``) and the relabelled rows are formed
when they are sampled (``ctr_her_sample``) from goal indices fixed per row, so a row costs no
HBM until it is drawn.  Sampled batches are device tensors in HERGoalEnvWrapper's flat layout
``[observation, achieved_goal, desired_goal]``.

Differences from stable-baselines (documented, not hidden):
  * capacity is in episodes: every env keeps its last ``slots - 1`` finished episodes (FIFO per
    env) instead of a global FIFO of rows;
  * the relabel draws come from Philox keyed (seed, global env id, reset number, t, j), not
    numpy's global RNG, so rows match the wrapper in distribution, not draw for draw.
"""
import ctypes

import numpy as np

from . import _abi, _abi_critic

STRATEGIES = {"future": _abi.CTR_HER_FUTURE, "final": _abi.CTR_HER_FINAL, "episode": _abi.CTR_HER_EPISODE}


def _torch():
    import torch
    return torch


class HerReplayBuffer(object):
    def __init__(self, venv, slots=4, n_sampled_goal=4, goal_selection_strategy="future", seed=None):
        torch = _torch()
        if goal_selection_strategy not in STRATEGIES:
            raise ValueError("goal_selection_strategy must be one of %s" % sorted(STRATEGIES))
        if int(slots) < 2:
            raise ValueError("slots must be >= 2 (one episode is always being recorded)")
        if venv.obs_dtype != torch.float32:
            # ctr_her_open / ctr_her_record / the fused recording read the env's observation
            # rows as float32
            raise ValueError("the HER feed records float32 observations: build the env with obs_dtype='float32'")
        self.venv = venv
        self.lib = venv.lib
        self.n_sampled_goal = int(n_sampled_goal)
        self.strategy = goal_selection_strategy
        self.slots = int(slots)
        self.t_max = int(venv.max_steps_per_episode)
        self.obs_dim = venv.obs_dim
        self.seed = int(venv.seed_value if seed is None else seed) & 0xFFFFFFFFFFFFFFFF
        n, dev, T = venv.num_envs, venv.device, self.t_max
        E = n * self.slots
        f32, f64, i32 = torch.float32, torch.float64, torch.int32
        S = self.slots                     # env-minor 96-B / 32-B rows (include/ctr_reach_amd.h ctr_her_t)
        self.state = torch.zeros((S, T + 1, n, 24), dtype=f32, device=dev)
        self.step_rows = torch.zeros((S, T, n, 8), dtype=f32, device=dev)
        self.obs = self.state[..., :self.obs_dim]                       # views
        self.ag = self.state[..., 16:22].view(f64)
        self.action = self.step_rows[..., :6]
        self.reward = self.step_rows[..., 6]
        self.dg = torch.zeros((E, 3), dtype=f64, device=dev)
        self.tol = torch.zeros(E, dtype=f64, device=dev)
        self.len = torch.zeros(E, dtype=i32, device=dev)
        self.epoch = torch.zeros(E, dtype=i32, device=dev)
        self.cur_t = torch.full((n,), -1, dtype=i32, device=dev)
        self.cur_epoch = torch.zeros(n, dtype=i32, device=dev)
        tile = _abi.CTR_HER_SCAN_TILE        # sampler scratch: CTR_HER_CDF_LEN(E) prefix sums
        self.cdf = torch.zeros(E + (E + tile - 1) // tile + 1, dtype=torch.int64, device=dev)
        p = _abi.ptr
        h = self._h = _abi.CtrHer()
        h.obs_dim, h.t_max, h.n_sampled_goal, h.strategy = self.obs_dim, T, self.n_sampled_goal, STRATEGIES[self.strategy]
        h.n, h.env_base, h.slots, h.seed = n, venv.env_base, self.slots, self.seed
        h.state, h.step = p(self.state), p(self.step_rows)
        h.dg, h.tol, h.len, h.epoch = p(self.dg), p(self.tol), p(self.len), p(self.epoch)
        h.cur_t, h.cur_epoch, h.cdf = p(self.cur_t), p(self.cur_epoch), p(self.cdf)
        self._counter = 0
        self.fused = True        # record inside the step (ctr_step_her); False: ctr_her_record after it
        venv._her = self

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.state, self.step_rows, self.dg, self.tol,
                                                           self.len, self.epoch, self.cur_t, self.cur_epoch,
                                                           self.cdf))

    # called by CtrReachVecEnv
    def _open(self, mask, stream):
        rc = self.lib.ctr_her_open(self._h, self.venv._batch, _abi.ptr(self.venv.obs), _abi.ptr(mask),
                                   _abi.stream_ptr(stream, self.venv.device.index))
        _abi.check(rc, "ctr_her_open")

    def _record(self, actions, stream):
        rc = self.lib.ctr_her_record(self._h, self.venv._batch, _abi.ptr(actions), self.venv._out,
                                     float(self.venv.cfg.tol), _abi.stream_ptr(stream, self.venv.device.index))
        _abi.check(rc, "ctr_her_record")

    def rows_per_episode(self, L):
        L = np.asarray(L, dtype=np.int64)
        if self.strategy == "future":
            return np.where(L > 0, L + self.n_sampled_goal * (L - 1), 0)
        return np.where(L > 0, L * (1 + self.n_sampled_goal), 0)

    def __len__(self):
        """Stored rows (len(ReplayBuffer) of the wrapper's buffer); synchronises."""
        return int(self.rows_per_episode(self.len.clamp(min=0).cpu().numpy()).sum())

    def _batch(self, batch_size, return_index):
        """The output tensors of a draw of ``batch_size`` rows and their ctr_her_batch_t."""
        torch = _torch()
        B = int(batch_size)
        d = self.obs_dim + 6
        dev = self.venv.device
        out = dict(obs=torch.empty((B, d), dtype=torch.float32, device=dev),
                   action=torch.empty((B, 6), dtype=torch.float32, device=dev),
                   reward=torch.empty(B, dtype=torch.float32, device=dev),
                   next_obs=torch.empty((B, d), dtype=torch.float32, device=dev),
                   done=torch.empty(B, dtype=torch.float32, device=dev))
        idx = torch.empty((B, 3), dtype=torch.int32, device=dev) if return_index else None
        hb = _abi.CtrHerBatch()
        p = _abi.ptr
        hb.obs, hb.action, hb.reward, hb.next_obs, hb.done, hb.index = (p(out["obs"]), p(out["action"]),
                                                                        p(out["reward"]), p(out["next_obs"]),
                                                                        p(out["done"]), p(idx))
        if return_index:
            out["index"] = idx
        return B, out, hb

    def _draw_seed(self, seed):
        return ((self.seed ^ 0x5DEECE66D) if seed is None else int(seed)) & 0xFFFFFFFFFFFFFFFF

    def sample(self, batch_size, seed=None, stream=None, return_index=False):
        """ReplayBuffer.sample(batch_size) on the device: dict of obs [B, d], action [B, 6],
        reward [B], next_obs [B, d], done [B] (d = obs_dim + 6) float32 tensors, plus index
        [B, 3] = (slot, t, j) with ``return_index``.  Asynchronous."""
        B, out, hb = self._batch(batch_size, return_index)
        rc = self.lib.ctr_her_sample(self._h, B, self._draw_seed(seed), self._counter, hb,
                                     _abi.stream_ptr(stream, self.venv.device.index))
        _abi.check(rc, "ctr_her_sample")
        self._counter += 1
        return out

    def sample_td(self, batch_size, actor, critic, gamma, seed=None, stream=None, return_index=False,
                  return_next=False):
        """``sample`` with the DDPG target of the drawn rows (ctr_her_sample_td): the same dict, plus
        target [B] = reward + gamma * (1 - done) * Q'(next_obs, pi'(next_obs)) from the target policy
        ``actor`` (an ``MlpActor``; its scale is not applied: pi' = tanh of its logits, in [-1, 1]) and
        the target critic ``critic`` (an ``MlpCritic``), both on this buffer's device.  With
        ``return_next`` also q_next [B] and next_action [B, 6].  One draw: the counter advances as in
        ``sample``, and two buffers in the same state give the same rows from either.  Asynchronous."""
        torch = _torch()
        B, out, hb = self._batch(batch_size, return_index)
        dev = self.venv.device
        for net, name in ((actor, "actor"), (critic, "critic")):
            if getattr(net, "blob", None) is None:
                raise ValueError("sample_td: the %s must be on the device" % name)
            if net.device.type != dev.type or (None not in (net.device.index, dev.index)
                                               and net.device.index != dev.index):
                raise ValueError("sample_td: the %s is on %s, the buffer on %s" % (name, net.device, dev))
        out["target"] = torch.empty(B, dtype=torch.float32, device=dev)
        if return_next:
            out["q_next"] = torch.empty(B, dtype=torch.float32, device=dev)
            out["next_action"] = torch.empty((B, 6), dtype=torch.float32, device=dev)
        td = _abi_critic.CtrHerTd()
        td.actor, td.critic, td.gamma = ctypes.pointer(actor._struct), ctypes.pointer(critic._struct), float(gamma)
        td.target, td.q_next, td.next_action = (_abi.ptr(out["target"]), _abi.ptr(out.get("q_next")),
                                                _abi.ptr(out.get("next_action")))
        rc = self.lib.ctr_her_sample_td(self._h, B, self._draw_seed(seed), self._counter, hb, td,
                                        _abi.stream_ptr(stream, self.venv.device.index))
        _abi.check(rc, "ctr_her_sample_td")
        self._counter += 1
        return out

    def sample_td3(self, batch_size, actor, critic1, critic2, gamma, sigma=0.2, clip=0.5, seed=None, stream=None,
                   return_index=False, return_next=False):
        """``sample`` with the TD3 target of the drawn rows (ctr_her_sample_td3): ``sample_td``'s dict,
        with target [B] = reward + gamma * (1 - done) * min(Q1', Q2')(next_obs, a'') from the target
        policy ``actor`` and the two target critics (``MlpCritic``; they may be the same object), all
        on this buffer's device.  a'' = clip(pi'(next_obs) + clip(sigma * z, -clip, clip), -1, 1) is
        the smoothed target action in the normalised box: z a standard Gaussian keyed by (seed,
        counter, row) (``policy.TargetSmoothing`` restates it), ``sigma`` >= 0 its std (0: no noise,
        nothing drawn) and ``clip`` >= 0 its bound (``inf``: none).  With ``return_next`` also
        q1_next [B], q2_next [B] and next_action [B, 6] = a''.  One draw: the counter advances as in
        ``sample``.  Asynchronous."""
        from . import _abi_td3
        dev = self.venv.device
        for net, name in ((actor, "actor"), (critic1, "critic1"), (critic2, "critic2")):
            if getattr(net, "blob", None) is None:
                raise ValueError("sample_td3: the %s must be on the device" % name)
            if net.device.type != dev.type or (None not in (net.device.index, dev.index)
                                               and net.device.index != dev.index):
                raise ValueError("sample_td3: the %s is on %s, the buffer on %s" % (name, net.device, dev))
        gamma, sigma, clip = float(gamma), float(sigma), float(clip)
        if not np.isfinite(gamma):
            raise ValueError("sample_td3: gamma must be finite")
        if not (np.isfinite(sigma) and sigma >= 0.0):
            raise ValueError("sample_td3: sigma must be finite and >= 0")
        if not clip >= 0.0:
            raise ValueError("sample_td3: clip must be >= 0 (inf: the noise is not clipped)")
        torch = _torch()
        B, out, hb = self._batch(batch_size, return_index)
        out["target"] = torch.empty(B, dtype=torch.float32, device=dev)
        if return_next:
            out["q1_next"] = torch.empty(B, dtype=torch.float32, device=dev)
            out["q2_next"] = torch.empty(B, dtype=torch.float32, device=dev)
            out["next_action"] = torch.empty((B, 6), dtype=torch.float32, device=dev)
        td = _abi_td3.CtrHerTd3()
        td.actor, td.critic1, td.critic2 = (ctypes.pointer(actor._struct), ctypes.pointer(critic1._struct),
                                            ctypes.pointer(critic2._struct))
        td.gamma, td.sigma, td.clip = gamma, sigma, clip
        td.target, td.q1_next, td.q2_next, td.next_action = (_abi.ptr(out["target"]), _abi.ptr(out.get("q1_next")),
                                                             _abi.ptr(out.get("q2_next")),
                                                             _abi.ptr(out.get("next_action")))
        rc = self.lib.ctr_her_sample_td3(self._h, B, self._draw_seed(seed), self._counter, hb, td,
                                         _abi.stream_ptr(stream, self.venv.device.index))
        _abi.check(rc, "ctr_her_sample_td3")
        self._counter += 1
        return out

    def sample_sac(self, batch_size, policy, critic1, critic2, gamma, log_alpha, seed=None, stream=None,
                   return_index=False, return_next=False):
        """``sample`` with SAC's soft target of the drawn rows (ctr_her_sample_sac): the same dict, plus
        target [B] = reward + gamma * (1 - done) * (min(Q1', Q2')(next_obs, a') - alpha * logp(a')) with
        a' the CURRENT ``policy``'s stochastic action on next_obs in the normalised box (a
        ``GaussianActor``; its scale is not applied and its own seed is not used), the two target
        critics (``MlpCritic``; they may be the same object) and alpha = exp(log_alpha), all on this
        buffer's device.  ``log_alpha``: a 0-d or 1-element float32 tensor on the buffer's device
        (``SacLearner.log_alpha``), passed by pointer and read by the kernel when it runs, never on the
        host; anything that would need a conversion or a copy is refused with ValueError.  With
        ``return_next`` also q1_next [B], q2_next [B], next_action [B, 6] = a' and next_logp [B].

        The noise of a' is keyed by this draw's own (seed, counter): it is ``GaussianActor(...,
        seed=<the draw seed>).sample(next_obs, counter=<the draw's counter>, row_base=0)``, bit for
        bit.  ``_draw_seed`` already keeps that key apart from the collection's, so the caller needs
        no counter offsets.  One draw: the counter advances by one, as in ``sample``.  Asynchronous."""
        from . import _abi_sac
        from .policy import GaussianActor, MlpCritic
        torch = _torch()
        dev = self.venv.device

        def elsewhere(d):
            return d.type != dev.type or (None not in (d.index, dev.index) and d.index != dev.index)

        if not isinstance(log_alpha, torch.Tensor):
            raise ValueError("sample_sac: log_alpha must be a torch tensor on the buffer's device (it is read there)")
        if elsewhere(log_alpha.device):
            raise ValueError("sample_sac: log_alpha is on %s, the buffer on %s" % (log_alpha.device, dev))
        if log_alpha.dtype != torch.float32:
            raise ValueError("sample_sac: log_alpha must be float32, not %s" % log_alpha.dtype)
        if log_alpha.dim() > 1 or log_alpha.numel() != 1:
            raise ValueError("sample_sac: log_alpha must be a 0-d or 1-element tensor, not %s" % list(log_alpha.shape))
        if not isinstance(policy, GaussianActor):
            raise ValueError("sample_sac: the policy must be a GaussianActor (the 12-row head), not %s"
                             % type(policy).__name__)
        for net, name in ((critic1, "critic1"), (critic2, "critic2")):
            if not isinstance(net, MlpCritic):
                raise ValueError("sample_sac: the %s must be an MlpCritic, not %s" % (name, type(net).__name__))
        for net, name in ((policy, "policy"), (critic1, "critic1"), (critic2, "critic2")):
            if getattr(net, "blob", None) is None:
                raise ValueError("sample_sac: the %s must be on the device" % name)
            if elsewhere(net.device):
                raise ValueError("sample_sac: the %s is on %s, the buffer on %s" % (name, net.device, dev))
        gamma = float(gamma)
        if not np.isfinite(gamma):
            raise ValueError("sample_sac: gamma must be finite")
        B, out, hb = self._batch(batch_size, return_index)
        out["target"] = torch.empty(B, dtype=torch.float32, device=dev)
        if return_next:
            out["q1_next"] = torch.empty(B, dtype=torch.float32, device=dev)
            out["q2_next"] = torch.empty(B, dtype=torch.float32, device=dev)
            out["next_action"] = torch.empty((B, 6), dtype=torch.float32, device=dev)
            out["next_logp"] = torch.empty(B, dtype=torch.float32, device=dev)
        td = _abi_sac.CtrHerSac()
        td.actor, td.critic1, td.critic2 = (ctypes.pointer(policy._struct), ctypes.pointer(critic1._struct),
                                            ctypes.pointer(critic2._struct))
        td.log_alpha, td.gamma = log_alpha.data_ptr(), gamma
        td.target, td.q1_next, td.q2_next = _abi.ptr(out["target"]), _abi.ptr(out.get("q1_next")), _abi.ptr(out.get("q2_next"))
        td.next_action, td.next_logp = _abi.ptr(out.get("next_action")), _abi.ptr(out.get("next_logp"))
        rc = self.lib.ctr_her_sample_sac(self._h, B, self._draw_seed(seed), self._counter, hb, td,
                                         _abi.stream_ptr(stream, self.venv.device.index))
        _abi.check(rc, "ctr_her_sample_sac")
        self._log_alpha = log_alpha        # stays referenced until the next draw: the launch reads it
        self._counter += 1
        return out
