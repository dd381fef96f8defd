"""The three fused target samplers (HerReplayBuffer.sample_td, sample_td3, sample_sac) on the stores and
keys of a training run, in one loop over the three: stores of more than one scan tile, with a partial
and an empty tile (the multi-tile cases of tests/test_gpu_her_sampler.py reach ctr_her_sample only, and
each fused entry point sizes the scan's grid itself); a draw seed with a high word and the buffer's own
counter across 2^32; and a store that grows and wraps between draws.

The batch is held to ``her_oracle.sample_rows`` (synthetic stores) or to ``sample`` on a second,
identically driven buffer (env-driven stores); the networks' outputs to the stand-alone launches and the
target to the float32 restatement, bit for bit, by the checks of tests/test_gpu_td_target.py,
test_gpu_td3_target.py and test_gpu_sac_target.py, whose network builders are shared too.

The synthetic stores' observations reach a few hundred, so every network's first layer is multiplied by
FIRST_GAIN = 2^-8, found with the numpy restatements (``GaussianActor.emulate`` and its kin) on the
restatement's rows: at that gain SAC's log standard deviations lie above, inside and below the clip,
the actions are saturated on some rows and not on others, and TD3's noise reaches its clip on some.
What the inputs cover is asserted here on the stand-alone launches, never on the kernels under test."""
import numpy as np
import pytest

import test_gpu_her_sampler as HS
import test_gpu_sac_target as ST
import test_gpu_td3_target as T3
import test_gpu_td_target as TD

pytestmark = pytest.mark.gpu

KINDS = ("td", "td3", "sac")
GAMMA = ST.GAMMA
DRAW_SEED, COUNTER = ST.DRAW_SEED, ST.COUNTER
FIRST_GAIN = 2.0 ** -8
BATCH_KEYS = ST.BATCH_KEYS
assert TD.GAMMA == T3.GAMMA == GAMMA and TD.DRAW_SEED == T3.DRAW_SEED == DRAW_SEED and T3.COUNTER == COUNTER


class Networks(object):
    """The networks of the three draws: ``test_gpu_sac_target.Nets``' policy and critics (the same
    generator, in the same order), behind them TD3's six-row policy, every first layer times ``first_gain``.
    ``reference`` is the policy keyed by ``draw_seed`` for the stand-alone launch.  ``critic2`` serves SAC and
    ``critic2_td3`` TD3: each is balanced on its own actions (``balance``).  ``device`` None: on the host,
    for the numpy restatements."""

    def __init__(self, device, obs_dim, draw_seed=DRAW_SEED, first_gain=1.0, seed=21):
        from ctr_reach_amd.policy import GaussianActor, MlpActor, MlpCritic
        rng = np.random.default_rng(seed)

        def scaled(layers):
            return [(layers[0][0] * np.float32(first_gain), layers[0][1])] + layers[1:]

        self.device, self.draw_seed = device, draw_seed
        self.policy_layers = scaled(ST._policy_layers(rng, obs_dim, (64, 96)))
        self.policy = GaussianActor(self.policy_layers, ST.SCALE, device=device, seed=999)
        self.reference = GaussianActor(self.policy_layers, ST.SCALE, device=device, seed=draw_seed)
        self.critic1 = MlpCritic(scaled(ST._layers(rng, [obs_dim + 12, 96, 64, 1])), device=device)
        self.layers2 = scaled(ST._layers(rng, [obs_dim + 12, 32, 1]))
        self.critic2 = self.critic2_td3 = MlpCritic(self.layers2, device=device)
        self.actor_layers = scaled(T3._layers(rng, [obs_dim + 6, 64, 96, 6], out_gain=8.0))
        self.actor = MlpActor(self.actor_layers, ST.SCALE, device=device)
        self.unit_actor = MlpActor(self.actor_layers, np.ones(6), device=device)

    def _shifted(self, shift):
        from ctr_reach_amd.policy import MlpCritic
        W, b = self.layers2[-1]
        return MlpCritic(self.layers2[:-1] + [(W, b - np.float32(shift))], device=self.device)

    def balance(self, rows, counter):
        """Critic 2's output bias moved so that q2 - q1 has median 0 on the reference rows ``rows``, under
        SAC's action (``critic2``) and under TD3's smoothed action (``critic2_td3``), both from stand-alone
        launches and the numpy restatement of the smoothing: min(q1, q2) then picks both critics."""
        import torch
        x = rows["next_obs"]
        unit = self.reference.sample(x, counter=counter, row_base=0)["unit"]
        smoothed = torch.from_numpy(smoothed_reference(self, rows, counter).astype(np.float32)).to(x.device)
        shifts = [np.median((self.critic2(x, a) - self.critic1(x, a)).cpu().numpy()) for a in (unit, smoothed)]
        self.critic2, self.critic2_td3 = self._shifted(shifts[0]), self._shifted(shifts[1])
        return self


def smoothed_reference(nets, rows, counter):
    """TD3's smoothed action of the reference rows in float64: the stand-alone unit-scale actor's a' under
    ``TargetSmoothing.emulate`` keyed by the full draw seed and counter."""
    import torch
    from ctr_reach_amd.policy import TargetSmoothing
    a1 = nets.unit_actor(rows["next_obs"])
    torch.cuda.synchronize()
    a1 = a1.cpu().numpy()
    return TargetSmoothing(T3.SIGMA, T3.CLIP).emulate(nets.draw_seed, counter, np.arange(len(a1)), a1)


def _device_rows(ref, cuda):
    """The restatement's batch as the draws return theirs."""
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(ref[k])).to(cuda) for k in BATCH_KEYS}


def _sac_reference(rows, nets, counter):
    """``test_gpu_sac_target._reference`` on reference rows already drawn: the stand-alone ctr_gauss_act keyed
    (the draw seed, counter, row_base 0) on their next_obs and the two ctr_critic calls on that action."""
    import torch
    st = nets.reference.sample(rows["next_obs"], counter=counter, row_base=0, logits=True)
    ref = dict(rows, unit=st["unit"], logp=st["logp"], logits=st["logits"])
    ref["q1"], ref["q2"] = nets.critic1(rows["next_obs"], st["unit"]), nets.critic2(rows["next_obs"], st["unit"])
    torch.cuda.synchronize()
    return ref


def _draw(her, kind, B, nets, log_alpha=None, seed=DRAW_SEED):
    """One fused draw at the counter the buffer holds."""
    import torch
    counter = her._counter
    kw = dict(seed=seed, return_index=True, return_next=True)
    if kind == "td":
        out = her.sample_td(B, nets.actor, nets.critic1, GAMMA, **kw)
    elif kind == "td3":
        out = her.sample_td3(B, nets.actor, nets.critic1, nets.critic2_td3, GAMMA, sigma=T3.SIGMA, clip=T3.CLIP, **kw)
    else:
        out = her.sample_sac(B, nets.policy, nets.critic1, nets.critic2, GAMMA, log_alpha, **kw)
    assert her._counter == counter + 1
    torch.cuda.synchronize()
    return out


def _check_noise(out, nets, rows, counter):
    """``test_gpu_td3_target._check_noise`` with the draw's own seed: next_action within 4x the measured
    error of the float64 restatement, inside the box, moved by the clip at the most.  -> (a', moved)."""
    want = smoothed_reference(nets, rows, counter)
    got = out["next_action"].cpu().numpy()
    err = np.abs(got.astype(np.float64) - want).max()
    print("B = %d: max |next_action - emulate| = %.3e" % (len(got), err))
    assert err <= 4 * T3.SMOOTH_ERR_MEASURED, err
    assert (np.abs(got) <= 1).all()
    a1 = nets.unit_actor(rows["next_obs"]).cpu().numpy()
    moved = got.astype(np.float64) - a1.astype(np.float64)
    assert (np.abs(moved) <= T3.CLIP + 2.0 ** -24).all(), np.abs(moved).max()
    return a1, moved


def _check_draw(kind, out, rows, nets, counter, log_alpha=None):
    """One draw against its reference rows: the batch bit for bit, then the kind's own checks."""
    import torch
    for k in BATCH_KEYS:
        assert out[k].dtype == rows[k].dtype and torch.equal(out[k], rows[k]), (kind, k, "counter", counter)
    B = rows["obs"].shape[0]
    if kind == "td":
        assert set(out) == set(BATCH_KEYS) | {"target", "q_next", "next_action"}
        assert out["target"].shape == out["q_next"].shape == (B,) and out["next_action"].shape == (B, 6)
        TD._check_against_stand_alone(out, nets.unit_actor, nets.critic1)
    elif kind == "td3":
        assert set(out) == set(BATCH_KEYS) | {"target", "q1_next", "q2_next", "next_action"}
        assert out["target"].shape == out["q1_next"].shape == out["q2_next"].shape == (B,) and out["next_action"].shape == (B, 6)
        T3._check_against_stand_alone(out, nets.critic1, nets.critic2_td3)
        if nets.draw_seed == T3.DRAW_SEED:
            T3._check_noise(out, nets.unit_actor, counter=counter)
        _check_noise(out, nets, rows, counter)
    else:
        ST._check(out, _sac_reference(rows, nets, counter), log_alpha, nets.critic1, nets.critic2)


# --- B1: more than one scan tile -----------------------------------------------------------------------------

def _store_two_tiles(cuda, store_seed=None):
    """E = 1 200 on a 13-float observation: tile 0 full, tile 1 of 176 slots."""
    her = HS._buffer(cuda, 300, 4, 6, "future", 4, store_seed=store_seed)
    assert her.obs_dim == 13
    return her, HS._fill(her, HS._random_lens(1200, 6, seed=11), seed=1)


def _store_four_tiles(cuda):
    """E = 3 084 on a 14-float observation, tile 1 emptied: four tiles, the last of 12 slots."""
    her = HS._buffer(cuda, 771, 4, 5, "episode", 1, systems=(0, 1, 2, 3))
    assert her.obs_dim == 14
    lens = HS._empty(HS._random_lens(3084, 5, seed=12), HS.TILE, 2 * HS.TILE)
    assert (lens[HS.TILE:2 * HS.TILE] <= 0).all() and (lens[3 * HS.TILE:] > 0).any() and len(lens) - 3 * HS.TILE == 12
    return her, HS._fill(her, lens, seed=2)


def _assert_td3_coverage(nets, rows, counter):
    """On the stand-alone launches: both critics give the minimum, the noise reaches its clip on some
    elements and not on others, the smoothed action sits on the box on some."""
    import torch
    a1 = nets.unit_actor(rows["next_obs"]).cpu().numpy()
    smoothed = smoothed_reference(nets, rows, counter)
    moved = smoothed - a1.astype(np.float64)
    a2 = torch.from_numpy(smoothed.astype(np.float32)).to(rows["next_obs"].device)
    q1, q2 = (c(rows["next_obs"], a2).cpu().numpy() for c in (nets.critic1, nets.critic2_td3))
    far = np.abs(a1) <= 1 - T3.CLIP - 1e-3                 # a' + e cannot reach the box
    clipped = far & (np.abs(moved) >= T3.CLIP - 1e-6)
    print("td3: q2 < q1 on %.3f; noise at its clip on %d elements of %d far from the box; |a''| = 1 on %.3f"
          % ((q2 < q1).mean(), clipped.sum(), far.sum(), (np.abs(smoothed) == 1).mean()))
    assert 0.25 <= (q2 < q1).mean() <= 0.75, (q2 < q1).mean()
    assert clipped.any() and (far & (np.abs(moved) < T3.CLIP - 1e-6) & (moved != 0)).any()
    assert (np.abs(smoothed) == 1).any() and len(np.unique(q1)) > 100 and len(np.unique(q2)) > 100


@pytest.mark.parametrize("make", [_store_two_tiles, _store_four_tiles], ids=["two_tiles", "four_tiles_one_empty"])
def test_more_than_one_scan_tile_against_the_restatement(cuda, oracle_mod, make):
    import her_oracle as H
    B = 2048
    her, store = make(cuda)
    ref = H.sample_rows(store, B, DRAW_SEED, COUNTER)
    HS._coverage(ref, store)                               # every non-empty tile is drawn from, on the restatement's rows
    rows = _device_rows(ref, cuda)
    nets = Networks(cuda, her.obs_dim, first_gain=FIRST_GAIN).balance(rows, COUNTER)
    # what the inputs cover, on the stand-alone launches: test_gpu_sac_target's own assertions, and TD3's
    ST.test_the_inputs_cover_the_head_the_minimum_and_the_flags((None, None, None, {300: _sac_reference(rows, nets, COUNTER)}))
    _assert_td3_coverage(nets, rows, COUNTER)
    log_alpha = ST._log_alpha(cuda, ST.LOG_ALPHAS[1])
    for kind in KINDS:
        her._counter = COUNTER
        out = _draw(her, kind, B, nets, log_alpha)
        HS._assert_scratch_and_store(her, store)
        _check_draw(kind, out, rows, nets, COUNTER, ST.LOG_ALPHAS[1])
        live = ref["done"] == 0
        assert live.any() and not np.array_equal(out["target"].cpu().numpy()[live], ref["reward"][live])


# --- B2: the key's high words, and the counter across 2^32 -----------------------------------------------------

STORE_SEED = (9 << 32) | 11
FIRST_COUNTER = 2 ** 32 - 2
SIZES = (300, 300, 257, 300)                             # 257: a block and one row


def test_the_key_s_high_words_and_the_counter_across_2_to_the_32(cuda, oracle_mod):
    import her_oracle as H
    import torch
    from ctr_reach_amd.policy import GaussianActor, TargetSmoothing
    her, store = _store_two_tiles(cuda, store_seed=STORE_SEED)
    draw_seed = her._draw_seed(None)
    assert her.seed == STORE_SEED and draw_seed >> 32 and draw_seed & 0xFFFFFFFF and draw_seed == STORE_SEED ^ 0x5DEECE66D
    nets = Networks(cuda, her.obs_dim, draw_seed=draw_seed, first_gain=FIRST_GAIN)
    low_seed = GaussianActor(nets.policy_layers, ST.SCALE, device=cuda, seed=draw_seed & 0xFFFFFFFF)
    counters = [FIRST_COUNTER + d for d in range(len(SIZES))]
    assert counters[1] == 2 ** 32 - 1 and counters[2] == 2 ** 32
    refs = {c: H.sample_rows(store, B, draw_seed, c) for c, B in zip(counters, SIZES)}
    # the high words matter to the restatement: without them it draws other rows
    for c, B in zip(counters, SIZES):
        assert (store["len"][refs[c]["index"][:, 0]] > 0).all()
        assert not np.array_equal(H.sample_rows(store, B, draw_seed & 0xFFFFFFFF, c)["index"], refs[c]["index"])
        if c >> 32:
            assert not np.array_equal(H.sample_rows(store, B, draw_seed, c & 0xFFFFFFFF)["index"], refs[c]["index"])
    log_alpha = ST._log_alpha(cuda, ST.LOG_ALPHAS[1])
    smoothing = TargetSmoothing(T3.SIGMA, T3.CLIP)
    for kind in KINDS:
        her._counter = FIRST_COUNTER                       # once: the four draws below advance it themselves
        for c, B in zip(counters, SIZES):
            assert her._counter == c
            out = _draw(her, kind, B, nets, log_alpha, seed=None)
            rows = _device_rows(refs[c], cuda)
            HS._assert_scratch_and_store(her, store)
            _check_draw(kind, out, rows, nets, c, ST.LOG_ALPHAS[1])
            # the noise with a low word in place of the seed, or of the counter past 2^32, is another noise
            got = out["next_action"]
            if kind == "sac":
                assert not torch.equal(low_seed.sample(rows["next_obs"], counter=c)["unit"], got)
                if c >> 32:
                    assert not torch.equal(nets.reference.sample(rows["next_obs"], counter=c & 0xFFFFFFFF)["unit"], got)
            elif kind == "td3":
                a1 = nets.unit_actor(rows["next_obs"]).cpu().numpy()
                index = np.arange(B)
                wrong = [smoothing.emulate(draw_seed & 0xFFFFFFFF, c, index, a1)]
                if c >> 32:
                    wrong.append(smoothing.emulate(draw_seed, c & 0xFFFFFFFF, index, a1))
                for other in wrong:
                    assert np.abs(got.cpu().numpy() - other).max() > 1000 * T3.SMOOTH_ERR_MEASURED
        assert her._counter == FIRST_COUNTER + len(SIZES) == 2 ** 32 + 2


# --- B3: a store that grows and wraps between draws --------------------------------------------------------------

ROUNDS = (20, 7, 7)                                      # steps of collect; the first is the modules' ``_store``'s own
ROUND_LOG_ALPHAS = (0.0, ST.LOG_ALPHAS[1], -1.25)        # SAC's temperature moves between the rounds


def test_a_store_that_grows_and_wraps_between_draws(cuda):
    import torch
    from ctr_reach_amd.policy import ExploreNoise, MlpActor
    systems = (0, 1, 2, 3)
    a, b = ST._store(cuda, systems), ST._store(cuda, systems)      # (round 1: 20 steps of collect)
    assert a.obs_dim == 14 and a.slots == 3 and a.t_max == 5
    behaviour = MlpActor(ST._layers(np.random.default_rng(2), [a.obs_dim + 6, 32, 6], out_gain=8.0), a.venv.action_space.high,
                         device=cuda)
    noise = ExploreNoise(0.2, random_eps=0.3, seed=1)
    nets = Networks(cuda, a.obs_dim)
    b._counter = 0
    nets.balance(b.sample(300, seed=DRAW_SEED, return_index=True), 0)
    log_alpha = ST._log_alpha(cuda, 0.0)
    assert a._counter == 0
    before = None
    for r, steps in enumerate(ROUNDS):
        if r:
            for her in (a, b):
                her.venv.collect(behaviour, steps, noise)
        torch.cuda.synchronize()
        stamp = dict(epoch=b.epoch.cpu().numpy().copy(), len=b.len.cpu().numpy().copy(), state=b.state.cpu().numpy().copy())
        for name in ("state", "step_rows", "len", "epoch", "cur_t", "cur_epoch"):
            x, y = getattr(a, name), getattr(b, name)
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (r, name)
        log_alpha.fill_(ROUND_LOG_ALPHAS[r])
        drawn = None
        for kind in KINDS:
            for B in (1, 65, 300):
                counter = b._counter = a._counter          # the counter the first buffer keeps; the second follows it
                rows = b.sample(B, seed=DRAW_SEED, return_index=True)
                out = _draw(a, kind, B, nets, log_alpha)
                _check_draw(kind, out, rows, nets, counter, ROUND_LOG_ALPHAS[r])
                if B == 300:
                    drawn = rows["index"].cpu().numpy()
        assert a._counter == 9 * (r + 1)
        # on the reference side: the rounds differ
        assert (drawn[:, 0] >= 0).all() and (stamp["len"][drawn[:, 0]] > 0).all()
        if before is not None:
            old, old_drawn = before
            overwritten = np.flatnonzero((stamp["epoch"] != old["epoch"]) & (old["len"] > 0) & (stamp["len"] > 0))
            assert len(overwritten) > 0 and stamp["state"].tobytes() != old["state"].tobytes()
            assert np.isin(drawn[:, 0], overwritten).any()             # rows of episodes stored since the last round are drawn
            assert not np.array_equal(drawn, old_drawn)
        before = (stamp, drawn)
