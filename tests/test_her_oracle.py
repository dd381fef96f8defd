"""CPU checks of the HER replay restatement (oracle/her_oracle.py) against the stable-baselines 2
HindsightExperienceReplayWrapper semantics it restates (row order, future-goal ranges, relabelled
reward / done, unchanged 'observation' part).  stable-baselines is absent: parity unpinned."""
import numpy as np
import pytest


def _episode(L, seed=0):
    rng = np.random.default_rng(seed)
    dg = rng.normal(size=3)
    obs = [dict(observation=rng.normal(size=13).astype(np.float32), achieved_goal=rng.normal(size=3) * 0.01,
                desired_goal=dg) for _ in range(L + 1)]
    return [(obs[t], rng.normal(size=6).astype(np.float32), -1.0, obs[t + 1], t == L - 1) for t in range(L)]


@pytest.mark.parametrize("strategy", ["future", "final", "episode"])
def test_store_episode_order_and_relabels(oracle_mod, strategy):
    import her_oracle as H
    L, k = 6, 4
    tr = _episode(L)
    rows = H.store_episode(tr, k, strategy, tol=0.02, seed=7, genv=3, epoch=2)
    n_rel = L - 1 if strategy == "future" else L
    assert len(rows) == L + k * n_rel
    # _store_episode order: the real transition, then its k relabels
    labels = [(r["t"], r["j"]) for r in rows]
    want = []
    for t in range(L):
        want.append((t, 0))
        if not (strategy == "future" and t == L - 1):
            want += [(t, j) for j in range(1, k + 1)]
    assert labels == want
    for r in rows:
        t = r["t"]
        obs_t, a, rew, obs_tp1, done = tr[t]
        np.testing.assert_array_equal(r["obs"][:13], obs_t["observation"])     # 'observation' kept
        np.testing.assert_array_equal(r["action"], a)
        if r["j"] == 0:
            assert r["reward"] == rew and r["done"] == float(done)
            np.testing.assert_array_equal(r["obs"][16:], np.float32(obs_t["desired_goal"]))
            continue
        assert r["done"] == 0.0
        goal = r["obs"][16:]
        np.testing.assert_array_equal(goal, r["next_obs"][16:])
        cands = {"future": range(t + 1, L), "final": [L - 1], "episode": range(L)}[strategy]
        matches = [s for s in cands if np.array_equal(np.float32(tr[s][0]["achieved_goal"]), goal)]
        assert matches, (t, r["j"])
        s = matches[0]
        want_r = -float(np.linalg.norm(obs_tp1["achieved_goal"] - tr[s][0]["achieved_goal"]) > 0.02)
        assert r["reward"] == want_r


def _store(n, slots, t_max, k, strategy, seed=0):
    rng = np.random.default_rng(seed)
    E = n * slots
    state = rng.normal(size=(slots, t_max + 1, n, 24)).astype(np.float32)
    state.view(np.float64)[..., 8:] = rng.normal(0.0, 0.02, (slots, t_max + 1, n, 4))
    return dict(state=state, step_rows=rng.normal(size=(slots, t_max, n, 8)).astype(np.float32),
                dg=rng.normal(0.0, 0.02, (E, 3)), tol=np.full(E, 0.04), epoch=rng.integers(-9, 9, E).astype(np.int32),
                len=rng.integers(-1, t_max + 1, E).astype(np.int32), n=n, slots=slots, t_max=t_max, k=k,
                strategy=strategy, obs_dim=13, env_base=2 ** 32 - 2, seed=(3 << 32) | 7)


@pytest.mark.parametrize("strategy,k", [("future", 4), ("final", 0), ("episode", 3)])
def test_sample_rows_draws_from_the_wrappers_buffer(oracle_mod, strategy, k):
    """sample_rows' row i is row idx of the buffer _store_episode fills when the stored episodes are
    added slot after slot, idx being the build's draw (stream 5) scaled to the buffer's length."""
    import her_oracle as H
    st = _store(5, 3, 4, k, strategy)
    ag = st["state"].view(np.float64)[..., 8:11]
    buf = []
    for slot in range(15):
        L = int(st["len"][slot])
        e, s = divmod(slot, 3)
        if L <= 0:
            continue
        obs = [dict(observation=st["state"][s, t, e, :13], achieved_goal=ag[s, t, e], desired_goal=st["dg"][slot])
               for t in range(L + 1)]
        tr = [(obs[t], st["step_rows"][s, t, e, :6], st["step_rows"][s, t, e, 6], obs[t + 1], t == L - 1)
              for t in range(L)]
        buf += [(slot, r) for r in H.store_episode(tr, k, strategy, st["tol"][slot], st["seed"], st["env_base"] + e,
                                                   int(st["epoch"][slot]))]
    assert len(buf) == H.rows_per_episode(st["len"], k, strategy).sum() > 12
    B, seed, counter = 6 * len(buf), (9 << 32) | 1, (1 << 32) | 5
    got = H.sample_rows(st, B, seed, counter)
    drawn = set()
    for i in range(B):
        c = oracle_mod.philox([0, 5, i, 1 ^ (5 << 24)], seed)
        idx = min(int(H.u53(c[0], c[1]) * len(buf)), len(buf) - 1)
        drawn.add(idx)
        slot, r = buf[idx]
        assert tuple(got["index"][i]) == (slot, r["t"], r["j"])
        for key in ("obs", "action", "next_obs"):
            np.testing.assert_array_equal(got[key][i], r[key])
        assert got["reward"][i] == np.float32(r["reward"]) and got["done"][i] == r["done"]
    assert len(drawn) > 0.9 * len(buf)
    assert not np.signbit(got["reward"][got["reward"] == 0]).any()       # a relabelled 0 is +0.0, as on the device
    empty = dict(st, len=np.minimum(st["len"], 0))
    none = H.sample_rows(empty, 4, seed, counter)
    assert (none["index"] == [-1, 0, 0]).all() and not none["obs"].any() and not none["reward"].any()


def test_scan_reference_restates_the_running_sum(oracle_mod):
    import her_oracle as H
    lens = np.random.default_rng(1).integers(-1, 7, 2500).astype(np.int32)
    lens[1024:2048] = 0                                   # an empty tile shares the next one's offset
    local, offsets, total = H.scan_reference(lens, 4, "future")
    rows = np.where(lens > 0, lens + 4 * (lens - 1), 0)
    np.testing.assert_array_equal(offsets[np.arange(2500) // 1024] + local, np.cumsum(rows))
    assert len(offsets) == 3 and offsets[0] == 0 and offsets[1] == offsets[2] and total == rows.sum()
    assert local.dtype == offsets.dtype == np.int64


def test_future_draws_cover_the_range(oracle_mod):
    import her_oracle as H
    L = 9
    for t in range(L - 1):
        sels = [H.sel_index(11, 5, e, t, j, L) for e in range(60) for j in range(1, 5)]
        assert min(sels) >= t + 1 and max(sels) <= L - 1
        assert set(sels) == set(range(t + 1, L))      # every later transition reachable
    # the next observation's own goal (sel = t + 1) earns reward 0
    tr = _episode(3)
    rows = H.store_episode(tr, 4, "future", tol=1e-9, seed=1, genv=0, epoch=0)
    r1 = [r for r in rows if r["t"] == 1 and r["j"] > 0]
    assert all(r["reward"] == 0.0 for r in r1)        # only sel = 2 = t + 1 is possible
