"""ctr_her_sample (k_her_scan_tiles, k_her_scan_tops, k_her_sample) on synthetic stores against
her_oracle.sample_rows, an independent numpy restatement of ReplayBuffer.sample that predicts the
drawn (slot, t, j) itself, and her_oracle.scan_reference for the sampler's scratch (ctr_her_t.cdf).

The sampler reads only the store, so each case writes a seeded random store straight into the
HerReplayBuffer's tensors (no env is reset or stepped) at the smallest size at which its path exists:
more than one scan tile (E > 1024 slots), a partial last tile, empty tiles, draws at tile edges, a
second pass of k_her_scan_tops (more than 256 tiles), batches whose last block is ragged, relabel
counts other than 4, key words above 2^32.

Bars: every output array, index included, bit-equal to the restatement; cdf equal to the scan
reference; every element past row B of over-allocated outputs untouched; the store byte-equal
after the call.  No tolerance anywhere.  Each case first asserts, on the restatement's output
alone, that its draws reach what it is about (_coverage), so none passes vacuously.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GTP = {"inc_tol_obs": False, "final_tol": 0.001, "initial_tol": 0.05, "N_ts": 1000, "function": "constant",
       "set_tol": 0}
TILE = 1024                   # CTR_HER_SCAN_TILE
SIGMA = 0.02                  # spread of the synthetic achieved / desired goals, metres
SENTINEL = 0x7FC5A5A5         # a quiet-NaN bit pattern no kernel output can equal
ROW_KEYS = ("index", "obs", "action", "reward", "next_obs", "done")


def _buffer(cuda, n, slots, t_max, strategy, k, systems=(0,), env_base=0, store_seed=None):
    from ctr_reach_amd import CtrReachVecEnv
    env = CtrReachVecEnv(n, device=cuda, seed=5, env_base=env_base, autoreset=False, record_info=False,
                         max_steps_per_episode=t_max, goal_tolerance_parameters=GTP, select_systems=list(systems))
    return env.enable_her(slots=slots, n_sampled_goal=k, goal_selection_strategy=strategy, seed=store_seed)


def _distinct(rng, count):
    """count finite float32 values, every one distinct (integers below 2^24 over 256, shuffled)."""
    assert count < 1 << 24
    return (rng.permutation(count).astype(np.int32) - count // 2).astype(np.float32) * np.float32(1.0 / 256)


def _fill(her, lens, seed=0):
    """Writes a random store with episode lengths ``lens`` into the buffer's tensors; returns it
    as her_oracle.sample_rows takes it.  The padding of the rows (floats 13 / 14 .. 15 and 22, 23
    of a state row, float 7 of a step row) is random too: none of it may reach a batch."""
    import torch
    import her_oracle as H
    rng = np.random.default_rng(seed)
    S, T, n = her.slots, her.t_max, her.venv.num_envs
    E = n * S
    state = np.empty((S, T + 1, n, 24), dtype=np.float32)
    state[..., :16] = _distinct(rng, S * (T + 1) * n * 16).reshape(S, T + 1, n, 16)
    state.view(np.float64)[..., 8:] = rng.normal(0.0, SIGMA, (S, T + 1, n, 4))     # achieved goals (+ padding)
    step = _distinct(rng, S * T * n * 8).reshape(S, T, n, 8)
    dg = rng.normal(0.0, SIGMA, (E, 3))
    # two points of that cloud are a median 2.18 sigma apart: relabelled rewards come out about even
    tol = 2.18 * SIGMA * rng.uniform(0.8, 1.2, E)
    epoch = rng.integers(-2 ** 31, 2 ** 31, E).astype(np.int32)
    lens = np.asarray(lens, dtype=np.int32)
    assert lens.shape == (E,) and lens.max() <= T
    arrays = dict(state=state, step_rows=step, dg=dg, tol=tol, len=lens, epoch=epoch)
    for name in H.STORE_BUFFERS:
        getattr(her, name).copy_(torch.from_numpy(arrays[name]))
    store = H.store_copy(her)
    for name in H.STORE_BUFFERS:
        assert np.array_equal(store[name].view(np.uint8), arrays[name].view(np.uint8)), name
    return store


def _random_lens(E, t_max, seed):
    return np.random.default_rng(seed).integers(-1, t_max + 1, E).astype(np.int32)     # {-1, 0, 1 .. t_max}


def _empty(lens, a, b, seed=1):
    """Slots a .. b - 1 hold nothing: dropped (0) or still recording (-1)."""
    lens[a:b] = np.random.default_rng(seed).integers(-1, 1, b - a)
    return lens


def _coverage(ref, store, must_draw=(), relabel_rewards=True):
    """The conditions under which a case tests what it claims, on the restatement's rows alone."""
    import her_oracle as H
    k, lens = store["k"], store["len"]
    slot, t, j = ref["index"].T
    assert (slot >= 0).all() and (lens[slot] > 0).all()                    # no drawn slot is empty
    rows = H.rows_per_episode(lens, k, store["strategy"])
    np.testing.assert_array_equal(np.unique(slot // TILE), np.unique(np.nonzero(rows)[0] // TILE))   # every non-empty tile
    for s in must_draw:
        assert (slot == s).any(), s
    assert (j == 0).any() and (j == k).any()
    assert (t == 0).any() and (t == lens[slot] - 1).any()
    rel = ref["reward"][j > 0]
    assert np.isin(rel, (0.0, -1.0)).all()
    if k and relabel_rewards:
        assert 0.1 <= (rel == 0.0).mean() <= 0.9                           # both rewards, each in >= 10 %


def _sample_abi(her, B, seed, counter, guard=64):
    """ctr_her_sample into outputs of B + guard rows pre-filled with SENTINEL; returns the raw
    int32 words of every output."""
    import torch
    from ctr_reach_amd import _abi
    d = her.obs_dim + 6
    dev = her.venv.device
    widths = dict(index=3, obs=d, action=6, reward=1, next_obs=d, done=1)
    bufs = {key: torch.full((B + guard, w), SENTINEL, dtype=torch.int32, device=dev) for key, w in widths.items()}
    hb = _abi.CtrHerBatch()
    for key in widths:
        setattr(hb, key, _abi.ptr(bufs[key]))
    rc = her.lib.ctr_her_sample(her._h, B, seed, counter, hb, _abi.stream_ptr(None, dev.index))
    _abi.check(rc, "ctr_her_sample")
    torch.cuda.synchronize()
    return {key: v.cpu().numpy() for key, v in bufs.items()}


def _assert_rows(got, ref):
    for key in ROW_KEYS:
        np.testing.assert_array_equal(got[key], ref[key], err_msg=key)


def _assert_scratch_and_store(her, store):
    import her_oracle as H
    E = store["n"] * store["slots"]
    tiles = (E + TILE - 1) // TILE
    local, offsets, total = H.scan_reference(store["len"], store["k"], store["strategy"])
    cdf = her.cdf.cpu().numpy()
    assert len(cdf) == E + tiles + 1                                       # CTR_HER_CDF_LEN(E)
    np.testing.assert_array_equal(cdf[:E], local)
    np.testing.assert_array_equal(cdf[E:E + tiles], offsets)
    assert cdf[E + tiles] == total
    after = H.store_copy(her)
    for name in H.STORE_BUFFERS:
        assert np.array_equal(after[name].view(np.uint8), store[name].view(np.uint8)), name


def _check(her, store, B=8192, seed=None, **coverage):
    """One her.sample(B) against the restatement: rows, scratch, store."""
    import her_oracle as H
    counter = her._counter
    s = (her.seed ^ 0x5DEECE66D) if seed is None else seed
    ref = H.sample_rows(store, B, s, counter)
    _coverage(ref, store, **coverage)
    b = her.sample(B, seed=seed, return_index=True)
    got = {key: b[key].cpu().numpy() for key in ROW_KEYS}
    assert her._counter == counter + 1
    _assert_rows(got, ref)
    _assert_scratch_and_store(her, store)
    return ref, got


def test_two_tiles_second_partial(cuda, oracle_mod):
    """E = 1200: tile 0 full, tile 1 of 176 slots (the clamp of the slot search at E)."""
    her = _buffer(cuda, 300, 4, 6, "future", 4)
    store = _fill(her, _random_lens(1200, 6, seed=11), seed=1)
    assert her.obs_dim == 13
    _check(her, store)


@pytest.mark.parametrize("empty_tile", [1, 3, 0])
def test_empty_tiles(cuda, oracle_mod, empty_tile):
    """E = 3084, four tiles, the last of 12 slots; one whole tile holds nothing, so its offset
    equals the next tile's (or, for the last tile, the stored-row count)."""
    her = _buffer(cuda, 771, 4, 5, "episode", 1, systems=(0, 1, 2, 3))
    assert her.obs_dim == 14
    lens = _empty(_random_lens(3084, 5, seed=12), empty_tile * TILE, min((empty_tile + 1) * TILE, 3084))
    store = _fill(her, lens, seed=2)
    _check(her, store)


def test_tile_edges(cuda, oracle_mod):
    """E = 3084 with rows only in the first and last slots of tiles 0 and 1 and in slot E - 1
    (tile 2 is empty), of lengths 1 and t_max: every draw sits at a tile edge, and the draws equal
    to a tile's offset (the first row of slots 1024 and E - 1) decide between two tiles."""
    E, T = 3084, 5
    her = _buffer(cuda, 771, 4, T, "episode", 1, systems=(0, 1, 2, 3))
    lens = _empty(np.zeros(E, dtype=np.int32), 0, E)
    edges = {0: T, 1023: 1, 1024: T, 2047: 1, E - 1: T}
    for s, L in edges.items():
        lens[s] = L
    store = _fill(her, lens, seed=3)
    ref, _ = _check(her, store, must_draw=tuple(edges))
    for s in (1024, E - 1):
        assert (ref["index"] == (s, 0, 0)).all(axis=1).any()


@pytest.mark.parametrize("k", [0, 7])
def test_relabel_counts_final(cuda, oracle_mod, k):
    """n_sampled_goal 0 (no relabelled row at all) and 7, strategy final, three slots per env:
    E = 3075, four tiles, the last of 3 slots."""
    her = _buffer(cuda, 1025, 3, 6, "final", k)
    store = _fill(her, _random_lens(3075, 6, seed=13), seed=4)
    ref, _ = _check(her, store)
    assert ((ref["index"][:, 2] > 0).sum() > 0) == (k > 0)


def _sparse_lens(E, nonempty, full):
    """Nothing stored but in the slots ``nonempty`` (one-step episodes) and ``full`` (two steps)."""
    lens = _empty(np.zeros(E, dtype=np.int32), 0, E)
    lens[list(nonempty)] = 1
    lens[list(full)] = 2
    return lens


def test_scan_tops_second_pass(cuda, oracle_mod):
    """E = 262152 = 257 tiles, the last of 8 slots: k_her_scan_tops takes a second pass, and the
    offset of tile 256 is the carry of the first.  Thirty sparse slots in tiles 0 .. 255 (tiles 0 and
    255 among them) against the eight full ones behind the carry."""
    E = 32769 * 8
    her = _buffer(cuda, 32769, 8, 2, "episode", 4)
    rng = np.random.default_rng(14)
    sparse = np.concatenate(([5, 255 * TILE + 1023], rng.choice(256 * TILE, 28, replace=False)))
    store = _fill(her, _sparse_lens(E, sparse, range(E - 8, E)), seed=5)
    ref, _ = _check(her, store)
    assert (ref["index"][:, 0] >= 256 * TILE).mean() >= 0.25
    assert (ref["index"][:, 0] < 256 * TILE).mean() >= 0.25


def test_scan_tops_carry_future(cuda, oracle_mod):
    """The 257-tile store once more under strategy future with four one-row episodes before the
    carry.  With t_max = 2 a future relabel can only pick the next observation's own goal, so
    every relabelled reward is 0 here: that one coverage condition cannot hold in this case and
    test_scan_tops_second_pass carries it."""
    E = 32769 * 8
    her = _buffer(cuda, 32769, 8, 2, "future", 4)
    store = _fill(her, _sparse_lens(E, [0, 77 * TILE + 500, 200 * TILE, 255 * TILE + 1023], range(E - 8, E)), seed=6)
    ref, _ = _check(her, store, relabel_rewards=False)
    assert (ref["index"][:, 0] >= 256 * TILE).mean() >= 0.25
    assert (ref["reward"][ref["index"][:, 2] > 0] == 0.0).all()


def test_exactly_256_tiles(cuda, oracle_mod):
    """E = 262144, the headline workload's own tile count: one full pass of k_her_scan_tops."""
    E = 32768 * 8
    her = _buffer(cuda, 32768, 8, 2, "episode", 4)
    rng = np.random.default_rng(15)
    sparse = np.concatenate(([0, 255 * TILE], rng.choice(E - 8, 28, replace=False)))
    store = _fill(her, _sparse_lens(E, sparse, range(E - 8, E)), seed=7)
    ref, _ = _check(her, store)
    assert (ref["index"][:, 0] >= 255 * TILE).mean() >= 0.25


@pytest.mark.parametrize("systems", [(0,), (0, 1, 2, 3)], ids=["d19", "d20"])
def test_ragged_batches_write_nothing_past_row_B(cuda, oracle_mod, systems):
    """Batch sizes whose last block's float count is no multiple of 4 (the scalar tail of
    her_flush: obs / next_obs rows of 19 floats, action rows of 6), into outputs with 64 spare rows
    of sentinel words: rows below B equal the restatement, nothing from row B on is written."""
    import her_oracle as H
    her = _buffer(cuda, 300, 4, 6, "future", 4, systems=systems)
    d = her.obs_dim + 6
    assert d == 19 + (len(systems) > 1)
    store = _fill(her, _random_lens(1200, 6, seed=16), seed=8)
    seed = 0x1234
    for counter, B in enumerate((1, 3, 257, 1021)):
        last = B % 256                                   # rows of the last block
        assert (last * 6) % 4 != 0 and ((last * d) % 4 != 0) == (d == 19)
        ref = H.sample_rows(store, B, seed, counter)
        assert (store["len"][ref["index"][:, 0]] > 0).all()
        raw = _sample_abi(her, B, seed, counter)
        for key in ROW_KEYS:
            rows = raw[key][:B] if key == "index" else raw[key][:B].view(np.float32)
            np.testing.assert_array_equal(rows.reshape(ref[key].shape), ref[key], err_msg="%s, B=%d" % (key, B))
            assert (raw[key][B:] == SENTINEL).all(), "%s written past row B=%d" % (key, B)
        _assert_scratch_and_store(her, store)


def test_high_key_words(cuda, oracle_mod):
    """Sample counter, sample seed and store seed with nonzero high words, and global env ids on
    both sides of 2^32 (env_base = 2^32 - 150, 300 envs)."""
    import her_oracle as H
    base = 2 ** 32 - 150
    her = _buffer(cuda, 300, 4, 6, "future", 4, env_base=base, store_seed=0x9E3779B97F4A7C15)
    assert her._h.env_base == base and her.venv.env_base == base      # the constructor takes the base as it is
    store = _fill(her, _random_lens(1200, 6, seed=17), seed=9)
    seed, counter = 0xDEADBEEF12345678, 2 ** 32 + 3
    her._counter = counter
    ref, _ = _check(her, store, seed=seed)
    env, rel = ref["index"][:, 0] // 4, ref["index"][:, 2] > 0
    assert (rel & (env < 150)).any() and (rel & (env >= 150)).any()
    # every high word matters to the restatement: another one gives another batch (the draws for
    # the counter and the sample seed, the relabelled goals for the store seed and the env ids)
    n = 512
    assert not np.array_equal(H.sample_rows(store, n, seed, 3)["index"], ref["index"][:n])
    assert not np.array_equal(H.sample_rows(store, n, seed & 0xFFFFFFFF, counter)["index"], ref["index"][:n])
    for other in (dict(store, seed=store["seed"] & 0xFFFFFFFF), dict(store, env_base=base + 2 ** 32)):
        alt = H.sample_rows(other, n, seed, counter)
        np.testing.assert_array_equal(alt["index"], ref["index"][:n])
        assert not np.array_equal(alt["obs"], ref["obs"][:n])


def test_same_key_same_batch(cuda, oracle_mod):
    her = _buffer(cuda, 300, 4, 6, "future", 4)
    _fill(her, _random_lens(1200, 6, seed=11), seed=1)
    batches = []
    for counter in (7, 7, 8):
        her._counter = counter
        b = her.sample(2048, seed=99, return_index=True)
        batches.append({key: b[key].cpu().numpy() for key in ROW_KEYS})
    for key in ROW_KEYS:
        assert batches[0][key].tobytes() == batches[1][key].tobytes(), key
    assert not np.array_equal(batches[0]["index"], batches[2]["index"])
