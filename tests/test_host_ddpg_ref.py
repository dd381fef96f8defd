"""The conditions of tests/test_gpu_ddpg_edges.py's inputs, which look at the references alone, checked
without a GPU: ``make_clear`` leaves a batch clear of the relu's kink within its caps on rows drawn
again and on passes, and with nothing to draw again it is ``make``; a gain of 100 saturates the policy
as far as the saturated cases need; and every integer case is exact in any order of summation: its
sums of absolute values stay below 2^24 units, and torch's float32 autograd on the CPU, which sums in
another order than float64's, gives float64's bits."""
import numpy as np
import pytest

import ddpg_ref as R

MAX_REDRAWN, MAX_PASSES = 0.15, 20


def _same(a, b):
    return np.array_equal(R.bits(a.numpy()), R.bits(b.numpy()))


@pytest.mark.parametrize("gain,case", [(1.0, c) for c in R.CLEAR_CASES] + [(R.GAIN, c) for c in R.SATURATED_CASES])
def test_make_clear_meets_its_conditions(gain, case):
    a_hidden, c_hidden, in_dim, B = case
    clear = R.case_clear(a_hidden, c_hidden, in_dim, B, gain)
    policy, critic, rows, actions, target = clear.made
    assert clear.ref64["kink"] >= 1e-5
    assert R.row_kinks(policy, critic, rows, actions).min() >= 1e-5
    assert clear.redrawn <= MAX_REDRAWN * B and clear.passes <= MAX_PASSES
    assert rows.shape == (B, in_dim) and actions.shape == (B, 6) and target.shape == (B,)
    # what was not drawn again is make's: the networks but the policy's output layer, the targets, and
    # all rows but as many as were drawn again at the most
    policy0, critic0, rows0, actions0, target0 = R.make(0, a_hidden, c_hidden, in_dim, B)
    assert _same(target, target0)
    for (W, b), (W0, b0) in zip(R.params(critic) + R.params(policy)[:-1], R.params(critic0) + R.params(policy0)[:-1]):
        assert _same(W, W0) and _same(b, b0)
    W, b = R.params(policy)[-1]
    W0, b0 = R.params(policy0)[-1]
    assert _same(W, W0 * gain) and _same(b, b0 * gain)
    moved = (rows != rows0).any(dim=1) | (actions != actions0).any(dim=1)
    assert int(moved.sum()) <= clear.redrawn
    if clear.redrawn:
        assert moved.any() and (R.row_kinks(policy, critic, rows0, actions0)[moved.numpy()] < 1e-5).all()
        assert (R.row_kinks(policy, critic, rows0, actions0)[~moved.numpy()] >= 1e-5).all()


def test_make_clear_with_nothing_to_draw_again_is_make():
    a_hidden, c_hidden, in_dim = R.SHAPES[0]
    seed, made, ref64, _ = R.case(a_hidden, c_hidden, in_dim, 70)           # (a seed that is clear as it stands)
    clear = R.make_clear(seed, a_hidden, c_hidden, in_dim, 70)
    assert clear.redrawn == 0 and clear.passes == 0
    for mine, theirs in zip(clear.made[:2], made[:2]):
        for (W, b), (W0, b0) in zip(R.params(mine), R.params(theirs)):
            assert _same(W, W0) and _same(b, b0)
    for mine, theirs in zip(clear.made[2:], made[2:]):
        assert _same(mine, theirs)
    assert clear.ref64["kink"] == ref64["kink"] and clear.ref64["critic_loss"] == ref64["critic_loss"]


def test_the_rows_drawn_again_do_not_come_from_the_batch_s_generator():
    """They are the first draws of a generator seeded 5000 + seed, in row order (a case of one pass)."""
    import torch
    a_hidden, c_hidden, in_dim, B = R.CLEAR_CASES[1]
    clear = R.case_clear(a_hidden, c_hidden, in_dim, B)
    rows0 = R.make(0, a_hidden, c_hidden, in_dim, B)[2]
    moved = np.flatnonzero((clear.made[2] != rows0).any(dim=1).numpy())
    assert clear.passes == 1 and len(moved) == clear.redrawn > 0
    g = torch.Generator().manual_seed(5000)
    assert _same(clear.made[2][moved], torch.rand((len(moved), in_dim), generator=g) * 2 - 1)
    assert _same(clear.made[3][moved], torch.rand((len(moved), 6), generator=g) * 2 - 1)


@pytest.mark.parametrize("case", R.SATURATED_CASES)
def test_a_gain_of_100_saturates_the_policy(case):
    a_hidden, c_hidden, in_dim, B = case
    clear = R.case_clear(a_hidden, c_hidden, in_dim, B, R.GAIN)
    pi = R.actions64(clear.made[0], clear.made[2])
    assert (np.abs(pi.astype(np.float32)) == 1).mean() >= 0.05
    assert (np.abs(pi) < 0.9).mean() >= 0.05
    assert all(np.abs(g).max() > 0 for pair in clear.ref64["actor_grads"] for g in pair)


def _integer_conditions(one, B, actor=True):
    assert one.report["integral"] and one.report["bound"] < 2 ** 24
    names = ("critic", "actor") if actor else ("critic",)
    for name in names:
        # float64 autograd is the restatement in numpy, and float32 autograd is float64's, bit for bit
        assert one.ref64[name + "_loss"] != 0
        assert one.ref64[name + "_loss"] == one.report[name + "_loss"] == one.ref32[name + "_loss"]
        for pair64, pair32, mine in zip(one.ref64[name + "_grads"], one.ref32[name + "_grads"], one.report[name + "_grads"]):
            for g64, g32, g in zip(pair64, pair32, mine):
                assert g32.dtype == np.float32 and np.array_equal(g32.astype(np.float64), g64)
                assert np.array_equal(g.reshape(g64.shape), g64)
                assert np.array_equal(g64 * B, np.rint(g64 * B))
                assert np.count_nonzero(g64) >= 0.01 * g64.size
    if actor:
        pi = one.report["pi"]
        assert (pi == 0).mean() >= 0.02 and (np.abs(pi) == 1).mean() >= 0.02 and np.isin(pi, (-1.0, 0.0, 1.0)).all()


@pytest.mark.parametrize("case", R.INTEGER_CASES)
def test_the_integer_cases_are_exact_in_any_order(case):
    _integer_conditions(R.integer_case(*case), case[3])


@pytest.mark.parametrize("case", R.TWIN_CASES)
def test_the_twin_integer_cases_are_exact_in_any_order(case):
    one, two = R.integer_twin(*case)
    _integer_conditions(one, case[3], actor=False)
    _integer_conditions(two, case[3], actor=False)
    assert all(t1 is t2 for t1, t2 in zip(one.made[2:], two.made[2:]))      # one batch
    assert one.ref64["critic_loss"] != two.ref64["critic_loss"]
    if case[0] == case[1]:
        assert not np.array_equal(one.ref64["critic_grads"][0][0], two.ref64["critic_grads"][0][0])


def test_the_tail_case_is_the_1024_rows_and_their_first_tile_again():
    made, ref64, ref32 = R.integer_tail_case(*R.TAIL_CASE)
    a_hidden, c_hidden, in_dim, densities, seed = R.TAIL_CASE
    base = R.integer_case(a_hidden, c_hidden, in_dim, R.T * R.SLOTS, densities, seed)
    B = R.T * R.SLOTS + R.T
    for t, t0 in zip(made[2:], base.made[2:]):
        assert len(t) == B and _same(t[:B - R.T], t0) and _same(t[B - R.T:], t0[:R.T])
    assert ref64["critic_loss"] != 0 and ref64["actor_loss"] != 0
    assert all(np.abs(g).max() > 0 for name in ("critic_grads", "actor_grads") for pair in ref64[name] for g in pair)
