"""The conditions of tests/test_gpu_learner_sequence.py's inputs, which look at the float64 references
alone, checked without a GPU at every size of ``seq_ref.SIZES``: every hidden pre-activation at least
1e-5 from the relu's kink; for SAC every |Q1 - Q2| at least 1e-4 and every log standard deviation 1e-3
from the clip's ends; no gradient tensor that is zero (at B = 1: the one row's relus are not all shut in
any layer); and on the sizes 1, 15, 16 and 17 every row's |Q - target| at least 0.1, so that the critic's
loss is not a cancellation that the bar of 8 times torch's float32 error could not judge.  The seeds
recorded in tests/seq_ref.py are the first ones from 0 upward that meet all of it."""
import numpy as np
import pytest

import ddpg_ref as R
import sac_ref as S
import seq_ref as Q

SIZES = sorted(set(Q.SIZES))


def test_the_sizes_are_the_ones_the_kernels_can_go_wrong_at():
    assert Q.MAX_BATCH == 1040 == R.T * R.SLOTS + R.T == max(Q.SIZES)
    assert Q.SIZES == (1040, 1, 17, 16, 300, 1024, 15, 1040) and Q.SMALL == (1, 15, 16, 17)
    assert all(a != b for a, b in zip(Q.SIZES[:-1], Q.SIZES[1:]))          # every step finds another size's workspace
    assert Q.SIZES[0] == Q.SIZES[-1] == Q.MAX_BATCH


def _assert_ddpg(cond, B, tag):
    assert cond["kink"] >= 1e-5, (tag, B, cond)
    assert cond["nonzero"], (tag, B)
    if B in Q.SMALL:
        assert cond["residual"] >= 0.1, (tag, B, cond)
    assert Q.holds(cond, B)


@pytest.mark.parametrize("i", [0, 1])
def test_the_ddpg_case_meets_its_conditions_at_every_size(i):
    clear = Q.ddpg_case(i)
    assert clear.redrawn <= 0.15 * Q.MAX_BATCH and clear.passes <= 20
    assert tuple(clear.made[2].shape) == (Q.MAX_BATCH, Q.DDPG_SHAPES[i][2])
    for B in SIZES:
        _assert_ddpg(Q.ddpg_conditions(i, B), B, "ddpg")
    # the whole batch's reference is case_clear's own
    ref64 = Q.ddpg_refs(i, Q.MAX_BATCH)[0]
    assert ref64["critic_loss"] == clear.ref64["critic_loss"] and ref64["kink"] == clear.ref64["kink"]


@pytest.mark.parametrize("i", [0, 1])
def test_the_twin_case_meets_its_conditions_at_every_size(i):
    policy, critic1, critic2, rows, actions, target, redrawn = Q.td3_case(i)
    made = Q.ddpg_case(i).made
    assert policy is made[0] and critic1 is made[1] and target is made[4]
    moved = ((rows != made[2]).any(dim=1) | (actions != made[3]).any(dim=1)).numpy()
    assert 0 < redrawn <= 8 and moved.sum() <= redrawn                    # DDPG's batch but for those rows
    assert (Q._row_kinks2(critic2, made[2], made[3])[moved] < 1e-5).all()
    widths = [[W.shape[0] for W, _ in R.params(c)][:-1] for c in (critic1, critic2)]
    assert widths == [list(Q.DDPG_SHAPES[i][1]), list(Q.TD3_CRITIC2[i])]
    assert (i == 0) == (widths[0] == widths[1])                           # the second pair's planes differ in size
    for B in SIZES:
        one, two = Q.td3_conditions(i, B)
        _assert_ddpg(one, B, "critic 1")
        _assert_ddpg(two, B, "critic 2")
    (one64, _), (two64, _) = Q.td3_refs(i, Q.MAX_BATCH)
    assert one64["critic_loss"] != two64["critic_loss"]


@pytest.mark.parametrize("i", [0, 1])
def test_the_sac_case_meets_its_conditions_at_every_size(i):
    clear = Q.sac_case(i)
    assert clear.redrawn <= S.MAX_REDRAWN * Q.MAX_BATCH and clear.passes <= S.MAX_PASSES
    shares = []
    for B in SIZES:
        cond = Q.sac_conditions(i, B)
        assert cond["kink"] >= 1e-5 and cond["gap"] >= 1e-4 and cond["clip"] >= 1e-3, (B, cond)
        assert cond["nonzero"], B
        assert Q.holds(cond, B)
        shares.append(Q.sac_refs(i, B)[0]["share"])
        assert np.array_equal(S.eps_for(B, 0, 0), clear.eps[:B])           # a prefix's noise is the prefix of the noise
    assert 0.1 <= shares[-1] <= 0.9                                        # both critics give the minimum on the whole batch
    ref64 = Q.sac_refs(i, Q.MAX_BATCH)[0]
    assert ref64["loss"] == clear.ref64["loss"] and ref64["kink"] == clear.ref64["kink"]


def test_no_earlier_seed_meets_the_conditions():
    """The recorded seeds are the first: the smallest shape's DDPG seeds below the recorded one each fail
    (one of the first 17 rows has |Q - target| below 0.1)."""
    for seed in range(Q.DDPG_SEEDS[0]):
        assert not all(Q.holds(Q.ddpg_conditions(0, B, seed), B) for B in SIZES), seed


def test_pow_after_is_eight_float32_products():
    pw = Q.pow_after(len(Q.SIZES))
    want = [np.float32(1), np.float32(1)]
    for _ in Q.SIZES:
        want = [want[0] * np.float32(0.9), want[1] * np.float32(0.999)]
    assert pw.dtype == np.float32 and np.array_equal(R.bits(pw), R.bits(np.array(want, dtype=np.float32)))
