"""The conditions of tests/test_gpu_sac_edges.py's inputs, which look at the float64 reference alone,
checked without a GPU: ``sac_ref.make_clear`` leaves every case clear of the relu's kink, of Q1 = Q2 and
of the clip's ends within its caps on rows drawn again and on passes, with nothing to draw again it is
``make``, and a row is drawn again on its own account; the saturated, clipped and end-of-clip heads
are what their tests need; another draw and another temperature are other gradients, far outside
the bar.

One condition is narrower than planned.  Every dimension of the log standard deviation was to have
both clipped and open rows in both clipped cases.  On ((32,), (32,), (32,), 19) at B = 70 all six have.
On ((32, 256, 32), (32,), (64,), 20) at B = 1 029 a dimension's 8 y[6 + i] stays within about 1 of its
bias (the last hidden layer is 32 wide), so dimension 0 is above 2 on every row and dimensions 2, 4 and
5 are open on every row; dimension 1 is above 2 on 0.89 of the rows and dimension 3 below -20 on 0.78.
No seed from 0 to 39 gives that shape six mixed dimensions under these gains.  There the condition is:
one dimension mixed at each end, one clipped throughout and one open throughout."""
import numpy as np
import pytest

import ddpg_ref as R
import sac_ref as S

CLEAR = [("tiles", c) for c in S.TILES_CASES] + [("saturated", c) for c in S.SATURATED_CASES] + \
    [("clip", c) for c in S.CLIP_CASES] + [("ends", S.ENDS_CASE), ("draw", S.DRAW_CASE), ("temperature", S.TEMP_CASE)]


def _case(kind, shape, B):
    if kind in ("tiles", "saturated", "clip"):
        return getattr(S, kind + "_case")(shape, B)
    return {"ends": S.ends_case, "draw": lambda: S.draw_case().clear, "temperature": S.temperature_case}[kind]()


def _same(a, b):
    return np.array_equal(R.bits(a.numpy()), R.bits(b.numpy()))


def _all_grads(ref):
    return [g for pair in ref["grads"] for g in pair]


@pytest.mark.parametrize("kind,case", CLEAR, ids=lambda v: v if isinstance(v, str) else "%s-%d" % ("x".join(map(str, v[0][0])), v[1]))
def test_every_case_is_clear_within_the_caps(kind, case):
    shape, B = case
    clear = _case(kind, shape, B)
    policy, c1, c2, rows = clear.made
    dims = (4, 5) if kind == "ends" else tuple(range(6))
    assert clear.ref64["kink"] >= S.MIN_KINK and clear.ref64["gap"] >= S.MIN_GAP
    assert S.clip_min(clear, dims) >= S.MIN_CLIP
    if kind == "ends":
        assert clear.ref64["clip"] == 0                    # dimensions 0 and 1 sit on the ends themselves
    else:
        assert clear.ref64["clip"] >= S.MIN_CLIP
    assert clear.redrawn <= S.MAX_REDRAWN * B and clear.passes <= S.MAX_PASSES
    assert rows.shape == (B, shape[3]) and clear.eps.shape == (B, 6)
    # the per-row conditions are autograd's, which takes its minima over the whole batch
    c = S.row_conditions(policy, c1, c2, rows, clear.eps, dims)
    assert c.kink.min() == pytest.approx(clear.ref64["kink"], rel=1e-6)
    assert c.gap.min() == pytest.approx(clear.ref64["gap"], rel=1e-6)
    assert c.first.mean() == pytest.approx(clear.ref64["share"])
    # every gradient tensor carries something
    assert all(np.abs(g).max() > 0 for g in _all_grads(clear.ref64))
    assert clear.ref64["loss"] != 0 and clear.ref64["logp_mean"] != 0 and clear.ref64["alpha_grad"] != 0
    # what was not drawn again is make's: the critics, the policy's hidden layers and all rows but as many as were
    # drawn again at the most; the rows drawn again were within reach of a kink, a tie or an end, the others were not
    policy0, c10, c20, rows0 = S.make(0, *shape, B)
    for (W, b), (W0, b0) in zip(R.params(c1) + R.params(c2) + R.params(policy)[:-1],
                                R.params(c10) + R.params(c20) + R.params(policy0)[:-1]):
        assert _same(W, W0) and _same(b, b0)
    moved = (rows != rows0).any(dim=1).numpy()
    assert int(moved.sum()) <= clear.redrawn
    c0 = S.row_conditions(policy, c1, c2, rows0, clear.eps, dims)
    bad0 = (c0.kink < S.MIN_KINK) | (c0.gap < S.MIN_GAP) | (c0.clip < S.MIN_CLIP)
    assert np.array_equal(bad0, moved)
    assert bool(clear.redrawn) == bool(moved.any())


@pytest.mark.parametrize("shape,B", [c for c in S.TILES_CASES if c[0] in S.TILES_MIXED])
def test_both_critics_give_the_minimum_across_the_tiles(shape, B):
    assert 0.1 <= S.tiles_case(shape, B).ref64["share"] <= 0.9


def test_the_default_call_is_make():
    shape, B = S.SHAPES[0], 70
    seed, made, eps, ref64, _ = S.case(*shape, B, mixed=True)              # (a seed that is clear as it stands)
    clear = S.make_clear(seed, *shape, B)
    assert clear.redrawn == 0 and clear.passes == 0
    for mine, theirs in zip(clear.made[:3], made[:3]):
        for (W, b), (W0, b0) in zip(R.params(mine), R.params(theirs)):
            assert _same(W, W0) and _same(b, b0)
    assert _same(clear.made[3], made[3]) and np.array_equal(clear.eps, eps)
    for name in ("loss", "logp_mean", "alpha_grad", "kink", "gap", "clip", "share"):
        assert clear.ref64[name] == ref64[name], name


def test_the_head_is_shaped_as_stated():
    """The gains multiply W and b of their six rows, the biases are added behind the gain, and exact_ends
    makes a row the constant."""
    shape, B = S.SHAPES[1], 70
    W0, b0 = R.params(S.make(0, *shape, B)[0])[-1]
    W, b = R.params(S.saturated_case(shape, B).made[0])[-1]
    assert _same(W[:6], W0[:6] * S.MEAN_GAIN) and _same(b[:6], b0[:6] * S.MEAN_GAIN) and _same(W[6:], W0[6:]) and _same(b[6:], b0[6:])
    W0, b0 = R.params(S.make(0, *S.SHAPES[0], B)[0])[-1]
    W, b = R.params(S.clip_case(S.SHAPES[0], B).made[0])[-1]
    assert _same(W[6:], W0[6:] * S.STD_GAIN) and _same(W[:6], W0[:6]) and _same(b[:6], b0[:6])
    import torch
    assert _same(b[6:], b0[6:] * S.STD_GAIN + torch.tensor(S.STD_BIAS))
    W0, b0 = R.params(S.make(0, *shape, B)[0])[-1]
    W, b = R.params(S.ends_case().made[0])[-1]
    assert not W[6:10].any() and _same(W[10:], W0[10:]) and _same(W[:6], W0[:6]) and _same(b[10:], b0[10:])
    assert b[6:10].numpy().astype(np.float64).tolist() == list(S.ENDS[:4])


def test_rows_are_drawn_again_one_by_one():
    """Another row in one place changes no other row's conditions, and the rows drawn again are the first
    draws of a generator seeded 5000 + seed, in row order (a case of one pass)."""
    import torch
    shape, B = S.TILES_CASES[1]
    clear = S.tiles_case(shape, B)
    policy, c1, c2, rows = clear.made
    before = S.row_conditions(policy, c1, c2, rows, clear.eps)
    changed = rows.clone()
    changed[17] = torch.rand(shape[3], generator=torch.Generator().manual_seed(1)) * 2 - 1
    after = S.row_conditions(policy, c1, c2, changed, clear.eps)
    others = np.arange(B) != 17
    for a, b in zip(before, after):
        assert np.array_equal(a[others], b[others])
    assert before.kink[17] != after.kink[17] and before.gap[17] != after.gap[17] and before.clip[17] != after.clip[17]
    # a row alone gives its own values (up to the order of a matrix product's sums)
    one = S.row_conditions(policy, c1, c2, rows[17:18], clear.eps[17:18])
    assert one.kink[0] == pytest.approx(before.kink[17], rel=1e-9) and one.gap[0] == pytest.approx(before.gap[17], rel=1e-6)
    assert one.first[0] == before.first[17]
    rows0 = S.make(0, *shape, B)[3]
    moved = np.flatnonzero((rows != rows0).any(dim=1).numpy())
    assert clear.passes == 1 and len(moved) == clear.redrawn > 0
    g = torch.Generator().manual_seed(5000)
    assert _same(rows[moved], torch.rand((len(moved), shape[3]), generator=g) * 2 - 1)


@pytest.mark.parametrize("shape,B", S.SATURATED_CASES)
def test_a_mean_gain_of_100_saturates_the_head(shape, B):
    one, low = S.saturation(S.saturated_case(shape, B))
    assert one >= 0.05 and low >= 0.05


@pytest.mark.parametrize("shape,B", S.CLIP_CASES)
def test_the_clip_is_active_on_some_rows_and_open_on_others(shape, B):
    clear = S.clip_case(shape, B)
    above, below, is_open, every_dimension = S.clipping(clear)
    assert above >= 0.05 and below >= 0.05 and is_open >= 0.30
    raw = S.head64(clear.made[0], clear.made[3], clear.eps)["raw"]
    up, down = (raw > S.LOG_STD_MAX).mean(axis=0), (raw < S.LOG_STD_MIN).mean(axis=0)
    mixed = lambda f: (f >= 0.05) & (f <= 0.95)  # noqa: E731
    if shape == S.SHAPES[0]:
        assert every_dimension and (mixed(up) | mixed(down)).all()
    else:
        # (the module's docstring) one dimension mixed at each end, one clipped and one open on every row
        assert mixed(up).any() and mixed(down).any() and ((up == 1) | (down == 1)).any() and ((up == 0) & (down == 0)).any()


def test_the_ends_case_sits_on_the_ends():
    """Dimensions 0..3 of the log standard deviation are 2, -20 and one float32 outside each, in float32
    and in float64 alike; torch's clamp passes the gradient at the ends and not outside them."""
    import torch
    clear = S.ends_case()
    raw = S.head64(clear.made[0], clear.made[3], clear.eps)["raw"]
    assert np.array_equal(raw[:, :4], np.tile(S.ENDS[:4], (len(raw), 1)))
    assert S.ENDS[2] > 2.0 and np.float32(S.ENDS[2]) == S.ENDS[2] and S.ENDS[3] < -20.0 and np.float32(S.ENDS[3]) == S.ENDS[3]
    with torch.no_grad():
        raw32 = clear.made[0](clear.made[3])[:, 6:10].numpy()
    assert raw32.dtype == np.float32 and np.array_equal(raw32.astype(np.float64), raw[:, :4])
    for ref in (clear.ref64, clear.ref32):
        gW, gb = ref["grads"][-1]
        assert gb[6] != 0 and gb[7] != 0 and gW[6].any() and gW[7].any()
        assert gb[8] == 0 and gb[9] == 0 and not gW[8:10].any()
    # d/ds of alpha * logp's -s alone: -alpha on every row at -20, where exp(s) eps is below 1e-8 of it
    assert clear.ref64["grads"][-1][1][7] == pytest.approx(-S.ALPHA, rel=1e-6)


def _far(wrong64, right64, right32, factor):
    """Every policy tensor of ``wrong64`` is at least ``factor`` times its bar from ``right64``'s."""
    bar, _ = S.bars(right64, right32)
    for pair_w, pair_r, pair_bar in zip(wrong64["grads"], right64["grads"], bar["grads"]):
        for gw, gr, b in zip(pair_w, pair_r, pair_bar):
            assert b > 0 and S.err(gw, gr) >= factor * b, (S.err(gw, gr), b)


def test_a_wrong_draw_is_far_outside_the_bar():
    import torch
    draw = S.draw_case()
    made, B = draw.clear.made, S.DRAW_CASE[1]
    second64, second32 = draw.second[1:]
    assert S.clear(second64) and 0.1 <= draw.clear.ref64["share"] <= 0.9 and 0.1 <= second64["share"] <= 0.9
    assert S.DRAW_SEED >> 32 and S.DRAW_COUNTER >> 32 and S.DRAW_SEED & 0xFFFFFFFF != S.DRAW_COUNTER & 0xFFFFFFFF
    for counter, (right64, right32) in ((S.DRAW_COUNTER, (draw.clear.ref64, draw.clear.ref32)),
                                        (S.DRAW_COUNTER + 1, (second64, second32))):
        for name, (s, c) in S.wrong_draws(S.DRAW_SEED, counter).items():
            _far(S.autograd(*made, S.eps_for(B, s, c), S.ALPHA, torch.float64), right64, right32, 100)
    # the second step drawn with the first step's counter, and either step with counter 0
    _far(draw.clear.ref64, second64, second32, 100)
    zero = S.autograd(*made, S.eps_for(B, S.DRAW_SEED, 0), S.ALPHA, torch.float64)
    _far(zero, draw.clear.ref64, draw.clear.ref32, 100)
    _far(zero, second64, second32, 100)


def test_the_temperature_s_first_step_is_far_outside_the_bar():
    """After one Adam step of log_alpha at lr 1e-2 the loss and the output layer's bias gradient are more
    than 10 bars from those at the initial temperature; the target entropy of -3.5 is in alpha_grad."""
    import torch
    from ctr_reach_amd.learner import adam_reference
    clear = S.temperature_case()
    ref64, ref32 = clear.ref64, clear.ref32
    assert ref64["alpha_grad"] == -(ref64["logp_mean"] + S.TEMP_TARGET) and S.TEMP_TARGET != S.TARGET_ENTROPY
    plain = S.case_clear(*S.TEMP_CASE[0], S.TEMP_CASE[1], noise=(0, S.TEMP_COUNTER)).ref64          # (with the default -6)
    assert plain["alpha_grad"] - ref64["alpha_grad"] == pytest.approx(S.TEMP_TARGET - S.TARGET_ENTROPY, rel=1e-12)
    la0 = np.float32(np.log(S.ALPHA))
    la1 = adam_reference(la0, np.float32(ref64["alpha_grad"]), 0.0, 0.0, [1.0, 1.0], S.TEMP_ALPHA_LR)[0]
    assert abs(float(la1) - float(la0)) == pytest.approx(S.TEMP_ALPHA_LR, rel=1e-3)
    alpha1 = float(np.exp(np.float64(la1)))
    next64 = S.autograd(*clear.made, clear.eps, alpha1, torch.float64, S.TEMP_TARGET)
    next32 = S.autograd(*clear.made, clear.eps, alpha1, torch.float32, S.TEMP_TARGET)
    assert S.clear(next64)
    bar, _ = S.bars(next64, next32, S.TEMP_TARGET)
    assert abs(ref64["loss"] - next64["loss"]) / abs(next64["loss"]) > 10 * bar["loss"]
    assert S.err(ref64["grads"][-1][1], next64["grads"][-1][1]) > 10 * bar["grads"][-1][1] > 0
