"""SacLearner.actor_step (ctr_sac_actor_step) where training takes it and tests/test_gpu_sac_grads.py
does not: several tiles per workspace slot up to the largest batch, a saturated head, the clip of the
log standard deviation row by row and at its two ends, a seed and a counter above 2^32 with the
learner's own count, and the temperature that the second of two steps reads; and ctr_gauss_act on the
last rows of the noise's index space.  tests/sac_ref.py makes the inputs and
tests/test_host_sac_ref.py checks their conditions without a GPU.

The comparison is test_gpu_sac_grads.py's: per tensor err = max|g - g64| / max|g64| against float64
autograd on the CPU, the bar 8 times the same quantity of torch's float32 CPU autograd, computed here
and printed; every learning rate 0 unless said otherwise.  The matrices and bias vectors get no floor.
The scalars take the floor tests/test_gpu_ddpg_edges.py derives: the bar of ``loss`` and ``logp_mean``
is max(8 x torch's, 2^-23), since float32's spacing is between 2^-24 and 2^-23 of the value; and
``alpha_grad`` is the float32 sum -(logp_mean + target_entropy), whose rounding belongs to the larger
addend, so its absolute error is held to max(8 x torch's, 2^-23 max(|logp_mean|, |target_entropy|))
(``sac_ref.bars``)."""
import numpy as np
import pytest

import ddpg_ref as R
import sac_ref as S
from test_gpu_sac_grads import _unmoved

pytestmark = pytest.mark.gpu

SCALARS = ("loss", "logp_mean", "alpha_grad")


def _ids(cases):
    return ["%s-%d" % ("x".join(map(str, shape[0])), B) for shape, B in cases]


def _learner(made, cuda, B, seed=0, **kw):
    from ctr_reach_amd.learner import SacLearner
    policy, c1, c2, _ = made
    for name in ("actor_lr", "critic_lr", "alpha_lr"):
        kw.setdefault(name, 0.0)
    kw.setdefault("target_entropy", S.TARGET_ENTROPY)
    return SacLearner(R.to_device(policy, cuda), R.to_device(c1, cuda), R.to_device(c2, cuda), init_alpha=S.ALPHA,
                      max_batch=B, seed=seed, **kw)


def _snapshot(learner):
    """A step's outputs on the host: dict(loss, logp_mean, alpha_grad: float32 scalars, grads)."""
    import torch
    torch.cuda.synchronize()
    out = {name: t.cpu().numpy().copy() for name, t in zip(SCALARS, (learner.actor_loss, learner.logp_mean, learner.alpha_grad))}
    out["grads"] = R.host(learner.actor_grads)
    return out


def _errors(got, ref64):
    """The step's errors in the units of ``sac_ref.bars``."""
    ours = {name: abs(float(got[name]) - ref64[name]) / abs(ref64[name]) for name in ("loss", "logp_mean")}
    ours["alpha_grad"] = abs(float(got["alpha_grad"]) - ref64["alpha_grad"])
    assert len(got["grads"]) == len(ref64["grads"])
    ours["grads"] = []
    for pair, pair64 in zip(got["grads"], ref64["grads"]):
        for g, g64 in zip(pair, pair64):
            assert g.dtype == np.float32 and g.shape == g64.shape and np.isfinite(g).all()
        ours["grads"].append(tuple(S.err(g, g64) for g, g64 in zip(pair, pair64)))
    return ours


def _compare(got, ref64, ref32, tag, capsys, target_entropy=S.TARGET_ENTROPY):
    """Prints every figure and returns what misses its bar."""
    bar, theirs = S.bars(ref64, ref32, target_entropy)
    ours = _errors(got, ref64)
    rows = [(name, ours[name], theirs[name], bar[name]) for name in SCALARS]
    for l in range(len(bar["grads"])):
        rows += [("g%s[%d]" % (which, l), ours["grads"][l][w], theirs["grads"][l][w], bar["grads"][l][w]) for w, which in enumerate("Wb")]
    report, failed, worst = [], [], (0.0, "")
    for name, mine, torchs, limit in rows:
        floor = " FLOOR" if mine > 8 * torchs and name in SCALARS and mine <= limit else ""
        report.append("%s %.3g (torch f32 %.3g)%s" % (name, mine, torchs, floor))
        if not mine <= limit:
            failed.append(report[-1])
        ratio = mine / torchs if torchs > 0 else (0.0 if mine == 0 else float("inf"))
        if not floor:
            worst = max(worst, (ratio, name))
    with capsys.disabled():
        print("\n%s: %s; worst ratio %.2f (%s)" % (tag, "; ".join(report), worst[0], worst[1]))
    return failed


def _frozen(learner, made, alpha=S.ALPHA):
    """Every learning rate 0: the three networks and the temperature are where they started."""
    _unmoved(learner, made)
    assert R.bits(learner.log_alpha.cpu().numpy()) == R.bits(np.float32(np.log(np.float64(alpha))))


def _run(clear, cuda, capsys, tag, B):
    learner = _learner(clear.made, cuda, B)
    learner.actor_step(clear.made[3].to(cuda), counter=0)
    got = _snapshot(learner)
    failed = _compare(got, clear.ref64, clear.ref32, "%s, redrawn %d in %d passes, kink %.3g, gap %.3g, critic 1's share %.2f"
                      % (tag, clear.redrawn, clear.passes, clear.ref64["kink"], clear.ref64["gap"], clear.ref64["share"]), capsys)
    assert not failed, failed
    _frozen(learner, clear.made)
    return got


def _assert_clear(clear, B, dims=(0, 1, 2, 3, 4, 5)):
    assert clear.ref64["kink"] >= S.MIN_KINK and clear.ref64["gap"] >= S.MIN_GAP and S.clip_min(clear, dims) >= S.MIN_CLIP
    assert clear.redrawn <= S.MAX_REDRAWN * B and clear.passes <= S.MAX_PASSES
    assert all(np.abs(g).max() > 0 for pair in clear.ref64["grads"] for g in pair)


# --- A: several tiles per slot -----------------------------------------------------------------------

@pytest.mark.parametrize("shape,B", S.TILES_CASES, ids=_ids(S.TILES_CASES))
def test_several_tiles_per_slot_against_float64_autograd(cuda, capsys, shape, B):
    """Past T * SLOTS = 1 024 rows a workgroup sums several tiles into its slot: the later tiles' noise
    index, the tile's head state used again, the gradients added to what the slot holds and the slot's
    loss and logp sums, up to max_B = 65 536 with 64 whole tiles in every slot."""
    clear = S.tiles_case(shape, B)
    _assert_clear(clear, B)
    if shape in S.TILES_MIXED:
        assert 0.1 <= clear.ref64["share"] <= 0.9
    _run(clear, cuda, capsys, "tiles %s, B %d" % (shape, B), B)


# --- B: a saturated head -------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,B", S.SATURATED_CASES, ids=_ids(S.SATURATED_CASES))
def test_a_saturated_head_against_float64_autograd(cuda, capsys, shape, B):
    """The mean rows times 100: where tanh(u) rounds to +-1.0f the critics see exactly +-1 and the
    float64 head still has 1 - t * t of 1e-8 or less; near it 1 - t * t is a cancellation."""
    clear = S.saturated_case(shape, B)
    _assert_clear(clear, B)
    one, low = S.saturation(clear)
    assert one >= 0.05 and low >= 0.05
    _run(clear, cuda, capsys, "saturated %s, B %d, +-1.0f %.3f, below 0.9 %.3f" % (shape, B, one, low), B)


# --- C: the clip, row by row ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape,B", S.CLIP_CASES, ids=_ids(S.CLIP_CASES))
def test_the_clip_row_by_row_against_float64_autograd(cuda, capsys, shape, B):
    """The log standard deviation rows times 8 with biases of 1.5 and -19: in one dimension some rows are
    clipped, where d/ds is zero, and others open (tests/test_host_sac_ref.py has the fractions per
    dimension and what the second shape does not reach)."""
    clear = S.clip_case(shape, B)
    _assert_clear(clear, B)
    above, below, is_open, every_dimension = S.clipping(clear)
    assert above >= 0.05 and below >= 0.05 and is_open >= 0.30 and (every_dimension or shape != S.SHAPES[0])
    _run(clear, cuda, capsys, "clip %s, B %d, above %.2f, below %.2f, open %.2f" % (shape, B, above, below, is_open), B)


# --- D: the clip's ends ----------------------------------------------------------------------------------

def test_the_clip_passes_the_gradient_at_its_ends_and_not_outside(cuda, capsys):
    """Log standard deviations of exactly 2, -20 and one float32 beyond each: as torch's clamp, the step
    passes d/ds at the ends and stops it outside.  (Rows 6 and 7 of gW are the sum of ds h over the rows
    and are not zero, in the float64 reference either: W = 0 there takes h out of y, not out of dW.)"""
    shape, B = S.ENDS_CASE
    clear = S.ends_case()
    _assert_clear(clear, B, dims=(4, 5))
    got = _run(clear, cuda, capsys, "ends %s, B %d" % (shape, B), B)
    gW, gb = got["grads"][-1]
    assert gb[6] != 0 and gb[7] != 0 and gW[6].any() and gW[7].any()
    assert gb[8] == 0 and gb[9] == 0 and not gW[8:10].any()
    gW64, gb64 = clear.ref64["grads"][-1]
    assert gb64[6] != 0 and gb64[7] != 0 and gb64[8] == 0 and gb64[9] == 0 and not gW64[8:10].any()


# --- E: the draw -----------------------------------------------------------------------------------------

def _same_bits(a, b):
    for name in SCALARS:
        assert R.bits(a[name]) == R.bits(b[name]), name
    for l, (pa, pb) in enumerate(zip(a["grads"], b["grads"])):
        for x, y in zip(pa, pb):
            assert np.array_equal(R.bits(x), R.bits(y)), l


def test_the_draw_is_the_learners_seed_and_count(cuda, capsys):
    """A seed and a count with different halves above and below 2^32: the first step draws (seed, count),
    the second (seed, count + 1), and that count given by hand repeats it.  tests/test_host_sac_ref.py
    shows that the swapped pair, the low words and the count not advanced are 100 bars away."""
    shape, B = S.DRAW_CASE
    draw = S.draw_case()
    _assert_clear(draw.clear, B)
    assert S.clear(draw.second[1]) and 0.1 <= draw.clear.ref64["share"] <= 0.9
    made = draw.clear.made
    rows = made[3].to(cuda)
    learner = _learner(made, cuda, B, seed=S.DRAW_SEED)
    assert learner.seed == S.DRAW_SEED and learner.counter == 0
    learner.counter = S.DRAW_COUNTER
    learner.actor_step(rows)
    first = _snapshot(learner)
    failed = _compare(first, draw.clear.ref64, draw.clear.ref32, "draw, first step", capsys)
    assert not failed, failed
    learner.actor_step(rows)
    second = _snapshot(learner)
    failed = _compare(second, draw.second[1], draw.second[2], "draw, second step", capsys)
    assert not failed, failed
    assert learner.counter == S.DRAW_COUNTER + 2
    _frozen(learner, made)
    fresh = _learner(made, cuda, B, seed=S.DRAW_SEED)
    fresh.actor_step(rows, counter=S.DRAW_COUNTER + 1)
    _same_bits(_snapshot(fresh), second)
    assert fresh.counter == 0
    _frozen(fresh, made)


# --- F: the temperature a step reads -----------------------------------------------------------------------

def test_the_second_step_reads_the_temperature_the_first_left(cuda, capsys):
    import torch
    shape, B = S.TEMP_CASE
    clear = S.temperature_case()
    _assert_clear(clear, B)
    made = clear.made
    rows = made[3].to(cuda)
    learner = _learner(made, cuda, B, alpha_lr=S.TEMP_ALPHA_LR, learn_alpha=True, target_entropy=S.TEMP_TARGET)
    learner.actor_step(rows, counter=S.TEMP_COUNTER)
    first = _snapshot(learner)
    failed = _compare(first, clear.ref64, clear.ref32, "temperature, first step at alpha %g" % S.ALPHA, capsys, S.TEMP_TARGET)
    assert not failed, failed
    log_alpha = learner.log_alpha.cpu().numpy().copy()
    assert log_alpha.dtype == np.float32 and abs(float(log_alpha) - np.log(S.ALPHA)) > 0.9 * S.TEMP_ALPHA_LR
    alpha = float(np.exp(np.float64(log_alpha)))
    next64, next32 = (S.autograd(*made, clear.eps, alpha, d, S.TEMP_TARGET) for d in (torch.float64, torch.float32))
    learner.actor_step(rows, counter=S.TEMP_COUNTER)
    second = _snapshot(learner)
    failed = _compare(second, next64, next32, "temperature, second step at alpha %.6g" % alpha, capsys, S.TEMP_TARGET)
    assert not failed, failed
    # and not the first step's: the loss and the output layer's bias gradient are more than 10 bars from that reference
    bar, _ = S.bars(next64, next32, S.TEMP_TARGET)
    stale = _errors(second, clear.ref64)
    assert stale["loss"] > 10 * bar["loss"] and stale["grads"][-1][1] > 10 * bar["grads"][-1][1] > 0
    _unmoved(learner, made)


# --- G: the last rows of the index space ---------------------------------------------------------------------

def test_gauss_act_on_the_last_rows_of_the_index_space(cuda, capsys):
    """row_base + n = 2^32: the noise index row_base + row as a 32-bit word, up to 2^32 - 1."""
    import test_gpu_gauss_actor as G
    n, counter = 300, (9 << 32) | 1234
    row_base = 2 ** 32 - n
    rng = np.random.default_rng(8)
    pi = G._policy(cuda, G._random_layers(rng, (64, 96), 20))
    rows = G._rows(rng, n, 20, cuda)
    out = G._host(pi.sample(rows, counter, row_base=row_base, logits=True))
    want = G._check_head(pi, out, counter, row_base, False, capsys, "row_base 2^32 - %d, n %d" % (n, n))
    assert np.abs(want["unit"]).max() > 0.5 and np.ptp(want["logp"]) > 1
    half = G._host(pi.sample(rows[:150], counter, row_base=row_base, logits=True))
    for k in half:
        assert np.array_equal(R.bits(half[k]), R.bits(out[k][:150])), k
    # the index matters up there: the same rows at base 0 are another draw on every row
    assert (G._host(pi.sample(rows, counter))["unit"] != out["unit"]).any(axis=1).all()
