"""The period loop's chunk rule (vec_env.period_chunk) and its bookkeeping (_stepped, _run_periods)
against step_raw's rule, restated here as a state machine over (since, pool_full, parity, refills,
sweeps): no GPU, no library call.

A step is POOLED iff ``pool_full and since < pooled``, else a SWEEP; a refill at ``since >= R``
clears ``pool_full`` iff ``since > pooled``, and resets ``since``.  A period kernel runs POOLED steps
only, so a chunk must hold steps of one mode, end where step_raw's refill falls due, and be refused
exactly where the next eager step would be a SWEEP."""
import functools
import itertools
import types

import pytest

from ctr_reach_amd import _abi
from ctr_reach_amd.vec_env import CtrReachVecEnv, period_chunk

OFF, SWEEP, POOLED = _abi.AUTORESET_OFF, _abi.AUTORESET_SWEEP, _abi.AUTORESET_POOLED
DEPTHS = (0, 1, 3, 4, 8, 64, 70, 152)
INTERVALS = (1, 3, 4, 20, 64, 100)
LEADS = (1, 4, 64)
STEPS = (0, 1, 2, 5, 63, 64, 65, 130, 257)


def eager(P, R, pooled, autoreset, state, steps):
    """step_raw's host rule, ``steps`` times: the mode of every step and the state after it."""
    since, full, parity, refills, sweeps = state
    modes, states = [], [state]
    for _ in range(steps):
        mode = OFF
        if autoreset:
            mode = POOLED if full and since < pooled else SWEEP
            sweeps += mode == SWEEP
            parity ^= 1
        if P:
            since += 1
            if since >= R:                     # refill_pool
                refills += 1
                full = full and not since > pooled
                since = 0
        modes.append(mode)
        states.append((since, full, parity, refills, sweeps))
    return modes, states


class Host(object):
    """The env's host state without a device: the env's own loop and bookkeeping, on a refill that
    only counts (refill_pool's rule as stated above)."""
    _run_periods = CtrReachVecEnv._run_periods
    _stepped = CtrReachVecEnv._stepped

    def __init__(self, P, R, pooled, autoreset, state):
        self.pool_depth, self.refill_interval, self.pooled, self.autoreset = P, R, pooled, autoreset
        self._steps_since_refill, self._pool_full, parity, self.refills, self.sweeps = state
        self._batch = types.SimpleNamespace(work_parity=parity)
        self.fused_launches = 0

    def _pooled_steps(self):
        return self.pooled

    def refill_pool(self, stream=None):
        self.refills += 1
        if self._steps_since_refill > self.pooled:
            self._pool_full = False
        self._steps_since_refill = 0

    def state(self):
        return (self._steps_since_refill, self._pool_full, self._batch.work_parity, self.refills, self.sweeps)


@functools.lru_cache(maxsize=None)
def cases():
    """Every distinct case of the grid, (P, R, pooled, autoreset, start state), with its eager run of
    max(STEPS) steps.  (The grid's 27 288 runs are 11 988 distinct ones: refill_lead and carry act
    through ``pooled`` alone.)"""
    seen = {}
    for P, R, lead, carry, autoreset, full in itertools.product(DEPTHS, INTERVALS, LEADS, (True, False), (True, False),
                                                                (True, False)):
        if autoreset and not P:
            continue                           # _period_ineligible refuses it before the loop
        pooled = min(P, lead) if carry else P  # _pooled_steps
        for since in {0, 1, R - 1, pooled - 1}:
            if not 0 <= since < (R if P else 1):
                continue                       # a refill resets the count at R; without a pool nothing counts
            case = (P, R, pooled, autoreset, (since, full, 0, 0, 0))
            if case not in seen:
                seen[case] = eager(P, R, pooled, autoreset, case[4], max(STEPS))
    return [case + run for case, run in seen.items()]


def test_period_chunk_is_step_raw_rule_in_chunks():
    runs = refusals = 0
    for P, R, pooled, autoreset, start, modes, states in cases():
        for steps in STEPS:
            host, i, refused = Host(P, R, pooled, autoreset, start), 0, False
            while i < steps:
                k, mode = period_chunk(steps - i, host._steps_since_refill, P, R, pooled, autoreset, host._pool_full)
                if k < 1:
                    refused = True
                    break
                assert 1 <= k <= 64 and i + k <= steps
                assert modes[i:i + k] == [mode] * k, (P, R, pooled, autoreset, start, steps, i, k)
                host._stepped(k, None)
                i += k
                assert host.state() == states[i], (P, R, pooled, autoreset, start, steps, i)
            # refused exactly where the next eager step would be a sweep, and nowhere else
            assert refused == (i < steps and modes[i] == SWEEP)
            assert SWEEP not in modes[:i] and host.state() == states[i]
            runs += 1
            refusals += refused
    print("runs %d, refused %d" % (runs, refusals))
    assert refusals > 0 and runs - refusals > 0


def test_run_periods_is_that_rule_with_one_launch_per_chunk():
    """_run_periods: the launches tile the steps, a whole period is flagged as one, a launch that
    says it ran the period's refill leaves step_raw's state too, and a refusal raises with the
    caller's name after the launches before it."""
    whole = tails = 0
    for P, R, pooled, autoreset, start, modes, states in cases():
        for steps, tail in itertools.product(STEPS, (False, True)):
            host, at = Host(P, R, pooled, autoreset, start), [0, 0, 0]     # next step, launches, whole periods

            def launch(i, k, mode, whole_period):
                assert i == at[0] and host.state() == states[i] and modes[i:i + k] == [mode] * k
                assert whole_period == (mode == POOLED and states[i][0] == 0 and k == R)
                at[:] = i + k, at[1] + 1, at[2] + whole_period
                return tail and whole_period
            try:
                host._run_periods("who", steps, launch, None)
                assert at[0] == steps
            except RuntimeError as e:
                assert str(e) == "who: the next step's resets are not all in the pool"
                assert at[0] < steps and modes[at[0]] == SWEEP
            assert host.fused_launches == at[1] and host.state() == states[at[0]]
            whole += at[2]
            tails += tail and at[2]
    assert whole > tails > 0


@pytest.mark.parametrize("remaining,since,want", [(257, 0, 64), (64, 0, 64), (3, 0, 3), (64, 2, 62), (64, 63, 1)])
def test_default_period(remaining, since, want):
    """The default env (64-slot pool, R = 64, the resumable refill's lead 64): one launch per period."""
    assert period_chunk(remaining, since, 64, 64, 64, True, True) == (want, POOLED)
    assert period_chunk(remaining, since, 64, 64, 64, True, False) == (0, POOLED)
    assert period_chunk(remaining, since, 0, 64, 0, False, False) == (min(remaining, 64), OFF)
