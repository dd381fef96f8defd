"""Diagnostic: where the waves of k_step_tail (ctr_step_period: a refill period's steps and its
refill in one kernel) spend the period's tail, from a library built with -DCTR_DIAG_WAVETIME (each
wave's lane 0 stores, on the 100 MHz real-time clock, the kernel's start, the end of its steps, the
end of its claim phase, the end of its own new resets and its end).  The bench's steady state:
65 536 envs, staggered episode clocks, 20-step periods.

build: the sources copied, tools/experiments/diag.patch applied, make EXTRA=-DCTR_DIAG_WAVETIME
       LIB=.../libab_wavet.so (tools/experiments/build_rev.sh does that for a committed revision)
usage: CTR_REACH_AMD_LIB=.../libab_wavet.so python tools/tail_wave_times.py [n_envs] [R]"""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-ctr-reach_amd"))
from ctr_reach_amd import CtrReachVecEnv, _abi  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
R = int(sys.argv[2]) if len(sys.argv) > 2 else 20
env = CtrReachVecEnv(n, device="cuda:0", seed=0, refill_interval=R, tail_refill=True)
env.reset()
lib = env.lib
lib.ctr_diag_wavetimes.argtypes = [ctypes.c_void_p, ctypes.c_int]
g = torch.Generator(device="cuda:0")
g.manual_seed(1)
hi = torch.tensor(env.action_space.high, device="cuda:0")
acts = [((torch.rand((n, 6), generator=g, device="cuda:0") * 2 - 1) * hi).contiguous() for _ in range(R)]
g0 = torch.Generator(device="cpu")
g0.manual_seed(2)
env.t.copy_(torch.randint(0, 150, (n,), generator=g0, dtype=torch.int32))
for _ in range(480 // R):                                  # to the steady state
    env.step_many(acts)
nw = (n + 63) // 64
names = ("steps", "claim phase", "own resets", "to the wave's end")
rows = {k: [] for k in names}
tails, slow = [], []
for rep in range(8):
    env.step_many(acts)
    torch.cuda.synchronize()
    t = np.zeros((nw, 6), dtype=np.uint64)
    _abi.check(lib.ctr_diag_wavetimes(t.ctypes.data, nw), "ctr_diag_wavetimes")
    t = t.astype(np.float64) * 0.01                        # us
    t0 = t[:, 0].min()
    for k, (a, b) in zip(names, ((0, 1), (1, 2), (2, 3), (3, 5))):
        rows[k].append(t[:, b] - t[:, a])
    end = t[:, 5].max()
    s = int(np.argmax(t[:, 1]))                            # the wave whose steps end last
    tails.append((t[:, 1].max() - t0, end - t[:, 1].max(), end - t0, (end - t[:, 5]).mean()))
    slow.append((t[s, 2] - t[s, 1], t[s, 3] - t[s, 2], t[s, 5] - t[s, 3], end - t[s, 5]))
assert env.tail_launches > 0
print("k_step_tail, %d envs, %d-step periods, suspended now %s" % (n, R, env.carried()))
for k in names:
    a = np.concatenate(rows[k])
    print("    %-18s us: p10 %.1f p50 %.1f p90 %.1f max %.1f mean %.1f" % (k, *np.percentile(a, [10, 50, 90, 100]), a.mean()))
a = np.array(tails).mean(axis=0)
print("    last wave's steps end at %.1f us, the kernel's last wave ends %.1f us later (%.1f us in all); a wave "
      "is idle %.1f us at the end on average" % tuple(a))
a = np.array(slow).mean(axis=0)
print("    the wave whose steps end last: claim phase %.1f us, own resets %.1f us, to its end %.1f us; the last "
      "wave of the kernel ends %.1f us after it" % tuple(a))
