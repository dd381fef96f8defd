"""Waypoint following on the host (no GPU): ctr_set_goal and ctr_follow refuse bad arguments with
CTR_EINVAL (-1) and a telling ctr_last_error before any HIP call (the device pointers are fake and
never dereferenced), ctr_follow wherever ctr_rollout does and with its messages; ctr_follow_t's
ctypes struct matches the header; the ABI number did not move; the path generators against their
closed forms."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_host_actor import _actor, _setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _follow(_abi, K=3, hold=4, reach=1):
    f = _abi.CtrFollow()
    f.waypoints = f.cursor = f.held = f.tip = f.err = f.steps = f.reached = 16
    f.K, f.hold, f.reach = K, hold, reach
    return f


def _refused(lib, rc, *words):
    assert rc == -1
    msg = lib.ctr_last_error()
    for w in words:
        assert w in msg, (w, msg)


def test_follow_refuses_bad_follow_arguments():
    _abi, lib, cfg, b, o = _setup(pool=False)
    a = _actor()
    _refused(lib, lib.ctr_follow(cfg, b, a, None, 4, o, None, None), b"ctr_follow: follow is NULL")
    for field in ("waypoints", "cursor", "held"):
        f = _follow(_abi)
        setattr(f, field, None)
        _refused(lib, lib.ctr_follow(cfg, b, a, f, 4, o, None, None), b"ctr_follow: waypoints, cursor or held is NULL")
    for K in (0, -2):
        _refused(lib, lib.ctr_follow(cfg, b, a, _follow(_abi, K=K), 4, o, None, None), b"ctr_follow: K must be >= 1")
    for hold in (0, -1):
        _refused(lib, lib.ctr_follow(cfg, b, a, _follow(_abi, hold=hold), 4, o, None, None),
                 b"ctr_follow: hold must be >= 1")
    for reach in (2, -1):
        _refused(lib, lib.ctr_follow(cfg, b, a, _follow(_abi, reach=reach), 4, o, None, None),
                 b"ctr_follow: reach must be 0 or 1")


def test_follow_refuses_what_rollout_refuses_with_its_messages():
    _abi, lib, cfg, b, o = _setup(pool=False)
    a, f = _actor(), _follow(_abi)
    for k in (0, -3, _abi.CTR_STEP_MANY_MAX + 1):
        _refused(lib, lib.ctr_follow(cfg, b, a, f, k, o, None, None), b"CTR_STEP_MANY_MAX")
    _refused(lib, lib.ctr_follow(cfg, b, _actor(in_dim=20), f, 4, o, None, None), b"in_dim must be obs_dim + 6")
    _refused(lib, lib.ctr_follow(cfg, b, _actor((48,)), f, 4, o, None, None), b"actor")
    for field in ("packed", "gather", "gather_prev"):
        setattr(o, field, 16)
        _refused(lib, lib.ctr_follow(cfg, b, a, f, 4, o, None, None), b"packed")
        setattr(o, field, None)
    o.obs = None
    _refused(lib, lib.ctr_follow(cfg, b, a, f, 4, o, None, None), b"output missing")
    o.obs = 16
    b.joints = None
    _refused(lib, lib.ctr_follow(cfg, b, a, f, 4, o, None, None), b"batch buffer missing")
    b.joints = 16
    assert lib.ctr_follow(None, b, a, f, 4, o, None, None) == -1
    assert lib.ctr_follow(cfg, None, a, f, 4, o, None, None) == -1
    assert lib.ctr_follow(cfg, b, None, f, 4, o, None, None) == -1
    assert lib.ctr_follow(cfg, b, a, f, 4, None, None, None) == -1


def test_follow_refuses_the_modes_rollout_refuses():
    a = _actor()
    _abi, lib, cfg, b, o = _setup(pool=False, integrator="rk4", rk4_steps_per_m=400, model="compliant")
    _refused(lib, lib.ctr_follow(cfg, b, a, _follow(_abi), 4, o, None, None), b"lane-pair")
    _abi, lib, cfg, b, o = _setup(pool=False, integrator="rk4", rk4_steps_per_m=100, model="rigid")
    _refused(lib, lib.ctr_follow(cfg, b, a, _follow(_abi), 4, o, None, None), b"8-lane group")
    # kernel mode 1 (the compliant model's scipy RK45 with a y pre-curvature): it would spill
    _abi, lib, cfg, b, o = _setup(pool=False)
    cfg.systems[0].Uy[1] = 2.0
    _refused(lib, lib.ctr_follow(cfg, b, a, _follow(_abi), 4, o, None, None), b"y pre-curvature", b"scratch",
             b"ctr_actor + ctr_step")


def test_follow_lds_budget_has_the_byte_counts():
    _abi, lib, cfg, b, o = _setup(pool=False)
    cfg.domain_rand = 0.05
    _refused(lib, lib.ctr_follow(cfg, b, _actor((128, 128, 128)), _follow(_abi), 4, o, None, None),
             b"83584 B", b"78976 B", b"61440 B", b"163840 B")
    # the fixed-step RK4 on the compliant model with a y pre-curvature (mode 3): a larger static LDS
    _abi, lib, cfg, b, o = _setup(pool=False, integrator="rk4", rk4_steps_per_m=100, model="compliant")
    cfg.systems[0].Uy[1] = 2.0
    _refused(lib, lib.ctr_follow(cfg, b, _actor((128, 128, 128)), _follow(_abi), 4, o, None, None),
             b"83584 B", b"90240 B", b"163840 B")


def test_an_empty_batch_is_a_no_op():
    _abi, lib, cfg, b, o = _setup(pool=False)
    empty = _abi.CtrBatch()
    empty.n = 0
    assert lib.ctr_follow(cfg, empty, _actor(), _follow(_abi), 4, _abi.CtrStepOut(), None, None) == 0
    assert lib.ctr_set_goal(cfg, empty, None, 16, 16, None) == 0


def test_set_goal_refuses_bad_arguments():
    _abi, lib, cfg, b, o = _setup(pool=False)
    _refused(lib, lib.ctr_set_goal(cfg, b, None, None, 16, None), b"ctr_set_goal: NULL argument")
    _refused(lib, lib.ctr_set_goal(cfg, b, None, 16, None, None), b"ctr_set_goal: NULL argument")
    _refused(lib, lib.ctr_set_goal(cfg, None, None, 16, 16, None), b"ctr_set_goal: NULL argument")
    _refused(lib, lib.ctr_set_goal(None, b, None, 16, 16, None), b"cfg is NULL")
    b.achieved_goal = None
    _refused(lib, lib.ctr_set_goal(cfg, b, None, 16, 16, None), b"ctr_set_goal: batch buffer missing")
    b.achieved_goal = 16
    b.n = -1
    _refused(lib, lib.ctr_set_goal(cfg, b, None, 16, 16, None), b"batch size out of range")
    b.n = 8
    cfg.n_systems = 0
    _refused(lib, lib.ctr_set_goal(cfg, b, None, 16, 16, None), b"n_systems")


def test_abi_number_and_follow_layout(tmp_path):
    """The two entry points were added within ABI 17; ctr_follow_t as the binding has it."""
    from ctr_reach_amd import _abi
    lib = _abi.load()
    assert lib.ctr_abi_version() == 17 == _abi.CTR_ABI_VERSION
    assert "ctr_follow" in _abi.EXPORTED and "ctr_set_goal" in _abi.EXPORTED
    fields = [name for name, _ in _abi.CtrFollow._fields_]
    assert fields == ["waypoints", "K", "hold", "reach", "pad", "cursor", "held", "tip", "err", "steps", "reached"]
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ctr_reach_amd.h"\nint main(void) {\n'
                    '  printf("%d %zu", CTR_ABI_VERSION, sizeof(ctr_follow_t));\n'
                    + "".join('  printf(" %%zu", offsetof(ctr_follow_t, %s));\n' % f for f in fields)
                    + '  printf("\\n");\n  return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(prog), "-o", str(exe)])
    got = list(map(int, subprocess.check_output([str(exe)]).split()))
    assert got == [17, ctypes.sizeof(_abi.CtrFollow)] + [getattr(_abi.CtrFollow, f).offset for f in fields]


# ---------------------------------------------------------------------------- the path generators
def test_line_path_closed_form_and_endpoints():
    from ctr_reach_amd.paths import line_path
    a, b = np.array([0.01, -0.02, 0.05]), np.array([0.04, 0.03, 0.11])
    p = line_path(a, b, 7)
    assert p.shape == (1, 7, 3) and p.dtype == np.float64
    assert np.array_equal(p[0, 0], a) and np.array_equal(p[0, -1], b)
    for j in range(7):
        assert np.allclose(p[0, j], a + (j / 6.0) * (b - a), rtol=0, atol=1e-17)
    assert np.allclose(np.diff(p[0], axis=0), (b - a) / 6.0, rtol=0, atol=1e-16)     # evenly spaced
    assert np.array_equal(line_path(a, b, 1), b[None, None, :])                       # one waypoint: the end
    assert np.array_equal(line_path(a, b, 2)[0], np.stack((a, b)))
    # batched: a start per path, one end
    starts = np.stack((a, 2 * a, 3 * a))
    q = line_path(starts, b, 5)
    assert q.shape == (3, 5, 3)
    for m in range(3):
        assert np.array_equal(q[m], line_path(starts[m], b, 5)[0])
    with pytest.raises(ValueError):
        line_path(a, b, 0)
    with pytest.raises(ValueError):
        line_path(a[:2], b, 3)


@pytest.mark.parametrize("axis,iu,iv,iw", [("z", 0, 1, 2), ("x", 1, 2, 0), ("y", 2, 0, 1)])
def test_circle_path_closed_form_and_closure(axis, iu, iv, iw):
    from ctr_reach_amd.paths import circle_path
    c, r, K = np.array([0.01, -0.02, 0.1]), 0.03, 9
    p = circle_path(c, r, K, axis)
    assert p.shape == (1, K, 3) and p.dtype == np.float64
    th = 2.0 * np.pi * np.arange(K) / (K - 1)
    assert np.allclose(p[0, :, iu], c[iu] + r * np.cos(th), rtol=0, atol=1e-16)
    assert np.allclose(p[0, :, iv], c[iv] + r * np.sin(th), rtol=0, atol=1e-16)
    assert np.array_equal(p[0, :, iw], np.full(K, c[iw]))                              # in the plane
    assert np.allclose(np.linalg.norm(p[0] - c, axis=1), r, rtol=0, atol=1e-16)
    assert np.array_equal(p[0, -1], p[0, 0])                                           # the circle closes
    start = c.copy()
    start[iu] += r
    assert np.array_equal(p[0, 0], start)
    assert np.array_equal(circle_path(c, r, 1, axis)[0, 0], start)                     # one waypoint: the start
    # quarter points of a 5-waypoint circle
    q = circle_path(c, r, 5, axis)[0] - c
    want = np.zeros((5, 3))
    want[:, iu], want[:, iv] = [r, 0, -r, 0, r], [0, r, 0, -r, 0]
    assert np.allclose(q, want, rtol=0, atol=1e-17)


def test_circle_path_broadcasts_and_refuses():
    from ctr_reach_amd.paths import circle_path
    cs = np.array([[0.0, 0.0, 0.1], [0.01, 0.0, 0.12]])
    p = circle_path(cs, [0.02, 0.03], 6)
    assert p.shape == (2, 6, 3)
    assert np.array_equal(p[1], circle_path(cs[1], 0.03, 6)[0])
    with pytest.raises(ValueError):
        circle_path(cs, 0.02, 6, axis="w")
    with pytest.raises(ValueError):
        circle_path(cs, 0.02, 0)


@pytest.mark.parametrize("axis,iu,iv,iw", [("z", 0, 1, 2), ("x", 1, 2, 0), ("y", 2, 0, 1)])
def test_helix_path_closed_form_and_endpoints(axis, iu, iv, iw):
    from ctr_reach_amd.paths import circle_path, helix_path
    c, r, pitch, turns, K = np.array([0.0, 0.01, 0.08]), 0.02, 0.015, 2.5, 21
    p = helix_path(c, r, pitch, turns, K, axis)
    assert p.shape == (1, K, 3) and p.dtype == np.float64
    rev = turns * np.arange(K) / (K - 1)
    assert np.allclose(p[0, :, iu], c[iu] + r * np.cos(2 * np.pi * rev), rtol=0, atol=1e-16)
    assert np.allclose(p[0, :, iv], c[iv] + r * np.sin(2 * np.pi * rev), rtol=0, atol=1e-16)
    assert np.allclose(p[0, :, iw], c[iw] + pitch * rev, rtol=0, atol=1e-17)
    # the ends: theta = 0 on the centre's level, and two and a half turns later opposite and 2.5 pitches up
    start, end = c.copy(), c.copy()
    start[iu] += r
    end[iu] -= r
    end[iw] += 2.5 * pitch
    assert np.array_equal(p[0, 0], start)
    assert np.allclose(p[0, -1], end, rtol=0, atol=1e-16)
    assert np.array_equal(helix_path(c, r, pitch, turns, 1, axis)[0, 0], start)       # one waypoint: the start
    # pitch 0, one turn: the circle (but for its exact closure)
    assert np.array_equal(helix_path(c, r, 0.0, 1.0, 8, axis)[0, :-1], circle_path(c, r, 8, axis)[0, :-1])
    with pytest.raises(ValueError):
        helix_path(c, r, pitch, turns, 0, axis)


def test_paths_have_dls_ik_path_and_follow_s_shape():
    """[M, K, 3] float64, C-contiguous: what dls_ik_path and follow take."""
    from ctr_reach_amd import paths
    for p in (paths.line_path(np.zeros((4, 3)), np.ones(3), 5), paths.circle_path(np.zeros((4, 3)), 0.1, 5),
              paths.helix_path(np.zeros((4, 3)), 0.1, 0.01, 2, 5, "x")):
        assert p.shape == (4, 5, 3) and p.dtype == np.float64 and p.flags["C_CONTIGUOUS"]


def test_follow_refuses_on_the_host_before_touching_the_device():
    """An env built with autoreset=True (no device needed to say no)."""
    from ctr_reach_amd import CtrReachVecEnv
    e = CtrReachVecEnv(8, device="cpu", autoreset=True, pool_depth=0)
    assert "auto-reset" in e.follow_ineligible()
    with pytest.raises(RuntimeError, match="autoreset=False"):
        e.follow(None, np.zeros((8, 3, 3)), 4)
    assert CtrReachVecEnv(8, device="cpu", autoreset=False).follow_ineligible() is None
