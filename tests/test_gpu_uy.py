"""Every GPU entry point with a y pre-curvature (the kernels' MODE bit 1, HAS_UY) against the
oracle.  The registered systems have U_y = 0, so the other GPU-vs-oracle tests run the HAS_UY =
false instantiations; the fused-period tests reach HAS_UY = true but only compare kernels with
each other.  The oracle's own U_y path is pinned in test_oracle_uy.py (rotation identity under
fixed-step RK4, RK45 against fine RK4), which also provides the two parameter sets used here:
``rotated_systems`` (every tube's pre-curvature turned about z) and ``uy_systems`` (U_y on tubes
0 and 1 only: mixed zero / nonzero).

Bars are the ones the U_y = 0 tests hold for the same operation (test_gpu_modes.py, test_gpu_parity
/ test_gpu_domain_rand.py, test_gpu_shape.py, test_gpu_jacobian.py).  Each test also runs the registered U_y = 0 systems on the
same rows as a control and prints both maxima; the docstrings record them as measured on an
MI355X (control / U_y != 0, the larger of the two parameter sets).  Deliberately negating the wy
terms of rhs_core moves every one of these rows' tips by 2e-7 m to 0.33 m (median 7e-3 m with
uy_systems, 7e-2 m with rotated_systems; the same mutation made in the oracle), in all five modes;
negating them for the rigid model only does the same in the two rigid modes.
"""
import os

import numpy as np
import pytest

from test_oracle_uy import PHI, mixed_rows, rotated_systems, uy_systems

# (the shared rows are read-only numpy arrays, which torch.as_tensor warns about before it copies them)
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

SEL = [0, 1, 2, 3]
SETS = {"rotated": rotated_systems, "uy": uy_systems}
# kernel modes 1, 3, 3, 5, 7 with U_y != 0
MODES = [("rk45_scipy", 100, "compliant"), ("rk4", 100, "compliant"), ("rk4", 400, "compliant"),
         ("rk45_scipy", 100, "rigid"), ("rk4", 100, "rigid")]
MODE_IDS = ["rk45_compliant", "rk4_100_compliant", "rk4_400_compliant", "rk45_rigid", "rk4_100_rigid"]
N = 2051          # no multiple of 256 (lanes per workgroup), of 36 (Jacobian envs) or of 9 (IK envs)


def _bar(integrator):
    return 1e-10 if integrator == "rk45_scipy" else 1e-11


def _env(cuda, params, n=1, **kw):
    from ctr_reach_amd import CtrReachVecEnv
    if params is not None:
        kw["ctr_systems_parameters"] = params
    return CtrReachVecEnv(n, device=cuda, select_systems=SEL, **kw)


def _solver(integrator, spm, model):
    return dict(integrator=integrator, rk4_steps_per_m=spm, model=model)


def _okw(integrator, spm, model):
    return dict(integrator=integrator, steps_per_m=spm, model=model)


@pytest.fixture(scope="module")
def rows(oracle_mod, golden_dir):
    """2 051 sampled rows over the four systems, +-10 rad angle offsets on every other one
    (test_gpu_modes._joints' offsets), then fk_edge.npz's 68 joints (ties, limits, reversed spans):
    2 119 rows.  Read-only."""
    q, sysid = mixed_rows(oracle_mod, N, 83)
    rng = np.random.default_rng(84)
    q[::2, 3:] += rng.uniform(-10, 10, (len(q[::2]), 3)).astype(np.float32)
    d = np.load(os.path.join(golden_dir, "fk_edge.npz"))
    q = np.concatenate((q, d["joints"].astype(np.float32)))
    sysid = np.concatenate((sysid, d["system"].astype(np.int32)))
    q.setflags(write=False)
    sysid.setflags(write=False)
    return q, sysid


def _check_fk(tip, st, ref, integrator, model):
    """test_gpu_modes.test_fk_modes_vs_oracle's assertions; returns the max tip difference."""
    err = np.linalg.norm(tip.cpu().numpy() - ref["tip"], axis=1).max()
    assert (st["status"].cpu().numpy() == 0).all() and (ref["status"] == 0).all()
    if integrator == "rk4":
        np.testing.assert_array_equal(st["nfev"].cpu().numpy(), ref["nfev"])
        if model == "rigid":
            assert (st["maps"].cpu().numpy() > 0).all()
    return err


@pytest.mark.parametrize("integrator,spm,model", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("which", sorted(SETS))
def test_fk_vs_oracle(cuda, oracle_mod, rows, which, integrator, spm, model):
    """ctr_fk in the five modes.  Measured max |gpu - oracle| (control / U_y): RK45 compliant
    1.4e-12 / 1.7e-12 m, rigid 7.6e-13 / 6.1e-13 m; RK4/100 compliant 1.7e-16 / 1.9e-16 m, RK4/400
    6.2e-16 / 4.7e-16 m, RK4/100 rigid 2.3e-16 / 2.2e-16 m."""
    q, sysid = rows
    errs = {}
    for name, params in (("control", None), (which, SETS[which]())):
        env = _env(cuda, params, **_solver(integrator, spm, model))
        tip, st = env.forward_kinematics(q, sysid, return_stats=True)
        ref = oracle_mod.fk(q, sysid, systems=oracle_mod.make_systems(params, select=SEL), **_okw(integrator, spm, model))
        errs[name] = _check_fk(tip, st, ref, integrator, model)
    print("fk %s %s: max |gpu - oracle| control %.3g m, U_y %.3g m" % (which, (integrator, spm, model),
                                                                      errs["control"], errs[which]))
    assert errs["control"] < _bar(integrator), errs
    assert errs[which] < _bar(integrator), errs


def _tables(oracle_mod, params, m, sysid, seed, turn=True):
    """Per-row tables from ``params``: row e is system sysid[e] with every tube's (U_x, U_y)
    scaled by its own factor in [0.9, 1.1] and (``turn``) turned by its own angle.  Returns
    ([m, 18] float64 in ctr_system_t order L, Lc, EI, GJ, Ux, Uy; the OracleSystem array holding
    the same bits: E = EI, I = 1, G = GJ, J = 1).  params = None, turn = False: the U_y = 0
    control (U_x scaled only)."""
    import oracle
    nom = oracle_mod.make_systems(params, select=SEL)
    tab = np.zeros((4, 6, 3))
    for k in range(4):
        for i in range(3):
            tab[k, :, i] = (nom[k].L[i], nom[k].Lc[i], nom[k].E[i] * nom[k].I[i], nom[k].G[i] * nom[k].J[i],
                            nom[k].Ux[i], nom[k].Uy[i])
    t = tab[sysid].copy()                                     # [m, 6, 3]
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.9, 1.1, (m, 3))
    th = rng.uniform(-np.pi, np.pi, (m, 3)) * (1.0 if turn else 0.0)
    ux, uy = t[:, 4].copy(), t[:, 5].copy()
    t[:, 4] = f * (np.cos(th) * ux - np.sin(th) * uy)
    t[:, 5] = f * (np.sin(th) * ux + np.cos(th) * uy)
    ds = (oracle.OracleSystem * m)()
    v = np.frombuffer(ds, dtype=np.float64).reshape(m, 8, 3)  # L, Lc, E, G, I, J, Ux, Uy
    v[:, 0], v[:, 1], v[:, 2], v[:, 3] = t[:, 0], t[:, 1], t[:, 2], t[:, 3]
    v[:, 4] = 1.0
    v[:, 5] = 1.0
    v[:, 6], v[:, 7] = t[:, 4], t[:, 5]
    return np.ascontiguousarray(t.reshape(m, 18)), ds


@pytest.mark.parametrize("integrator,spm,model", MODES, ids=MODE_IDS)
def test_fk_tables_vs_oracle(cuda, oracle_mod, rows, integrator, spm, model):
    """ctr_fk_tables with a nonzero U_y in every row, all five modes (the suite's other tables
    have U_y = 0: randomize_value of 0 is 0).  Measured max |gpu - oracle| (control / U_y): RK45
    compliant 1.4e-12 / 2.1e-12 m, rigid 8.1e-13 / 5.0e-13 m; RK4/100 compliant 1.4e-16 / 1.2e-16 m,
    RK4/400 1.1e-15 / 2.8e-16 m, RK4/100 rigid 1.7e-16 / 1.7e-16 m."""
    import torch
    q, sysid = rows
    m = len(q)
    idx = np.arange(m, dtype=np.int32)
    env = _env(cuda, None, **_solver(integrator, spm, model))
    errs = {}
    for name, (tab, ds) in (("control", _tables(oracle_mod, None, m, sysid, 85, turn=False)),
                            ("U_y", _tables(oracle_mod, rotated_systems(), m, sysid, 85))):
        assert (tab[:, 15:18] != 0).all() == (name == "U_y") and (tab[:, 15:18] != 0).any() == (name == "U_y")
        tip, st = env.forward_kinematics(q, tables=torch.tensor(tab, device=cuda), return_stats=True)
        ref = oracle_mod.fk(q, idx, systems=ds, **_okw(integrator, spm, model))
        errs[name] = _check_fk(tip, st, ref, integrator, model)
    print("fk tables %s: max |gpu - oracle| control %.3g m, U_y %.3g m" % ((integrator, spm, model), errs["control"],
                                                                         errs["U_y"]))
    assert errs["control"] < _bar(integrator), errs
    assert errs["U_y"] < _bar(integrator), errs


def _check_shape(out, ref):
    """test_gpu_shape.test_shape_batch_vs_oracle's bars; returns max |dr|."""
    np.testing.assert_array_equal(out["npts"].cpu().numpy(), ref["npts"])
    np.testing.assert_allclose(out["s"].cpu().numpy(), ref["s"], rtol=0, atol=1e-15)
    r = out["r"].cpu().numpy()
    assert np.array_equal(np.isnan(r), np.isnan(ref["r"]))
    return np.nanmax(np.abs(r - ref["r"]))


def _bits(t):
    return t.cpu().numpy().view(np.int64)


@pytest.mark.parametrize("model", ["compliant", "rigid"])
@pytest.mark.parametrize("which", sorted(SETS))
def test_shape_vs_oracle(cuda, oracle_mod, rows, which, model):
    """ctr_fk_shape by system index and by per-row tables (no other test passes it tables).
    Measured max |dr| (control / U_y): compliant 1.8e-12 / 1.5e-12 m by index, 8.9e-13 / 1.8e-12 m
    by tables; rigid 1.1e-12 / 9.0e-13 m by index, 8.0e-13 / 9.9e-13 m by tables."""
    import torch
    q, sysid = rows
    m = len(q)
    idx = np.arange(m, dtype=np.int32)
    env = _env(cuda, None, model=model)       # (the tables replace the env's systems)
    errs = {}
    for name, params in (("control", None), (which, SETS[which]())):
        ref = oracle_mod.fk_shape(q, sysid, systems=oracle_mod.make_systems(params, select=SEL), model=model)
        errs[name] = _check_shape(_env(cuda, params, model=model).forward_kinematics_shape(q, sysid), ref)
        tab, ds = _tables(oracle_mod, params, m, sysid, 86, turn=params is not None)
        ref = oracle_mod.fk_shape(q, idx, systems=ds, model=model)
        errs[name + " tables"] = _check_shape(env.forward_kinematics_shape(q, tables=torch.tensor(tab, device=cuda)), ref)
    print("shape %s %s: max |dr| " % (which, model) + ", ".join("%s %.3g m" % kv for kv in errs.items()))
    for k, v in errs.items():
        assert v < 1e-10, errs


@pytest.mark.parametrize("model", ["compliant", "rigid"])
@pytest.mark.parametrize("which", sorted(SETS))
def test_shape_cap_below_the_point_count(cuda, rows, which, model):
    """cap = 100 on rows of 120 to 180 points: the points past cap are not stored.  r and s are
    [M, cap, 3] and [M, cap] contiguous, so a store past cap would land in the next row, at points
    0 .. npts - 101.  The next row would overwrite (or race with) the points it stores itself, so
    every big row is followed by a one-segment row (30 points; fk_edge.npz has eight): a big row
    of 150 or 180 points would hit that row's NaN tail.  Every row is compared bit for bit with
    the first 100 points of the cap = 270 run."""
    import torch
    q, sysid = rows
    env = _env(cuda, SETS[which](), model=model)
    npts = env.forward_kinematics_shape(q, sysid)["npts"].cpu().numpy()
    big = np.nonzero((npts >= 120) & (npts <= 180))[0][:192]
    small = np.nonzero(npts == 30)[0]
    assert len(big) == 192 and len(small) >= 4
    assert (npts[big] == 120).sum() > 10 and (npts[big] >= 150).sum() > 100
    pick = np.stack((big, small[np.arange(192) % len(small)]), axis=1).reshape(-1)
    a = env.forward_kinematics_shape(q[pick], sysid[pick], cap=270)
    b = env.forward_kinematics_shape(q[pick], sysid[pick], cap=100)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(a["npts"].cpu().numpy(), npts[pick])
    np.testing.assert_array_equal(b["npts"].cpu().numpy(), npts[pick])           # the full count
    np.testing.assert_array_equal(b["status"].cpu().numpy(), a["status"].cpu().numpy())
    np.testing.assert_array_equal(_bits(b["tip"]), _bits(a["tip"]))
    assert b["r"].shape == (len(pick), 100, 3) and b["s"].shape == (len(pick), 100)
    np.testing.assert_array_equal(_bits(b["r"]), _bits(a["r"][:, :100].contiguous()))
    np.testing.assert_array_equal(_bits(b["s"]), _bits(a["s"][:, :100].contiguous()))
    rb = b["r"].cpu().numpy()
    assert np.isfinite(rb[0::2]).all() and np.isfinite(rb[1::2, :30]).all() and np.isnan(rb[1::2, 30:]).all()


JAC_MODES = [("rk45_scipy", 100, "compliant"), ("rk4", 100, "rigid")]     # kernel modes 1 and 7


def _jac_rows(rows):
    q, sysid = rows
    q64 = q.astype(np.float64)
    q64[:, :3] = np.minimum(q64[:, :3], -2e-4)
    return q64, sysid


@pytest.mark.parametrize("integrator,spm,model", JAC_MODES, ids=["rk45_compliant", "rk4_100_rigid"])
@pytest.mark.parametrize("which", sorted(SETS))
def test_jacobian_vs_oracle(cuda, oracle_mod, rows, which, integrator, spm, model):
    """test_gpu_jacobian.test_jacobian_batch_vs_oracle's bars.  Measured (control / U_y): RK45
    compliant max |dtip| 1.0e-12 / 1.3e-12 m, max |dJ| 1.5e-8 / 5.0e-8 (bar 2e-6), entries within
    1e-8: 99.984 % / 99.953 %; RK4 rigid 2.2e-16 / 2.2e-16 m, 2.8e-12 / 3.9e-12, all entries."""
    q64, sysid = _jac_rows(rows)
    res = {}
    for name, params in (("control", None), (which, SETS[which]())):
        env = _env(cuda, params, **_solver(integrator, spm, model))
        tip, jac = env.jacobian(q64, sysid)
        rt, rj = oracle_mod.jacobian(q64, sysid, systems=oracle_mod.make_systems(params, select=SEL),
                                     **_okw(integrator, spm, model))
        dj = np.abs(jac.cpu().numpy() - rj)
        res[name] = (np.abs(tip.cpu().numpy() - rt).max(), dj.max(), (dj < 1e-8).mean())
    print("jacobian %s %s: (max |dtip|, max |dJ|, share of |dJ| < 1e-8) control %.3g %.3g %.5f, U_y %.3g %.3g %.5f"
          % ((which, (integrator, spm, model)) + res["control"] + res[which]))
    for name in ("control", which):
        dt, dj, share = res[name]
        assert dt < 1e-10, res
        assert dj < 2e-10 / 1e-4, res
        assert share > 0.999, res


@pytest.mark.parametrize("integrator,spm,model", JAC_MODES, ids=["rk45_compliant", "rk4_100_rigid"])
@pytest.mark.parametrize("which", sorted(SETS))
def test_ik_one_step_vs_oracle(cuda, oracle_mod, rows, which, integrator, spm, model):
    """One fused DLS step against the host update from the oracle's (p, J): test_gpu_jacobian's
    95 % cap (the FK is piecewise smooth; the oracle alone decides the rows that branch).
    Measured (control / U_y): RK45 compliant 99.72 % / 99.43 % of rows within 1e-9 (95th percentile
    1.5e-10 / 1.6e-10), max |err - |e|| 1.3e-12 / 1.4e-12 m; RK4 rigid all rows (2.4e-13 / 2.4e-13),
    1.7e-16 / 1.4e-16 m."""
    q64, sysid = _jac_rows(rows)
    m = len(q64)
    lam = 0.25
    res = {}
    for name, params in (("control", None), (which, SETS[which]())):
        sy = oracle_mod.make_systems(params, select=SEL)
        # targets: the tips of the rows taken in reverse order within each system
        targets = np.zeros((m, 3))
        for s in range(4):
            k = np.nonzero(sysid == s)[0]
            targets[k] = oracle_mod.jacobian(q64[k[::-1]], sysid[k], systems=sy, **_okw(integrator, spm, model))[0]
        p, jac = oracle_mod.jacobian(q64, sysid, systems=sy, **_okw(integrator, spm, model))
        e = targets - p
        jjt = jac @ jac.transpose(0, 2, 1) + lam * np.eye(3)
        want = q64 + (jac.transpose(0, 2, 1) @ np.linalg.solve(jjt, e[..., None]))[..., 0]
        env = _env(cuda, params, **_solver(integrator, spm, model))
        q, err, iters, status = env.ik_dls(targets, q64, sysid, lam=lam, num=1)
        dq = np.abs(q.cpu().numpy() - want).max(axis=1)
        de = np.abs(err.cpu().numpy() - np.linalg.norm(e, axis=1)).max()
        assert (iters.cpu().numpy() == 1).all() and (status.cpu().numpy() & 4 == 0).all()
        res[name] = ((dq < 1e-9).mean(), np.quantile(dq, 0.95), de)
    print("ik %s %s: (share dq < 1e-9, p95 dq, max |err - |e||) control %.4f %.3g %.3g, U_y %.4f %.3g %.3g"
          % ((which, (integrator, spm, model)) + res["control"] + res[which]))
    for name in ("control", which):
        share, _, de = res[name]
        assert share >= 0.95, res
        assert de < 1e-10, res


def _reset_and_steps(cuda, oracle_mod, params, integrator, spm, model, n=1024):
    """reset() and three steps against the oracle (test_gpu_modes.test_step_modes_vs_oracle's
    assertions); returns the max goal / achieved-goal difference."""
    import torch
    env = _env(cuda, params, n=n, seed=5, autoreset=False, **_solver(integrator, spm, model))
    env.enable_nfev()
    env.reset()
    torch.cuda.synchronize()
    sy = oracle_mod.make_systems(params, select=SEL)
    okw = _okw(integrator, spm, model)
    sysid = env.system.cpu().numpy()
    worst = 0.0
    for got, joints in ((env.desired_goal, env.desired_joints), (env.achieved_goal, env.joints)):
        ref = oracle_mod.fk(joints.cpu().numpy(), sysid, systems=sy, **okw)["tip"]
        worst = max(worst, np.abs(got.cpu().numpy() - ref).max())
    rng = np.random.default_rng(3)
    hi = env.action_space.high
    for _ in range(3):
        q = env.joints.cpu().numpy()
        dg = env.desired_goal.cpu().numpy()
        t = env.t.cpu().numpy()
        a = ((rng.random((n, 6)) * 2 - 1) * hi).astype(np.float32)
        obs, rew, done, info = env.step(torch.tensor(a, device=cuda))
        torch.cuda.synchronize()
        ref = oracle_mod.step(q, a, dg, t, env.goal_tolerance.get_tol(), system=sysid, systems=sy, multi=True, **okw)
        np.testing.assert_array_equal(env.joints.cpu().numpy(), ref["joints"])
        worst = max(worst, np.abs(env.achieved_goal.cpu().numpy() - ref["achieved_goal"]).max())
        np.testing.assert_array_equal(rew.cpu().numpy(), ref["reward"].astype(np.float32))
        np.testing.assert_array_equal(done.cpu().numpy(), ref["done"])
        assert np.abs(obs["observation"].cpu().numpy() - ref["observation"]).max() < 1e-6
        if integrator == "rk4":
            assert (env.nfev.cpu().numpy() == ref["nfev"]).mean() > 0.999
        if done.any():
            break
    return worst


@pytest.mark.parametrize("integrator,spm,model", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("which", sorted(SETS))
def test_reset_and_steps_vs_oracle(cuda, oracle_mod, which, integrator, spm, model):
    """reset() and three steps of 1 024 envs in the five modes (mode 3 is the one-lane RK4 step,
    mode 7 the 8-lane group step).  Measured max |goal - oracle| (control / U_y): RK45 compliant
    2.9e-12 / 2.8e-12 m, rigid 6.8e-13 / 6.4e-13 m; RK4/100 compliant 1.7e-16 / 1.7e-16 m, RK4/400
    2.2e-16 / 3.5e-16 m, RK4/100 rigid 1.7e-16 / 2.2e-16 m."""
    control = _reset_and_steps(cuda, oracle_mod, None, integrator, spm, model)
    uy = _reset_and_steps(cuda, oracle_mod, SETS[which](), integrator, spm, model)
    print("step %s %s: max |goal - oracle| control %.3g m, U_y %.3g m" % (which, (integrator, spm, model), control, uy))
    assert control < _bar(integrator), (control, uy)
    assert uy < _bar(integrator), (control, uy)


def test_domain_rand_steps_vs_oracle(cuda, oracle_mod):
    """Domain randomisation on the rotated systems: U_y is kept (model_utils.py re-samples E, G,
    U_x and the diameters), so every env's table has U_y != 0 next to a re-sampled U_x.
    test_gpu_domain_rand.test_reset_and_steps_vs_oracle's assertions.  Measured max |goal -
    oracle| (control / U_y): 3.2e-12 / 1.8e-12 m."""
    import torch
    n, rand = 1024, 0.05
    worst = {}
    for name, params in (("control", None), ("U_y", rotated_systems())):
        env = _env(cuda, params, n=n, seed=22, autoreset=False, domain_rand=rand)
        env.reset()
        torch.cuda.synchronize()
        ds = oracle_mod.domain_systems(n, rand, seed=env.seed_value, epoch=env.epoch.cpu().numpy(),
                                       env_base=env.env_base, system=env.system.cpu().numpy(), params=params,
                                       select=SEL)
        uy = env.domain_parameters()["U_y"].cpu().numpy()
        np.testing.assert_array_equal(uy, np.array([[ds[i].Uy[j] for j in range(3)] for i in range(n)]))
        assert (uy != 0).all() == (name == "U_y")
        idx = np.arange(n, dtype=np.int32)
        dg = oracle_mod.fk(env.desired_joints.cpu().numpy(), idx, systems=ds)["tip"]
        ag = oracle_mod.fk(env.joints.cpu().numpy(), idx, systems=ds)["tip"]
        w = max(np.abs(env.desired_goal.cpu().numpy() - dg).max(), np.abs(env.achieved_goal.cpu().numpy() - ag).max())
        rng = np.random.default_rng(6)
        for _ in range(3):
            q = env.joints.cpu().numpy()
            t = env.t.cpu().numpy()
            a = ((rng.random((n, 6)) * 2 - 1) * env.action_space.high).astype(np.float32)
            obs, rew, done, info = env.step(torch.tensor(a, device=cuda))
            torch.cuda.synchronize()
            ref = oracle_mod.step(q, a, dg, t, env.goal_tolerance.get_tol(), system=idx, systems=ds)
            np.testing.assert_array_equal(env.joints.cpu().numpy(), ref["joints"])
            w = max(w, np.abs(env.achieved_goal.cpu().numpy() - ref["achieved_goal"]).max())
            np.testing.assert_array_equal(rew.cpu().numpy(), ref["reward"].astype(np.float32))
            np.testing.assert_array_equal(done.cpu().numpy(), ref["done"])
            assert np.abs(obs["observation"].cpu().numpy()[:, :13] - ref["observation"]).max() < 1e-6
        worst[name] = w
    print("domain rand: max |goal - oracle| control %.3g m, U_y %.3g m" % (worst["control"], worst["U_y"]))
    assert worst["control"] < 1e-10 and worst["U_y"] < 1e-10, worst


@pytest.mark.parametrize("model", ["compliant", "rigid"])
def test_rotation_identity_on_the_gpu(cuda, oracle_mod, rows, model):
    """The HAS_UY = true kernel on the rotated systems at q against the HAS_UY = false kernel on
    the registered systems at q + PHI (test_oracle_uy.py's identity), fixed-step RK4 over float64
    joints.  Each side is within 1e-11 m of the oracle and the oracle's pair agrees to 1e-13 m:
    2.1e-11 m.  Measured: 1.2e-15 m compliant, 1.6e-15 m rigid."""
    q, sysid = rows
    q64 = q.astype(np.float64)
    shift = np.concatenate((np.zeros(3), PHI))
    kw = _solver("rk4", 100, model)
    a = _env(cuda, rotated_systems(), **kw).jacobian(q64, sysid)[0].cpu().numpy()
    b = _env(cuda, None, **kw).jacobian(q64 + shift, sysid)[0].cpu().numpy()
    o = oracle_mod.jacobian(q64, sysid, systems=oracle_mod.make_systems(rotated_systems(), select=SEL),
                            **_okw("rk4", 100, model))[0]
    d = np.linalg.norm(a - b, axis=1).max()
    print("rotation %s: max |rotated(q) - registered(q + phi)| = %.3g m, |rotated - oracle| = %.3g m"
          % (model, d, np.linalg.norm(a - o, axis=1).max()))
    assert np.isfinite(a).all()
    assert d < 2.1e-11, d
