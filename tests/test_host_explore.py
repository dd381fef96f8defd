"""The exploration noise on the host (no GPU): policy.ExploreNoise's numpy Philox against the oracle's,
the distribution of ExploreNoise.emulate (the specification of ctr_explore / ctr_collect's noise),
its key structure, clip and no-op; ctr_explore and ctr_collect refuse bad arguments with CTR_EINVAL
(-1) and a telling ctr_last_error before any HIP call (the device pointers are fake and never
dereferenced); ctr_explore_t's ctypes struct matches the header."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_host_actor import _actor, _setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# sigma = 2^-20 of a box of 2^20: the Gaussian's std is exactly 1 and the clip is out of reach
BIG = np.full(6, 2.0 ** 20, dtype=np.float32)
UNIT = 2.0 ** -20
N_ENV, N_T = 4096, 8


def _noise(*a, **kw):
    from ctr_reach_amd.policy import ExploreNoise
    return ExploreNoise(*a, **kw)


def _grid():
    genv = np.repeat(np.arange(N_ENV), N_T)
    t = np.tile(np.arange(N_T), N_ENV)
    return genv, t


@pytest.fixture(scope="module")
def normals():
    """emulate on zero actions with unit std, genv 0..4095 x t 0..7: [4096, 8, 6] normals."""
    genv, t = _grid()
    z = _noise(UNIT, seed=11).emulate(genv, 3, t, np.zeros((genv.size, 6), dtype=np.float32), BIG)
    return z.reshape(N_ENV, N_T, 6)


def test_numpy_philox_equals_the_oracles(oracle_mod):
    from ctr_reach_amd.policy import philox4x32
    rng = np.random.default_rng(5)
    ctr = rng.integers(0, 2 ** 32, (1000, 4), dtype=np.uint64).astype(np.uint32)
    seed = rng.integers(0, 2 ** 64, 1000, dtype=np.uint64)
    ctr[:4] = [[0, 0, 0, 0], [0xFFFFFFFF] * 4, [1, 0, 0, 6 << 24], [0, 0xFFFFFFFF, 0, 0]]
    seed[:2] = [0, 0xFFFFFFFFFFFFFFFF]
    key = np.stack((seed & np.uint64(0xFFFFFFFF), seed >> np.uint64(32)), axis=-1).astype(np.uint32)
    got = philox4x32(ctr, key)
    want = np.stack([oracle_mod.philox(ctr[i], int(seed[i])) for i in range(1000)])
    assert got.dtype == np.uint32 and np.array_equal(got, want)


def test_gaussian_branch_is_standard_normal(normals):
    from scipy import stats
    z = normals.reshape(-1)
    assert z.size == 196608
    p = stats.kstest(z, "norm").pvalue
    assert p > 1e-3, p
    per_dim = normals.reshape(-1, 6)
    m = per_dim.shape[0]
    assert (np.abs(per_dim.mean(axis=0)) < 5.0 / np.sqrt(m)).all(), per_dim.mean(axis=0)
    assert (np.abs(per_dim.var(axis=0) - 1.0) < 5.0 * np.sqrt(2.0 / m)).all(), per_dim.var(axis=0)


def test_gaussian_dimensions_and_consecutive_steps_are_uncorrelated(normals):
    per_dim = normals.reshape(-1, 6)
    c = np.corrcoef(per_dim.T)
    off = c[~np.eye(6, dtype=bool)]
    assert (np.abs(off) < 5.0 / np.sqrt(per_dim.shape[0])).all(), off
    for d in range(6):
        a, b = normals[:, :-1, d].reshape(-1), normals[:, 1:, d].reshape(-1)
        r = np.corrcoef(a, b)[0, 1]
        assert abs(r) < 5.0 / np.sqrt(a.size), (d, r)


def test_random_branch_share_and_distribution():
    from scipy import stats
    genv, t = _grid()
    nz = _noise(0.1, random_eps=0.25, seed=11)
    scale = np.array([0.001, 0.002, 0.003, 0.1, 0.2, -0.3], dtype=np.float32)
    start = np.full((genv.size, 6), 7.0, dtype=np.float32)            # outside the box: a Gaussian row clips to it
    out = nz.emulate(genv, 3, t, start, scale)
    rnd = nz.last_random
    n = genv.size
    assert abs(rnd.mean() - 0.25) < 5.0 * np.sqrt(0.25 * 0.75 / n), rnd.mean()
    assert (out[~rnd] == np.abs(scale).astype(np.float64)).all()     # the others sit on the box's face
    u = out[rnd] / scale.astype(np.float64)
    assert (np.abs(u) <= 1.0).all()
    assert stats.kstest(u.reshape(-1), stats.uniform(-1, 2).cdf).pvalue > 1e-3
    # float32 values: the random branch is exact
    assert np.array_equal(out[rnd].astype(np.float32).astype(np.float64), out[rnd])


def test_clip_stays_in_the_box_and_noop_keeps_the_bits():
    genv, t = _grid()
    scale = np.array([0.001, 0.002, 0.003, 0.1, 0.2, 0.3], dtype=np.float32)
    rng = np.random.default_rng(1)
    act = (rng.uniform(-1, 1, (genv.size, 6)) * scale).astype(np.float32)
    out = _noise(1.5, seed=2).emulate(genv, 0, t, act, scale)
    assert (np.abs(out) <= scale.astype(np.float64)).all()
    assert ((np.abs(out) == scale.astype(np.float64)).mean(axis=0) > 0.3).all()   # sigma 1.5: about half clip
    act[0, 0], act[1, 1] = -0.0, 5.0                                             # -0 and a value outside the box stay
    nz = _noise(0.0, random_eps=0.0, seed=2)
    same = nz.emulate(genv, 0, t, act, scale)
    assert np.array_equal(same.astype(np.float32).view(np.uint32), act.view(np.uint32))
    assert not nz.last_random.any()


def test_the_key_is_seed_env_epoch_and_clock():
    act = np.zeros((1, 6), dtype=np.float32)
    row = lambda seed=1, genv=5, epoch=2, t=3: _noise(UNIT, seed=seed).emulate(genv, epoch, t, act, BIG)[0]  # noqa: E731
    base = row()
    assert np.array_equal(base, row())
    for other in (row(seed=2), row(genv=6), row(epoch=3), row(t=4), row(genv=5 + 2 ** 32), row(seed=1 + 2 ** 32)):
        assert not (other == base).any()
    # an env's row does not depend on its neighbours in the call
    many = _noise(UNIT, seed=1).emulate(np.arange(10), 2, 3, np.zeros((10, 6), dtype=np.float32), BIG)
    assert np.array_equal(many[5], base)
    # the uniforms are 24-bit fractions in [0, 1)
    u = _noise(UNIT, seed=1).uniforms(np.arange(1000), 0, 0)
    assert u.dtype == np.float32 and u.shape == (1000, 7) and (u >= 0).all() and (u < 1).all()
    assert np.array_equal(u * np.float32(2 ** 24), np.floor(u * np.float32(2 ** 24)))


def test_explore_noise_validates_its_arguments():
    for bad in (-0.1, float("nan"), float("inf"), [0.1] * 5):
        with pytest.raises(ValueError):
            _noise(bad)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            _noise(0.1, random_eps=bad)
    nz = _noise([0.1, 0.2, 0.3, 0.4, 0.5, 0.6], random_eps=1.0, seed=2 ** 64 + 3)
    assert nz.seed == 3 and nz._struct.seed == 3
    assert list(nz._struct.sigma) == [float(v) for v in np.float32([0.1, 0.2, 0.3, 0.4, 0.5, 0.6])]
    assert (_noise(0.25).sigma == np.float32(0.25)).all() and _noise(0.25).sigma.shape == (6,)


def _explore(sigma=0.3, eps=0.1):
    from ctr_reach_amd import _abi
    x = _abi.CtrExplore()
    x.seed, x.random_eps = 9, eps
    for i in range(6):
        x.sigma[i] = sigma
    return x


def _scale(v=0.5):
    return (ctypes.c_float * 6)(*([v] * 6))


def test_ctr_explore_validates_arguments_without_gpu():
    _abi, lib, cfg, b, o = _setup()
    fake = ctypes.c_void_p(16)

    def refused(word, b=b, x=_explore(), scale=_scale(), actions=fake):
        assert lib.ctr_explore(b, x, scale, actions, None) == -1, word
        assert word in lib.ctr_last_error(), (word, lib.ctr_last_error())

    refused(b"batch is NULL", b=None)
    refused(b"NULL argument", x=None)
    refused(b"NULL argument", scale=None)
    refused(b"actions", actions=None)
    for bad in (-0.5, float("nan"), float("inf")):
        refused(b"sigma", x=_explore(sigma=bad))
    for bad in (-0.01, 1.01, float("nan")):
        refused(b"random_eps", x=_explore(eps=bad))
    for bad in (float("nan"), float("-inf")):
        refused(b"scale", scale=_scale(bad))
    nb = _abi.CtrBatch()
    nb.n = 8
    nb.t = fake
    refused(b"epoch", b=nb)
    nb.n = -1
    refused(b"out of range", b=nb)
    assert lib.ctr_explore(_abi.CtrBatch(), _explore(), _scale(), None, None) == 0      # an empty batch


def _her(_abi, b, cfg, **kw):
    h = _abi.CtrHer()
    h.obs_dim, h.t_max, h.n_sampled_goal, h.strategy, h.slots = 13, cfg.max_steps, 4, 0, 3
    h.n, h.env_base = b.n, b.env_base
    for name in ("state", "step", "dg", "tol", "len", "epoch", "cur_t", "cur_epoch", "cdf"):
        setattr(h, name, 1 << 12)
    for k, v in kw.items():
        setattr(h, k, v)
    return h


def test_ctr_collect_validates_arguments_without_gpu():
    _abi, lib, cfg, b, o = _setup()
    a = _actor()
    P = _abi.AUTORESET_POOLED

    def refused(word, cfg=cfg, b=b, a=a, x=None, her=None, k=4, o=o, mode=P, aux=None):
        her = _her(_abi, b, cfg) if her is None else her
        assert lib.ctr_collect(cfg, b, a, x, her, k, o, mode, aux, None) == -1, word
        assert word in lib.ctr_last_error(), (word, lib.ctr_last_error())

    # ctr_rollout's refusals, with its messages
    refused(b"in_dim", a=_actor(in_dim=20))
    for k in (0, _abi.CTR_STEP_MANY_MAX + 1):
        refused(b"CTR_STEP_MANY_MAX", k=k)
    refused(b"CTR_AUTORESET_OFF or CTR_AUTORESET_POOLED", mode=_abi.AUTORESET_SWEEP)
    refused(b"lane-pair", cfg=_setup(integrator="rk4", rk4_steps_per_m=400, model="compliant")[2])
    refused(b"8-lane group", cfg=_setup(integrator="rk4", rk4_steps_per_m=100, model="rigid")[2])
    aux = _abi.CtrRolloutAux()
    aux.episodes = 16
    refused(b"statistics", mode=_abi.AUTORESET_OFF, aux=aux)
    uy = _setup()[2]
    uy.systems[0].Uy[0] = 5.0
    refused(b"scratch", cfg=uy)
    dr = _setup()[2]
    dr.domain_rand = 0.05
    refused(b"LDS", cfg=dr, a=_actor((128, 128, 128)))
    bad_actor = _actor()
    bad_actor.scale[2] = float("nan")
    refused(b"scale", a=bad_actor)
    # ctr_step_her's checks of the store
    assert lib.ctr_collect(cfg, b, a, None, None, 4, o, P, None, None) == -1 and b"her is NULL" in lib.ctr_last_error()
    refused(b"t_max", her=_her(_abi, b, cfg, t_max=cfg.max_steps + 1))
    refused(b"sizes differ", her=_her(_abi, b, cfg, n=b.n + 1))
    refused(b"env_base differ", her=_her(_abi, b, cfg, env_base=64))
    refused(b"buffer missing", her=_her(_abi, b, cfg, cur_t=None))
    refused(b"slots", her=_her(_abi, b, cfg, slots=1))
    # ctr_explore's checks of the noise
    refused(b"sigma", x=_explore(sigma=-1.0))
    refused(b"sigma", x=_explore(sigma=float("nan")))
    refused(b"random_eps", x=_explore(eps=2.0))
    for args in ((None, b, a), (cfg, None, a), (cfg, b, None)):
        assert lib.ctr_collect(args[0], args[1], args[2], None, _her(_abi, b, cfg), 4, o, P, None, None) == -1
    assert lib.ctr_collect(cfg, b, a, None, _her(_abi, b, cfg), 4, None, P, None, None) == -1
    # an empty batch with an empty store is a no-op
    nb = _abi.CtrBatch()
    assert lib.ctr_collect(cfg, nb, a, _explore(), _her(_abi, nb, cfg), 4, o, P, None, None) == 0


def test_explore_struct_layout_matches_header(tmp_path):
    """ctypes.sizeof(CtrExplore) and every field offset equal ctr_explore_t's (gcc, the header as C11)."""
    from ctr_reach_amd import _abi
    lines, want = ['  printf("%zu\\n", sizeof(ctr_explore_t));', '  printf("%d\\n", CTR_ABI_VERSION);'], \
        [ctypes.sizeof(_abi.CtrExplore), _abi.CTR_ABI_VERSION]
    for fname, _ in _abi.CtrExplore._fields_:
        lines.append('  printf("%%zu\\n", offsetof(ctr_explore_t, %s));' % fname)
        want.append(getattr(_abi.CtrExplore, fname).offset)
    prog = tmp_path / "explore_layout.c"
    prog.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"ctr_reach_amd.h\"\nint main(void) {\n"
                    + "\n".join(lines) + "\n  return 0; }\n")
    exe = tmp_path / "explore_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(prog), "-o", str(exe)])
    assert list(map(int, subprocess.check_output([str(exe)]).split())) == want
    assert ctypes.sizeof(_abi.CtrExplore) == 40 and _abi.CTR_ABI_VERSION == 17
    lib = _abi.load()
    assert lib.ctr_abi_version() == 17 and hasattr(lib, "ctr_explore") and hasattr(lib, "ctr_collect")
