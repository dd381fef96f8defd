"""The MLP actor on the host (no GPU): ctr_actor_blob_bytes, ctr_actor_pack, ctr_actor and ctr_rollout
refuse bad arguments with CTR_EINVAL (-1) and a telling ctr_last_error before any HIP call (the
device pointers are fake and never dereferenced); the packed blob holds bf16(W) and b where the
header says; the ctypes structs match the header; MlpActor.emulate is the specification."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _actor(hidden=(64, 64), in_dim=19):
    from ctr_reach_amd import _abi
    a = _abi.CtrActor()
    a.in_dim, a.n_hidden = in_dim, len(hidden)
    for l, w in enumerate(hidden):
        a.width[l] = w
    for i in range(6):
        a.scale[i] = 0.5
    a.blob = 1 << 20
    return a


def _setup(pool=True, n_systems=1, **solver):
    from ctr_reach_amd import _abi, systems
    lib = _abi.load()
    codes = systems.solver_codes(solver.get("integrator", "rk45_scipy"), solver.get("rk4_steps_per_m", 100),
                                 solver.get("model", "compliant"))
    cfg = systems.make_config(systems.tubes_from_params(systems.default_systems_parameters())[:n_systems],
                              integrator=codes[0], rk4_steps_per_m=codes[1], model=codes[2])
    fake = ctypes.c_void_p(16)
    b = _abi.CtrBatch()
    b.n = 8
    b.joints = b.desired_goal = b.achieved_goal = b.t = b.system = b.epoch = b.work = fake
    if pool:
        b.pool_depth, b.pool, b.refill, b.refill_cap = 4, ctypes.c_void_p(128), fake, 64
    o = _abi.CtrStepOut()
    o.obs = o.reward = o.done = o.success = o.error = fake
    return _abi, lib, cfg, b, o


def _all_refuse(actor, word):
    """The four entry points refuse `actor` (ctr_actor_blob_bytes and ctr_actor_pack read only its
    shape: `word` None = they accept it)."""
    _abi, lib, cfg, b, o = _setup()
    calls = [("ctr_actor", lambda: lib.ctr_actor(actor, 16, 8, 16, None, None)),
             ("ctr_rollout", lambda: lib.ctr_rollout(cfg, b, actor, 4, o, _abi.AUTORESET_POOLED, None, None))]
    for name, call in calls:
        assert call() == -1, name
        assert word in lib.ctr_last_error(), (name, lib.ctr_last_error())


def _shape_refuse(actor, word):
    _abi, lib, cfg, b, o = _setup()
    assert lib.ctr_actor_blob_bytes(actor) == -1
    assert word in lib.ctr_last_error(), lib.ctr_last_error()
    W = (ctypes.c_void_p * 4)(16, 16, 16, 16)
    assert lib.ctr_actor_pack(actor, W, W, 16) == -1
    assert word in lib.ctr_last_error(), lib.ctr_last_error()
    _all_refuse(actor, word)


def test_actor_shapes_are_validated():
    for nh in (0, 4):
        a = _actor()
        a.n_hidden = nh
        _shape_refuse(a, b"n_hidden")
    for w in (0, 48, 288):
        a = _actor((64, w))
        _shape_refuse(a, b"width")
    for d in (18, 21):
        _shape_refuse(_actor(in_dim=d), b"in_dim")
    _abi, lib, cfg, b, o = _setup()
    assert lib.ctr_actor_blob_bytes(None) == -1
    assert lib.ctr_actor(None, 16, 8, 16, None, None) == -1
    assert lib.ctr_rollout(cfg, b, None, 4, o, _abi.AUTORESET_POOLED, None, None) == -1


def test_actor_lds_budget_and_blob_sizes():
    _abi, lib, cfg, b, o = _setup()
    assert _abi.CTR_ACTOR_MAX_BYTES == 98304
    assert lib.ctr_actor_blob_bytes(_actor((128, 128, 128))) == 81920 + 1664
    assert lib.ctr_actor_blob_bytes(_actor((32,))) == 2048 + 2048 + 256
    # the wide shapes of tests/test_gpu_actor.py (weights + biases); [224, 160] is 384 B under the budget
    for hidden, weights, biases, nbytes in (((256,), 32768, 1152, 33920), ((256, 128), 90112, 1664, 91776),
                                            ((224, 160), 96256, 1664, 97920), ((160, 192, 32), 86016, 1664, 87680),
                                            ((32, 256, 32), 36864, 1408, 38272)):
        assert lib.ctr_actor_blob_bytes(_actor(hidden)) == nbytes == weights + biases, hidden
    _shape_refuse(_actor((256, 256)), b"CTR_ACTOR_MAX_BYTES")
    assert lib.ctr_actor_blob_bytes(_actor((256, 256))) == -1
    msg = lib.ctr_last_error()
    assert b"163840 B of weights" in msg and b"2176 B of biases" in msg, msg     # 16 K + 128 K + 16 K; 544 floats


def test_actor_scale_and_blob_are_validated():
    a = _actor()
    for bad in (float("nan"), float("inf")):
        a.scale[3] = bad
        _all_refuse(a, b"scale")
    a = _actor()
    a.blob = None
    _all_refuse(a, b"blob")
    a.blob = (1 << 20) + 8
    _all_refuse(a, b"16-B aligned")
    _abi, lib, cfg, b, o = _setup()
    a = _actor()
    assert lib.ctr_actor(a, None, 8, 16, None, None) == -1 and b"rows" in lib.ctr_last_error()
    assert lib.ctr_actor(a, 16, 8, None, None, None) == -1
    assert lib.ctr_actor(a, 16, -1, 16, None, None) == -1
    assert lib.ctr_actor(a, None, 0, None, None, None) == 0                     # an empty batch


def test_rollout_eligibility():
    _abi, lib, cfg, b, o = _setup()
    a = _actor()
    P = _abi.AUTORESET_POOLED

    def refused(word, cfg=cfg, b=b, a=a, k=4, o=o, mode=P, aux=None):
        assert lib.ctr_rollout(cfg, b, a, k, o, mode, aux, None) == -1, word
        assert word in lib.ctr_last_error(), (word, lib.ctr_last_error())

    # the actor's inputs against the config's observation
    cfg4 = _setup(n_systems=4)[2]
    refused(b"in_dim", cfg=cfg4)
    refused(b"in_dim", a=_actor(in_dim=20))
    # ctr_step_many's refusals, with its messages
    for k in (0, _abi.CTR_STEP_MANY_MAX + 1):
        refused(b"CTR_STEP_MANY_MAX", k=k)
    refused(b"CTR_AUTORESET_OFF or CTR_AUTORESET_POOLED", mode=_abi.AUTORESET_SWEEP)
    o.packed = 16
    refused(b"packed")
    o.packed = None
    refused(b"lane-pair", cfg=_setup(integrator="rk4", rk4_steps_per_m=400, model="compliant")[2])
    refused(b"8-lane group", cfg=_setup(integrator="rk4", rk4_steps_per_m=100, model="rigid")[2])
    assert lib.ctr_rollout(None, b, a, 4, o, P, None, None) == -1
    assert lib.ctr_rollout(cfg, None, a, 4, o, P, None, None) == -1
    assert lib.ctr_rollout(cfg, b, a, 4, None, P, None, None) == -1
    # the statistics need the pooled auto-reset; recording the actions does not
    aux = _abi.CtrRolloutAux()
    aux.episodes = 16
    refused(b"statistics", mode=_abi.AUTORESET_OFF, aux=aux)
    for name in ("successes", "error_sum", "length_sum"):
        aux = _abi.CtrRolloutAux()
        setattr(aux, name, 16)
        refused(b"statistics", mode=_abi.AUTORESET_OFF, aux=aux)
    # an empty batch is a no-op
    b.n = 0
    assert lib.ctr_rollout(cfg, b, a, 4, o, P, None, None) == 0
    assert lib.ctr_rollout(cfg, b, a, 4, o, _abi.AUTORESET_OFF, None, None) == 0


def test_rollout_lds_budget_with_domain_randomisation():
    """The blob, the kernel's static LDS and the per-lane domain tables share 160 KB."""
    _abi, lib, cfg, b, o = _setup()
    cfg.domain_rand = 0.05
    assert lib.ctr_rollout(cfg, b, _actor((128, 128, 128)), 4, o, _abi.AUTORESET_POOLED, None, None) == -1
    msg = lib.ctr_last_error()
    assert b"83584 B" in msg and b"61440 B" in msg and b"163840 B" in msg and b"ctr_actor + ctr_step" in msg, msg


def _unpack(a, blob, hidden, in_dim):
    """The blob's layout as the header documents it -> [(Wq [out, in] as bf16 bit patterns, b)]."""
    dims = [in_dim] + list(hidden) + [6]
    off, out = 0, []
    layers = []
    for l in range(len(dims) - 1):
        tiles = dims[l + 1] // 32 if l < len(hidden) else 1
        ksteps = 2 if l == 0 else dims[l] // 16
        layers.append((off, tiles, ksteps))
        off += tiles * ksteps * 1024
    for l, (w_off, tiles, ksteps) in enumerate(layers):
        rows, cols = dims[l + 1], dims[l]
        W = np.zeros((tiles * 32, ksteps * 16), dtype=np.uint16)
        frag = blob[w_off:w_off + tiles * ksteps * 1024].view(np.uint16).reshape(tiles, ksteps, 64, 8)
        for T in range(tiles):
            for S in range(ksteps):
                for lane in range(64):
                    h = lane >> 5
                    for j in range(8):
                        k = 16 * S + 8 * h + j if l == 0 else 32 * (S >> 1) + 16 * (S & 1) + 8 * (j >> 2) + 4 * h + (j & 3)
                        W[32 * T + (lane & 31), k] = frag[T, S, lane, j]
        assert not W[rows:].any() and not W[:, cols:].any()          # the padding is zero
        bias = blob[off:off + tiles * 32 * 4].view(np.float32)
        assert not bias[rows:].any()
        out.append((W[:rows, :cols], bias[:rows].copy()))
        off += tiles * 32 * 4
    assert off == blob.size
    return out


@pytest.mark.parametrize("hidden,in_dim", [((32,), 19), ((64, 96), 20), ((128, 128, 128), 20),
                                           ((256, 128), 20), ((224, 160), 19), ((32, 256, 32), 20)])
def test_pack_round_trip(hidden, in_dim):
    """Asymmetric, bf16-exact weights (W[i][j] = (1 + i + 100 j) / 256 has at most 8 significant
    bits below 2^15): the unpacked blob is bf16(W) and b, exactly."""
    from ctr_reach_amd.policy import MlpActor
    dims = [in_dim] + list(hidden) + [6]
    layers = []
    for l in range(len(dims) - 1):
        i, j = np.meshgrid(np.arange(dims[l + 1]), np.arange(dims[l]), indexing="ij")
        W = ((1 + i + 100 * j) % 251 * (1 << (j % 7))).astype(np.float32) / 256.0
        layers.append((W, (np.arange(dims[l + 1]) * 0.37 - 1.0).astype(np.float32)))
    act = MlpActor(layers, np.ones(6), device=None)
    lib = __import__("ctr_reach_amd")._abi.load()
    nb = lib.ctr_actor_blob_bytes(act._struct)
    blob = np.full(nb, 0xAB, dtype=np.uint8)
    n = len(layers)
    W = (ctypes.c_void_p * n)(*[w.ctypes.data for w in act.weights])
    b = (ctypes.c_void_p * n)(*[v.ctypes.data for v in act.biases])
    assert lib.ctr_actor_pack(act._struct, W, b, blob.ctypes.data) == 0
    for (Wq, bq), (W0, b0) in zip(_unpack(act._struct, blob, hidden, in_dim), layers):
        want = (W0.view(np.uint32) >> 16).astype(np.uint16)
        assert (W0.view(np.uint32) & 0xFFFF == 0).all()               # exact in bf16
        assert np.array_equal(Wq, want)
        assert np.array_equal(bq, b0)
    # an inexact weight is rounded to nearest even
    layers[0][0][3, 5] = np.float32(1.0 + 2.0 ** -8 + 2.0 ** -20)     # above the tie: up
    layers[0][0][4, 6] = np.float32(1.0 + 2.0 ** -8)                  # the tie: to even (down)
    act = MlpActor(layers, np.ones(6), device=None)
    assert lib.ctr_actor_pack(act._struct, W.__class__(*[w.ctypes.data for w in act.weights]), b, blob.ctypes.data) == 0
    Wq = _unpack(act._struct, blob, hidden, in_dim)[0][0]
    assert Wq[3, 5] == 0x3F81 and Wq[4, 6] == 0x3F80


def test_struct_layout_matches_header(tmp_path):
    from ctr_reach_amd import _abi
    lines, want = [], []
    for cname, cls in (("ctr_actor_t", _abi.CtrActor), ("ctr_rollout_aux_t", _abi.CtrRolloutAux)):
        lines.append('  printf("%%zu\\n", sizeof(%s));' % cname)
        want.append(ctypes.sizeof(cls))
        for fname, _ in cls._fields_:
            lines.append('  printf("%%zu\\n", offsetof(%s, %s));' % (cname, fname))
            want.append(getattr(cls, fname).offset)
    for macro in ("CTR_ACTOR_MAX_HIDDEN", "CTR_ACTOR_MAX_WIDTH", "CTR_ACTOR_MAX_BYTES", "CTR_ABI_VERSION"):
        lines.append('  printf("%%d\\n", %s);' % macro)
        want.append(getattr(_abi, macro))
    prog = tmp_path / "actor_layout.c"
    prog.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"ctr_reach_amd.h\"\nint main(void) {\n"
                    + "\n".join(lines) + "\n  return 0; }\n")
    exe = tmp_path / "actor_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(prog), "-o", str(exe)])
    assert list(map(int, subprocess.check_output([str(exe)]).split())) == want
    assert _abi.CTR_ABI_VERSION == 17


def _uniform_actor(rng, hidden, in_dim, device=None):
    from ctr_reach_amd.policy import MlpActor
    dims = [in_dim] + list(hidden) + [6]
    layers = []
    for l in range(len(dims) - 1):
        s = 1.0 / np.sqrt(dims[l])
        layers.append((rng.uniform(-s, s, (dims[l + 1], dims[l])).astype(np.float32),
                       rng.uniform(-s, s, dims[l + 1]).astype(np.float32)))
    return MlpActor(layers, np.array([0.001, 0.001, 0.001, 0.087, 0.087, 0.087]), device=device)


def _box_rows(rng, n):
    """Rows drawn from the four-system env's observation space box."""
    from ctr_reach_amd import systems
    from ctr_reach_amd.goal_tolerance import GoalTolerance
    from ctr_reach_amd.vec_env import observation_space
    kw = systems.default_kwargs()
    tubes = systems.tubes_from_params(kw["ctr_systems_parameters"])[:4]
    sp = observation_space(tubes, GoalTolerance(kw["goal_tolerance_parameters"]))
    lo = np.concatenate([sp["observation"].low, sp["achieved_goal"].low, sp["desired_goal"].low]).astype(np.float64)
    hi = np.concatenate([sp["observation"].high, sp["achieved_goal"].high, sp["desired_goal"].high]).astype(np.float64)
    assert lo.shape == (20,)
    return rng.uniform(lo, hi, (n, 20)).astype(np.float32)


@pytest.mark.parametrize("hidden", [(32,), (64, 96), (128, 128, 128), (256, 128), (224, 160), (32, 256, 32)])
def test_emulate_is_close_to_the_float64_mlp(hidden):
    """emulate (bf16 weights and activations, split input) against the plain float64 MLP on
    U(+-1/sqrt(fan_in)) weights and rows from the observation box: max |actions / scale| difference
    measured 1.51e-3 ([32]), 1.21e-3 ([64, 96]), 4.71e-4 ([128, 128, 128]), 1.09e-3 ([256, 128]),
    8.26e-4 ([224, 160]), 4.58e-4 ([32, 256, 32]) over 2000 rows (seed 11); asserted with 2x headroom.  A
    property of bf16, pinned against a typo in the emulation."""
    measured = {(32,): 1.51e-3, (64, 96): 1.21e-3, (128, 128, 128): 4.71e-4,
                (256, 128): 1.09e-3, (224, 160): 8.26e-4, (32, 256, 32): 4.58e-4}[hidden]
    rng = np.random.default_rng(11)
    act = _uniform_actor(rng, hidden, 20)
    rows = _box_rows(rng, 2000)
    a, y = act.emulate(rows)
    ref = act.reference(rows)
    err = np.abs(a / act.scale - ref / act.scale).max()
    print("emulate vs float64 MLP, hidden %s: max |d action / scale| = %.3g" % (list(hidden), err))
    assert np.isfinite(a).all() and a.shape == (2000, 6) and y.shape == (2000, 6)
    assert err <= 2 * measured
    assert err > 0                                                   # (bf16 is in there)
