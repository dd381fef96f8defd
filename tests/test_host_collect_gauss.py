"""ctr_collect_gauss on the host (no GPU): the symbol is declared, listed and exported within ABI 17; its
ctypes prototype is the header's; every refusal the header lists returns CTR_EINVAL (-1) with a
ctr_last_error that starts with the function's name, before any HIP call (the device pointers are fake
and never dereferenced); an empty batch is a checked no-op; collect_gauss refuses a policy that is not
a GaussianActor before it looks at the env."""
import ctypes
import os
import re
import subprocess

import pytest

from test_host_actor import _actor, _setup
from test_host_explore import _her

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FN = "ctr_collect_gauss"


def test_declared_listed_and_exported():
    _abi, lib = _setup()[:2]
    header = open(os.path.join(ROOT, "include", "ctr_reach_amd.h")).read()
    assert re.search(r"^int ctr_collect_gauss\(const ctr_env_config_t \*cfg, const ctr_batch_t \*batch, "
                     r"const ctr_actor_t \*policy,\n +uint64_t seed, uint64_t counter, const ctr_her_t \*her, int32_t k,\n"
                     r" +const ctr_step_out_t \*out, int32_t autoreset, const ctr_rollout_aux_t \*aux, void \*stream\);",
                     header, re.M)
    assert re.search(r"^#define CTR_ABI_VERSION 17$", header, re.M)
    assert FN in _abi.EXPORTED and hasattr(lib, FN)
    assert lib.ctr_abi_version() == _abi.CTR_ABI_VERSION == 17
    nm = subprocess.check_output(["nm", "-D", "--defined-only", lib._name]).decode()
    assert re.search(r" T ctr_collect_gauss$", nm, re.M)
    assert re.search(r" T ctr_collect$", nm, re.M) and re.search(r" T ctr_gauss_act$", nm, re.M)
    import ctr_reach_amd
    assert hasattr(ctr_reach_amd.CtrReachVecEnv, "collect_gauss")


def test_prototype_matches_the_header(tmp_path):
    """The ctypes argument list, type by type, and against a C caller compiled with the header (gcc,
    C11, -Werror: a pointer of another struct or an argument too many would not compile)."""
    _abi, lib = _setup()[:2]
    P = ctypes.POINTER
    fn = lib.ctr_collect_gauss
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [P(_abi.CtrEnvConfig), P(_abi.CtrBatch), P(_abi.CtrActor), ctypes.c_uint64, ctypes.c_uint64,
                                 P(_abi.CtrHer), ctypes.c_int32, P(_abi.CtrStepOut), ctypes.c_int32, P(_abi.CtrRolloutAux),
                                 ctypes.c_void_p]
    prog = tmp_path / "collect_gauss_proto.c"
    prog.write_text('#include <stdio.h>\n#include "ctr_reach_amd.h"\n'
                    "typedef int (*fn_t)(const ctr_env_config_t *, const ctr_batch_t *, const ctr_actor_t *, uint64_t,\n"
                    "                    uint64_t, const ctr_her_t *, int32_t, const ctr_step_out_t *, int32_t,\n"
                    "                    const ctr_rollout_aux_t *, void *);\n"
                    "int main(void) { fn_t f = ctr_collect_gauss; fn_t g = f; (void)g;\n"
                    '  printf("%d\\n", CTR_ABI_VERSION); return 0; }\n')
    obj = tmp_path / "collect_gauss_proto.o"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c",
                           str(prog), "-o", str(obj)])


def test_refusals():
    _abi, lib, cfg, b, o = _setup()
    a = _actor()
    P = _abi.AUTORESET_POOLED

    def call(cfg=cfg, b=b, a=a, her=None, k=4, o=o, mode=P, aux=None, counter=0):
        her = _her(_abi, b, cfg) if her is None else her
        return lib.ctr_collect_gauss(cfg, b, a, 9, counter, her, k, o, mode, aux, None), lib.ctr_last_error()

    def refused(word, **kw):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith(b"ctr_collect_gauss: ") and word in msg, (word, rc, msg)

    # NULL arguments
    h = _her(_abi, b, cfg)
    for args, word in (((None, b, a, 9, 0, h, 4, o), b"cfg"), ((cfg, None, a, 9, 0, h, 4, o), b"NULL"),
                       ((cfg, b, None, 9, 0, h, 4, o), b"actor is NULL"), ((cfg, b, a, 9, 0, None, 4, o), b"her is NULL"),
                       ((cfg, b, a, 9, 0, h, 4, None), b"NULL")):
        assert lib.ctr_collect_gauss(*(args + (P, None, None))) == -1, word
        msg = lib.ctr_last_error()
        assert msg.startswith(b"ctr_collect_gauss: ") and word in msg, (word, msg)
    # the policy's shape, box and blob, as ctr_gauss_act judges them
    refused(b"in_dim", a=_actor(in_dim=20))
    refused(b"in_dim", a=_actor(in_dim=18))
    bad = _actor()
    bad.n_hidden = 4
    refused(b"n_hidden", a=bad)
    refused(b"every hidden width", a=_actor((64, 48)))
    refused(b"CTR_ACTOR_MAX_BYTES", a=_actor((256, 256)))
    bad = _actor()
    bad.scale[2] = float("nan")
    refused(b"scale", a=bad)
    bad = _actor()
    bad.blob = None
    refused(b"blob is NULL", a=bad)
    bad.blob = (1 << 20) + 8
    refused(b"16-B aligned", a=bad)
    # ctr_rollout's refusals
    for k in (0, -1, _abi.CTR_STEP_MANY_MAX + 1):
        refused(b"CTR_STEP_MANY_MAX", k=k)
    refused(b"CTR_AUTORESET_OFF or CTR_AUTORESET_POOLED", mode=_abi.AUTORESET_SWEEP)
    refused(b"lane-pair", cfg=_setup(integrator="rk4", rk4_steps_per_m=400, model="compliant")[2])
    refused(b"8-lane group", cfg=_setup(integrator="rk4", rk4_steps_per_m=100, model="rigid")[2])
    aux = _abi.CtrRolloutAux()
    aux.episodes = 16
    refused(b"statistics", mode=_abi.AUTORESET_OFF, aux=aux)
    # mode 1, by name
    uy = _setup()[2]
    uy.systems[0].Uy[0] = 5.0
    refused(b"scratch", cfg=uy)
    assert call(cfg=uy)[1].startswith(b"ctr_collect_gauss: not for the compliant model's scipy RK45")
    assert b"ctr_gauss_act + ctr_step_her" in call(cfg=uy)[1]
    # the LDS budget, with the byte counts: the blob of [128, 128, 128] beside the static LDS and the tables
    dr = _setup()[2]
    dr.domain_rand = 0.05
    wide = _actor((128, 128, 128))
    refused(b"LDS", cfg=dr, a=wide)
    msg = call(cfg=dr, a=wide)[1].decode()
    m = re.search(r"the actor's blob \((\d+) B\) \+ the kernel's static LDS \((\d+) B\) \+ the domain randomisation "
                  r"tables \((\d+) B\) exceed the (\d+) B of LDS", msg)
    assert m, msg
    blob, fixed, lane, total = map(int, m.groups())
    assert blob == lib.ctr_gauss_blob_bytes(wide) == lib.ctr_actor_blob_bytes(wide) and total == 160 * 1024
    assert fixed == 78976 and lane > 0 and blob + fixed + lane + 16 > total
    # ctr_collect's checks of the store
    refused(b"t_max", her=_her(_abi, b, cfg, t_max=cfg.max_steps + 1))
    refused(b"sizes differ", her=_her(_abi, b, cfg, n=b.n + 1))
    refused(b"env_base differ", her=_her(_abi, b, cfg, env_base=64))
    refused(b"buffer missing", her=_her(_abi, b, cfg, cur_t=None))
    refused(b"slots", her=_her(_abi, b, cfg, slots=1))
    # the global env id is the noise key's 32-bit row word
    for base in (-1, (1 << 32) - b.n + 1, 1 << 40):
        nb = _setup()[3]
        nb.env_base = base
        refused(b"env_base + n must stay within 0..2^32", b=nb, her=_her(_abi, nb, cfg))


def test_an_empty_batch_is_a_checked_no_op():
    _abi, lib, cfg, b, o = _setup()
    nb = _abi.CtrBatch()
    P = _abi.AUTORESET_POOLED
    assert lib.ctr_collect_gauss(cfg, nb, _actor(), 9, 0, _her(_abi, nb, cfg), 4, o, P, None, None) == 0
    assert lib.ctr_collect_gauss(cfg, nb, _actor(), 9, 0, None, 4, o, P, None, None) == -1
    assert lib.ctr_last_error().startswith(b"ctr_collect_gauss: ")
    assert lib.ctr_collect_gauss(cfg, nb, _actor(in_dim=20), 9, 0, _her(_abi, nb, cfg), 4, o, P, None, None) == -1
    # the range of the env ids is judged on an empty batch too: 2^32 + 0 is its upper end, and every counter is one
    nb.env_base = 1 << 32
    assert lib.ctr_collect_gauss(cfg, nb, _actor(), 9, (1 << 64) - 1, _her(_abi, nb, cfg), 4, o, P, None, None) == 0
    nb.env_base = (1 << 32) + 1
    assert lib.ctr_collect_gauss(cfg, nb, _actor(), 9, 0, _her(_abi, nb, cfg), 4, o, P, None, None) == -1
    assert b"env_base + n" in lib.ctr_last_error()


def test_collect_gauss_takes_a_gaussian_actor_only():
    """The type check comes first: an env that has nothing but the method is enough to see it."""
    import numpy as np
    from ctr_reach_amd import CtrReachVecEnv
    from ctr_reach_amd.policy import MlpActor
    rng = np.random.default_rng(3)
    dims = [19, 32, 6]
    layers = [(rng.uniform(-1, 1, (dims[l + 1], dims[l])).astype(np.float32),
               rng.uniform(-1, 1, dims[l + 1]).astype(np.float32)) for l in range(2)]
    env = CtrReachVecEnv.__new__(CtrReachVecEnv)
    with pytest.raises(TypeError, match="collect_gauss: the policy must be a GaussianActor"):
        env.collect_gauss(MlpActor(layers, np.full(6, 0.5, np.float32), device=None), 4, counter=0)
    with pytest.raises(TypeError, match="GaussianActor"):
        env.collect_gauss(None, 4, counter=0)
