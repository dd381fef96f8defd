"""ctr_step_period (a refill period's steps and its refill in one launch) on the host: it
is refused wherever ctr_step_many is, and without a reset pool, with CTR_EINVAL (-1) and a
ctr_last_error message before any HIP call (no GPU needed); the ABI number and the struct the call
takes; the keyword and the environment variable that choose between it and ctr_step_many +
ctr_pool_refill."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _setup(pool=True, **solver):
    from ctr_reach_amd import _abi, systems
    lib = _abi.load()
    codes = systems.solver_codes(solver.get("integrator", "rk45_scipy"), solver.get("rk4_steps_per_m", 100),
                                 solver.get("model", "compliant"))
    cfg = systems.make_config(systems.tubes_from_params(systems.default_systems_parameters())[:1],
                              integrator=codes[0], rk4_steps_per_m=codes[1], model=codes[2])
    fake = ctypes.c_void_p(16)
    b = _abi.CtrBatch()
    b.n = 8
    b.joints = b.desired_goal = b.achieved_goal = b.t = b.system = b.epoch = b.work = fake
    if pool:
        b.pool_depth, b.pool, b.refill, b.refill_cap = 4, ctypes.c_void_p(128), fake, 64
    o = _abi.CtrStepOut()
    o.obs = o.reward = o.done = o.success = o.error = fake
    seq = _abi.CtrActionSeq()
    for i in range(_abi.CTR_STEP_MANY_MAX):
        seq.a[i] = 16
    return _abi, lib, cfg, b, o, seq


def test_step_period_rejects_bad_step_counts_and_tables():
    _abi, lib, cfg, b, o, seq = _setup()
    for k in (0, -3, _abi.CTR_STEP_MANY_MAX + 1):
        assert lib.ctr_step_period(cfg, b, seq, k, o, None) == -1, k
        assert b"CTR_STEP_MANY_MAX" in lib.ctr_last_error()
    seq.a[2] = None
    assert lib.ctr_step_period(cfg, b, seq, 4, o, None) == -1
    assert b"NULL action buffer" in lib.ctr_last_error()
    assert lib.ctr_step_period(cfg, b, None, 4, o, None) == -1
    assert lib.ctr_step_period(cfg, None, seq, 4, o, None) == -1
    assert lib.ctr_step_period(cfg, b, seq, 4, None, None) == -1
    assert lib.ctr_step_period(None, b, seq, 4, o, None) == -1


def test_step_period_needs_the_reset_pool():
    _abi, lib, cfg, b, o, seq = _setup(pool=False)
    assert lib.ctr_step_period(cfg, b, seq, 4, o, None) == -1
    assert b"reset pool" in lib.ctr_last_error()
    _abi, lib, cfg, b, o, seq = _setup()
    b.work = None
    assert lib.ctr_step_period(cfg, b, seq, 4, o, None) == -1
    assert b"batch->work" in lib.ctr_last_error()
    b.work = 16
    b.pool = ctypes.c_void_p(128 + 64)
    assert lib.ctr_step_period(cfg, b, seq, 4, o, None) == -1
    assert b"128-B aligned" in lib.ctr_last_error()
    b.pool = ctypes.c_void_p(128)
    cfg.resample_joints = 0
    assert lib.ctr_step_period(cfg, b, seq, 4, o, None) == -1
    assert b"resample_joints" in lib.ctr_last_error()
    cfg.resample_joints = 1
    b.carry, b.carry_cap = 16, 0
    assert lib.ctr_step_period(cfg, b, seq, 4, o, None) == -1
    assert b"carry" in lib.ctr_last_error()


def test_step_period_rejects_pair_and_group_modes():
    """The two modes whose refill is not the two-lane resumable one."""
    _abi, lib, cfg, b, o, seq = _setup(integrator="rk4", rk4_steps_per_m=400, model="compliant")
    assert lib.ctr_step_period(cfg, b, seq, 4, o, None) == -1
    assert b"lane-pair" in lib.ctr_last_error()
    _abi, lib, cfg, b, o, seq = _setup(integrator="rk4", rk4_steps_per_m=100, model="rigid")
    assert lib.ctr_step_period(cfg, b, seq, 4, o, None) == -1
    assert b"8-lane group" in lib.ctr_last_error()


def test_step_period_rejects_the_compliant_rk45_with_y_pre_curvature():
    """Kernel mode 1, whose kernel would spill to scratch: ctr_step_many takes it, ctr_step_period not."""
    _abi, lib, cfg, b, o, seq = _setup()
    cfg.systems[0].Uy[1] = 2.0
    assert lib.ctr_step_period(cfg, b, seq, 4, o, None) == -1
    assert b"y pre-curvature" in lib.ctr_last_error()
    # the rigid model with the same tubes is not refused for its mode (the fake pool is: alignment)
    _abi, lib, cfg, b, o, seq = _setup(model="rigid")
    cfg.systems[0].Uy[1] = 2.0
    b.pool = ctypes.c_void_p(128 + 64)
    assert lib.ctr_step_period(cfg, b, seq, 4, o, None) == -1
    assert b"128-B aligned" in lib.ctr_last_error()


def test_step_period_rejects_packed_rows_and_the_push_gather():
    _abi, lib, cfg, b, o, seq = _setup()
    for field in ("packed", "gather", "gather_prev"):
        setattr(o, field, 16)
        assert lib.ctr_step_period(cfg, b, seq, 4, o, None) == -1, field
        assert b"packed" in lib.ctr_last_error()
        setattr(o, field, None)


def test_step_period_rejects_what_ctr_step_rejects_and_accepts_an_empty_batch():
    _abi, lib, cfg, b, o, seq = _setup()
    o.obs = None
    assert lib.ctr_step_period(cfg, b, seq, 4, o, None) == -1
    assert b"output missing" in lib.ctr_last_error()
    o.obs = 16
    b.joints = None
    assert lib.ctr_step_period(cfg, b, seq, 4, o, None) == -1
    assert b"batch buffer missing" in lib.ctr_last_error()
    cfg.n_systems = 0
    assert lib.ctr_step_period(cfg, b, seq, 4, o, None) == -1
    assert b"n_systems" in lib.ctr_last_error()
    cfg.n_systems = 1
    empty = _abi.CtrBatch()
    empty.n = 0
    assert lib.ctr_step_period(cfg, empty, seq, 4, _abi.CtrStepOut(), None) == 0


def test_abi_number_and_action_table_layout(tmp_path):
    """One ABI number in the header, the binding and the library (ctr_step_period adds a symbol and
    changes no struct or existing entry point, so the number did not move); ctr_action_seq_t as the
    binding has it."""
    from ctr_reach_amd import _abi
    assert _abi.load().ctr_abi_version() == _abi.CTR_ABI_VERSION >= 17
    assert "ctr_step_period" in _abi.EXPORTED
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ctr_reach_amd.h"\nint main(void) {\n'
                    '  printf("%d %zu %zu %d\\n", CTR_ABI_VERSION, sizeof(ctr_action_seq_t), '
                    'offsetof(ctr_batch_t, carry), CTR_STEP_MANY_MAX);\n  return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(prog), "-o", str(exe)])
    assert list(map(int, subprocess.check_output([str(exe)]).split())) == [
        _abi.CTR_ABI_VERSION, ctypes.sizeof(_abi.CtrActionSeq), _abi.CtrBatch.carry.offset, _abi.CTR_STEP_MANY_MAX]
    # the carry header stays 1 KB (ctr_step_period's words live in its padding)
    assert _abi.load().ctr_refill_carry_bytes(0) == 1024


def test_keyword_and_environment_variable_select_the_capture(monkeypatch):
    """tail_refill (off unless asked for: DESIGN 4.0f) and CTR_TAIL_REFILL, which overrides it both
    ways: 0 keeps step_many on ctr_step_many + ctr_pool_refill, 1 selects ctr_step_period."""
    from ctr_reach_amd import CtrReachVecEnv
    # (no auto-reset: no device pool to allocate on the host)
    mk = lambda **kw: CtrReachVecEnv(8, device="cpu", autoreset=False, **kw)   # noqa: E731
    monkeypatch.delenv("CTR_TAIL_REFILL", raising=False)
    assert not mk().tail_refill
    assert mk(tail_refill=True).tail_refill
    monkeypatch.setenv("CTR_TAIL_REFILL", "0")
    assert not mk().tail_refill and not mk(tail_refill=True).tail_refill
    monkeypatch.setenv("CTR_TAIL_REFILL", "1")
    assert mk().tail_refill and mk(tail_refill=False).tail_refill
    monkeypatch.delenv("CTR_TAIL_REFILL")
    e = mk(tail_refill=True)
    assert e.tail_launches == 0 and e.fused_period
