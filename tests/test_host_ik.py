"""ctr_ik_dls validates its arguments on the host: every refused case returns CTR_EINVAL (-1) with a
ctr_last_error message naming the field, before any HIP call (no GPU needed; the device pointers
are fake and never dereferenced), and an empty batch is a no-op."""
import ctypes
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTERS = ("targets", "q0", "q", "err", "iters")


def _setup():
    from ctr_reach_amd import _abi, systems
    lib = _abi.load()
    cfg = systems.make_config(systems.tubes_from_params(systems.default_systems_parameters())[:1])
    ik = _abi.CtrIk()
    ik.n, ik.waypoints, ik.num = 8, 1, 10
    ik.lam, ik.tol, ik.eps = 0.25, 1e-3, 1e-4
    # distinct fake device buffers, far enough apart not to overlap
    for i, name in enumerate(POINTERS + ("sys_idx", "status")):
        setattr(ik, name, 1 << 20 << i)
    return _abi, lib, cfg, ik


def _refused(lib, cfg, ik, word):
    rc = lib.ctr_ik_dls(cfg, ik, None)
    msg = lib.ctr_last_error()
    assert rc == -1, (word, rc)
    assert word in msg, (word, msg)


def test_ik_rejects_null_arguments():
    _abi, lib, cfg, ik = _setup()
    assert lib.ctr_ik_dls(None, ik, None) == -1
    assert b"cfg" in lib.ctr_last_error()
    assert lib.ctr_ik_dls(cfg, None, None) == -1
    assert b"ik is NULL" in lib.ctr_last_error()
    for name in POINTERS:
        keep = getattr(ik, name)
        setattr(ik, name, None)
        _refused(lib, cfg, ik, name.encode())
        setattr(ik, name, keep)


def test_ik_rejects_bad_counts():
    _abi, lib, cfg, ik = _setup()
    ik.n = -1
    _refused(lib, cfg, ik, b" n ")
    ik.n = 8
    for k in (0, -1):
        ik.waypoints = k
        _refused(lib, cfg, ik, b"waypoints")
    ik.waypoints = 1
    ik.num = -1
    _refused(lib, cfg, ik, b"num")
    assert _abi.CTR_IK_MAX_ITERS == 8192
    # one past the cap as K = 1 and as a product (8193 = 3 x 2731), and 91 x 91 = 8281, where
    # neither factor is over the cap
    for k, num in ((1, _abi.CTR_IK_MAX_ITERS + 1), (3, 2731), (91, 91)):
        assert k * num > _abi.CTR_IK_MAX_ITERS and (k, num) == (91, 91) or k * num == _abi.CTR_IK_MAX_ITERS + 1
        ik.waypoints, ik.num = k, num
        _refused(lib, cfg, ik, b"CTR_IK_MAX_ITERS")


@pytest.mark.parametrize("field,values", [("lam", (0.0, -1.0, math.nan, math.inf)), ("tol", (math.nan,)),
                                          ("eps", (0.0, math.nan, math.inf))])
def test_ik_rejects_bad_scalars(field, values):
    _abi, lib, cfg, ik = _setup()
    for v in values:
        setattr(ik, field, v)
        _refused(lib, cfg, ik, field.encode())


def test_ik_rejects_a_bad_config_and_overlapping_q0():
    _abi, lib, cfg, ik = _setup()
    cfg.n_systems = 0
    _refused(lib, cfg, ik, b"n_systems")
    cfg.n_systems = 1
    ik.q0 = ik.q + 8
    _refused(lib, cfg, ik, b"overlap")


def test_ik_accepts_an_empty_batch():
    _abi, lib, cfg, _ = _setup()
    ik = _abi.CtrIk()
    ik.n, ik.waypoints, ik.num = 0, 1, 10
    ik.lam, ik.tol, ik.eps = 0.25, 1e-3, 1e-4
    assert lib.ctr_ik_dls(cfg, ik, None) == 0


def test_ik_struct_layout_matches_header(tmp_path):
    """ctypes.sizeof(CtrIk) and every field offset equal ctr_ik_t's (gcc, the header as C11)."""
    from ctr_reach_amd import _abi
    lines, want = ['  printf("%zu\\n", sizeof(ctr_ik_t));', '  printf("%d\\n", CTR_IK_MAX_ITERS);',
                   '  printf("%d\\n", CTR_ABI_VERSION);'], \
        [ctypes.sizeof(_abi.CtrIk), _abi.CTR_IK_MAX_ITERS, _abi.CTR_ABI_VERSION]
    for fname, _ in _abi.CtrIk._fields_:
        lines.append('  printf("%%zu\\n", offsetof(ctr_ik_t, %s));' % fname)
        want.append(getattr(_abi.CtrIk, fname).offset)
    prog = tmp_path / "ik_layout.c"
    prog.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"ctr_reach_amd.h\"\nint main(void) {\n"
                    + "\n".join(lines) + "\n  return 0; }\n")
    exe = tmp_path / "ik_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(prog), "-o", str(exe)])
    assert list(map(int, subprocess.check_output([str(exe)]).split())) == want
    assert _abi.CTR_ABI_VERSION == 17
