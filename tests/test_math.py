"""Host check of the kernels' fp64 sincos (gym-ctr-reach_amd/csrc/ctr_math.hpp): the same
source compiled with g++ must stay within 2 ulp of libm over the arguments the RHS sees.
This is the host branch of the header, without FMA contraction; tests/test_gpu_math.py runs the
device branches on the GPU over the same argument sets (the *_args functions below)."""
import ctypes
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def makefile_var(name):
    """The default of a `NAME ?= value` line of gym-ctr-reach_amd/Makefile."""
    with open(os.path.join(ROOT, "gym-ctr-reach_amd", "Makefile")) as fh:
        for line in fh:
            m = re.match(r"%s\s*\??=\s*(.*)$" % re.escape(name), line)
            if m:
                return m.group(1).strip()
    raise KeyError(name)


def _lib(tmp_path, cxx="g++", flags=("-ffp-contract=off",), stem="m"):
    src = tmp_path / (stem + ".cpp")
    src.write_text('#include "ctr_math.hpp"\n'
                   'extern "C" void vsincos(const double* x, double* s, double* c, long n) {\n'
                   '  for (long i = 0; i < n; ++i) ctr_math::sincos_cw(x[i], s + i, c + i); }\n'
                   'extern "C" void vsincos_tab(const double* x, double* s, double* c, long n) {\n'
                   '  for (long i = 0; i < n; ++i) ctr_math::sincos_tab(x[i], ctr_math::TRIG_TAB, s[i], c[i]); }\n'
                   'extern "C" const double* trig_tab() { return &ctr_math::TRIG_TAB[0][0]; }\n'
                   )
    so = tmp_path / (stem + ".so")
    subprocess.check_call([cxx, "-O2", *flags, "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "gym-ctr-reach_amd", "csrc"), str(src), "-o", str(so)])
    lib = ctypes.CDLL(str(so))
    lib.vsincos.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_long]
    lib.vsincos_tab.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_long]
    lib.trig_tab.restype = ctypes.POINTER(ctypes.c_double * 1024)
    return lib


def _ulp_err(got, want):
    return np.abs(got - want) / np.spacing(np.maximum(np.abs(want), 1e-300))


import pytest


def sincos_args():
    """The arguments of test_sincos_accuracy, all |x| < 2^20 (tests/test_gpu_math.py runs the
    device build over the same set)."""
    rng = np.random.default_rng(0)
    return np.concatenate([rng.uniform(-np.pi, np.pi, 200000), rng.uniform(-300, 300, 200000),
                           rng.uniform(-1e5, 1e5, 50000), np.array([0.0, -0.0, 1e-300, np.pi / 2, -np.pi]),
                           np.arange(-40, 41) * (np.pi / 2), np.arange(-40, 41) * (np.pi / 2) + 1e-9,
                           np.arange(-400, 401) * (np.pi / 32), np.arange(-400, 401) * (np.pi / 32) + 1e-12,
                           np.arange(-1600, 1601) * (np.pi / 256), np.arange(-1600, 1601) * (np.pi / 512)])


def sincos_edge_args(step=np.pi / 512, kmax=1600):
    """Edges of the table reduction: zeros, every fl(k step) for |k| <= kmax with both nextafter
    neighbours (the ties of rint(x 256/pi) lie at odd multiples of pi/512), and the ends of the
    table's range +-(2^20 - 2^-32)."""
    t = np.arange(-kmax, kmax + 1) * step
    top = 2.0 ** 20 - 2.0 ** -32
    return np.concatenate([np.array([0.0, -0.0, 1e-300, top, -top]), t, np.nextafter(t, np.inf),
                           np.nextafter(t, -np.inf)])


def check_sincos(x, s, c, what=""):
    """The sincos bar: < 4e-16 absolute everywhere (values near zero crossings), <= 2 ulp where
    the value is above 1e-3; against np.sin / np.cos.  Returns the measured maxima."""
    es = np.abs(s - np.sin(x))
    ec = np.abs(c - np.cos(x))
    assert es.max() < 4e-16 and ec.max() < 4e-16, (what, es.max(), ec.max())
    big = np.abs(np.sin(x)) > 1e-3
    us = _ulp_err(s[big], np.sin(x[big])).max()
    assert us <= 2.0, (what, us)
    big = np.abs(np.cos(x)) > 1e-3
    uc = _ulp_err(c[big], np.cos(x[big])).max()
    assert uc <= 2.0, (what, uc)
    return max(es.max(), ec.max()), max(us, uc)


def _run_sincos(lib, fn, x):
    s = np.empty_like(x)
    c = np.empty_like(x)
    getattr(lib, fn)(x.ctypes.data, s.ctypes.data, c.ctypes.data, len(x))
    return s, c


@pytest.mark.parametrize("fn", ["vsincos", "vsincos_tab"])
def test_sincos_accuracy(tmp_path, fn):
    lib = _lib(tmp_path)
    x = sincos_args()
    if fn == "vsincos":          # sincos_cw has the exact large-argument path; sincos_tab is |x| < 2^20
        x = np.concatenate([x, [1e6, 3e7]])
    s, c = _run_sincos(lib, fn, x)
    check_sincos(x, s, c, fn)


def test_trig_table_correctly_rounded(tmp_path):
    """TRIG_TAB[k] is the correctly rounded (sin, cos)(k pi/256) for all 512 k (mpmath at 60
    digits on the exact rational k/256), with exact 0 and +-1 at the quadrant entries."""
    import mpmath
    tab = np.array(_lib(tmp_path).trig_tab().contents).reshape(512, 2)
    with mpmath.workdps(60):
        want = np.array([[float(mpmath.sinpi(mpmath.mpf(k) / 256)), float(mpmath.cospi(mpmath.mpf(k) / 256))]
                         for k in range(512)])
    bad = np.argwhere(tab.view(np.uint64) != want.view(np.uint64))
    assert len(bad) == 0, [(int(k), int(j), tab[k, j].hex(), want[k, j].hex()) for k, j in bad[:8]]
    quad = tab[[0, 128, 256, 384]]
    assert np.array_equal(quad, [[0.0, 1.0], [1.0, 0.0], [0.0, -1.0], [-1.0, 0.0]]), quad
    assert not np.signbit(quad[quad == 0.0]).any()


def _cpu_has_fma():
    try:
        with open("/proc/cpuinfo") as fh:
            return any(line.startswith("flags") and " fma" in line for line in fh)
    except OSError:
        return False


def test_sincos_contraction_invariance(tmp_path):
    """sincos_tab contracted to FMA (the ROCm clang, -ffp-contract=fast -mfma: what the device
    build does) is bit-equal to the -ffp-contract=off build test_sincos_accuracy checks: every
    operation of sincos_tab2_pre / _post is an explicit fma, a lone product or rint, so there is
    nothing to fuse.  This is the premise of the device bit-equality bar of tests/test_gpu_math.py.
    sincos_cw does change under contraction, and stays within the 2 ulp bar."""
    if not _cpu_has_fma():
        pytest.skip("CPU without FMA")
    clang = os.path.join(os.path.dirname(os.path.dirname(makefile_var("HIPCC"))), "llvm", "bin", "clang++")
    off = _lib(tmp_path)
    fast = _lib(tmp_path, cxx=clang, flags=("-ffp-contract=fast", "-mfma"), stem="m_fma")
    x = np.concatenate([sincos_args(), sincos_edge_args(), sincos_edge_args(np.pi / 256)])
    s0, c0 = _run_sincos(off, "vsincos_tab", x)
    s1, c1 = _run_sincos(fast, "vsincos_tab", x)
    same = (s0.view(np.uint64) == s1.view(np.uint64)) & (c0.view(np.uint64) == c1.view(np.uint64))
    assert same.all(), (x[~same][:5], s0[~same][:5], s1[~same][:5])
    sw, cw = _run_sincos(fast, "vsincos", x)
    d0 = _run_sincos(off, "vsincos", x)
    print("sincos_cw contracted: max abs %.3g, max ulp %.3f; %d of %d results differ from the uncontracted build"
          % (*check_sincos(x, sw, cw, "sincos_cw -ffp-contract=fast"), int(((sw != d0[0]) | (cw != d0[1])).sum()), len(x)))


def _lib2(tmp_path):
    src = tmp_path / "m2.cpp"
    src.write_text('#include "ctr_math.hpp"\n'
                   'extern "C" void vir10(const double* x, double* y, long n) {\n'
                   '  for (long i = 0; i < n; ++i) y[i] = ctr_math::inv_root10(x[i]); }\n'
                   'extern "C" void vsqrt(const double* x, double* y, long n) {\n'
                   '  for (long i = 0; i < n; ++i) y[i] = ctr_math::sqrt_rsq(x[i]); }\n')
    so = tmp_path / "m2.so"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "gym-ctr-reach_amd", "csrc"), str(src), "-o", str(so)])
    lib = ctypes.CDLL(str(so))
    lib.vir10.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_long]
    lib.vsqrt.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_long]
    return lib


def inv_root10_sqrt_args():
    """(x, xs): the arguments of inv_root10 (the whole positive range, the 8 edge values last)
    and of sqrt_rsq."""
    rng = np.random.default_rng(1)
    x = np.concatenate([10.0 ** rng.uniform(-300, 300, 200000), rng.uniform(0.5, 2, 100000),
                        np.array([1.0, 2.0, 1024.0, 1e-310, 5e-324, 1.7e308, 18.0, 1e-30])])
    xs = 10.0 ** rng.uniform(-30, 30, 100000)
    return x, xs


def inv_root10_reference(x, stride=97):
    """(idx, x[idx] ** -0.1): 50-digit decimal arithmetic (libm and numpy pow are themselves
    ~30 ulp off at the extremes of the range); a subsample keeps the test fast."""
    from decimal import Decimal, getcontext
    getcontext().prec = 50
    idx = np.concatenate([np.arange(0, len(x), stride), np.arange(len(x) - 8, len(x))])
    return idx, np.array([float(Decimal(float(v)) ** Decimal("-0.1")) for v in x[idx]])


def test_inv_root10_and_sqrt(tmp_path):
    """x^(-1/10) (RK45 step factor 0.9 en^-0.2 = 0.9 (en^2)^-0.1) within 2 ulp of libm pow over
    the whole positive double range, including subnormals."""
    lib = _lib2(tmp_path)
    x, xs = inv_root10_sqrt_args()
    y = np.empty_like(x)
    lib.vir10(x.ctypes.data, y.ctypes.data, len(x))
    idx, want = inv_root10_reference(x)
    assert _ulp_err(y[idx], want).max() <= 2.0, _ulp_err(y[idx], want).max()
    s = np.empty_like(xs)
    lib.vsqrt(xs.ctypes.data, s.ctypes.data, len(xs))
    assert _ulp_err(s, np.sqrt(xs)).max() <= 2.0


def test_sampler_round_tables():
    """The wave sampler's per-round constants (ctr_device.hpp SampleTabs): for k = 1..64 unresolved
    lanes, x // k == (x * ceil(2^16 / k)) >> 16 for every 0 <= x <= 128 (the sampler divides
    lane, ctz(hit) - rank <= 63 and 64 - rank + k - 1 <= 127 by k), and stride[k] << rank is the
    set {rank, rank + k, ...} below 64 that the former loop built."""
    for k in range(1, 65):
        m = -(-65536 // k)
        for x in range(129):
            assert (x * m) >> 16 == x // k, (k, x)
        stride = sum(1 << i for i in range(0, 64, k))
        for rank in range(k):
            want = sum(1 << i for i in range(rank, 64, k))
            assert (stride << rank) & ((1 << 64) - 1) == want, (k, rank)


def gap_up_args():
    """(t, nextafter(t, inf) - t) over normals, subnormals, signed zeros, powers of two and their
    neighbours, the extremes and non-finite values."""
    rng = np.random.default_rng(2)
    p2 = np.ldexp(1.0, np.arange(-1074, 1024))
    x = np.concatenate([rng.uniform(-1, 1, 100000), rng.uniform(0, 0.6, 100000),
                        10.0 ** rng.uniform(-320, 308, 100000) * rng.choice([-1.0, 1.0], 100000),
                        p2, -p2, np.nextafter(p2, 0), -np.nextafter(p2, 0), np.nextafter(p2, np.inf),
                        np.array([0.0, -0.0, 5e-324, -5e-324, 1.7976931348623157e308,
                                  -1.7976931348623157e308, np.inf, -np.inf, np.nan])])
    with np.errstate(invalid="ignore", over="ignore"):
        want = np.nextafter(x, np.inf) - x
    return x, want


def test_gap_up_matches_nextafter(tmp_path):
    """ctr_math::gap_up(t) == nextafter(t, inf) - t bit for bit (the RK45 min_step, rk.py:114-119):
    normals, subnormals, signed zeros, negative powers of two (where the gap toward zero halves),
    the extremes and non-finite values."""
    src = tmp_path / "m3.cpp"
    src.write_text('#include "ctr_math.hpp"\n'
                   'extern "C" void vgap(const double* x, double* y, long n) {\n'
                   '  for (long i = 0; i < n; ++i) y[i] = ctr_math::gap_up(x[i]); }\n')
    so = tmp_path / "m3.so"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "gym-ctr-reach_amd", "csrc"), str(src), "-o", str(so)])
    lib = ctypes.CDLL(str(so))
    lib.vgap.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_long]
    x, want = gap_up_args()
    y = np.empty_like(x)
    lib.vgap(x.ctypes.data, y.ctypes.data, len(x))
    same = (y.view(np.uint64) == want.view(np.uint64)) | (np.isnan(y) & np.isnan(want))
    assert same.all(), (x[~same][:5], y[~same][:5], want[~same][:5])


def test_inv_root10_exponent_split():
    """inv_root10's branch-free k = floor((e - 1) / 10) over every frexp exponent of a double."""
    for e in range(-1075, 1026):
        em1 = e - 1
        assert ((em1 + 1100) // 10) - 110 == em1 // 10, e


UNGUARDED_TAIL = np.array([1e300, 3e300, 1e305, 1.7976931348623157e308, np.inf, np.nan])


def test_inv_root10_unguarded_tail(tmp_path):
    """The RK45 step factor is 0.9 inv_root10(err^2) without a guard (ctr_device.hpp): for a huge,
    infinite or NaN err^2 it must stay below 0.2 or be NaN, so that a rejection's fmax(0.2, .)
    gives 0.2 as rk.py:171 does for an infinite norm."""
    lib = _lib2(tmp_path)
    x = UNGUARDED_TAIL.copy()
    y = np.empty_like(x)
    lib.vir10(x.ctypes.data, y.ctypes.data, len(x))
    f = 0.9 * y
    assert np.all(np.isnan(f) | (f < 0.2)), f
    assert np.all(np.fmax(0.2, f) == 0.2)
