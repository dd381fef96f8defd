"""The device builds of the fp64 primitives of csrc/ctr_math.hpp and of the trig-table helpers of
csrc/ctr_device.hpp, run on the GPU.  tests/test_math.py compiles the header for the host without
FMA contraction, which is the `#else` of every `#if defined(__HIP_DEVICE_COMPILE__)` and another
instruction sequence than the kernels'; here tests/probes/ctr_math_probe.hip (one elementwise kernel
per function) is built with the compiler and flags of gym-ctr-reach_amd/Makefile and compared with
mpmath at 40+ digits, with numpy, and bit for bit with the host build where that is derivable.

What this pins: the primitives as compiled stand-alone with the product's flags.  Inlined into a
product kernel, contraction across a call boundary could in principle differ (a product of the
caller fused into the callee's sum); the end-to-end parity tests cover the kernels, at 1e-10 m.

No bar below is tuned to the device's output: each is a claim of the header, test_math.py's bar for
the host build, or derived in the test's docstring.  Every test prints the maximum it measured.

Not fed to any kernel: rcp1(0.0), which is inf or NaN.  Its one caller with a possibly zero argument
is select_initial_step's h0n = 0.01 sqrt_rsq(s0 rcp1(s1)) in ctr_device.hpp, and the select on the
next line replaces h0n by 1e-6 whenever d1sq = s1 / 18 < 1e-10 (so for s1 = 0) before any use; the
other caller passes h0 >= min(1e-6, interval) > 0."""
import ctypes
import os
import shlex
import subprocess

import numpy as np
import pytest

from test_math import (ROOT, UNGUARDED_TAIL, _lib, _run_sincos, _ulp_err, check_sincos, gap_up_args,
                       inv_root10_sqrt_args, makefile_var, sincos_args, sincos_edge_args)

pytestmark = pytest.mark.gpu

MAX_N = (1 << 18) - 1          # points per launch: at most 2^18 and no multiple of the 256-lane workgroup
PAD = 300                      # sentinel doubles behind every output: lanes past n must not store
SENTINEL = 0x7FF8_0BAD_5EED_0001
FILL_LOOP, FILL_SPLIT = 0, 1   # trig_table_fill | trig_table_load + trig_table_store
UNARY = ("rcp_est", "rcp1", "sqrt_rsq", "inv_root10", "gap_up")


class Probe:
    def __init__(self, lib, device):
        import torch
        self.torch, self.lib, self.device = torch, lib, device
        ptr, i64 = ctypes.c_void_p, ctypes.c_long
        lib.probe_sincos_cw.argtypes = [ptr, ptr, ptr, i64, ptr]
        lib.probe_sincos_lds.argtypes = [ptr, ptr, ptr, i64, ctypes.c_int, ptr]
        lib.probe_tab_dump.argtypes = [ptr, ctypes.c_int, ptr]
        lib.probe_trig_of.argtypes = [ptr, ptr, i64, ctypes.c_int, ptr]
        for f in UNARY:
            getattr(lib, "probe_" + f).argtypes = [ptr, ptr, i64, ptr]
        lib.probe_absmax.argtypes = [ptr, ptr, ptr, i64, ptr]

    def stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.device)

    def out(self, n):
        return self.dev(np.full(n + PAD, SENTINEL, dtype=np.uint64).view(np.float64))

    def host(self, t, n):
        """The first n doubles of output t, after checking that nothing was stored behind them."""
        self.torch.cuda.synchronize(self.device)
        a = t.cpu().numpy()
        assert (a[n:].view(np.uint64) == SENTINEL).all(), "a lane past n stored"
        return a[:n].copy()

    def map(self, fn, ins, extra=(), nout=1):
        """Launcher fn(ins..., outs..., n, extra..., stream) over the float64 vectors `ins`, in
        launches of at most MAX_N points, each no multiple of 256 (the last workgroup has lanes
        past n)."""
        n = len(ins[0])
        outs = [[] for _ in range(nout)]
        for lo in range(0, n, MAX_N):
            m = min(MAX_N, n - lo)
            assert m % 256 != 0, m
            di = [self.dev(a[lo:lo + m]) for a in ins]
            do = [self.out(m) for _ in range(nout)]
            rc = getattr(self.lib, fn)(*[t.data_ptr() for t in di], *[t.data_ptr() for t in do], m, *extra, self.stream())
            assert rc == 0, (fn, rc)
            for k, t in enumerate(do):
                outs[k].append(self.host(t, m))
        return [np.concatenate(o) for o in outs]

    def unary(self, f, x):
        return self.map("probe_" + f, [x])[0]

    def sincos_cw(self, x):
        return self.map("probe_sincos_cw", [x], nout=2)

    def sincos_lds(self, x, fill):
        return self.map("probe_sincos_lds", [x], nout=2, extra=(fill,))

    def trig_of(self, al, careful):
        """al: n x 3 -> n x 6 (s10, c10, s20, c20, s21, c21)."""
        n = len(al)
        assert n <= MAX_N and n % 256 != 0
        di, do = self.dev(al.reshape(-1)), self.out(6 * n)
        rc = self.lib.probe_trig_of(di.data_ptr(), do.data_ptr(), n, int(careful), self.stream())
        assert rc == 0, rc
        return self.host(do, 6 * n).reshape(n, 6)

    def tab_dump(self, fill):
        do = self.out(1024)
        rc = self.lib.probe_tab_dump(do.data_ptr(), fill, self.stream())
        assert rc == 0, rc
        return self.host(do, 1024)


@pytest.fixture(scope="module")
def probe(cuda, tmp_path_factory):
    """The probe, built as the Makefile builds the product: its HIPCC and HIPFLAGS lines (the
    include paths are relative to gym-ctr-reach_amd, so hipcc runs there)."""
    flags = shlex.split(makefile_var("HIPFLAGS").replace("$(ARCH)", makefile_var("ARCH")))
    assert "-shared" in flags and "--offload-arch=gfx950" in flags, flags
    so = tmp_path_factory.mktemp("ctr_math_probe") / "ctr_math_probe.so"
    subprocess.check_call([makefile_var("HIPCC"), *flags, os.path.join(ROOT, "tests", "probes", "ctr_math_probe.hip"),
                           "-o", str(so)], cwd=os.path.join(ROOT, "gym-ctr-reach_amd"))
    return Probe(ctypes.CDLL(str(so)), cuda)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """The host build of test_math.py (g++, -ffp-contract=off)."""
    return _lib(tmp_path_factory.mktemp("ctr_math_host"))


def host_tab(host, x):
    return _run_sincos(host, "vsincos_tab", np.ascontiguousarray(x))


def mp_sincos(x):
    """(sin hi, sin lo, cos hi, cos lo): mpmath at 40 digits as double-double."""
    import mpmath
    out = np.empty((len(x), 4))
    with mpmath.workdps(40):
        for i, v in enumerate(x):
            c, s = mpmath.cos_sin(mpmath.mpf(float(v)))
            sh, ch = float(s), float(c)
            out[i] = sh, float(s - sh), ch, float(c - ch)
    return out.T


def dd_err(got, hi, lo):
    """|got - (hi + lo)|: got - hi is exact for a result within a few ulp of hi."""
    return np.abs((got - hi) - lo)


def check_sincos_mp(s, c, ref, what):
    """The sincos bar against the 40-digit reference: < 4e-16 absolute, <= 2 ulp above 1e-3."""
    sh, sl, ch, cl = ref
    es, ec = dd_err(s, sh, sl), dd_err(c, ch, cl)
    assert es.max() < 4e-16 and ec.max() < 4e-16, (what, es.max(), ec.max())
    us = (es / np.spacing(np.abs(sh)))[np.abs(sh) > 1e-3].max()
    uc = (ec / np.spacing(np.abs(ch)))[np.abs(ch) > 1e-3].max()
    assert us <= 2.0 and uc <= 2.0, (what, us, uc)
    return max(es.max(), ec.max()), max(us, uc)


def same_bits(a, b):
    return a.view(np.uint64) == b.view(np.uint64)


@pytest.fixture(scope="module")
def sincos_set():
    """x: test_math.py's sincos arguments plus the edges of the table reduction (all |x| < 2^20);
    idx / ref: the subsample (every 20th random argument, 22 500, and every structured and edge
    point) with its mpmath reference."""
    base, edge = sincos_args(), sincos_edge_args()
    x = np.concatenate([base, edge])
    idx = np.concatenate([np.arange(0, 450000, 20), np.arange(450000, len(x))])
    return x, idx, mp_sincos(x[idx])


def test_launchers_validate(probe):
    y = probe.out(8)
    for f in UNARY:
        fn = getattr(probe.lib, "probe_" + f)
        assert fn(None, y.data_ptr(), 8, probe.stream()) == -1
        assert fn(y.data_ptr(), None, 8, probe.stream()) == -1
        assert fn(y.data_ptr(), y.data_ptr(), 0, probe.stream()) == -1
        assert fn(y.data_ptr(), y.data_ptr(), -3, probe.stream()) == -1
    p = y.data_ptr()
    assert probe.lib.probe_sincos_cw(p, None, p, 8, probe.stream()) == -1
    assert probe.lib.probe_sincos_lds(p, p, None, 8, FILL_LOOP, probe.stream()) == -1
    assert probe.lib.probe_sincos_lds(p, p, p, 8, 2, probe.stream()) == -1
    assert probe.lib.probe_tab_dump(None, FILL_LOOP, probe.stream()) == -1
    assert probe.lib.probe_trig_of(p, None, 1, 1, probe.stream()) == -1
    assert probe.lib.probe_absmax(p, p, None, 8, probe.stream()) == -1
    probe.host(y, 8)


@pytest.mark.parametrize("fill", [FILL_LOOP, FILL_SPLIT])
def test_table_in_lds(probe, host, fill):
    """Both copies of the table into LDS give the 1024 doubles of TRIG_TAB bit for bit
    (test_math.py checks TRIG_TAB itself against mpmath)."""
    want = np.array(host.trig_tab().contents)
    got = probe.tab_dump(fill)
    bad = np.flatnonzero(~same_bits(got, want))
    print("s_trig_tab after fill %d: %d of 1024 doubles differ" % (fill, len(bad)))
    assert len(bad) == 0, (bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("fill", [FILL_LOOP, FILL_SPLIT])
def test_sincos_lds_matches_host_bits(probe, host, sincos_set, fill):
    """sincos_lds for |x| < 2^20 is bit-equal to the host build of sincos_tab: every operation of
    sincos_tab2_pre / _post is an explicit fma, a lone product or rint, so contraction has nothing
    to fuse (test_math.py::test_sincos_contraction_invariance shows it on the host), and rint, fma
    and the products are correctly rounded on both.  Also test_math.py's accuracy bar, against
    np.sin / np.cos over the whole set and against mpmath on the subsample."""
    x, idx, ref = sincos_set
    s, c = probe.sincos_lds(x, fill)
    hs, hc = host_tab(host, x)
    same = same_bits(s, hs) & same_bits(c, hc)
    print("sincos_lds fill %d: %d of %d arguments differ from the host bits" % (fill, (~same).sum(), len(x)))
    assert same.all(), (x[~same][:5], s[~same][:5], hs[~same][:5], c[~same][:5], hc[~same][:5])
    a_np, u_np = check_sincos(x, s, c, "sincos_lds")
    a_mp, u_mp = check_sincos_mp(s[idx], c[idx], ref, "sincos_lds")
    print("sincos_lds fill %d: max abs %.3g / %.3f ulp vs numpy (%d points), %.3g / %.3f ulp vs mpmath (%d points)"
          % (fill, a_np, u_np, len(x), a_mp, u_mp, len(idx)))


BIG = [2.0 ** 20, 2.0 ** 20 + 0.5, -3e7, 1e9, -1e15, np.inf, np.nan]


@pytest.mark.parametrize("fill", [FILL_LOOP, FILL_SPLIT])
def test_sincos_lds_mixed_waves(probe, host, fill):
    """The wave-uniform ballot of sincos_lds.  Four workgroups, one per pair of BIG values, each of
    three waves (and a fourth of ordinary angles in all but the last, so that n is no multiple of
    256): every lane >= 2^20; no lane; only lanes 3 and 40.  Ordinary lanes keep the host bits of
    sincos_tab whatever their wave does; finite big lanes are within 2 ulp (above 1e-3) and 4e-16
    of mpmath, the header's claim for the exact path and the accuracy HIP documents for fp64 sin /
    cos; inf and NaN give NaN in both outputs."""
    rng = np.random.default_rng(10)
    pairs = [(BIG[i], BIG[(i + 1) % len(BIG)]) for i in range(0, 8, 2)]
    blocks = []
    for a, b in pairs:
        blk = rng.uniform(-300, 300, 256)
        blk[:64] = rng.uniform(2.0 ** 20, 1e9, 64) * rng.choice([-1.0, 1.0], 64)
        blk[128 + 3], blk[128 + 40] = a, b
        blocks.append(blk)
    x = np.concatenate(blocks)[:-64]
    assert len(x) == 960
    s, c = probe.sincos_lds(x, fill)
    with np.errstate(invalid="ignore"):
        big = ~(np.abs(x) < 2.0 ** 20)
    assert big.sum() == 4 * 64 + 8
    hs, hc = host_tab(host, x[~big])
    assert (same_bits(s[~big], hs) & same_bits(c[~big], hc)).all()
    fin = big & np.isfinite(x)
    a_mp, u_mp = check_sincos_mp(s[fin], c[fin], mp_sincos(x[fin]), "sincos_lds exact path")
    assert np.isnan(s[~np.isfinite(x)]).all() and np.isnan(c[~np.isfinite(x)]).all()
    assert (~np.isfinite(x)).sum() == 2
    print("sincos_lds fill %d, exact path: max abs %.3g / %.3f ulp vs mpmath (%d lanes)" % (fill, a_mp, u_mp, fin.sum()))


def test_sincos_cw_device(probe, host, sincos_set):
    """sincos_cw on the device within test_math.py's bar.  Not bit-equal to the host build: its
    polynomial sums contract differently."""
    x, idx, ref = sincos_set
    s, c = probe.sincos_cw(x)
    hs, hc = _run_sincos(host, "vsincos", x)
    a_np, u_np = check_sincos(x, s, c, "sincos_cw")
    a_mp, u_mp = check_sincos_mp(s[idx], c[idx], ref, "sincos_cw")
    print("sincos_cw: max abs %.3g / %.3f ulp vs numpy (%d points), %.3g / %.3f ulp vs mpmath (%d points); "
          "%d results differ from the uncontracted host build"
          % (a_np, u_np, len(x), a_mp, u_mp, len(idx), (~(same_bits(s, hs) & same_bits(c, hc))).sum()))
    xb = np.concatenate([[1e6, 3e7, 2.0 ** 20, -2.0 ** 20 - 0.5, -1e15], x[:250]])      # the exact path, 255 lanes
    sb, cb = probe.sincos_cw(xb)
    a_b, u_b = check_sincos_mp(sb, cb, mp_sincos(xb), "sincos_cw exact path")
    print("sincos_cw with big lanes: max abs %.3g / %.3f ulp vs mpmath" % (a_b, u_b))


def _alphas():
    rng = np.random.default_rng(11)
    return np.concatenate([rng.uniform(-300, 300, (12000, 3)), rng.uniform(-np.pi, np.pi, (12001, 3))])


def test_trig_of(probe, host):
    """trig_of: s10, c10, s20, c20 are the host bits of sincos_tab of the float64 differences
    al[1] - al[0], al[2] - al[0]; trig_of<false> equals trig_of<true> bit for bit (all |d| < 2^20);
    c21 / s21 from the angle-difference identity are within 2e-15 of mpmath's cos / sin of
    d20 - d10 (exact difference): four factors each within 4e-16 of a value of magnitude <= 1
    (asserted above) give 1.6e-15, plus three roundings of 1.1e-16."""
    import mpmath
    al = _alphas()
    d10, d20 = al[:, 1] - al[:, 0], al[:, 2] - al[:, 0]
    t = probe.trig_of(al, True)
    f = probe.trig_of(al, False)
    assert same_bits(t, f).all(), np.argwhere(~same_bits(t, f))[:5]
    s10, c10 = host_tab(host, d10)
    s20, c20 = host_tab(host, d20)
    want = np.stack([s10, c10, s20, c20], axis=1)
    same = same_bits(t[:, :4], want)
    print("trig_of: %d of %d table results differ from the host bits" % ((~same).sum(), same.size))
    assert same.all(), (al[~same.all(axis=1)][:3], t[~same.all(axis=1)][:3])
    ref = np.empty((len(al), 4))
    with mpmath.workdps(40):
        for i in range(len(al)):
            c, s = mpmath.cos_sin(mpmath.mpf(float(d20[i])) - mpmath.mpf(float(d10[i])))
            sh, ch = float(s), float(c)
            ref[i] = sh, float(s - sh), ch, float(c - ch)
    e = max(dd_err(t[:, 4], ref[:, 0], ref[:, 1]).max(), dd_err(t[:, 5], ref[:, 2], ref[:, 3]).max())
    print("trig_of: s21 / c21 max abs error %.3g vs mpmath (%d rows)" % (e, len(al)))
    assert e <= 2e-15, e


def test_trig_of_careful_big(probe, host):
    """trig_of<true> with lanes whose differences reach 2^20: those pairs take the exact path
    (2 ulp / 4e-16 of mpmath, NaN for non-finite), every other pair keeps the host bits."""
    al = _alphas()[:191].copy()
    al[5, 1] = 3e7                      # d10 big, d20 ordinary
    al[70, 2] = -1e15                   # d20 big
    al[71, 0] = 2.0 ** 21               # both big
    al[130, 1] = np.inf                 # d10 inf
    with np.errstate(invalid="ignore"):
        d = np.stack([al[:, 1] - al[:, 0], al[:, 2] - al[:, 0]], axis=1)
        big = ~(np.abs(d) < 2.0 ** 20)
    assert big.sum() == 5
    t = probe.trig_of(al, True)
    s, c = t[:, [0, 2]], t[:, [1, 3]]
    hs, hc = host_tab(host, d[~big])
    assert (same_bits(s[~big], hs) & same_bits(c[~big], hc)).all()
    fin = big & np.isfinite(d)
    a_mp, u_mp = check_sincos_mp(s[fin], c[fin], mp_sincos(d[fin]), "trig_of exact path")
    assert np.isnan(s[130, 0]) and np.isnan(c[130, 0])
    print("trig_of<true>, exact path: max abs %.3g / %.3f ulp vs mpmath" % (a_mp, u_mp))


def _two_prod_err(a, b):
    """a * b - fl(a * b) exactly (Dekker; no overflow or underflow for the magnitudes used here)."""
    def split(v):
        t = 134217729.0 * v
        hi = t - (t - v)
        return hi, v - hi
    p = a * b
    ah, al = split(a)
    bh, bl = split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _rcp_args():
    """Random mantissas with exponents -40..40, both signs, and the powers of two."""
    rng = np.random.default_rng(12)
    x = np.ldexp(rng.uniform(1, 2, 200001), rng.integers(-40, 41, 200001)) * rng.choice([-1.0, 1.0], 200001)
    p2 = np.ldexp(1.0, np.arange(-40, 41))
    return np.concatenate([x, p2, -p2, np.nextafter(p2, 0), np.nextafter(p2, np.inf)])


def _rcp_rel(x, r):
    """|x r - 1|, the relative error of r as 1/x, exact to ~1e-32 (fl(x r) - 1 is exact near 1)."""
    p, e = _two_prod_err(x, r)
    return np.abs((p - 1.0) + e)


def test_rcp_est(probe):
    """The bare v_rcp_f64 estimate: relative error <= 2^-24 (the header's bound)."""
    x = _rcp_args()
    r = probe.unary("rcp_est", x)
    rel = _rcp_rel(x, r)
    print("rcp_est: max relative error %.4g = 2^%.2f, %.3g ulp (%d points)"
          % (rel.max(), np.log2(rel.max()), _ulp_err(r, 1.0 / x).max(), len(x)))
    assert rel.max() <= 2.0 ** -24


def test_rcp1(probe):
    """rcp1 = one Newton step on the estimate r0 = (1 - e0) / x, |e0| <= 2^-24 (asserted above):
    fl(1 - x r0) = e0 (1 + d1) and r1 = r0 (1 + e) (1 + d2) with |d| <= 2^-53, so
    x r1 = (1 - e0^2 + e0 d1 (1 - e0)) (1 + d2): relative error <= 2^-48 + 2^-53 + 2^-77, below
    the asserted 2^-48 + 2^-52."""
    x = _rcp_args()
    r = probe.unary("rcp1", x)
    rel = _rcp_rel(x, r)
    print("rcp1: max relative error %.4g = 2^%.2f, %.3f ulp of the exact quotient (%d points)"
          % (rel.max(), np.log2(rel.max()), (rel / (np.spacing(np.abs(1.0 / x)) * np.abs(x))).max(), len(x)))
    assert rel.max() <= 2.0 ** -48 + 2.0 ** -52


def test_sqrt_rsq(probe):
    """sqrt_rsq within 2 ulp of np.sqrt on 10^U(-30, 30): test_math.py's bar and domain."""
    xs = inv_root10_sqrt_args()[1]
    s = probe.unary("sqrt_rsq", xs)
    u = _ulp_err(s, np.sqrt(xs))
    print("sqrt_rsq: max %.3f ulp vs np.sqrt, %d of %d not correctly rounded" % (u.max(), (u > 0).sum(), len(xs)))
    assert u.max() <= 2.0


def test_inv_root10(probe):
    """inv_root10 within 2 ulp of x^-0.1 over test_math.py's set (the whole positive range,
    1e-310 and 5e-324 included).  Reference: 1 / root(x, 10) in mpmath at 50 digits on every 13th
    point (23 077) and the 8 edge values; Decimal, as test_math.py uses on 3 101 points, takes
    2 ms a point."""
    import mpmath
    x = inv_root10_sqrt_args()[0]
    y = probe.unary("inv_root10", x)
    idx = np.concatenate([np.arange(0, len(x) - 8, 13), np.arange(len(x) - 8, len(x))])
    hi, lo = np.empty(len(idx)), np.empty(len(idx))
    with mpmath.workdps(50):
        for i, v in enumerate(x[idx]):
            w = 1 / mpmath.root(mpmath.mpf(float(v)), 10)
            hi[i] = float(w)
            lo[i] = float(w - hi[i])
    u = dd_err(y[idx], hi, lo) / np.spacing(hi)
    print("inv_root10: max %.3f ulp vs mpmath (%d points)" % (u.max(), len(idx)))
    assert u.max() <= 2.0


def test_inv_root10_unguarded_tail(probe):
    """test_math.py::test_inv_root10_unguarded_tail on the device: 0.9 inv_root10(err^2) is NaN or
    below 0.2 for a huge, infinite or NaN err^2."""
    x = np.concatenate([UNGUARDED_TAIL, np.full(5, 1e300)])
    f = 0.9 * probe.unary("inv_root10", x)
    print("inv_root10 tail: 0.9 y =", f[:len(UNGUARDED_TAIL)])
    assert np.all(np.isnan(f) | (f < 0.2)), f
    assert np.all(np.fmax(0.2, f) == 0.2)


def test_gap_up(probe):
    """gap_up(t) == nextafter(t, inf) - t bit for bit over test_math.py's whole set."""
    x, want = gap_up_args()
    y = probe.unary("gap_up", x)
    same = same_bits(y, want) | (np.isnan(y) & np.isnan(want))
    print("gap_up: %d of %d differ" % ((~same).sum(), len(x)))
    assert same.all(), (x[~same][:5], y[~same][:5], want[~same][:5])


QNAN = np.nan
SNAN = np.array([0x7FF0_0000_0000_0001], dtype=np.uint64).view(np.float64)[0]


def test_absmax(probe):
    """absmax(a, b) (one v_max_f64 with abs modifiers) is np.fmax(|a|, |b|) bit for bit over every
    pair of finite values, infinities, signed zeros and subnormals.  With one NaN operand the result
    may be NaN or the other operand's magnitude; with two it is NaN."""
    # What the MI355X gives (printed below): with a quiet NaN of either sign, on either side, the
    # other operand's magnitude in all 50 cases, as fmax does; with a signalling NaN, NaN in all 50.
    rng = np.random.default_rng(13)
    v = np.concatenate([[0.0, -0.0, 5e-324, -5e-324, 2.2250738585072009e-308, -1e-310, 2.2250738585072014e-308,
                         1.0, -1.0, np.nextafter(1.0, 2), -np.nextafter(1.0, 0), 1.7976931348623157e308,
                         -1.7976931348623157e308, np.inf, -np.inf],
                        rng.normal(0, 1, 100), 10.0 ** rng.uniform(-320, 308, 80) * rng.choice([-1.0, 1.0], 80)])
    a, b = [m.reshape(-1) for m in np.meshgrid(v, v, indexing="ij")]
    assert len(a) % 256 != 0
    y = probe.map("probe_absmax", [a, b])[0]
    want = np.fmax(np.abs(a), np.abs(b))
    same = same_bits(y, want)
    print("absmax: %d of %d pairs differ from fmax(|a|, |b|)" % ((~same).sum(), len(a)))
    assert same.all(), (a[~same][:5], b[~same][:5], y[~same][:5])
    # one NaN operand, either side, quiet and signalling; two NaNs
    w = np.concatenate([v[:15], v[15:25]])
    for name, nan in (("quiet", QNAN), ("signalling", SNAN), ("negative quiet", -QNAN)):
        n1 = np.full(len(w), nan)
        got = probe.map("probe_absmax", [np.concatenate([n1, w, n1[:3]]), np.concatenate([w, n1, n1[:3]])])[0]
        other = np.abs(np.concatenate([w, w]))
        one = got[:2 * len(w)]
        is_other = same_bits(one, other)
        print("absmax with one %s NaN: %d NaN, %d the other operand's magnitude (of %d)"
              % (name, np.isnan(one).sum(), is_other.sum(), len(one)))
        assert (np.isnan(one) | is_other).all(), (one, other)
        assert np.isnan(got[2 * len(w):]).all()
