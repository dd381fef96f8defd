// ctr_math_probe.hip -- test-only device probe of csrc/ctr_math.hpp and of the trig-table helpers
// of csrc/ctr_device.hpp (tests/test_gpu_math.py builds it with the product's compiler and flags).
// Not part of libctr_reach_amd.so: one elementwise kernel per probed function, so the device
// branches (#if __HIP_DEVICE_COMPILE__) and the FMA-contracted code are what the tests see.
//
// Every kernel runs 256-lane workgroups; a lane past n computes on the clamped last element and
// does not store, so every lane of a wave reaches the ballots of sincos_lds / trig_of.
// Launchers return 0, -1 for a null pointer or n <= 0, or the hipError_t of the launch.
#include "ctr_device.hpp"

namespace {

using namespace ctr;

enum { FILL_LOOP = 0, FILL_SPLIT = 1 };   // trig_table_fill | trig_table_load + trig_table_store
enum { OP_RCP_EST = 0, OP_RCP1, OP_SQRT_RSQ, OP_INV_ROOT10, OP_GAP_UP };

// Element of this lane (clamped to n - 1) and whether it may store.
__device__ __forceinline__ long probe_elem(long n, bool &live)
{
    const long i = (long)blockIdx.x * CTR_BLOCK + threadIdx.x;
    live = i < n;
    return live ? i : n - 1;
}

template <int FILL>
__device__ __forceinline__ void probe_fill()
{
    if (FILL == FILL_LOOP) {
        trig_table_fill();
    } else {
        TrigRegs t;
        trig_table_load(t);
        trig_table_store(t);
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_probe_sincos_cw(const double *x, double *s, double *c, long n)
{
    bool live;
    const long i = probe_elem(n, live);
    double sv, cv;
    ctr_math::sincos_cw(x[i], &sv, &cv);
    if (live) {
        s[i] = sv;
        c[i] = cv;
    }
}

template <int FILL>
__global__ __launch_bounds__(256) void k_probe_sincos_lds(const double *x, double *s, double *c, long n)
{
    probe_fill<FILL>();
    bool live;
    const long i = probe_elem(n, live);
    double sv, cv;
    sincos_lds(x[i], sv, cv);
    if (live) {
        s[i] = sv;
        c[i] = cv;
    }
}

// One workgroup: the 1024 doubles of s_trig_tab after the fill.
template <int FILL>
__global__ __launch_bounds__(256) void k_probe_tab_dump(double *out)
{
    probe_fill<FILL>();
    #pragma unroll
    for (int k = 0; k < 4; ++k) out[threadIdx.x + k * CTR_BLOCK] = (&s_trig_tab[0][0])[threadIdx.x + k * CTR_BLOCK];
}

// al: n x 3 row-major; out: n x 6 row-major (s10, c10, s20, c20, s21, c21).
template <bool CAREFUL>
__global__ __launch_bounds__(256) void k_probe_trig_of(const double *al, double *out, long n)
{
    probe_fill<FILL_LOOP>();
    bool live;
    const long i = probe_elem(n, live);
    const double a[3] = {al[3 * i], al[3 * i + 1], al[3 * i + 2]};
    const Trig t = trig_of<CAREFUL>(a);
    if (live) {
        double *o = out + 6 * i;
        o[0] = t.s10;
        o[1] = t.c10;
        o[2] = t.s20;
        o[3] = t.c20;
        o[4] = t.s21;
        o[5] = t.c21;
    }
}

template <int OP>
__global__ __launch_bounds__(256) void k_probe_unary(const double *x, double *y, long n)
{
    bool live;
    const long i = probe_elem(n, live);
    const double v = x[i];
    double r = 0.0;
    if (OP == OP_RCP_EST) r = ctr_math::rcp_est(v);
    if (OP == OP_RCP1) r = ctr_math::rcp1(v);
    if (OP == OP_SQRT_RSQ) r = ctr_math::sqrt_rsq(v);
    if (OP == OP_INV_ROOT10) r = ctr_math::inv_root10(v);
    if (OP == OP_GAP_UP) r = ctr_math::gap_up(v);
    if (live) y[i] = r;
}

__global__ __launch_bounds__(256) void k_probe_absmax(const double *a, const double *b, double *y, long n)
{
    bool live;
    const long i = probe_elem(n, live);
    const double r = ctr_math::absmax(a[i], b[i]);
    if (live) y[i] = r;
}

inline unsigned probe_blocks(long n) { return (unsigned)((n + CTR_BLOCK - 1) / CTR_BLOCK); }

inline int probe_status() { return (int)hipGetLastError(); }

template <int OP>
int probe_unary(const double *x, double *y, long n, hipStream_t stream)
{
    if (!x || !y || n <= 0) return -1;
    hipLaunchKernelGGL(k_probe_unary<OP>, dim3(probe_blocks(n)), dim3(CTR_BLOCK), 0, stream, x, y, n);
    return probe_status();
}

}  // namespace

extern "C" {

int probe_sincos_cw(const double *x, double *s, double *c, long n, hipStream_t stream)
{
    if (!x || !s || !c || n <= 0) return -1;
    hipLaunchKernelGGL(k_probe_sincos_cw, dim3(probe_blocks(n)), dim3(CTR_BLOCK), 0, stream, x, s, c, n);
    return probe_status();
}

// fill: 0 = trig_table_fill, 1 = trig_table_load + trig_table_store
int probe_sincos_lds(const double *x, double *s, double *c, long n, int fill, hipStream_t stream)
{
    if (!x || !s || !c || n <= 0 || (fill != FILL_LOOP && fill != FILL_SPLIT)) return -1;
    if (fill == FILL_LOOP)
        hipLaunchKernelGGL(k_probe_sincos_lds<FILL_LOOP>, dim3(probe_blocks(n)), dim3(CTR_BLOCK), 0, stream, x, s, c, n);
    else
        hipLaunchKernelGGL(k_probe_sincos_lds<FILL_SPLIT>, dim3(probe_blocks(n)), dim3(CTR_BLOCK), 0, stream, x, s, c, n);
    return probe_status();
}

// out: 1024 doubles
int probe_tab_dump(double *out, int fill, hipStream_t stream)
{
    if (!out || (fill != FILL_LOOP && fill != FILL_SPLIT)) return -1;
    if (fill == FILL_LOOP)
        hipLaunchKernelGGL(k_probe_tab_dump<FILL_LOOP>, dim3(1), dim3(CTR_BLOCK), 0, stream, out);
    else
        hipLaunchKernelGGL(k_probe_tab_dump<FILL_SPLIT>, dim3(1), dim3(CTR_BLOCK), 0, stream, out);
    return probe_status();
}

int probe_trig_of(const double *al, double *out, long n, int careful, hipStream_t stream)
{
    if (!al || !out || n <= 0) return -1;
    if (careful)
        hipLaunchKernelGGL(k_probe_trig_of<true>, dim3(probe_blocks(n)), dim3(CTR_BLOCK), 0, stream, al, out, n);
    else
        hipLaunchKernelGGL(k_probe_trig_of<false>, dim3(probe_blocks(n)), dim3(CTR_BLOCK), 0, stream, al, out, n);
    return probe_status();
}

int probe_rcp_est(const double *x, double *y, long n, hipStream_t stream) { return probe_unary<OP_RCP_EST>(x, y, n, stream); }
int probe_rcp1(const double *x, double *y, long n, hipStream_t stream) { return probe_unary<OP_RCP1>(x, y, n, stream); }
int probe_sqrt_rsq(const double *x, double *y, long n, hipStream_t stream) { return probe_unary<OP_SQRT_RSQ>(x, y, n, stream); }
int probe_inv_root10(const double *x, double *y, long n, hipStream_t stream) { return probe_unary<OP_INV_ROOT10>(x, y, n, stream); }
int probe_gap_up(const double *x, double *y, long n, hipStream_t stream) { return probe_unary<OP_GAP_UP>(x, y, n, stream); }

int probe_absmax(const double *a, const double *b, double *y, long n, hipStream_t stream)
{
    if (!a || !b || !y || n <= 0) return -1;
    hipLaunchKernelGGL(k_probe_absmax, dim3(probe_blocks(n)), dim3(CTR_BLOCK), 0, stream, a, b, y, n);
    return probe_status();
}

}  // extern "C"
