// detmath_probe.hip -- TEST ONLY (tests/test_gpu_detmath.py): the device math library csrc/nig_detmath.hpp evaluated
// elementwise, one grid-stride kernel per function, built as its own shared library with the product's compiler flags
// (_build.HIPCC_FLAGS) and loaded through ctypes.  libnig.so is not involved.  Every kernel writes only y[0 .. n) (the
// caller passes buffers of n elements) or its own few counters.
#include "../neorl-industrial-gym_amd/csrc/nig_detmath.hpp"

using namespace nig;

#define GRID_STRIDE(i, n) for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < (n); i += (uint64_t)gridDim.x * blockDim.x)

// unary float32 functions at x = the float with bits base + i
template <int F> __device__ __forceinline__ float unary(float x)
{
    if constexpr (F == 0) return det_expf(x);
    else if constexpr (F == 1) return det_logf(x);
    else if constexpr (F == 2) return det_tanhf(x);
    else if constexpr (F == 3) return det_sigmoidf(x);
    else return det_sinf(x);
}
template <int F> __global__ void k_unary(uint32_t base, uint64_t n, float *y)
{
    GRID_STRIDE(i, n) y[i] = unary<F>(__uint_as_float(base + (uint32_t)i));
}

// det_powf(x, yexp) at x = the float with bits base + i step (i < n)
__global__ void k_powf(uint32_t base, uint32_t step, uint64_t n, float yexp, float *y)
{
    GRID_STRIDE(i, n) y[i] = det_powf(__uint_as_float(base + (uint32_t)i * step), yexp);
}

// fdiv_c at every divisor literal of the product (csrc/nig_envs.hpp, csrc/nig_pg_lds.hpp; the test checks the list)
#define FDIV_DIVISORS(X) X(100.0f) X(418000.0f) X(20.0f) X(1000.0f) X(5.0f) X(4180000.0f) X(25000.0f) X(0.001f) X(0.1f) \
    X(673.15f) X(17.0f) X(50.0f) X(3.14159265358979323846f) X(0.05f) X(10.0f)
__host__ __device__ constexpr float fdiv_divisor(int id)
{
    int k = 0;
#define FDIV_VAL(c) if (id == k++) return c;
    FDIV_DIVISORS(FDIV_VAL)
#undef FDIV_VAL
    return 0.0f;
}
#define FDIV_COUNT_ONE(c) +1
constexpr int N_FDIV = 0 FDIV_DIVISORS(FDIV_COUNT_ONE);

// fdiv_c(x, c) against the device's own IEEE x / c (c passed at run time: the generic correctly rounded division) for
// x = bits base .. base + n - 1.  cnt[0], cnt[1]: number and bit sum of the mismatches with |x| < 2^-100; cnt[2], cnt[3]:
// the same for the rest.  NaN == NaN.
template <int ID> __global__ void k_fdiv_check(uint32_t base, uint64_t n, float c_rt, unsigned long long *cnt)
{
    unsigned long long c0 = 0, s0 = 0, c1 = 0, s1 = 0;
    GRID_STRIDE(i, n) {
        const uint32_t b = base + (uint32_t)i;
        const float x = __uint_as_float(b);
        const float q = fdiv_c(x, fdiv_divisor(ID)), w = x / c_rt;
        const bool same = __float_as_uint(q) == __float_as_uint(w) || (q != q && w != w);
        if (!same) {
            if (__builtin_fabsf(x) < 0x1p-100f) { c0++; s0 += b; } else { c1++; s1 += b; }
        }
    }
    if (c0) { atomicAdd(&cnt[0], c0); atomicAdd(&cnt[1], s0); }
    if (c1) { atomicAdd(&cnt[2], c1); atomicAdd(&cnt[3], s1); }
}
// fdiv_c(x, c) itself at x = bits base + i (compared with the oracle's restatement where |x| < 2^-100)
template <int ID> __global__ void k_fdiv_values(uint32_t base, uint64_t n, float *y)
{
    GRID_STRIDE(i, n) y[i] = fdiv_c(__uint_as_float(base + (uint32_t)i), fdiv_divisor(ID));
}
// x / c at run time for given pairs (the test confirms it is IEEE's quotient)
__global__ void k_fdiv_ieee(const float *x, const float *c, uint64_t n, float *y)
{
    GRID_STRIDE(i, n) y[i] = x[i] / c[i];
}

__global__ void k_exp(const double *x, uint64_t n, double *y)
{
    GRID_STRIDE(i, n) y[i] = det_exp(x[i]);
}
__global__ void k_sincos(const double *x, uint64_t n, double *s, double *c)
{
    GRID_STRIDE(i, n) { double sv, cv; det_sincos(x[i], sv, cv); s[i] = sv; c[i] = cv; }
}
// ddiv_y(a, b, RN(1 / b)) against the device's IEEE a / b: mismatches counted in cnt[0]
__global__ void k_ddiv_check(const double *a, const double *b, uint64_t n, unsigned long long *cnt)
{
    unsigned long long bad = 0;
    GRID_STRIDE(i, n) {
        const double y = 1.0 / b[i];
        bad += __double_as_longlong(ddiv_y(a[i], b[i], y)) != __double_as_longlong(a[i] / b[i]);
    }
    if (bad) atomicAdd(&cnt[0], bad);
}
__global__ void k_probit(const uint32_t *w, uint64_t n, float *z)
{
    GRID_STRIDE(i, n) z[i] = probit_normal(w[i], NIG_PROBIT);
}
__global__ void k_philox(const uint32_t *ctr, const uint32_t *key, uint64_t n, uint32_t *out)
{
    GRID_STRIDE(i, n) {
        const u32x4 r = philox4x32(ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3], key[2 * i], key[2 * i + 1]);
        out[4 * i] = r.x; out[4 * i + 1] = r.y; out[4 * i + 2] = r.z; out[4 * i + 3] = r.w;
    }
}

static unsigned grid_for(uint64_t n) { const uint64_t g = (n + 255) / 256; return (unsigned)(g < 8192 ? (g ? g : 1) : 8192); }
static int finish() { return hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess ? 0 : -1; }

template <int ID> static void fdiv_launch(uint32_t base, uint64_t n, unsigned long long *cnt)
{
    k_fdiv_check<ID><<<grid_for(n), 256>>>(base, n, fdiv_divisor(ID), cnt);
}
template <int... I> static int fdiv_dispatch(int id, uint32_t base, uint64_t n, unsigned long long *cnt, std::integer_sequence<int, I...>)
{
    bool hit = false;
    ((id == I ? (fdiv_launch<I>(base, n, cnt), hit = true) : false), ...);
    return hit ? 0 : -2;
}
template <int... I> static int fdiv_values_dispatch(int id, uint32_t base, uint64_t n, float *y, std::integer_sequence<int, I...>)
{
    bool hit = false;
    ((id == I ? (k_fdiv_values<I><<<grid_for(n), 256>>>(base, n, y), hit = true) : false), ...);
    return hit ? 0 : -2;
}

extern "C" {
int probe_n_fdiv(void) { return N_FDIV; }
float probe_fdiv_divisor(int id) { return fdiv_divisor(id); }

int probe_unary(int fn, uint32_t base, uint64_t n, float *y)
{
    switch (fn) {
    case 0: k_unary<0><<<grid_for(n), 256>>>(base, n, y); break;
    case 1: k_unary<1><<<grid_for(n), 256>>>(base, n, y); break;
    case 2: k_unary<2><<<grid_for(n), 256>>>(base, n, y); break;
    case 3: k_unary<3><<<grid_for(n), 256>>>(base, n, y); break;
    case 4: k_unary<4><<<grid_for(n), 256>>>(base, n, y); break;
    default: return -2;
    }
    return finish();
}
int probe_powf(uint32_t base, uint32_t step, uint64_t n, float yexp, float *y)
{
    k_powf<<<grid_for(n), 256>>>(base, step, n, yexp, y);
    return finish();
}
int probe_fdiv_check(int id, uint32_t base, uint64_t n, unsigned long long *cnt)
{
    if (id < 0 || id >= N_FDIV) return -2;
    const int r = fdiv_dispatch(id, base, n, cnt, std::make_integer_sequence<int, N_FDIV>{});
    return r ? r : finish();
}
int probe_fdiv_values(int id, uint32_t base, uint64_t n, float *y)
{
    if (id < 0 || id >= N_FDIV) return -2;
    const int r = fdiv_values_dispatch(id, base, n, y, std::make_integer_sequence<int, N_FDIV>{});
    return r ? r : finish();
}
int probe_fdiv_ieee(const float *x, const float *c, uint64_t n, float *y) { k_fdiv_ieee<<<grid_for(n), 256>>>(x, c, n, y); return finish(); }
int probe_exp(const double *x, uint64_t n, double *y) { k_exp<<<grid_for(n), 256>>>(x, n, y); return finish(); }
int probe_sincos(const double *x, uint64_t n, double *s, double *c) { k_sincos<<<grid_for(n), 256>>>(x, n, s, c); return finish(); }
int probe_ddiv_check(const double *a, const double *b, uint64_t n, unsigned long long *cnt)
{
    k_ddiv_check<<<grid_for(n), 256>>>(a, b, n, cnt);
    return finish();
}
int probe_probit(const uint32_t *w, uint64_t n, float *z) { k_probit<<<grid_for(n), 256>>>(w, n, z); return finish(); }
int probe_philox(const uint32_t *ctr, const uint32_t *key, uint64_t n, uint32_t *out)
{
    k_philox<<<grid_for(n), 256>>>(ctr, key, n, out);
    return finish();
}
}
