// rsqrt_probe.hip -- TEST ONLY (tests/test_gpu_rsqrt.py): det_rsqrtf of csrc/nig_detmath.hpp evaluated elementwise by a grid-stride
// kernel, built as its own shared library with the product's compiler flags (_build.HIPCC_FLAGS, tests/detmath_probe.hip's pattern) and
// loaded through ctypes.  libnig.so is not involved.  The kernel writes only y[0 .. n): the caller passes a buffer of n elements.
#include "../neorl-industrial-gym_amd/csrc/nig_detmath.hpp"

using namespace nig;

// det_rsqrtf at x = the float with bits base + i
__global__ void k_rsqrt(uint32_t base, uint64_t n, float *y)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        y[i] = det_rsqrtf(__uint_as_float(base + (uint32_t)i));
}

extern "C" int probe_rsqrt(uint32_t base, uint64_t n, float *y)
{
    const uint64_t g = (n + 255) / 256;
    k_rsqrt<<<(unsigned)(g < 8192 ? (g ? g : 1) : 8192), 256>>>(base, n, y);
    return hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess ? 0 : -1;
}
