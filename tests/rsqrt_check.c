/* rsqrt_check.c -- test infrastructure: accuracy of det_rsqrtf (neorl-industrial-gym_amd/csrc/nig_detmath.hpp) over its whole domain,
 * every positive normal float32, measured on the host restatement (tests/mlp_ln_ref.c, included below: IEEE sqrt, then IEEE
 * division), which tests/test_gpu_rsqrt.py shows equal to the device bit for bit on every one of these inputs.  The reference is
 * 1 / sqrtl(x) in long double; the error is in units of the float32 ulp of the reference's binade.
 * Asserted (tests/test_mlp_ln_host.py; the table in DESIGN.md section 4): <= 1.5 ulp (measured: 1.490349 at 0x1.019566p+2), a normal result for every input.
 * Output: one line, "rsqrtf.normal <worst ulp> <results that are not normal floats> <n> <worst input (hex)>".
 * Build: gcc -O2 -std=gnu11 -ffp-contract=off -fno-fast-math -fopenmp -mfma rsqrt_check.c -lm */
#include "mlp_ln_ref.c"

#include <stdio.h>

int main(void)
{
    double worst = 0.0;
    float at = 0.0f;
    int64_t bad = 0, n = 0;
#pragma omp parallel
    {
        double w = 0.0;
        float a = 0.0f;
        int64_t b = 0, c = 0;
#pragma omp for schedule(static)
        for (int64_t i = 0x00800000; i < 0x7f800000; i++) {
            const uint32_t u = (uint32_t)i;
            float x;
            memcpy(&x, &u, 4);
            const float y = ln_rsqrtf(x);
            const long double r = 1.0L / sqrtl((long double)x);
            int e;
            frexpl(r, &e);
            const double err = (double)(fabsl((long double)y - r) / ldexpl(1.0L, e - 1 - 23));
            c++;
            if (!(y >= 0x1p-126f && y < INFINITY)) b++;
            if (!(err <= w)) { w = err; a = x; }
        }
#pragma omp critical
        {
            if (w > worst || w != w) { worst = w; at = a; }
            bad += b; n += c;
        }
    }
    printf("rsqrtf.normal %.6f %lld %lld %a\n", worst, (long long)bad, (long long)n, (double)at);
    return 0;
}
