/* det_expf (csrc/nig_detmath.hpp) scales its polynomial p by 2^k.  The former form split k = k1 + k2 and multiplied twice,
 * (p 2^k1) 2^k2 -- the first product exact, the second rounding once; the present form is ldexpf(p, k), one rounding of the
 * same exact value (v_ldexp_f32 on the device).  This program compares the two bit for bit on the function's own p and k:
 *   - every float x with -103 <= x < -87: the only inputs whose result can be subnormal, i.e. where anything is rounded;
 *   - the rest of [-103, 88.72283]: every STRIDE-th float (by bit pattern; default 127 -> 17.6 M inputs), or every float
 *     when run with the argument "all" (2.2e9 inputs, recorded in profiles/split_once/expf_exhaustive.txt);
 *   - the overridden ranges (x < -103 -> 0, x > 88.72283 -> inf, NaN -> x): the same bits from both.
 * The oracle (oracle/) keeps the two-step form: device == oracle bit for bit rests on this identity.
 * Test infrastructure (tests/test_expf_scale.py).  Compile with -ffp-contract=off. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

static float bits_f32(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t f32_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

/* the part both forms share: k (clamped as the former form clamped it) and the polynomial */
static float poly_and_k(float x, int *k)
{
    float fk = floorf(fmaf(x, 1.44269504088896341f, 0.5f));
    float r = fmaf(-fk, 0.693359375f, x);
    r = fmaf(-fk, -2.12194440e-4f, r);
    const float z = r * r;
    float p = 1.9875691500e-4f;
    p = fmaf(p, r, 1.3981999507e-3f);
    p = fmaf(p, r, 8.3334519073e-3f);
    p = fmaf(p, r, 4.1665795894e-2f);
    p = fmaf(p, r, 1.6666665459e-1f);
    p = fmaf(p, r, 5.0000001201e-1f);
    p = fmaf(p, z, r);
    p = p + 1.0f;
    fk = fminf(fmaxf(fk, -200.0f), 200.0f);      /* (a NaN becomes -200, as on the device) */
    *k = (int)fk;
    return p;
}
static float override(float x, float res)
{
    res = (x < -103.0f) ? 0.0f : res;
    res = (x > 88.72283f) ? INFINITY : res;
    res = (x != x) ? x : res;
    return res;
}
static float expf_two_step(float x)
{
    int k;
    const float p = poly_and_k(x, &k);
    const int k1 = k / 2, k2 = k - k1;
    return override(x, (p * bits_f32((uint32_t)(k1 + 127) << 23)) * bits_f32((uint32_t)(k2 + 127) << 23));
}
static float expf_ldexp(float x)
{
    int k;
    const float p = poly_and_k(x, &k);
    return override(x, ldexpf(p, k));
}

static long n_checked, n_bad, n_subnormal;
static void check(uint32_t xb)
{
    const float x = bits_f32(xb);
    const uint32_t a = f32_bits(expf_two_step(x)), b = f32_bits(expf_ldexp(x));
    n_checked++;
    if ((a & 0x7f800000u) == 0 && (a & 0x007fffffu) != 0) n_subnormal++;
    if (a != b) { if (n_bad < 8) printf("x = %a (0x%08x): two-step 0x%08x, ldexp 0x%08x\n", x, xb, a, b); n_bad++; }
}

int main(int argc, char **argv)
{
    const uint32_t stride = (argc > 1 && strcmp(argv[1], "all") == 0) ? 1u : 127u;
    const uint32_t M103 = f32_bits(-103.0f), M87 = f32_bits(-87.0f), TOP = f32_bits(88.72283f);
    /* 1. every float of [-103, -87) (negative floats: a larger bit pattern is a smaller value) */
    for (uint32_t b = M87 + 1u; b <= M103; b++) check(b);
    const long n_low = n_checked, sub_low = n_subnormal;
    /* 2. the rest of the domain: [-87, -0] and [+0, 88.72283] */
    for (uint32_t b = 0x80000000u; b <= M87; b += stride) check(b);
    check(M87);
    for (uint32_t b = 0u; b <= TOP; b += stride) check(b);
    check(TOP);
    const long n_rest = n_checked - n_low;
    if (n_subnormal != sub_low) { printf("a subnormal result outside [-103, -87)\n"); return 2; }
    /* 3. the overridden ranges: below -103 to -inf, above 88.72283 to +inf, NaNs of both signs */
    for (uint32_t b = M103 + 1u; b <= 0xff800000u; b += 4099u) check(b);
    check(0xff800000u);
    for (uint32_t b = TOP + 1u; b <= 0x7f800000u; b += 4099u) check(b);
    check(0x7f800000u);
    for (uint32_t b = 0x7f800001u; b < 0x80000000u; b += 65537u) check(b);
    for (uint32_t b = 0xff800001u; b >= 0xff800001u; b += 65537u) check(b);      /* (ends when the pattern wraps) */
    const long n_over = n_checked - n_low - n_rest;
    printf("stride %u: [-103, -87) %ld inputs (%ld subnormal results), rest of the domain %ld, overridden %ld, mismatches=%ld\n",
           stride, n_low, sub_low, n_rest, n_over, n_bad);
    return n_bad != 0;
}
