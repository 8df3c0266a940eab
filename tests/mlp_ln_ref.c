/* The host restatement of "nig-mlp-ln-v1" (csrc/nig_mlp_ln.hpp states the law): the head pre-activations of the LayerNorm actor
 * S -> 256 -> LayerNorm -> ReLU -> 256 -> LayerNorm -> ReLU -> A in the law's float32 order, and det_rsqrtf restated on its own.
 *   Dense     layer 1 in natural k order, layer 2 in the order the accumulator registers of the 32-row tiles below expose their rows
 *             (register t of tile kt: rows 32 kt + rho(t) and 32 kt + rho(t) + 4, rho(t) = (t & 3) + 8 (t >> 2)), two inputs per k-step
 *             as fma(a1, b1, fma(a0, b0, c)), the bias as a last k-step (b x 1, then 0 x 0).
 *   LayerNorm per lane half hf the 128 rows 32 mm + rho(t) + 4 hf, mm ascending, t ascending: the sum as one chain of adds from 0,
 *             mean = (p_0 + p_1) 2^-8; d = z - mean; the squares as one chain q = fma(d, d, q) from 0 in the same order,
 *             var = (q_0 + q_1) 2^-8; rs = 1 / sqrt(var + eps) (IEEE sqrt, IEEE division); h = max(fma(d, rs gamma, beta), 0).
 *   head      two chains, one per lane half, joined by one add; the bias behind half 0's chain.
 * Compiled with gcc -O2 -ffp-contract=off -mfma -fopenmp (tests/mlp_ln_ref.py): fmaf is the one fused operation. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define H 256

static int rho(int t) { return (t & 3) + 8 * (t >> 2); }

float ln_rsqrtf(float x)
{
    const float r = sqrtf(x);
    return 1.0f / r;
}

/* 1 / sqrt of the floats with bits base .. base + n - 1 */
void ln_rsqrt_array(uint32_t base, int64_t n, float *out)
{
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; i++) {
        const uint32_t u = base + (uint32_t)i;
        float x;
        memcpy(&x, &u, 4);
        out[i] = ln_rsqrtf(x);
    }
}

/* how many of got[0 .. n) differ in their bits from ln_rsqrtf of the float with bits base + i; *first: the first such i */
int64_t ln_rsqrt_mismatches(uint32_t base, int64_t n, const float *got, int64_t *first)
{
    int64_t bad = 0, at = n;
#pragma omp parallel for schedule(static) reduction(+ : bad) reduction(min : at)
    for (int64_t i = 0; i < n; i++) {
        const uint32_t u = base + (uint32_t)i;
        float x;
        memcpy(&x, &u, 4);
        const float w = ln_rsqrtf(x);
        if (memcmp(&w, &got[i], 4) != 0) {
            bad++;
            if (i < at) at = i;
        }
    }
    *first = at;
    return bad;
}

/* steps 2 .. 5 of the law on z[256] in place */
static void layer_norm(float *z, const float *g, const float *be, float eps)
{
    float p[2], q[2];
    for (int hf = 0; hf < 2; hf++) {
        float s = 0.0f;
        for (int mm = 0; mm < H / 32; mm++)
            for (int t = 0; t < 16; t++) s = s + z[32 * mm + rho(t) + 4 * hf];
        p[hf] = s;
    }
    const float mean = (p[0] + p[1]) * 0x1p-8f;
    for (int r = 0; r < H; r++) z[r] = z[r] - mean;
    for (int hf = 0; hf < 2; hf++) {
        float s = 0.0f;
        for (int mm = 0; mm < H / 32; mm++)
            for (int t = 0; t < 16; t++) {
                const float d = z[32 * mm + rho(t) + 4 * hf];
                s = fmaf(d, d, s);
            }
        q[hf] = s;
    }
    const float var = (q[0] + q[1]) * 0x1p-8f;
    const float rs = ln_rsqrtf(var + eps);
    for (int r = 0; r < H; r++) z[r] = fmaxf(fmaf(z[r], rs * g[r], be[r]), 0.0f);
}

/* W1 [S][256], W2 [256][256], W3 [256][A] row-major; g / be [256]; obs [n][S]; pre [n][A]; hid (may be NULL) [n][2][256]: h1 and h2.
 * Returns 0, or 1 for a shape outside the law. */
int ln_pre(int64_t n, int S, int A, const float *W1, const float *b1, const float *g1, const float *be1, const float *W2, const float *b2,
           const float *g2, const float *be2, const float *W3, const float *b3, float eps, const float *obs, float *pre, float *hid)
{
    if (A < 1 || A > 16 || S < 2 || (S & 1)) return 1;              /* (the MFMA actor exists for an even state dim) */
    for (int64_t i = 0; i < n; i++) {
        const float *x = obs + (size_t)i * S;
        float h1[H], h2[H];
        for (int u = 0; u < H; u++) {
            float acc = 0.0f;
            for (int k = 0; k < S; k++) acc = fmaf(W1[(size_t)k * H + u], x[k], acc);
            acc = fmaf(b1[u], 1.0f, acc);
            h1[u] = fmaf(0.0f, 0.0f, acc);
        }
        layer_norm(h1, g1, be1, eps);
        for (int u = 0; u < H; u++) {
            float acc = 0.0f;
            for (int kt = 0; kt < H / 32; kt++)
                for (int t = 0; t < 16; t++) {
                    const int k0 = 32 * kt + rho(t), k1 = k0 + 4;
                    acc = fmaf(W2[(size_t)k0 * H + u], h1[k0], acc);
                    acc = fmaf(W2[(size_t)k1 * H + u], h1[k1], acc);
                }
            acc = fmaf(b2[u], 1.0f, acc);
            h2[u] = fmaf(0.0f, 0.0f, acc);
        }
        layer_norm(h2, g2, be2, eps);
        for (int j = 0; j < A; j++) {
            float acc0 = 0.0f, acc1 = 0.0f;
            for (int m = 0; m < H / 32; m++)
                for (int t = 0; t < 16; t++) {
                    const int k0 = 32 * m + rho(t), k1 = k0 + 4;
                    acc0 = fmaf(W3[(size_t)k0 * A + j], h2[k0], acc0);
                    acc1 = fmaf(W3[(size_t)k1 * A + j], h2[k1], acc1);
                }
            acc0 = fmaf(b3[j], 1.0f, acc0);
            acc1 = fmaf(b3[j], 0.0f, acc1);
            pre[(size_t)i * A + j] = acc0 + acc1;
        }
        if (hid) {
            memcpy(hid + (size_t)i * 2 * H, h1, sizeof h1);
            memcpy(hid + (size_t)i * 2 * H + H, h2, sizeof h2);
        }
    }
    return 0;
}
