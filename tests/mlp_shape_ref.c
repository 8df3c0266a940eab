/* The host restatement of "nig-mlp-shape-v1" (include/nig.h): the head pre-activations of a ReLU actor with nh hidden layers of
 * any widths, in the law's float32 fma order -- layer 1 in natural k order, every later layer in the order the accumulator
 * registers of the 32-row tiles below expose their rows (register t of tile kt: rows 32 kt + rho(t) and 32 kt + rho(t) + 4,
 * rho(t) = (t & 3) + 8 (t >> 2)), the bias as a last k-step, the head as two chains (one per lane half) joined by one add.
 * A unit index at or beyond a layer's width is a unit of the class's zero padding: its term fma(0, 0, c) leaves c as it is
 * (the sign of a zero aside) and is skipped here, so the same routine states the unpadded and the padded network.
 * Compiled with gcc -O2 -ffp-contract=off -mfma (tests/mlp_shape_ref.py): fmaf is the one fused operation. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#define MAXW 512

static int rho(int t) { return (t & 3) + 8 * (t >> 2); }

/* W[l] is [in_l][out_l] row-major; obs [n][S]; pre [n][A].  Returns 0, or 1 for a shape outside the law. */
int shape_pre(int64_t n, int S, int A, int nh, const int32_t *dims, const float *const *W, const float *const *b, const float *obs, float *pre)
{
    if (nh < 1 || nh > 3 || A < 1 || A > 16 || S < 1) return 1;
    for (int l = 0; l < nh; l++)
        if (dims[l] < 1 || dims[l] > MAXW) return 1;
    for (int64_t i = 0; i < n; i++) {
        const float *x = obs + (size_t)i * S;
        float h[2][MAXW];
        int cur = 0;
        const int H1 = dims[0];
        for (int u = 0; u < H1; u++) {
            float acc = 0.0f;
            for (int k = 0; k < S; k++) acc = fmaf(W[0][(size_t)k * H1 + u], x[k], acc);
            acc = fmaf(b[0][u], 1.0f, acc);
            h[cur][u] = fmaxf(acc, 0.0f);
        }
        for (int l = 1; l < nh; l++) {
            const int K = dims[l - 1], H = dims[l];
            for (int u = 0; u < H; u++) {
                float acc = 0.0f;
                for (int kt = 0; 32 * kt < K; kt++)
                    for (int t = 0; t < 16; t++) {
                        const int k0 = 32 * kt + rho(t), k1 = k0 + 4;
                        if (k0 < K) acc = fmaf(W[l][(size_t)k0 * H + u], h[cur][k0], acc);
                        if (k1 < K) acc = fmaf(W[l][(size_t)k1 * H + u], h[cur][k1], acc);
                    }
                acc = fmaf(b[l][u], 1.0f, acc);
                h[cur ^ 1][u] = fmaxf(acc, 0.0f);
            }
            cur ^= 1;
        }
        const int K = dims[nh - 1];
        for (int j = 0; j < A; j++) {
            float acc0 = 0.0f, acc1 = 0.0f;
            for (int kt = 0; 32 * kt < K; kt++)
                for (int t = 0; t < 16; t++) {
                    const int k0 = 32 * kt + rho(t), k1 = k0 + 4;
                    if (k0 < K) acc0 = fmaf(W[nh][(size_t)k0 * A + j], h[cur][k0], acc0);
                    if (k1 < K) acc1 = fmaf(W[nh][(size_t)k1 * A + j], h[cur][k1], acc1);
                }
            acc0 = fmaf(b[nh][j], 1.0f, acc0);
            acc1 = fmaf(b[nh][j], 0.0f, acc1);
            pre[(size_t)i * A + j] = acc0 + acc1;
        }
    }
    return 0;
}
