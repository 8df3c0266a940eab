/* mlp_project_ref.c -- the constraint projection ("nig-project-v1", include/nig.h) restated on the host in plain C with fmaf,
 * in the device's summation order.  Compiled by the tests (gcc -O2 -ffp-contract=off -mfma -fopenmp -shared -fPIC); it has no sigmoid: the
 * acceptance test takes p0 = det_sigmoidf(z0), which the tests form with the oracle's det_sigmoidf from proj_forward's logits
 * and hand to proj_loop as `projected`.
 *
 * One routine is the network IN -> 256 -> 256 -> OUT in the order of the MFMA kernels (the oracle's mlp_pre): layer 1 in natural
 * k order, two inputs per k-step (an odd IN is padded with a zero input), layers 2 and 3 in the order an accumulator tile
 * exposes its rows (register t of a 32-row tile: rows rho(t) and rho(t) + 4, rho(t) = (t & 3) + 8 (t >> 2)), every bias as a
 * last k-step, the head as two lane-half chains joined by one add.  Its activation is either ReLU, recording the masks z > 0
 * of both hidden layers, or the backward pass's select on recorded masks.  The backward pass is the same routine on the
 * transposed network 4 -> 256 -> 256 -> A (W3^T zero-padded to four rows, W2^T, W1[S:S+A, :]^T, zero biases), whose first
 * hidden layer is selected by the forward pass's SECOND mask and whose second by its first. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define HMAX 256       /* the device's width; a narrower network (a multiple of 32) runs the same chains over its own units */
static int rho(int t) { return (t & 3) + 8 * (t >> 2); }

/* select == 0: ReLU, k1 / k2 receive the masks.  select == 1: hidden value = mask ? acc : 0 with the masks k1 / k2 given. */
static void network(int IN, int OUT, const float *W1, const float *b1, const float *W2, const float *b2, const float *W3,
                    const float *b3, const float *x, float *pre, int select, unsigned char *k1, unsigned char *k2, int H)
{
    /* (k outermost, the unit innermost: per unit the same chain of fmaf in the same order, over contiguous weights) */
    float h1[HMAX], h2[HMAX], acc[HMAX];
    for (int u = 0; u < H; u++) acc[u] = 0.0f;
    for (int ks = 0; 2 * ks < IN; ks++) {
        const float x0 = x[2 * ks], x1 = (2 * ks + 1 < IN) ? x[2 * ks + 1] : 0.0f;
        const float *w0 = W1 + (size_t)(2 * ks) * H, *w1 = W1 + (size_t)(2 * ks + 1) * H;
        if (2 * ks + 1 < IN) for (int u = 0; u < H; u++) acc[u] = fmaf(w1[u], x1, fmaf(w0[u], x0, acc[u]));
        else for (int u = 0; u < H; u++) acc[u] = fmaf(0.0f, 0.0f, fmaf(w0[u], x0, acc[u]));
    }
    for (int u = 0; u < H; u++) {
        const float v = fmaf(0.0f, 0.0f, fmaf(b1[u], 1.0f, acc[u]));
        if (select) h1[u] = k1[u] ? v : 0.0f;
        else { h1[u] = fmaxf(v, 0.0f); k1[u] = h1[u] > 0.0f; }
    }
    for (int v = 0; v < H; v++) acc[v] = 0.0f;
    for (int kt = 0; kt < H / 32; kt++)
        for (int t = 0; t < 16; t++) {
            const int k0 = 32 * kt + rho(t), k4 = k0 + 4;
            const float *w0 = W2 + (size_t)k0 * H, *w4 = W2 + (size_t)k4 * H;
            const float a0 = h1[k0], a4 = h1[k4];
            for (int v = 0; v < H; v++) acc[v] = fmaf(w4[v], a4, fmaf(w0[v], a0, acc[v]));
        }
    for (int v = 0; v < H; v++) {
        const float y = fmaf(0.0f, 0.0f, fmaf(b2[v], 1.0f, acc[v]));
        if (select) h2[v] = k2[v] ? y : 0.0f;
        else { h2[v] = fmaxf(y, 0.0f); k2[v] = y > 0.0f; }
    }
    /* the head: each lane half sums the hidden rows its accumulator registers hold as its own chain -- half 0 rows rho(t),
     * half 1 rows rho(t) + 4 --, the bias record is fma(b, 1, .) on half 0 and fma(b, 0, .) on half 1, one add joins them */
    for (int j = 0; j < OUT; j++) {
        float acc0 = 0.0f, acc1 = 0.0f;
        for (int kt = 0; kt < H / 32; kt++)
            for (int t = 0; t < 16; t++) {
                const int k0 = 32 * kt + rho(t), k4 = k0 + 4;
                acc0 = fmaf(W3[(size_t)k0 * OUT + j], h2[k0], acc0);
                acc1 = fmaf(W3[(size_t)k4 * OUT + j], h2[k4], acc1);
            }
        acc0 = fmaf(b3[j], 1.0f, acc0); acc1 = fmaf(b3[j], 0.0f, acc1);
        pre[j] = acc0 + acc1;
    }
}

/* the predictor's weights, row-major [in][out], and the backward network built from them */
typedef struct {
    int S, A, C, H;
    const float *W1, *b1, *W2, *b2, *W3, *b3;
    float *T1, *T2, *T3, *zero;       /* W3^T padded to [4][H]; W2^T [H][H]; W1[S:S+A, :]^T [H][A]; H zeros */
} net_t;

static int net_init(net_t *n, int H, int S, int A, int C, const float *W1, const float *b1, const float *W2, const float *b2,
                    const float *W3, const float *b3)
{
    n->S = S; n->A = A; n->C = C; n->H = H; n->W1 = W1; n->b1 = b1; n->W2 = W2; n->b2 = b2; n->W3 = W3; n->b3 = b3;
    n->T1 = calloc((size_t)4 * H, sizeof(float)); n->T2 = calloc((size_t)H * H, sizeof(float));
    n->T3 = calloc((size_t)H * A, sizeof(float)); n->zero = calloc(H, sizeof(float));
    if (!n->T1 || !n->T2 || !n->T3 || !n->zero) return -1;
    for (int c = 0; c < C; c++) for (int u = 0; u < H; u++) n->T1[(size_t)c * H + u] = W3[(size_t)u * C + c];
    for (int k = 0; k < H; k++) for (int j = 0; j < H; j++) n->T2[(size_t)j * H + k] = W2[(size_t)k * H + j];
    for (int j = 0; j < A; j++) for (int u = 0; u < H; u++) n->T3[(size_t)u * A + j] = W1[(size_t)(S + j) * H + u];
    return 0;
}
static void net_free(net_t *n) { free(n->T1); free(n->T2); free(n->T3); free(n->zero); }

static void forward(const net_t *n, const float *s, const float *a, float *z, unsigned char *k1, unsigned char *k2)
{
    float x[64];
    memcpy(x, s, n->S * sizeof(float)); memcpy(x + n->S, a, n->A * sizeof(float));
    network(n->S + n->A, n->C, n->W1, n->b1, n->W2, n->b2, n->W3, n->b3, x, z, 0, k1, k2, n->H);
}
static void backward(const net_t *n, const float *z, unsigned char *k1, unsigned char *k2, float *g)
{
    float d[4];
    for (int c = 0; c < 4; c++) d[c] = (c < n->C && z[c] > 0.0f) ? 1.0f : 0.0f;
    network(4, n->A, n->T1, n->zero, n->T2, n->zero, n->T3, n->zero, d, g, 1, k2, k1, n->H);
}

/* logits z [n][C] and the first gradient g [n][A] at (obs [n][S], act [n][A]); masks (optional) [n][2][H] */
int proj_forward(int64_t n, int H, int S, int A, int C, const float *W1, const float *b1, const float *W2, const float *b2,
                 const float *W3, const float *b3, const float *obs, const float *act, float *z, float *g, unsigned char *masks)
{
    net_t N;
    if (H < 32 || H > HMAX || H % 32 || S + A > 64 || C < 1 || C > 4 || A > 16 || net_init(&N, H, S, A, C, W1, b1, W2, b2, W3, b3)) return -1;
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t i = 0; i < n; i++) {
        unsigned char k1[HMAX], k2[HMAX];
        forward(&N, obs + i * S, act + i * A, z + i * C, k1, k2);
        if (masks) { memcpy(masks + i * 2 * H, k1, H); memcpy(masks + i * 2 * H + H, k2, H); }
        if (g) backward(&N, z + i * C, k1, k2, g + i * A);
    }
    net_free(&N);
    return 0;
}

/* The loop of the law on lanes whose acceptance test the caller has made (projected[i] != 0: some p0[c] is not below the
 * threshold).  act [n][A] in: the actor's action; out: the action the env receives.  iters [n]: -1 kept, else the gradient
 * steps taken.  z [n][C]: the logits of the action the env receives.  g0 [n][A]: the first gradient, written where
 * iters >= 1 only. */
int proj_loop(int64_t n, int H, int S, int A, int C, const float *W1, const float *b1, const float *W2, const float *b2,
              const float *W3, const float *b3, const float *obs, const unsigned char *projected, float tolerance, int max_iters,
              float step, float *act, int32_t *iters, float *z, float *g0)
{
    net_t N;
    if (H < 32 || H > HMAX || H % 32 || S + A > 64 || C < 1 || C > 4 || A > 16 || net_init(&N, H, S, A, C, W1, b1, W2, b2, W3, b3)) return -1;
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t i = 0; i < n; i++) {
        unsigned char k1[HMAX], k2[HMAX];
        float *a = act + i * A, *zi = z + i * C, g[16];
        forward(&N, obs + i * S, a, zi, k1, k2);
        iters[i] = -1;
        if (!projected[i]) continue;
        int k = 0;
        for (; k < max_iters; k++) {
            int met = 1;
            for (int c = 0; c < C; c++) met = met && zi[c] < tolerance;
            if (met) break;
            backward(&N, zi, k1, k2, g);
            if (k == 0) memcpy(g0 + i * A, g, A * sizeof(float));
            for (int j = 0; j < A; j++) {
                float v = a[j] - step * g[j];
                a[j] = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
            }
            forward(&N, obs + i * S, a, zi, k1, k2);
        }
        iters[i] = k;
    }
    net_free(&N);
    return 0;
}
