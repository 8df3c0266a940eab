// nig_mlp_shape_stream.hpp -- the MFMA operand stream of a ReLU actor of one of the SHAPE CLASSES ("nig-mlp-shape-v1",
// include/nig.h): two or three hidden layers of up to 512 units, zero-padded to the class's tile counts.  Its plan and its ONE builder.
//
// Plain C++17, no HIP: nig_mlp_shape.hpp derives the kernel's constants from shape_plan, nig_api.hip builds the image with
// put_shape_network, and tests/mlp_shape_probe.hip calls the same builder on the host (tests/test_mlp_shape_host.py).
// nig_mlp_stream.hpp -- the reference class (IN -> 256 -> 256 -> OUT) and every image it builds -- is not touched by this file.
#pragma once
#include <cstddef>
#include "nig_mlp_stream.hpp"        // mfma_row

namespace nig {

// A shape class: NH hidden layers of T[n] tiles of 32 units each (T[2] = 0 with two layers).
struct MlpShapeClass { int nh, t[3]; };
constexpr int SHAPE_KIND_NONE = 0, SHAPE_KIND_REFERENCE = 1, SHAPE_KIND_128 = 2, SHAPE_KIND_512x256 = 3, SHAPE_KIND_512 = 4, SHAPE_KIND_3 = 5;
constexpr MlpShapeClass SHAPE_CLASSES[6] = {{0, {0, 0, 0}}, {2, {8, 8, 0}}, {2, {4, 4, 0}}, {2, {16, 8, 0}}, {2, {16, 16, 0}}, {3, {8, 8, 8}}};
constexpr int SHAPE_MAX_WIDTH = 512;

// 32 x 32 x 2 instructions per step of a class on an env with S (even) inputs: the cost that "cheapest" compares
constexpr int shape_mfmas(const MlpShapeClass &c, int S)
{
    int n = c.t[0] * (S / 2 + 1);
    for (int l = 1; l < c.nh; ++l) n += c.t[l] * (16 * c.t[l - 1] + 1);
    return n;
}
constexpr bool shape_holds(const MlpShapeClass &c, int nh, const int *hidden)
{
    if (c.nh != nh) return false;
    for (int l = 0; l < nh; ++l)
        if (hidden[l] < 1 || hidden[l] > 32 * c.t[l]) return false;
    return true;
}
// the cheapest class that holds the hidden widths (SHAPE_KIND_*), SHAPE_KIND_NONE where none does
constexpr int shape_class_of(int nh, const int *hidden, int S)
{
    int best = SHAPE_KIND_NONE;
    for (int k = SHAPE_KIND_REFERENCE; k <= SHAPE_KIND_3; ++k)
        if (shape_holds(SHAPE_CLASSES[k], nh, hidden) && (best == SHAPE_KIND_NONE || shape_mfmas(SHAPE_CLASSES[k], S) < shape_mfmas(SHAPE_CLASSES[best], S)))
            best = k;
    return best;
}

// The stream is cut into CHUNKS of `chrec` record slots (a record = 64 floats = 256 bytes); a chunk is what one fill of an LDS buffer
// holds.  In consumption order:
//   layer 1   tile m (32 units) is width / 2 weight records + 1 bias record, `l1_tiles` tiles to a chunk, `l1_chunks` chunks.
//             Record ks of a tile, lane l = (i = l & 31, hf = l >> 5): W1[2 ks + hf][32 m + i] (natural k order); the bias record
//             holds b1[32 m + i] on lane half 0.
//   layer n   (n = 2 .. NH) output tile m is kch(n) chunks, kch = 1 where the layer below has at most 8 tiles (K <= 256, at most 128
//             records) and 2 where it has 16: chunk j of the tile holds the weight records of input tiles 8 j .. 8 j + 7 -- record
//             16 (kt - 8 j) + t, lane (i, hf): Wn[32 kt + mfma_row(t, hf)][32 m + i], the accumulator-register order of the tiles the
//             layer reads -- and the tile's LAST chunk the bias record behind them (bn[32 m + i] on lane half 0).  The accumulator is
//             carried across a tile's chunks.
//   head      the last chunk of output tile m of the LAST hidden layer carries, behind the bias record, the 16 head records of that
//             tile: record t, lane l: W_head[32 m + mfma_row(t, hf)][l & row] where (l & row) < OUT, row = 3 (OUT <= 4, v_mfma_f32_4x4x1)
//             or 15 (v_mfma_f32_16x16x1) -- put_network's head.  The head's bias record lies behind the last chunk's head records.
// Everything not named is +0.0.
struct ShapePlan {
    int nh, t[3];
    int width, l1_rec, l1_tiles, l1_chunks, l1_pieces;     // layer 1: padded input; records per tile; tiles per chunk; chunks; KiB pieces per chunk
    int kch[3];                                            // chunks per output tile of layer n + 1 (kch[0] unused)
    int base[3];                                           // first chunk of layer n + 1 (base[0] = 0)
    int chrec, pieces, chunks;                             // record slots per chunk; KiB pieces per chunk slot; chunks of the image
    constexpr size_t floats() const { return (size_t)chunks * chrec * 64; }
    constexpr int ktiles(int n, int j) const { const int left = t[n - 1] - 8 * j; return left < 8 ? left : 8; }   // input tiles in chunk j of layer n + 1
    constexpr bool last_k(int n, int j) const { return j == kch[n] - 1; }
    constexpr int chunk_of(int n, int m, int j) const { return base[n] + m * kch[n] + j; }
};
constexpr ShapePlan shape_plan(const MlpShapeClass &c, int in)
{
    ShapePlan p = {};
    p.nh = c.nh;
    for (int l = 0; l < 3; ++l) p.t[l] = c.t[l];
    int widest = 0;                                        // weight records of the largest layer chunk
    for (int l = 1; l < c.nh; ++l) {
        p.kch[l] = (c.t[l - 1] + 7) / 8;
        const int w = 16 * (c.t[l - 1] < 8 ? c.t[l - 1] : 8);
        widest = w > widest ? w : widest;
    }
    p.chrec = (widest + 1 + 16 + 1 + 3) / 4 * 4;           // + bias, head, head's bias: 148 where a layer reads 8 tiles or more, 84 for the 128-wide class
    p.pieces = p.chrec / 4;
    p.width = (in + 1) & ~1;
    p.l1_rec = p.width / 2 + 1;
    p.l1_tiles = c.t[0];
    while (p.l1_tiles > 1 && p.l1_tiles * p.l1_rec > p.chrec) p.l1_tiles /= 2;      // (the tile counts are powers of two)
    p.l1_chunks = c.t[0] / p.l1_tiles;
    p.l1_pieces = (p.l1_tiles * p.l1_rec + 3) / 4;
    int ch = p.l1_chunks;
    for (int l = 1; l < c.nh; ++l) { p.base[l] = ch; ch += c.t[l] * p.kch[l]; }
    p.chunks = ch;
    return p;
}
constexpr bool shape_plan_fits(const ShapePlan &p) { return p.l1_tiles * p.l1_rec <= p.chrec; }

// The image of the network IN -> hidden[0] -> .. -> hidden[nh - 1] -> OUT (W[l] [in_l][out_l] row-major, unpadded) in class `c`, into
// the zeroed host[floats].  Units beyond a layer's width are the class's zero padding: they are simply never written.
inline bool put_shape_network(const MlpShapeClass &c, int IN, int OUT, int nh, const int *hidden, const float *const *W, const float *const *b,
                              float *host, size_t floats)
{
    if (!shape_holds(c, nh, hidden) || OUT < 1 || OUT > 16 || IN < 1) return false;
    const ShapePlan p = shape_plan(c, IN);
    if (!shape_plan_fits(p) || p.floats() > floats) return false;
    auto rec = [&](int chunk, int r) { return host + ((size_t)chunk * p.chrec + r) * 64; };
    const int H1 = hidden[0];
    for (int m = 0; m < c.t[0]; ++m) {                      // layer 1, natural k order: k = 2 ks + hf
        const int ch = m / p.l1_tiles, base = (m % p.l1_tiles) * p.l1_rec;
        for (int ks = 0; ks < p.width / 2; ++ks)
            for (int l = 0; l < 64; ++l) {
                const int k = 2 * ks + (l >> 5), u = 32 * m + (l & 31);
                if (k < IN && u < H1) rec(ch, base + ks)[l] = W[0][(size_t)k * H1 + u];
            }
        for (int l = 0; l < 32; ++l)
            if (32 * m + l < H1) rec(ch, base + p.width / 2)[l] = b[0][32 * m + l];
    }
    const int row = OUT <= 4 ? 3 : 15;
    const int HL = hidden[nh - 1];
    for (int n = 1; n < nh; ++n) {                          // layer n + 1: K = hidden[n - 1] inputs, hidden[n] outputs
        const int K = hidden[n - 1], H = hidden[n];
        for (int m = 0; m < c.t[n]; ++m)
            for (int j = 0; j < p.kch[n]; ++j) {
                const int ch = p.chunk_of(n, m, j), kts = p.ktiles(n, j);
                int r = 0;
                for (int kt = 8 * j; kt < 8 * j + kts; ++kt)
                    for (int t = 0; t < 16; ++t, ++r)
                        for (int l = 0; l < 64; ++l) {
                            const int k = 32 * kt + mfma_row(t, l >> 5), u = 32 * m + (l & 31);
                            if (k < K && u < H) rec(ch, r)[l] = W[n][(size_t)k * H + u];
                        }
                if (!p.last_k(n, j)) continue;
                for (int l = 0; l < 32; ++l)
                    if (32 * m + l < H) rec(ch, r)[l] = b[n][32 * m + l];
                ++r;
                if (n != nh - 1) continue;
                for (int t = 0; t < 16; ++t, ++r)           // the head's slice on this tile's 32 hidden rows
                    for (int l = 0; l < 64; ++l) {
                        const int k = 32 * m + mfma_row(t, l >> 5);
                        if ((l & row) < OUT && k < HL) rec(ch, r)[l] = W[nh][(size_t)k * OUT + (l & row)];
                    }
                if (m == c.t[n] - 1)                        // the head's bias behind the last chunk (B = 1 on lane half 0, 0 on half 1)
                    for (int l = 0; l < 64; ++l)
                        if ((l & row) < OUT) rec(ch, r)[l] = b[nh][l & row];
            }
    }
    return true;
}

// The reference class: the network IN -> h1 -> h2 -> OUT with h1, h2 <= 256, zero-padded to 256 x 256 and built by put_network --
// bit for bit the image nig_set_mlp_policy builds from the padded arrays.  pad: scratch of reference_pad_floats(IN, OUT) zeroed floats.
constexpr size_t reference_pad_floats(int IN, int OUT) { return (size_t)IN * MLP_H + MLP_H + (size_t)MLP_H * MLP_H + MLP_H + (size_t)MLP_H * OUT; }
inline bool put_reference_padded(int IN, int OUT, const int *hidden, const float *const *W, const float *const *b, float *pad, float *host, size_t floats)
{
    const int H1 = hidden[0], H2 = hidden[1];
    if (H1 < 1 || H1 > MLP_H || H2 < 1 || H2 > MLP_H) return false;
    float *W1 = pad, *b1 = W1 + (size_t)IN * MLP_H, *W2 = b1 + MLP_H, *b2 = W2 + (size_t)MLP_H * MLP_H, *W3 = b2 + MLP_H;
    for (int k = 0; k < IN; ++k)
        for (int u = 0; u < H1; ++u) W1[(size_t)k * MLP_H + u] = W[0][(size_t)k * H1 + u];
    for (int u = 0; u < H1; ++u) b1[u] = b[0][u];
    for (int k = 0; k < H1; ++k)
        for (int u = 0; u < H2; ++u) W2[(size_t)k * MLP_H + u] = W[1][(size_t)k * H2 + u];
    for (int u = 0; u < H2; ++u) b2[u] = b[1][u];
    for (int k = 0; k < H2; ++k)
        for (int j = 0; j < OUT; ++j) W3[(size_t)k * OUT + j] = W[2][(size_t)k * OUT + j];
    return put_network(IN, OUT, W1, b1, W2, b2, W3, b[2], host, floats);
}

}  // namespace nig
