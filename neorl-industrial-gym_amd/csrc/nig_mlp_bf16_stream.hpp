// nig_mlp_bf16_stream.hpp -- the bf16 MFMA operand image of the 256-wide ReLU actor (S -> 256 -> 256 -> A) under the law
// "nig-mlp-bf16-v1" (include/nig.h): its rounding, its chunk plan and its ONE builder.
//
// Plain C++17, no HIP (as nig_mlp_stream.hpp): nig_mlp_bf16.hpp reads the chunk plan, nig_api.hip builds the image with
// put_network_bf16 and exports the rounding as nig_bf16_from_f32.  What is stated here is stated nowhere else.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include "nig_mlp_stream.hpp"        // MLP_H, MLP_MT, mfma_row

namespace nig {

// bf(x): float32 -> bfloat16, round to nearest even; a NaN stays a (quiet) NaN with its sign and upper payload bits.
inline uint16_t bf16_from_f32(float x)
{
    uint32_t u;
    std::memcpy(&u, &x, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// A RECORD is the A operand of one v_mfma_f32_32x32x16_bf16: 64 lanes x 8 bf16 = 1 KiB, lane l = (r = l & 31, h = l >> 5) holding
// A[row r][k = 8 h + j] in element j, read by one ds_read_b128 and filled by one LDS-DMA wave-instruction (a "piece").  A BIAS
// record is 256 float32: blocks of 32, block b = [lane half h][register t] -> the bias of row mfma_row(t, h) of tile b, which is
// what a 32 x 32 accumulator starts from.
// The image is cut into BF16_CHUNKS chunks of BF16_CHREC record slots, a chunk being what one fill of an LDS buffer holds:
//   chunk 0      layer 1: tile m's bf16_l1_ksteps(S) records at m * ksteps, natural k order over x = [hi_0 .. hi_{S-1}, lo_0 ..
//                lo_{S-1}, 0 ..] (W1's rows used twice), then the bias record of b1 (tile m: block m)
//   chunk 1 + c  hidden tiles m2 = 2 c and 2 c + 1 of layer 2, tile tt at record 18 tt: 16 records (k-tile kt, k-step s at 2 kt + s)
//                whose k follows the accumulator registers of the layer-1 tiles (bf16_acc_k), then that tile's two head records
//                (W3^T zero-padded to 32 rows, k over the tile's own 32 hidden rows in the same order); then the bias record at 36:
//                block tt = b2 of tile 2 c + tt, block 2 = b3 zero-padded to 32 rows (read in chunk 1 only)
constexpr int BF16_REC_BYTES = 1024;
constexpr int BF16_TILE_REC = 2 * MLP_MT + 2;                 // 16 layer-2 records + 2 head records per hidden tile
constexpr int BF16_CH_TILES = 2;                              // hidden tiles per chunk
constexpr int BF16_BIAS_REC = BF16_CH_TILES * BF16_TILE_REC;  // 36
constexpr int BF16_CHREC = BF16_BIAS_REC + 1;                 // 37 record slots per chunk: the f32 image's 37 KiB LDS buffer
constexpr int BF16_CHUNKS = 1 + MLP_MT / BF16_CH_TILES;       // 5
constexpr size_t BF16_STREAM_BYTES = (size_t)BF16_CHUNKS * BF16_CHREC * BF16_REC_BYTES;
constexpr int bf16_l1_ksteps(int S) { return (2 * S + 15) / 16; }
constexpr int bf16_l1_pieces(int S) { return MLP_MT * bf16_l1_ksteps(S) + 1; }
constexpr bool bf16_l1_fits(int S) { return bf16_l1_pieces(S) <= BF16_CHREC; }
// Row (within its 32-row tile) of an accumulator tile that element j of lane half h carries in k-step s once registers 8 s .. 8 s + 7
// are converted pairwise: register 8 s + j is row mfma_row(8 s + j, h).
constexpr int bf16_acc_k(int s, int h, int j) { return mfma_row(8 * s + j, h); }
static_assert(bf16_acc_k(1, 1, 5) == 16 + 8 + 4 + 1, "16 s + 8 (j >> 2) + 4 h + (j & 3)");

// The image of the network (W1 [S][256], W2 [256][256], W3 [256][A], row-major; biases float32), weights rounded with
// bf16_from_f32, in exactly the order the kernel consumes it, into the zeroed host[bytes].  False: it does not fit.
inline bool put_network_bf16(int S, int A, const float *W1, const float *b1, const float *W2, const float *b2, const float *W3,
                             const float *b3, unsigned char *host, size_t bytes)
{
    const int H = MLP_H, KS = bf16_l1_ksteps(S);
    if (!bf16_l1_fits(S) || A > 32 || bytes < BF16_STREAM_BYTES) return false;
    auto rec = [&](int chunk, int r) { return host + ((size_t)chunk * BF16_CHREC + r) * BF16_REC_BYTES; };
    auto put = [&](int chunk, int r, int l, int j, float w) {
        const uint16_t v = bf16_from_f32(w);
        std::memcpy(rec(chunk, r) + 16 * l + 2 * j, &v, 2);
    };
    auto put_bias = [&](int chunk, int r, int block, const float *b, int rows) {
        for (int h = 0; h < 2; ++h)
            for (int t = 0; t < 16; ++t) {
                const int row = mfma_row(t, h);
                const float v = row < rows ? b[row] : 0.0f;
                std::memcpy(rec(chunk, r) + 4 * (32 * block + 16 * h + t), &v, 4);
            }
    };
    for (int m = 0; m < MLP_MT; ++m) {
        for (int s = 0; s < KS; ++s)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 8; ++j) {
                    const int k = 16 * s + 8 * (l >> 5) + j;
                    if (k < 2 * S) put(0, m * KS + s, l, j, W1[(size_t)(k < S ? k : k - S) * H + 32 * m + (l & 31)]);
                }
        put_bias(0, MLP_MT * KS, m, b1 + 32 * m, 32);
    }
    for (int m2 = 0; m2 < MLP_MT; ++m2) {
        const int ch = 1 + m2 / BF16_CH_TILES, tt = m2 % BF16_CH_TILES, base = tt * BF16_TILE_REC;
        for (int l = 0; l < 64; ++l)
            for (int j = 0; j < 8; ++j) {
                for (int kt = 0; kt < MLP_MT; ++kt)
                    for (int s = 0; s < 2; ++s)
                        put(ch, base + 2 * kt + s, l, j, W2[(size_t)(32 * kt + bf16_acc_k(s, l >> 5, j)) * H + 32 * m2 + (l & 31)]);
                for (int s = 0; s < 2; ++s)
                    if ((l & 31) < A) put(ch, base + 2 * MLP_MT + s, l, j, W3[(size_t)(32 * m2 + bf16_acc_k(s, l >> 5, j)) * A + (l & 31)]);
            }
        put_bias(ch, BF16_BIAS_REC, tt, b2 + 32 * m2, 32);
        if (tt == 0) put_bias(ch, BF16_BIAS_REC, BF16_CH_TILES, b3, A);
    }
    return true;
}

}  // namespace nig
