// nig_mlp_ln_stream.hpp -- the MFMA operand stream of a LayerNorm actor (IN -> 256 -> LayerNorm -> ReLU -> 256 -> LayerNorm -> ReLU
// -> OUT, "nig-mlp-ln-v1": nig_mlp_ln.hpp states the law).  Its plan and its ONE builder.
//
// Plain C++17, no HIP: nig_mlp_ln.hpp derives the kernel's constants from ln_plan, nig_api.hip builds the image with put_ln_network,
// and tests/mlp_ln_probe.hip calls the same builder on the host (tests/test_mlp_ln_host.py).  A plan of its own: nig_mlp_stream.hpp
// and nig_mlp_shape_stream.hpp, and every image they build, are not touched by this file.
#pragma once
#include <cstddef>
#include "nig_mlp_stream.hpp"        // MLP_H, MLP_MT, MLP_CHREC, mlp_layer1, mfma_row

namespace nig {

// The image is L1 + MLP_MT + 1 CHUNKS of MLP_CHREC (148) record slots (a record = 64 floats; lane l = (i = l & 31, hf = l >> 5)), in
// consumption order, and a TABLE of LN_TABLE_FLOATS floats behind the last chunk.  Everything not named is +0.0.
//   layer 1   put_network's: mlp_layer1(IN) -- L1 = 1 chunk of eight tiles (IN <= 34) or 2 of four; tile m is width / 2 weight records
//             + 1 bias record; record ks of a tile: W1[2 ks + hf][32 m + i] (natural k order), the bias record b1[32 m + i] on lane half 0.
//   layer 2   chunk L1 + m (output tile m): record 16 kt + t: W2[32 kt + mfma_row(t, hf)][32 m + i] -- put_layer2's 128 weight records
//             and its bias record (b2[32 m + i] on lane half 0) at record 128.  No head records ride with them: the head reads the
//             NORMALISED layer, which exists only behind the last tile.
//   head      chunk L1 + 8: record 16 m + t: W3[32 m + mfma_row(t, hf)][l & row] where (l & row) < OUT, row = 3 (OUT <= 4,
//             v_mfma_f32_4x4x1) or 15 (v_mfma_f32_16x16x1) -- put_network's head records, tile after tile -- and the head's bias
//             b3[l & row] on the same lanes of record 128.
//   table     gamma and beta of both LayerNorms in the order the accumulator registers hold the units: entry
//             ln_table_at(layer, which, hf, m, t) = (which ? beta : gamma)_layer[32 m + mfma_row(t, hf)] -- the sixteen values of a
//             tile and lane half are 64 contiguous bytes, four 16-byte vectors.
constexpr int LN_HEAD_REC = MLP_MT * 16 + 1;                   // 128 head records + the head's bias
constexpr int LN_TABLE_FLOATS = 2 * 2 * 2 * MLP_H / 2;         // 1 024 floats = 4 KiB = 16 records
static_assert(LN_HEAD_REC <= MLP_CHREC && MLP_MT * 16 + 1 <= MLP_CHREC);
constexpr int ln_table_at(int layer, int which, int hf, int m, int t) { return (((layer * 2 + which) * 2 + hf) * MLP_MT + m) * 16 + t; }

struct LnPlan {
    MlpLayer1 l1;
    int chunks, head_chunk;                                    // chunks of the image; the head's
    int l2_pieces, head_pieces;                                // KiB pieces a layer-2 chunk and the head's chunk fill
    constexpr size_t table() const { return (size_t)chunks * MLP_CHREC * 64; }        // first float of the table
    constexpr size_t floats() const { return table() + LN_TABLE_FLOATS; }
};
constexpr LnPlan ln_plan(int in)
{
    const MlpLayer1 L = mlp_layer1(in);
    return {L, L.chunks + MLP_MT + 1, L.chunks + MLP_MT, (MLP_MT * 16 + 1 + 3) / 4, (LN_HEAD_REC + 3) / 4};
}
constexpr size_t LN_STREAM_MAX_FLOATS = (size_t)(2 + MLP_MT + 1) * MLP_CHREC * 64 + LN_TABLE_FLOATS;

// The image of the network (W1 [IN][256], W2 [256][256], W3 [256][OUT], row-major; g / be: gamma and beta of LayerNorm 1 and 2)
// into the zeroed host[floats].
inline bool put_ln_network(int IN, int OUT, const float *W1, const float *b1, const float *g1, const float *be1, const float *W2,
                           const float *b2, const float *g2, const float *be2, const float *W3, const float *b3, float *host, size_t floats)
{
    const int H = MLP_H;
    const LnPlan P = ln_plan(IN);
    if (!P.l1.fits() || OUT < 1 || OUT > 16 || IN < 1 || P.floats() > floats) return false;
    for (int m = 0; m < MLP_MT; ++m) {                      // layer 1, natural k order: k = 2 ks + hf (k >= IN: zero pad)
        const int ch = m / P.l1.tiles, base = (m % P.l1.tiles) * P.l1.records;
        for (int ks = 0; ks < P.l1.width / 2; ++ks)
            for (int l = 0; l < 64; ++l) {
                const int k = 2 * ks + (l >> 5);
                if (k < IN) stream_rec(host, ch, base + ks)[l] = W1[(size_t)k * H + 32 * m + (l & 31)];
            }
        for (int l = 0; l < 32; ++l) stream_rec(host, ch, base + P.l1.width / 2)[l] = b1[32 * m + l];
    }
    for (int m = 0; m < MLP_MT; ++m)
        if (put_layer2(host, P.l1.chunks + m, m, W2, b2) != MLP_MT * 16 + 1) return false;
    const int row = OUT <= 4 ? 3 : 15;
    for (int m = 0; m < MLP_MT; ++m)
        for (int t = 0; t < 16; ++t)
            for (int l = 0; l < 64; ++l)
                if ((l & row) < OUT) stream_rec(host, P.head_chunk, 16 * m + t)[l] = W3[(size_t)(32 * m + mfma_row(t, l >> 5)) * OUT + (l & row)];
    for (int l = 0; l < 64; ++l)                            // (B = 1 on lane half 0, 0 on half 1)
        if ((l & row) < OUT) stream_rec(host, P.head_chunk, MLP_MT * 16)[l] = b3[l & row];
    const float *const tab[2][2] = {{g1, be1}, {g2, be2}};
    for (int layer = 0; layer < 2; ++layer)
        for (int which = 0; which < 2; ++which)
            for (int hf = 0; hf < 2; ++hf)
                for (int m = 0; m < MLP_MT; ++m)
                    for (int t = 0; t < 16; ++t)
                        host[P.table() + ln_table_at(layer, which, hf, m, t)] = tab[layer][which][32 * m + mfma_row(t, hf)];
    return true;
}

}  // namespace nig
