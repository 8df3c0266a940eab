// nig_mlp_stream.hpp -- the MFMA operand stream of a 256-wide ReLU network (IN -> 256 -> 256 -> OUT): its shape and its ONE builder.
//
// Plain C++17, no HIP: nig_mlp.hpp derives the kernels' layer-1 constants from mlp_layer1, nig_api.hip builds every image with
// put_network (the actor is the network (S, A), the safety critic the network (S + A, 1)), and tests/mlp_stream_probe.hip
// calls the same builder on the host (tests/test_mlp_stream.py).  The stream is the contract between host and kernel: what is
// stated here is stated nowhere else.
#pragma once
#include <cstddef>

namespace nig {

constexpr int MLP_H = 256, MLP_MT = MLP_H / 32;
// The operand stream is cut into CHUNKS of MLP_CHREC records (256 bytes each, padded): first layer 1 (MLP_MT tiles of IN/2
// weight records + 1 bias record, in one chunk or two: mlp_layer1), then chunk m2 = hidden tile m2 of layer 2 with its slice of
// the head (128 + 1 + 16 records; the last chunk also carries the head's bias record).  A chunk is what one fill of an LDS
// buffer holds: MLP_PIECES wave-instructions of 1 KiB (64 lanes x 16 bytes, LDS-DMA).
constexpr int MLP_PER = MLP_MT * 16 + 1 + 16;                 // 145 records per hidden tile
constexpr int MLP_PIECES = (MLP_PER + 1 + 3) / 4;             // 37 KiB pieces per chunk
constexpr int MLP_CHREC = MLP_PIECES * 4;                     // 148 records per chunk slot
constexpr int MLP_CHUNKS = 1 + MLP_MT;
constexpr int MLP_STREAM_FLOATS = MLP_CHUNKS * MLP_CHREC * 64;          // a network whose layer 1 is one chunk (every actor)
constexpr int MLP_CSTREAM_FLOATS = (2 + MLP_MT) * MLP_CHREC * 64;       // room for either layer-1 form (the critic)

// Layer 1 of a network with `in` inputs: the input is zero-padded to an even width (an MFMA k-step is two inputs, one per lane
// half), a tile is width / 2 weight records + 1 bias record, and the MLP_MT tiles share one chunk, or two chunks of four tiles
// each when eight tiles exceed a chunk slot (width >= 36: the critics of PowerGrid, AdvancedPowerGrid, SupplyChain).
struct MlpLayer1 {
    int width, records, chunks, tiles, pieces;    // padded input; records per tile; chunks; tiles per chunk; KiB pieces per chunk
    constexpr bool fits() const { return tiles * records <= MLP_CHREC; }
};
constexpr MlpLayer1 mlp_layer1(int in)
{
    const int width = (in + 1) & ~1, records = width / 2 + 1, chunks = MLP_MT * records <= MLP_CHREC ? 1 : 2, tiles = MLP_MT / chunks;
    return {width, records, chunks, tiles, (tiles * records + 3) / 4};
}

// Row of a 32x32 MFMA result tile held in register t by lane half hf (MI355X_MICROARCH / guide section 3).
constexpr int mfma_row(int t, int hf) { return (t & 3) + 8 * (t >> 2) + 4 * hf; }

// Record r of chunk `chunk`.  Record = 64 floats; lane l = (i = l & 31, hf = l >> 5) holds W[k(hf)][32*tile + i].
inline float *stream_rec(float *host, int chunk, int r) { return host + ((size_t)chunk * MLP_CHREC + r) * 64; }

// Layer 2 of hidden tile m2 at the head of `chunk`: the weight records, k following the accumulator register order of the
// layer-1 tiles, then the bias record.  Returns the index of the next record.
inline int put_layer2(float *host, int chunk, int m2, const float *W2, const float *b2)
{
    const int H = MLP_H;
    int r = 0;
    for (int kt = 0; kt < MLP_MT; ++kt)
        for (int t = 0; t < 16; ++t, ++r)
            for (int l = 0; l < 64; ++l)
                stream_rec(host, chunk, r)[l] = W2[(size_t)(32 * kt + mfma_row(t, l >> 5)) * H + 32 * m2 + (l & 31)];
    for (int l = 0; l < 32; ++l) stream_rec(host, chunk, r)[l] = b2[32 * m2 + l];
    return r + 1;
}

// The operand stream of the network IN -> 256 -> 256 -> OUT (W1 [IN][256], W2 [256][256], W3 [256][OUT], row-major), built in
// exactly the order the kernels consume it, into the zeroed host[floats].  False: the image does not fit, or an internal
// record count mismatch.
inline bool put_network(int IN, int OUT, const float *W1, const float *b1, const float *W2, const float *b2, const float *W3,
                        const float *b3, float *host, size_t floats)
{
    const int H = MLP_H;
    const MlpLayer1 L = mlp_layer1(IN);
    if (!L.fits() || (size_t)(L.chunks + MLP_MT) * MLP_CHREC * 64 > floats) return false;
    auto rec = [&](int chunk, int r) { return stream_rec(host, chunk, r); };
    for (int m = 0; m < MLP_MT; ++m) {                      // layer 1, natural k order: k = 2*ks + hf (k >= IN: zero pad)
        const int ch = m / L.tiles, base = (m % L.tiles) * L.records;
        for (int ks = 0; ks < L.width / 2; ++ks)
            for (int l = 0; l < 64; ++l) {
                const int k = 2 * ks + (l >> 5);
                if (k < IN) rec(ch, base + ks)[l] = W1[(size_t)k * H + 32 * m + (l & 31)];
            }
        for (int l = 0; l < 32; ++l) rec(ch, base + L.width / 2)[l] = b1[32 * m + l];
    }
    // The head: v_mfma_f32_4x4x1 (OUT <= 4) -- lane 4 b + i of every 4-lane block holds head row i of ITS half's hidden row --
    // or v_mfma_f32_16x16x1 (four blocks): lane 16 b + i holds head row i of block b's hidden row.  Rows i >= OUT are zero.
    const int row = OUT <= 4 ? 3 : 15;
    for (int m2 = 0; m2 < MLP_MT; ++m2) {                   // chunk L.chunks + m2: layer 2, then the head
        int r = put_layer2(host, L.chunks + m2, m2, W2, b2);
        for (int t = 0; t < 16; ++t, ++r)
            for (int l = 0; l < 64; ++l)
                if ((l & row) < OUT) rec(L.chunks + m2, r)[l] = W3[(size_t)(32 * m2 + mfma_row(t, l >> 5)) * OUT + (l & row)];
        if (r != MLP_PER) return false;
    }
    for (int l = 0; l < 64; ++l)                            // the head's bias rides at the end of the last chunk (B = 1 on lane half 0, 0 on half 1)
        if ((l & row) < OUT) rec(L.chunks + MLP_MT - 1, MLP_PER)[l] = b3[l & row];
    return true;
}

// ---- a head of up to 64 rows ("nig-categorical-v1", include/nig.h): four 16-row passes of the v_mfma_f32_16x16x1 head ----
// Pass 0 (rows 0 .. 15) is the 16-row head of put_network, in the chunks, so the image keeps the 148-record slot and every
// existing image its bytes.  Passes 1 .. 3 (rows 16 .. 63) do not travel through LDS: they lie in a TAIL of their own that the
// lanes read from global memory, one 16-byte entry per lane and hidden register.  Entry e = 16 m2 + t of lane l holds the words
// (pass 1, pass 2, pass 3, 0) = W3[32 m2 + mfma_row(t, l >> 5)][16 P + (l & 15)], zero for rows >= OUT; entry MLP_H / 2 holds the
// head's bias b3[16 P + (l & 15)] in the same words (B = 1 on lane half 0, 0 on half 1, as the chunk's bias record).
constexpr int MLP_WIDE_ROWS = 64, MLP_WIDE_PASSES = MLP_WIDE_ROWS / 16;
constexpr int MLP_TAIL_ENTRIES = MLP_MT * 16 + 1;                      // 129 entries of 64 lanes x 4 floats
constexpr int MLP_TAIL_FLOATS = MLP_TAIL_ENTRIES * 64 * 4;             // 129 KiB

// The image of the network IN -> 256 -> 256 -> OUT, 2 <= OUT <= 64 (W3 [256][OUT], row-major): put_network's image of the network
// whose head is columns 0 .. 15 of W3 (zero-padded to 16: the 16 x 16 x 1 layout whatever OUT is) into host[floats], and the tail
// of columns 16 .. 63 into the zeroed tail[MLP_TAIL_FLOATS].
inline bool put_network_wide(int IN, int OUT, const float *W1, const float *b1, const float *W2, const float *b2, const float *W3,
                             const float *b3, float *host, size_t floats, float *tail)
{
    if (OUT < 2 || OUT > MLP_WIDE_ROWS) return false;
    float W16[MLP_H * 16], b16[16];                         // (16 KiB of stack on the host's set-up path)
    for (int k = 0; k < MLP_H; ++k)
        for (int i = 0; i < 16; ++i) W16[k * 16 + i] = i < OUT ? W3[(size_t)k * OUT + i] : 0.0f;
    for (int i = 0; i < 16; ++i) b16[i] = i < OUT ? b3[i] : 0.0f;
    if (!put_network(IN, 16, W1, b1, W2, b2, W16, b16, host, floats)) return false;
    for (int e = 0; e < MLP_TAIL_ENTRIES; ++e)
        for (int l = 0; l < 64; ++l)
            for (int P = 1; P < MLP_WIDE_PASSES; ++P) {
                const int row = 16 * P + (l & 15);
                float v = 0.0f;
                if (row < OUT) v = e < MLP_MT * 16 ? W3[(size_t)(32 * (e / 16) + mfma_row(e % 16, l >> 5)) * OUT + row] : b3[row];
                tail[((size_t)e * 64 + l) * 4 + (P - 1)] = v;
            }
    return true;
}

}  // namespace nig
