// nig_mlp_bf16.hpp -- the fused MLP actor on the bf16 matrix unit (device code only): MlpBf16Args and rollout_mlp_bf16_kernel, the
// kernel of nig_rollout_mlp_bf16 under the law "nig-mlp-bf16-v1" (include/nig.h).  A family of its own: rollout_mlp_body and its
// kernels (nig_mlp.hpp) are not touched by it.
#pragma once
#include "nig_mlp.hpp"
#include "nig_mlp_bf16_stream.hpp"   // the image's chunk plan (shared with the host's builder)

namespace nig {

// rollout_mlp_body's shape on v_mfma_f32_32x32x16_bf16 (32 cycles for K = 16, where v_mfma_f32_32x32x2_f32 takes 64 for K = 2):
// one wave = 32 envs with the env on the lane, both lane halves carry the state, everything transposed (h^T = W^T x^T), the
// image through the double-buffered LDS buffers filled by LDS-DMA, two blocks per CU.
//   * A operand = weights, 8 bf16 per lane: one ds_read_b128 of a record per MFMA.
//   * B operand = activations in registers.  Layer 1: element j of lane half h in k-step s is x[16 s + 8 h + j], x = the
//     observation as bf16 hi and lo parts.  Layers 2 and 3: registers 8 s .. 8 s + 7 of a 32 x 32 result tile, through ReLU,
//     converted pairwise (v_cvt_pk_bf16_f32, round to nearest even), ARE k-step s's fragment -- no lane movement; the k order
//     inside the step is bf16_acc_k's, which the image's builder follows.
//   * An accumulator starts from its float32 biases (16 per lane half, from the chunk's bias record).
//   * The head runs on the same instruction, W3^T zero-padded to 32 rows, accumulated over the eight h2 tiles as they are made;
//     action row j lands in register (j & 3) + 4 (j >> 3) of lane half (j >> 2) & 1, and one exchange across the halves per
//     register hands both halves the whole action.
// MFMAs per step: 8 bf16_l1_ksteps(S) + 128 + 16 (ChemicalReactor 160, PowerGrid 176) against the f32 kernel's 1 217.
struct MlpBf16Args {
    MlpArgs m;                  // m.wstream: the bf16 image built by nig_set_mlp_policy_bf16 (BF16_STREAM_BYTES bytes)
    uint16_t *hid_out;          // h1, h2 as bf16 words: step k, layer L, unit u of a lane at hid_out + k * hid_step_stride + (L * 256 + u) * ld_hid + lane; may be NULL
    uint32_t ld_hid; uint64_t hid_step_stride;
};

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using u32x4v = __attribute__((ext_vector_type(4))) uint32_t;
using f32x2v = __attribute__((ext_vector_type(2))) float;

// two float32 -> one word of two bf16 (lo in the low half), round to nearest even: v_cvt_pk_bf16_f32
__device__ __forceinline__ uint32_t bf16_pack(float lo, float hi)
{
    const f32x2v v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ float bf16_round(float x) { return (float)(__bf16)x; }

template <class Env>
__global__ void __launch_bounds__(BLOCK, 2) rollout_mlp_bf16_kernel(const MlpBf16Args qq)
{
    constexpr int S = Env::S, A = Env::A, KS = Env::KS, KR = Env::KR;
    constexpr int KSN = KS > 0 ? KS : 1;
    static_assert(has_mlp_actor<Env>, "MFMA actor needs an even state dim and at most 16 actions");
    static_assert(bf16_l1_fits(S), "layer 1 must fit one chunk");
    constexpr int K1 = bf16_l1_ksteps(S), L1_PIECES = bf16_l1_pieces(S);
    constexpr int RING = 4;                                  // LDS reads in flight ahead of their MFMA (32 cycles apart)
    // two buffers of one chunk each: 74 KiB per block, two blocks per CU (the generator's table stays in global memory)
    __shared__ __attribute__((aligned(16))) unsigned char s_w[2][BF16_CHREC * BF16_REC_BYTES];
    const float4 *const s_probit = NIG_PROBIT;
    const MlpArgs &q = qq.m;
    const StepArgs &p = q.s;
    const unsigned tid = threadIdx.x, lane = tid & 63u, half = lane >> 5, e = lane & 31u, wave = tid >> 6;
    const uint32_t li = blockIdx.x * (BLOCK / 2) + wave * 32u + e;
    const bool in_range = li < p.B;
    const bool writer = in_range && half == 0;
    const uint32_t t_base = (p.t_ptr ? *p.t_ptr : 0u) + p.t_off;
    const uint64_t gi = p.env0 + (uint64_t)li;
    const bool autoreset = (p.hflags & NIG_F_AUTORESET) != 0;
    const bool tally = p.tally != nullptr;

    uint32_t ctr = in_range ? p.ctr[li] : (uint32_t)NIG_CTR_DONE;
    float s[S], a[A], n[S];
    typename Env::fast_noise_t nz[KSN];
#pragma unroll
    for (int k = 0; k < S; ++k) s[k] = in_range ? (p.state + k * p.ld_state)[li] : 0.0f;
    double ret = (tally && in_range) ? p.ep_ret[li] : 0.0;
    LaneTally lt;
    lt.clear();
    // fill LDS buffer `buf` with the first `pieces` records of chunk `c`: this wave's quarter of them
    auto fill = [&](int c, int buf, int pieces) __attribute__((always_inline)) {
        const unsigned char *src = (const unsigned char *)q.wstream + (size_t)c * (BF16_CHREC * BF16_REC_BYTES) + lane * 16u;
        for (int pc = (int)wave; pc < pieces; pc += BLOCK / 64)
            __builtin_amdgcn_global_load_lds((nig_glb_void *)(src + pc * BF16_REC_BYTES), (nig_lds_void *)(&s_w[buf][pc * BF16_REC_BYTES]), 16, 0, 0);
    };
    auto a_op = [&](int buf, int r) __attribute__((always_inline)) { return *(const bf16x8 *)(&s_w[buf][r * BF16_REC_BYTES + lane * 16u]); };
    // the float32 biases a tile's accumulator starts from: block `b` of the bias record `r`
    auto bias_tile = [&](int buf, int r, int b) __attribute__((always_inline)) {
        const float4 *bb = (const float4 *)(&s_w[buf][r * BF16_REC_BYTES + (32 * b + 16 * half) * 4]);
        const float4 b0 = bb[0], b1 = bb[1], b2 = bb[2], b3 = bb[3];
        f32x16 acc = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w, b2.x, b2.y, b2.z, b2.w, b3.x, b3.y, b3.z, b3.w};
        return acc;
    };
    // ReLU, then the tile as two k-step fragments; the lane's 16 units of layer `layer`, tile `m` to hid_out
    auto pack_tile = [&](const f32x16 &acc, u32x4v (&frag)[2], uint16_t *hid, int layer, int m) __attribute__((always_inline)) {
#pragma unroll
        for (int w = 0; w < 8; ++w) frag[w >> 2][w & 3] = bf16_pack(fmaxf(acc[2 * w], 0.0f), fmaxf(acc[2 * w + 1], 0.0f));
        if (hid) {
            // (the lane's address is formed here, tile by tile: hoisted out of the step loop, the 32 tiles' addresses were spilled)
            uint32_t lo = li;
            asm volatile("" : "+v"(lo));
            uint16_t *hp = hid + (size_t)((uint32_t)(layer * MLP_H + 32 * m) + 4u * half) * qq.ld_hid + lo;
#pragma unroll
            for (int t = 0; t < 16; ++t)
                hp[(size_t)((t & 3) + 8 * (t >> 2)) * qq.ld_hid] = (uint16_t)(frag[t >> 3][(t >> 1) & 3] >> (16 * (t & 1)));
        }
    };
    fill(0, 0, L1_PIECES);
    int gbuf = 0;                                            // buffer that holds (or receives) the chunk consumed next
    for (int it = 0; it < q.n_steps; ++it) {
        const bool frozen = (ctr & NIG_CTR_DONE) != 0;
        // h1, h2 leave from BOTH lane halves (each holds its own rows of a tile); frozen lanes and lanes past the batch store nothing
        uint16_t *const hid = (qq.hid_out && in_range && !frozen) ? qq.hid_out + (size_t)it * qq.hid_step_stride : nullptr;
        // ---------------- the observation as bf16 hi / lo parts: layer 1's B fragments ----------------
        u32x4v xf[K1];
        {
            float x[16 * K1];
#pragma unroll
            for (int k = 0; k < 16 * K1; ++k) x[k] = 0.0f;
#pragma unroll
            for (int k = 0; k < S; ++k) {
                const float hi = bf16_round(s[k]);
                const float lo = s[k] - hi;                  // exact
                x[k] = hi;
                x[S + k] = (__builtin_fabsf(hi) < __builtin_inff()) ? lo : 0.0f;
            }
#pragma unroll
            for (int ks = 0; ks < K1; ++ks)
#pragma unroll
                for (int w = 0; w < 4; ++w)
                    xf[ks][w] = half ? bf16_pack(x[16 * ks + 8 + 2 * w], x[16 * ks + 9 + 2 * w]) : bf16_pack(x[16 * ks + 2 * w], x[16 * ks + 2 * w + 1]);
        }
        // ---------------- layer 1: chunk 0 ----------------
        u32x4v h1[MLP_MT][2];
        __syncthreads();                                    // every wave's share of the fill has landed; the other buffer is free
        fill(1, gbuf ^ 1, BF16_CHREC);
        {
            // LDS reads RING records ahead of their MFMA, the source order pinned: hipcc's scheduler otherwise hoists every read of
            // the unrolled code to its top and spills the operands it then holds
            bf16x8 ring[RING];
#pragma unroll
            for (int j = 0; j < RING; ++j) ring[j] = a_op(gbuf, j);
#pragma unroll
            for (int m = 0; m < MLP_MT; ++m) {
                f32x16 acc = bias_tile(gbuf, MLP_MT * K1, m);
#pragma unroll
                for (int ks = 0; ks < K1; ++ks) {
                    const int i = m * K1 + ks;
                    const bf16x8 aop = ring[i % RING];
                    if (i + RING < MLP_MT * K1) ring[i % RING] = a_op(gbuf, i + RING);
                    __builtin_amdgcn_sched_barrier(0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aop, __builtin_bit_cast(bf16x8, xf[ks]), acc, 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                pack_tile(acc, h1[m], hid, 0, m);
            }
        }
        gbuf ^= 1;
        // ---------------- layer 2 and the head: chunks 1 .. 4, two hidden tiles each ----------------
        f32x16 out = {};
        for (int c = 0; c < MLP_MT / BF16_CH_TILES; ++c) {  // a real loop: the body is 36 MFMAs of straight-line code
            __syncthreads();                                // chunk 1 + c is in s_w[gbuf]; s_w[gbuf ^ 1] is free
            if (c + 1 < MLP_MT / BF16_CH_TILES) fill(2 + c, gbuf ^ 1, BF16_CHREC);
            else if (it + 1 < q.n_steps) fill(0, gbuf ^ 1, L1_PIECES);      // layer 1 of the NEXT step (the weights do not change)
            if (c == 0) out = bias_tile(gbuf, BF16_BIAS_REC, BF16_CH_TILES);
            bf16x8 ring[RING];
#pragma unroll
            for (int j = 0; j < RING; ++j) ring[j] = a_op(gbuf, j);
            // one MFMA on record i of the chunk (the tile's records follow each other: 16 of layer 2, 2 of the head)
            auto mfma_rec = [&](int i, const u32x4v &b, f32x16 acc) __attribute__((always_inline)) {
                const bf16x8 aop = ring[i % RING];
                if (i + RING < BF16_BIAS_REC) ring[i % RING] = a_op(gbuf, i + RING);
                __builtin_amdgcn_sched_barrier(0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aop, __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                return acc;
            };
#pragma unroll
            for (int tt = 0; tt < BF16_CH_TILES; ++tt) {
                f32x16 acc = bias_tile(gbuf, BF16_BIAS_REC, tt);
#pragma unroll
                for (int i = 0; i < 2 * MLP_MT; ++i) acc = mfma_rec(tt * BF16_TILE_REC + i, h1[i >> 1][i & 1], acc);
                u32x4v h2[2];
                pack_tile(acc, h2, hid, 1, BF16_CH_TILES * c + tt);
#pragma unroll
                for (int sx = 0; sx < 2; ++sx) out = mfma_rec(tt * BF16_TILE_REC + 2 * MLP_MT + sx, h2[sx], out);
            }
            gbuf ^= 1;
        }
        // action row j: register (j & 3) + 4 (j >> 3) of lane half (j >> 2) & 1; lanes l and l ^ 32 carry the same env
#pragma unroll
        for (int j = 0; j < A; ++j) {
            const float mine = out[(j & 3) + 4 * (j >> 3)];
            const float other = __shfl_xor(mine, 32);
            a[j] = det_tanhf((int)half == ((j >> 2) & 1) ? mine : other);
        }

        // ---------------- IndustrialEnv.step (both lane halves, identical results): rollout_mlp_body's ----------------
        const uint32_t orow = (uint32_t)it * q.out_stride;
        if (writer && !frozen) {
            if (q.obs_out) {
                float *oo = q.obs_out + (size_t)it * q.obs_step_stride + (size_t)li * S;
                if constexpr (S % 4 == 0) {
#pragma unroll
                    for (int k = 0; k < S / 4; ++k) store16(oo + 4 * k, s[4 * k], s[4 * k + 1], s[4 * k + 2], s[4 * k + 3]);
                } else {
#pragma unroll
                    for (int k = 0; k < S; ++k) oo[k] = s[k];
                }
            }
            if (q.act_out) {
                float *ao = q.act_out + (size_t)it * q.act_step_stride;
#pragma unroll
                for (int j = 0; j < A; ++j) (ao + j * q.ld_act_out)[li] = a[j];
            }
        }
        const RngKey key = make_key(gi, t_base + (uint32_t)it + 1u, p.seed_lo, p.seed_hi, s_probit);
        if constexpr (KS > 0) Env::draw_step(key, nz); else nz[0] = 0;
        const int step_pre = (int)(ctr & NIG_CTR_STEP_MASK);
        StepResult<Env, reward_of<Env, float>> res;
        step_core<Env>(s, a, nz, step_pre, p.max_steps, p.dt32, p.dt, p.cmask, n, res);
        const int step = step_pre + 1;
        const uint32_t viol_ep = episode_violations(ctr, res.nviol);
        const bool done = (res.terminated || res.truncated) && !frozen;
        uint32_t fl = pack_flags<Env>(res, step) | did_reset_flag(done && autoreset);
        float rew = (float)res.reward;
        if (frozen) {
            fl = NIG_FLAG_INACTIVE | ((ctr & NIG_CTR_STEP_MASK) << NIG_FLAG_STEP_SHIFT);
            rew = 0.0f;
#pragma unroll
            for (int k = 0; k < S; ++k) n[k] = s[k];
        } else {
            ctr = counter_word(step, viol_ep);
            if (tally) ret = add_reward<Env, false>(ret, res.reward);
        }
        if (writer) {
            if (p.reward) (p.reward + orow)[li] = rew;
            if (p.flags) (p.flags + orow)[li] = fl;
        }
        if (done) {
            ret = lt.finish(tally, ret, step, viol_ep, res.ncrit);
            if (autoreset) {
                double rn[KR > 0 ? KR : 1];
                Env::draw_init(key, rn);
                Env::init(rn, n);
                ctr = 0u;
            } else {
                ctr |= NIG_CTR_DONE;
            }
        }
#pragma unroll
        for (int k = 0; k < S; ++k) s[k] = n[k];
    }
    if (!writer) return;
#pragma unroll
    for (int k = 0; k < S; ++k) (p.state + k * p.ld_state)[li] = s[k];
    store_episode(p.ctr, p.life_viol, p.ep_ret, p.tally, p.ld, p.n_en, 0u, li, tally, ctr, lt.life, ret, lt);
}

}  // namespace nig
