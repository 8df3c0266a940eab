// nig_mlp_shape.hpp -- the fused MLP actor on MFMA for the hidden shapes beside 256 x 256 (device code only): MlpShapeArgs<> and
// rollout_mlp_shape_kernel<Env, Shape>, the kernels nig_rollout_mlp launches when the handle's actor slot holds a shaped actor, under
// the law "nig-mlp-shape-v1" (include/nig.h).  A family of its own: rollout_mlp_body and its kernels (nig_mlp.hpp) are not touched by it.
#pragma once
#include "nig_mlp.hpp"
#include "nig_mlp_shape_stream.hpp"  // the classes and the image's chunk plan (shared with the host's builder)

namespace nig {

// A shape class as a type: KIND names the class (SHAPE_KIND_*), WAVES the waves per SIMD the kernel is compiled for -- 2 where the
// hidden tiles that are live at once leave room in 256 registers (the 128-wide class: 64), 1 elsewhere (256 registers of h1, or
// 128 + 128 of h1 and h2: the unified 512-entry file, one block per CU) -- and NBUF the LDS buffers of one chunk slot each: the
// fill of chunk c + NBUF - 1 is in flight while chunk c is consumed.  The buffer counts are measured (DESIGN.md section 5a,
// profiles/shapes/buffers.txt): a third buffer takes 4.6 % off the two 512-wide classes on PowerGrid, whose layer 1 is two chunks
// behind the longest env step, and moves nothing else by more than its spread.
// Experiment builds only (profiles/mkvariant.sh; never libnig.so): -DNIG_SHAPE_NBUF=n gives every class n buffers.
#ifndef NIG_SHAPE_NBUF
#define NIG_SHAPE_NBUF 0
#endif
template <int KIND_, int WAVES_, int NBUF_>
struct MlpShapeT {
    static constexpr int KIND = KIND_, WAVES = WAVES_, NBUF = NIG_SHAPE_NBUF ? NIG_SHAPE_NBUF : NBUF_;
    static constexpr MlpShapeClass CLS = SHAPE_CLASSES[KIND_];
};
using Shape128 = MlpShapeT<SHAPE_KIND_128, 2, 2>;
using Shape512x256 = MlpShapeT<SHAPE_KIND_512x256, 1, 3>;
using Shape512 = MlpShapeT<SHAPE_KIND_512, 1, 3>;
using Shape3 = MlpShapeT<SHAPE_KIND_3, 1, 2>;

template <class Shape>
struct MlpShapeArgs {
    MlpArgs m;                  // m.wstream: the image built by nig_set_mlp_policy_dims (put_shape_network)
};

// rollout_mlp_body's transposed scheme (nig_mlp.hpp: env on the lane, hidden unit in the register, v_mfma_f32_32x32x2_f32, the
// 4 x 4 x 1 / 16 x 16 x 1 head, weights through LDS buffers filled by LDS-DMA) on the chunk plan of nig_mlp_shape_stream.hpp:
//   * every hidden layer but the last is held whole in registers (its tile loop is unrolled: a register array takes no run-time
//     index), the last is produced tile by tile in a real loop and consumed at once by its slice of the head;
//   * a layer that reads 16 tiles (K = 512) takes two chunks per output tile, the accumulator carried across them, the bias and the
//     head's slice behind the second;
//   * the fills follow one cyclic chunk sequence (the weights do not change from step to step): a counter names the chunk filled
//     next, so layer 1 of the next step is in flight behind the last tile of this one.
template <class Env, class Shape>
__global__ void __launch_bounds__(BLOCK, Shape::WAVES) rollout_mlp_shape_kernel(const MlpShapeArgs<Shape> qq)
{
    constexpr int S = Env::S, A = Env::A, KS = Env::KS, KR = Env::KR;
    constexpr int KSN = KS > 0 ? KS : 1;
    static_assert(has_mlp_actor<Env>, "MFMA actor needs an even state dim and at most 16 actions");
    constexpr ShapePlan P = shape_plan(Shape::CLS, S);
    static_assert(shape_plan_fits(P), "a layer-1 chunk must fit the chunk slot");
    constexpr int NH = P.nh, TA = P.t[0], TB = NH == 3 ? P.t[1] : 1, TL = P.t[NH - 1];
    constexpr int NBUF = Shape::NBUF, RING = 8;
    static_assert(NBUF >= 2 && NBUF * P.chrec * 256 * Shape::WAVES <= 160 * 1024, "the LDS buffers of the blocks of a CU must fit 160 KiB");
    __shared__ __attribute__((aligned(16))) float s_w[NBUF][P.chrec * 64];
    const float4 *const s_probit = NIG_PROBIT;               // the generator's table stays in global memory (rollout_mlp_body's choice)
    const MlpArgs &q = qq.m;
    const StepArgs &p = q.s;
    const unsigned tid = threadIdx.x, lane = tid & 63u, half = lane >> 5, e = lane & 31u, wave = tid >> 6;
    const uint32_t li = blockIdx.x * (BLOCK / 2) + wave * 32u + e;
    const bool in_range = li < p.B;
    const bool writer = in_range && half == 0;
    const uint32_t t_base = (p.t_ptr ? *p.t_ptr : 0u) + p.t_off;
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

    // ---------------- the fill chain: chunk `f_chunk` of the cyclic sequence into buffer `f_buf`, `f_left` fills to go ----------------
    int f_chunk = 0, f_buf = 0, f_left = q.n_steps * P.chunks;
    auto fill_next = [&]() __attribute__((always_inline)) {
        if (f_left <= 0) return;
        const int pieces = f_chunk < P.l1_chunks ? P.l1_pieces : P.pieces;       // this wave's quarter of the KiB pieces
        const float *src = q.wstream + (size_t)f_chunk * (P.chrec * 64) + lane * 4u;
        for (int pc = (int)wave; pc < pieces; pc += BLOCK / 64)
            __builtin_amdgcn_global_load_lds((nig_glb_void *)(src + pc * 256), (nig_lds_void *)(&s_w[f_buf][pc * 256]), 16, 0, 0);
        --f_left;
        f_chunk = f_chunk + 1 == P.chunks ? 0 : f_chunk + 1;
        f_buf = f_buf + 1 == NBUF ? 0 : f_buf + 1;
    };
    int c_buf = 0;                                           // buffer that holds (or receives) the chunk consumed next
    // chunk boundary: every wave's share of the fills has landed (vmcnt is drained before the barrier) and every wave is done with
    // the buffer the next fill overwrites -- the one consumed last
    auto next_chunk = [&]() __attribute__((always_inline)) {
        __builtin_amdgcn_s_waitcnt(0x0F70);                 // vmcnt(0): this wave's LDS-DMA pieces are in LDS before any wave reads them
        __syncthreads();
        fill_next();
    };
    auto done_chunk = [&]() __attribute__((always_inline)) { c_buf = c_buf + 1 == NBUF ? 0 : c_buf + 1; };
#pragma unroll
    for (int j = 0; j < NBUF - 1; ++j) fill_next();

    const float one = half ? 0.0f : 1.0f;                    // the bias records' B operand
    // One chunk of layer n + 1 (in s_w[c_buf]): KT input tiles of `hin` into `acc`; LASTK: the bias record behind them; HEAD: then the
    // tile's 16 head records into `out` (and, behind the last tile, the head's bias).  LDS reads run RING records ahead of their
    // MFMA, the source order pinned (rollout_mlp_body's layer2_chunk).
    auto layer_chunk = [&](auto kt_, auto lastk_, auto head_, const f32x16 *hin, f32x16 &acc, auto &out, bool last_tile) __attribute__((always_inline)) {
        constexpr int KT = decltype(kt_)::value;
        constexpr bool LASTK = decltype(lastk_)::value != 0, HEAD = decltype(head_)::value != 0;
        constexpr int N = 16 * KT + (LASTK ? 1 : 0) + (HEAD ? 16 : 0), NREAD = N + (HEAD ? 1 : 0);
        static_assert(N >= RING && (!HEAD || LASTK));
        const float *wb = &s_w[c_buf][lane];
        float ring[RING];
#pragma unroll
        for (int j = 0; j < RING; ++j) ring[j] = wb[j * 64];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const float aop = ring[i % RING];
            if (i + RING < NREAD) ring[i % RING] = wb[(i + RING) * 64];
            __builtin_amdgcn_sched_barrier(0);
            if (i < 16 * KT) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aop, hin[i / 16][i % 16], acc, 0, 0, 0);
            } else if (i == 16 * KT) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aop, one, acc, 0, 0, 0);      // + bias
            } else if constexpr (HEAD) {
                const float hv = fmaxf(acc[(i - 16 * KT - 1) & 15], 0.0f);              // own value x the weights of the lane's block
                if constexpr (mlp_head4<Env>) out = __builtin_amdgcn_mfma_f32_4x4x1f32(aop, hv, out, 0, 0, 0);
                else out = __builtin_amdgcn_mfma_f32_16x16x1f32(aop, hv, out, 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (HEAD) {
            if (last_tile) {                                // + the head's bias
                if constexpr (mlp_head4<Env>) out = __builtin_amdgcn_mfma_f32_4x4x1f32(ring[N % RING], one, out, 0, 0, 0);
                else out = __builtin_amdgcn_mfma_f32_16x16x1f32(ring[N % RING], one, out, 0, 0, 0);
            }
        }
    };
    // all chunks of one output tile of layer n + 1 (TIN input tiles): the accumulator carried across them
    auto layer_tile = [&](auto tin_, auto head_, const f32x16 *hin, auto &out, bool last_tile) __attribute__((always_inline)) {
        constexpr int TIN = decltype(tin_)::value;
        f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if constexpr (TIN > 8) {
            static_assert(TIN == 16);
            int none = 0;
            next_chunk();
            layer_chunk(mlp_int<8>{}, mlp_int<0>{}, mlp_int<0>{}, hin, acc, none, false);
            done_chunk();
            next_chunk();
            layer_chunk(mlp_int<8>{}, mlp_int<1>{}, head_, hin + 8, acc, out, last_tile);
            done_chunk();
        } else {
            next_chunk();
            layer_chunk(tin_, mlp_int<1>{}, head_, hin, acc, out, last_tile);
            done_chunk();
        }
        return acc;
    };

    for (int it = 0; it < q.n_steps; ++it) {
        // ---------------- actor: NH hidden layers and the head of f32 MFMA, whole wave (EXEC all ones) ----------------
        f32x16 ha[TA];
        [[maybe_unused]] f32x16 hb[TB];
#pragma unroll
        for (int c1 = 0; c1 < P.l1_chunks; ++c1) {           // layer 1: natural k order, two inputs per record
            next_chunk();
            const float *wb = &s_w[c_buf][lane];
#pragma unroll
            for (int mm = 0; mm < P.l1_tiles; ++mm) {
                f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int ks = 0; ks < P.l1_rec - 1; ++ks) {
                    const float b = half ? s[2 * ks + 1] : s[2 * ks];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wb[(mm * P.l1_rec + ks) * 64], b, acc, 0, 0, 0);
                }
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wb[(mm * P.l1_rec + P.l1_rec - 1) * 64], one, acc, 0, 0, 0);   // + bias
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = fmaxf(acc[r], 0.0f);                               // ReLU
                ha[c1 * P.l1_tiles + mm] = acc;
            }
            done_chunk();
        }
        if constexpr (NH == 3) {                             // layer 2 of three: held whole, beside h1
            int none = 0;
#pragma unroll
            for (int m = 0; m < TB; ++m) {
                f32x16 acc = layer_tile(mlp_int<TA>{}, mlp_int<0>{}, ha, none, false);
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = fmaxf(acc[r], 0.0f);
                hb[m] = acc;
            }
        }
        std::conditional_t<mlp_head4<Env>, f32x4, f32x16> out = {};     // this lane half's partial sums of the head rows
        for (int m = 0; m < TL; ++m) {                       // the last hidden layer: a real loop, consumed by the head tile by tile
            if constexpr (NH == 3) (void)layer_tile(mlp_int<TB>{}, mlp_int<1>{}, hb, out, m + 1 == TL);
            else (void)layer_tile(mlp_int<TA>{}, mlp_int<1>{}, ha, out, m + 1 == TL);
        }
        if constexpr (mlp_head4<Env>) {
            // action r = this half's partial sum + the other half's (lane l and l + 32 carry the same env)
#pragma unroll
            for (int r = 0; r < A; ++r) a[r] = det_tanhf(out[r] + __shfl_xor(out[r], 32));
        } else {
            // head row r of env column c (env 16 beta + c): lane 16 (r >> 2) + c, registers 4 beta + (r & 3) and 8 + 4 beta + (r & 3)
            const int beta = (int)(e >> 4);
#pragma unroll
            for (int r = 0; r < A; ++r) {
                const int src = 16 * (r >> 2) + (int)(e & 15u);
                const float v0 = __shfl(out[r & 3] + out[8 + (r & 3)], src);
                const float v1 = __shfl(out[4 + (r & 3)] + out[12 + (r & 3)], src);
                a[r] = det_tanhf(beta ? v1 : v0);
            }
        }

        // ---------------- IndustrialEnv.step (both lane halves, identical results): rollout_mlp_body's ----------------
        const uint32_t orow = (uint32_t)it * q.out_stride;
        // the lane's index in this step's output addresses and generator key, formed here step by step: no address is kept in registers
        // across the layers (with 256 registers of h1 beside the state, a hoisted address pair is a spilled one)
        uint32_t lo = li;
        asm volatile("" : "+v"(lo));
        const bool frozen = (ctr & NIG_CTR_DONE) != 0;
        if (writer && !frozen) {
            if (q.obs_out) {
                float *oo = q.obs_out + (size_t)it * q.obs_step_stride + (size_t)lo * S;
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
                for (int j = 0; j < A; ++j) (ao + j * q.ld_act_out)[lo] = a[j];
            }
        }
        const RngKey key = make_key(p.env0 + (uint64_t)lo, t_base + (uint32_t)it + 1u, p.seed_lo, p.seed_hi, s_probit);
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
            if (p.reward) (p.reward + orow)[lo] = rew;
            if (p.flags) (p.flags + orow)[lo] = fl;
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
