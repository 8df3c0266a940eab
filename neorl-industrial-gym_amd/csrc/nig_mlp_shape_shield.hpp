// nig_mlp_shape_shield.hpp -- the fused shaped actor with its shaped safety-critic shield (device code only): MlpShapeShieldArgs<> and
// rollout_mlp_shape_shield_kernel<Env, Shape>, the kernels nig_rollout_mlp_safe launches when the handle's actor slot holds a shaped
// actor of class K (nig_set_mlp_policy_dims) AND its critic slot a shaped critic of the same class K (nig_set_mlp_safety_dims).  A
// family of its own: rollout_mlp_shape_kernel, rollout_mlp_body and every other kernel are not touched by it.
//
// THE LAW "nig-mlp-shape-shield-v1" (stated here once; restated in include/nig.h; agents/cql.py predict_with_safety for an agent
// whose actor and SafetyCritic share hidden_dims of a shape class).  For one live lane and one step on state s:
//   a      = actor(s): "nig-mlp-shape-v1" (nig_mlp_shape.hpp) bit for bit -- the action nig_rollout_mlp computes with the same actor.
//   x      = [s_0 .. s_{S-1}, a_0 .. a_{A-1}, 0 ..], zero-padded to the even layer-1 width of shape_plan(K, S + A).
//   pre    = the head pre-activation of the critic under "nig-mlp-shape-v1" with IN = S + A, OUT = 1, its hidden widths zero-padded
//            to the class K of the actor: layer 1 the fma chain in natural k order on x, the hidden layers that law's chains in the
//            accumulator-register order, the head the one-row case of the v_mfma_f32_4x4x1 head ON EVERY ENV (OUT = 1: the image's
//            row = 3 form) -- per lane half the chain over the last hidden layer's tiles in order, the head's bias on half 0 behind
//            the last tile, pre = c_0 + c_1.
//   p      = det_sigmoidf(pre);  shield = !(p < threshold).
//   The env receives a_j * 0.5f where shield and a_j otherwise, and steps on it as nig_step does (the shared step_core path of
//   rollout_mlp_shape_kernel); NIG_FLAG_SHIELDED is set on shielded live lanes; prob_out gets p of the unshielded action and act_out
//   the action the env received (nig_rollout_mlp_safe's outputs).
// A frozen lane writes what nig_rollout_mlp_safe's frozen lanes write (the INACTIVE flag word and a zero reward) and leaves its obs /
// act / prob words untouched.  Tallies and the launch counter behave as in nig_rollout_mlp_safe.  Non-finite inputs are outside the law.
#pragma once
#include "nig_mlp_shape.hpp"

namespace nig {

template <class Shape>
struct MlpShapeShieldArgs {
    MlpShapeArgs<Shape> a;      // a.m.wstream: the actor's image (nig_set_mlp_policy_dims: put_shape_network(K, S, A, ..))
    const float *cstream;       // the critic's image built by nig_set_mlp_safety_dims: put_shape_network(K, S + A, 1, ..)
    float *prob_out;            // [n_steps][>= B] p of the unshielded action (row k at prob_out + k * a.m.out_stride), may be NULL
    float threshold;            // shield when !(p < threshold)
};

// rollout_mlp_shape_kernel's scheme with a second pass (rollout_mlp_ln_shield_kernel's pattern):
//   * TWO compile-time plans, PA = shape_plan(K, S) and PC = shape_plan(K, S + A).  They share chrec (the LDS buffers are the actor
//     kernel's: NBUF of the class, one chunk slot each) and the chunking of every layer but the first: the critic's layer 1 may take
//     more chunks of fewer tiles than the actor's (PowerGrid, 512 wide: 2 chunks of 8 tiles -> 4 of 4);
//   * ONE fill chain over ONE cyclic chunk sequence -- the actor's PA.chunks chunks, then the critic's PC.chunks chunks; the source
//     pointer and the piece count are chosen by the chunk's index.  The chain runs NBUF - 1 chunks ahead, so the critic's first chunk
//     is on its way while the actor's head computes, and the next step's actor layer 1 while the critic's head does;
//   * the accumulator registers of the actor's hidden layers are the critic's (the actor's are dead once its head is reduced): a[A]
//     and s[S] stay live across its pass;
//   * the critic's layer-1 B operand is indexed at compile time out of [s, a, 0];
//   * the critic's head is the four-row head whatever the actor's is (OUT = 1).
template <class Env, class Shape>
__global__ void __launch_bounds__(BLOCK, Shape::WAVES) rollout_mlp_shape_shield_kernel(const MlpShapeShieldArgs<Shape> qq)
{
    constexpr int S = Env::S, A = Env::A, KS = Env::KS, KR = Env::KR;
    constexpr int KSN = KS > 0 ? KS : 1;
    static_assert(has_mlp_actor<Env>, "MFMA actor needs an even state dim and at most 16 actions");
    constexpr ShapePlan PA = shape_plan(Shape::CLS, S), PC = shape_plan(Shape::CLS, S + A);
    static_assert(shape_plan_fits(PA), "a layer-1 chunk must fit the chunk slot");
    static_assert(shape_plan_fits(PC), "a layer-1 chunk of the critic must fit the chunk slot");
    static_assert(PA.chrec == PC.chrec && PA.pieces == PC.pieces && PA.chunks - PA.l1_chunks == PC.chunks - PC.l1_chunks,
                  "the two plans differ in layer 1 alone");
    constexpr int NH = PA.nh, TA = PA.t[0], TB = NH == 3 ? PA.t[1] : 1, TL = PA.t[NH - 1];
    constexpr int NBUF = Shape::NBUF, RING = 8, CHUNKS = PA.chunks + PC.chunks;
    static_assert(NBUF >= 2 && NBUF * PA.chrec * 256 * Shape::WAVES <= 160 * 1024, "the LDS buffers of the blocks of a CU must fit 160 KiB");
    __shared__ __attribute__((aligned(16))) float s_w[NBUF][PA.chrec * 64];
    const float4 *const s_probit = NIG_PROBIT;               // the generator's table stays in global memory (rollout_mlp_body's choice)
    const MlpArgs &q = qq.a.m;
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

    // ---------------- the fill chain: chunk `f_chunk` of the cyclic sequence (actor, then critic) into buffer `f_buf` ----------------
    int f_chunk = 0, f_buf = 0, f_left = q.n_steps * CHUNKS;
    auto fill_next = [&]() __attribute__((always_inline)) {
        if (f_left <= 0) return;
        const bool critic = f_chunk >= PA.chunks;
        const int c = critic ? f_chunk - PA.chunks : f_chunk;
        const int pieces = critic ? (c < PC.l1_chunks ? PC.l1_pieces : PC.pieces)        // this wave's quarter of the KiB pieces
                                  : (c < PA.l1_chunks ? PA.l1_pieces : PA.pieces);
        const float *src = (critic ? qq.cstream : q.wstream) + (size_t)c * (PA.chrec * 64) + lane * 4u;
        for (int pc = (int)wave; pc < pieces; pc += BLOCK / 64)
            __builtin_amdgcn_global_load_lds((nig_glb_void *)(src + pc * 256), (nig_lds_void *)(&s_w[f_buf][pc * 256]), 16, 0, 0);
        --f_left;
        f_chunk = f_chunk + 1 == CHUNKS ? 0 : f_chunk + 1;
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
    // rollout_mlp_shape_kernel's chunk of layer n + 1 (in s_w[c_buf]): KT input tiles of `hin` into `acc`; LASTK: the bias record
    // behind them; HEAD 1 / 2: then the tile's 16 head records into `out` through the 4 x 4 x 1 / 16 x 16 x 1 head (and, behind the
    // last tile, the head's bias).  LDS reads run RING records ahead of their MFMA, the source order pinned.
    auto layer_chunk = [&](auto kt_, auto lastk_, auto head_, const f32x16 *hin, f32x16 &acc, auto &out, bool last_tile) __attribute__((always_inline)) {
        constexpr int KT = decltype(kt_)::value, HEADK = decltype(head_)::value;
        constexpr bool LASTK = decltype(lastk_)::value != 0, HEAD = HEADK != 0;
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
                if constexpr (HEADK == 1) out = __builtin_amdgcn_mfma_f32_4x4x1f32(aop, hv, out, 0, 0, 0);
                else out = __builtin_amdgcn_mfma_f32_16x16x1f32(aop, hv, out, 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (HEAD) {
            if (last_tile) {                                // + the head's bias
                if constexpr (HEADK == 1) out = __builtin_amdgcn_mfma_f32_4x4x1f32(ring[N % RING], one, out, 0, 0, 0);
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
    // Layer 1 of the actor (critic_ = 0, plan PA) or the critic (1, plan PC) into `h`: natural k order, two inputs per record, bias
    // and ReLU; x(k): input k of the network, a compile-time index
    auto layer1 = [&](auto critic_, auto x, f32x16 (&h)[TA]) __attribute__((always_inline)) {
        constexpr ShapePlan L = decltype(critic_)::value ? shape_plan(Shape::CLS, S + A) : shape_plan(Shape::CLS, S);
#pragma unroll
        for (int c1 = 0; c1 < L.l1_chunks; ++c1) {
            next_chunk();
            const float *wb = &s_w[c_buf][lane];
#pragma unroll
            for (int mm = 0; mm < L.l1_tiles; ++mm) {
                f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int ks = 0; ks < L.l1_rec - 1; ++ks) {
                    const float b = half ? x(2 * ks + 1) : x(2 * ks);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wb[(mm * L.l1_rec + ks) * 64], b, acc, 0, 0, 0);
                }
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wb[(mm * L.l1_rec + L.l1_rec - 1) * 64], one, acc, 0, 0, 0);   // + bias
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = fmaxf(acc[r], 0.0f);                               // ReLU
                h[c1 * L.l1_tiles + mm] = acc;
            }
            done_chunk();
        }
    };
    // the hidden layers behind layer 1 and the head, rollout_mlp_shape_kernel's: layer 2 of three held whole beside h1, the last
    // hidden layer a real loop, consumed by the head tile by tile
    auto hidden_and_head = [&](auto head_, f32x16 (&ha)[TA], [[maybe_unused]] f32x16 (&hb)[TB], auto &out) __attribute__((always_inline)) {
        if constexpr (NH == 3) {
            int none = 0;
#pragma unroll
            for (int m = 0; m < TB; ++m) {
                f32x16 acc = layer_tile(mlp_int<TA>{}, mlp_int<0>{}, ha, none, false);
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = fmaxf(acc[r], 0.0f);
                hb[m] = acc;
            }
        }
        for (int m = 0; m < TL; ++m) {
            if constexpr (NH == 3) (void)layer_tile(mlp_int<TB>{}, head_, hb, out, m + 1 == TL);
            else (void)layer_tile(mlp_int<TA>{}, head_, ha, out, m + 1 == TL);
        }
    };

    for (int it = 0; it < q.n_steps; ++it) {
        f32x16 ha[TA];
        [[maybe_unused]] f32x16 hb[TB];
        // ---------------- actor: "nig-mlp-shape-v1", rollout_mlp_shape_kernel's pass ----------------
        layer1(mlp_int<0>{}, [&](int k) __attribute__((always_inline)) { return s[k]; }, ha);
        {
            std::conditional_t<mlp_head4<Env>, f32x4, f32x16> out = {};     // this lane half's partial sums of the head rows
            hidden_and_head(mlp_int<mlp_head4<Env> ? 1 : 2>{}, ha, hb, out);
            if constexpr (mlp_head4<Env>) {
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
        }

        // ---------------- critic on x = [s, a, 0]: the class's network (S + A, 1) in the actor's registers ----------------
        layer1(mlp_int<1>{}, [&](int k) __attribute__((always_inline)) { return k < S ? s[k] : (k < S + A ? a[k - S] : 0.0f); }, ha);
        f32x4 z4 = {0, 0, 0, 0};
        hidden_and_head(mlp_int<1>{}, ha, hb, z4);
        const float prob = det_sigmoidf(z4[0] + __shfl_xor(z4[0], 32));
        const bool shield = !(prob < qq.threshold);
#pragma unroll
        for (int r = 0; r < A; ++r) a[r] = shield ? a[r] * 0.5f : a[r];

        // ---------------- IndustrialEnv.step (both lane halves, identical results): rollout_mlp_shape_kernel's ----------------
        const uint32_t orow = (uint32_t)it * q.out_stride;
        // the lane's index in this step's output addresses and generator key, formed here step by step: no address is kept in registers
        // across the layers
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
            if (qq.prob_out) (qq.prob_out + orow)[lo] = prob;
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
        fl |= shield ? NIG_FLAG_SHIELDED : 0u;
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
