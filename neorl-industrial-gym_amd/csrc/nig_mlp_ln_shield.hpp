// nig_mlp_ln_shield.hpp -- the fused LayerNorm actor with its LayerNorm safety-critic shield (device code only): MlpLnShieldArgs and
// rollout_mlp_ln_shield_kernel<Env>, the kernel nig_rollout_mlp_safe launches when the handle's actor slot holds a LayerNorm actor
// (nig_set_mlp_policy_ln) AND its critic slot a LayerNorm critic (nig_set_mlp_safety_ln).  A family of its own: rollout_mlp_ln_kernel,
// rollout_mlp_body and every other kernel are not touched by it.
//
// THE LAW "nig-mlp-ln-shield-v1" (stated here once; restated in include/nig.h; agents/cql.py predict_with_safety for an agent built
// with use_layer_norm=True).  For one live lane and one step on state s:
//   a      = actor(s): "nig-mlp-ln-v1" (nig_mlp_ln.hpp) bit for bit -- the action nig_rollout_mlp computes with the same actor.
//   x      = [s_0 .. s_{S-1}, a_0 .. a_{A-1}, 0 ..], zero-padded to the layer-1 width of mlp_layer1(S + A).
//   pre    = the head pre-activation of the critic under "nig-mlp-ln-v1" with IN = S + A, OUT = 1 -- (S + A) -> 256 -> LayerNorm ->
//            ReLU -> 256 -> LayerNorm -> ReLU -> 1 with the critic's own eps: layer 1 the fma chain in natural k order on x, steps
//            2 .. 5 of that law on both layers, the head the one-row case of the v_mfma_f32_4x4x1 head -- the two lane-half chains
//            c_h = fma(C3[32 m + rho_h(t)], h[32 m + rho_h(t)], c_h) over m = 0 .. 7, t = 0 .. 15, the bias on half 0
//            (c_0 = fma(c3, 1, c_0), c_1 = fma(c3, 0, c_1)), pre = c_0 + c_1.
//   p      = det_sigmoidf(pre);  shield = !(p < threshold).
//   The env receives a_j * 0.5f where shield and a_j otherwise, and steps on it as nig_step does; NIG_FLAG_SHIELDED is set on
//   shielded live lanes; prob_out gets p and act_out the action the env received (nig_rollout_mlp_safe's outputs).
// A frozen lane writes what nig_rollout_mlp_safe's frozen lanes write (the INACTIVE flag word and a zero reward) and leaves its obs /
// act / prob words untouched.  Non-finite inputs are outside the law, as in "nig-mlp-ln-v1".
#pragma once
#include "nig_mlp_ln.hpp"

namespace nig {

struct MlpLnShieldArgs {
    MlpLnArgs a;                // a.m.wstream: the actor's image (nig_set_mlp_policy_ln); a.eps: the actor's
    const float *cstream;       // the critic's image built by nig_set_mlp_safety_ln: put_ln_network(S + A, 1, ..)
    float *prob_out;            // [n_steps][>= B] p of the unshielded action (row k at prob_out + k * a.m.out_stride), may be NULL
    float threshold;            // shield when !(p < threshold)
    float ceps;                 // the critic's eps
};

// rollout_mlp_ln_kernel's scheme with a second pass:
//   * ONE fill chain over ONE cyclic chunk sequence -- the actor's ln_plan(S) chunks, then the critic's ln_plan(S + A) chunks; the
//     source pointer is chosen by the chunk's index.  The chain runs one chunk ahead, so the critic's first chunk is on its way
//     while the actor's head computes, and the next step's actor layer 1 while the critic's head does;
//   * both gamma / beta tables (2 x 4 KiB) are staged in LDS once per launch;
//   * the 128 + 128 accumulator registers of the actor's two layers are the critic's: a[A] and s[S] stay live across its pass;
//   * the critic's layer-1 B operand is indexed at compile time out of s and a (rollout_mlp_body's x(k));
//   * the critic's head is the four-row head whatever the actor's is (OUT = 1).
template <class Env>
__global__ void __launch_bounds__(BLOCK, 1) rollout_mlp_ln_shield_kernel(const MlpLnShieldArgs qq)
{
    constexpr int S = Env::S, A = Env::A, KS = Env::KS, KR = Env::KR;
    constexpr int KSN = KS > 0 ? KS : 1;
    static_assert(has_mlp_actor<Env>, "MFMA actor needs an even state dim and at most 16 actions");
    constexpr LnPlan P = ln_plan(S), C = ln_plan(S + A);
    static_assert(P.l1.fits(), "a layer-1 chunk must fit the chunk slot");
    static_assert(C.l1.fits(), "a layer-1 chunk of the critic must fit the chunk slot");
    constexpr int NBUF = 2, RING = 8, CHUNKS = P.chunks + C.chunks;
    __shared__ __attribute__((aligned(16))) float s_w[NBUF][MLP_CHREC * 64];
    __shared__ __attribute__((aligned(16))) float s_tab[2 * LN_TABLE_FLOATS];       // the actor's table, then the critic's
    const float4 *const s_probit = NIG_PROBIT;
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
        const bool critic = f_chunk >= P.chunks;
        const int c = critic ? f_chunk - P.chunks : f_chunk;
        const int pieces = critic ? (c < C.l1.chunks ? C.l1.pieces : c < C.head_chunk ? C.l2_pieces : C.head_pieces)
                                  : (c < P.l1.chunks ? P.l1.pieces : c < P.head_chunk ? P.l2_pieces : P.head_pieces);
        const float *src = (critic ? qq.cstream : q.wstream) + (size_t)c * (MLP_CHREC * 64) + lane * 4u;
        for (int pc = (int)wave; pc < pieces; pc += BLOCK / 64)
            __builtin_amdgcn_global_load_lds((nig_glb_void *)(src + pc * 256), (nig_lds_void *)(&s_w[f_buf][pc * 256]), 16, 0, 0);
        --f_left;
        f_chunk = f_chunk + 1 == CHUNKS ? 0 : f_chunk + 1;
        f_buf = f_buf + 1 == NBUF ? 0 : f_buf + 1;
    };
    int c_buf = 0;                                           // buffer that holds (or receives) the chunk consumed next
    auto next_chunk = [&]() __attribute__((always_inline)) {
        __builtin_amdgcn_s_waitcnt(0x0F70);                 // vmcnt(0): this wave's LDS-DMA pieces are in LDS before any wave reads them
        __syncthreads();
        fill_next();
    };
    auto done_chunk = [&]() __attribute__((always_inline)) { c_buf = c_buf + 1 == NBUF ? 0 : c_buf + 1; };
#pragma unroll
    for (int j = 0; j < NBUF - 1; ++j) fill_next();
    {                                                        // gamma / beta of both networks: 256 threads x 16 bytes each, once per launch
        static_assert(LN_TABLE_FLOATS == BLOCK * 4);
        const float4 va = reinterpret_cast<const float4 *>(q.wstream + P.table())[tid];
        const float4 vc = reinterpret_cast<const float4 *>(qq.cstream + C.table())[tid];
        reinterpret_cast<float4 *>(s_tab)[tid] = va;
        reinterpret_cast<float4 *>(s_tab + LN_TABLE_FLOATS)[tid] = vc;
        __syncthreads();
    }

    const float one = half ? 0.0f : 1.0f;                    // the bias records' B operand
    auto join = [&](float x) __attribute__((always_inline)) {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
        return __uint_as_float(r[0]) + __uint_as_float(r[1]);
    };
    // steps 2 .. 5 of "nig-mlp-ln-v1" on a whole layer in place: z -> d -> h; `tab`: the network's table, 0 or LN_TABLE_FLOATS
    auto layer_norm = [&](f32x16 (&h)[MLP_MT], int tab, int layer, float eps) __attribute__((always_inline)) {
        float ps = 0.0f;
#pragma unroll
        for (int mm = 0; mm < MLP_MT; ++mm)
#pragma unroll
            for (int t = 0; t < 16; ++t) ps = ps + h[mm][t];
        const float mean = join(ps) * 0x1p-8f;
        float qs = 0.0f;
#pragma unroll
        for (int mm = 0; mm < MLP_MT; ++mm)
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const float d = h[mm][t] - mean;
                h[mm][t] = d;
                qs = __builtin_fmaf(d, d, qs);
            }
        const float var = join(qs) * 0x1p-8f;
        const float rs = det_rsqrtf(var + eps);
        const float4 *g = reinterpret_cast<const float4 *>(&s_tab[tab + ln_table_at(layer, 0, (int)half, 0, 0)]);
        const float4 *b = reinterpret_cast<const float4 *>(&s_tab[tab + ln_table_at(layer, 1, (int)half, 0, 0)]);
#pragma unroll
        for (int mm = 0; mm < MLP_MT; ++mm)
#pragma unroll
            for (int t4 = 0; t4 < 4; ++t4) {
                const float4 gv = g[4 * mm + t4], bv = b[4 * mm + t4];
                h[mm][4 * t4 + 0] = fmaxf(__builtin_fmaf(h[mm][4 * t4 + 0], rs * gv.x, bv.x), 0.0f);
                h[mm][4 * t4 + 1] = fmaxf(__builtin_fmaf(h[mm][4 * t4 + 1], rs * gv.y, bv.y), 0.0f);
                h[mm][4 * t4 + 2] = fmaxf(__builtin_fmaf(h[mm][4 * t4 + 2], rs * gv.z, bv.z), 0.0f);
                h[mm][4 * t4 + 3] = fmaxf(__builtin_fmaf(h[mm][4 * t4 + 3], rs * gv.w, bv.w), 0.0f);
            }
    };
    // rollout_mlp_ln_kernel's chunk of 129 records (in s_w[c_buf]); MODE 0: an output tile of layer 2 into `acc`; 1: the four-row
    // head into `acc` (f32x4); 2: the sixteen-row head (f32x16)
    auto chunk129 = [&](auto mode_, const f32x16 *hin, auto &acc) __attribute__((always_inline)) {
        constexpr int MODE = decltype(mode_)::value;
        constexpr int N = 16 * MLP_MT + 1;
        const float *wb = &s_w[c_buf][lane];
        float ring[RING];
#pragma unroll
        for (int j = 0; j < RING; ++j) ring[j] = wb[j * 64];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const float aop = ring[i % RING];
            if (i + RING < N) ring[i % RING] = wb[(i + RING) * 64];
            __builtin_amdgcn_sched_barrier(0);
            const float bop = i < 16 * MLP_MT ? hin[i / 16][i % 16] : one;
            if constexpr (MODE == 0) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aop, bop, acc, 0, 0, 0);
            else if constexpr (MODE == 1) acc = __builtin_amdgcn_mfma_f32_4x4x1f32(aop, bop, acc, 0, 0, 0);
            else acc = __builtin_amdgcn_mfma_f32_16x16x1f32(aop, bop, acc, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    // Layer 1 of the actor (critic_ = 0) or the critic (1) into `h`: natural k order, two inputs per record; x(k): input k of the
    // network, a compile-time index
    auto layer1 = [&](auto critic_, auto x, f32x16 (&h)[MLP_MT]) __attribute__((always_inline)) {
        constexpr MlpLayer1 L1 = decltype(critic_)::value ? ln_plan(S + A).l1 : ln_plan(S).l1;
#pragma unroll
        for (int c1 = 0; c1 < L1.chunks; ++c1) {
            next_chunk();
            const float *wb = &s_w[c_buf][lane];
#pragma unroll
            for (int mm = 0; mm < L1.tiles; ++mm) {
                f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int ks = 0; ks < L1.records - 1; ++ks) {
                    const float b = half ? x(2 * ks + 1) : x(2 * ks);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wb[(mm * L1.records + ks) * 64], b, acc, 0, 0, 0);
                }
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wb[(mm * L1.records + L1.records - 1) * 64], one, acc, 0, 0, 0);   // + bias
                h[c1 * L1.tiles + mm] = acc;
            }
            done_chunk();
        }
    };

    for (int it = 0; it < q.n_steps; ++it) {
        f32x16 ha[MLP_MT], hb[MLP_MT];
        // ---------------- actor: "nig-mlp-ln-v1", rollout_mlp_ln_kernel's pass ----------------
        layer1(mlp_int<0>{}, [&](int k) __attribute__((always_inline)) { return s[k]; }, ha);
        layer_norm(ha, 0, 0, qq.a.eps);
#pragma unroll
        for (int m = 0; m < MLP_MT; ++m) {
            f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            next_chunk();
            chunk129(mlp_int<0>{}, ha, acc);
            done_chunk();
            hb[m] = acc;
        }
        layer_norm(hb, 0, 1, qq.a.eps);
        {
            std::conditional_t<mlp_head4<Env>, f32x4, f32x16> out = {};     // this lane half's partial sums of the head rows
            next_chunk();
            chunk129(mlp_int<mlp_head4<Env> ? 1 : 2>{}, hb, out);
            done_chunk();
            if constexpr (mlp_head4<Env>) {
#pragma unroll
                for (int r = 0; r < A; ++r) a[r] = det_tanhf(out[r] + __shfl_xor(out[r], 32));
            } else {
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

        // ---------------- critic on x = [s, a, 0]: the LayerNorm network (S + A, 1) in the actor's registers ----------------
        layer1(mlp_int<1>{}, [&](int k) __attribute__((always_inline)) { return k < S ? s[k] : (k < S + A ? a[k - S] : 0.0f); }, ha);
        layer_norm(ha, LN_TABLE_FLOATS, 0, qq.ceps);
#pragma unroll
        for (int m = 0; m < MLP_MT; ++m) {
            f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            next_chunk();
            chunk129(mlp_int<0>{}, ha, acc);
            done_chunk();
            hb[m] = acc;
        }
        layer_norm(hb, LN_TABLE_FLOATS, 1, qq.ceps);
        f32x4 z4 = {0, 0, 0, 0};
        next_chunk();
        chunk129(mlp_int<1>{}, hb, z4);
        done_chunk();
        const float prob = det_sigmoidf(z4[0] + __shfl_xor(z4[0], 32));
        const bool shield = !(prob < qq.threshold);
#pragma unroll
        for (int r = 0; r < A; ++r) a[r] = shield ? a[r] * 0.5f : a[r];

        // ---------------- IndustrialEnv.step (both lane halves, identical results): rollout_mlp_ln_kernel's ----------------
        const uint32_t orow = (uint32_t)it * q.out_stride;
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
