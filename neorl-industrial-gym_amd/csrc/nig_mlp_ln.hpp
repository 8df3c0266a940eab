// nig_mlp_ln.hpp -- the fused MLP actor on MFMA with LayerNorm (device code only): MlpLnArgs and rollout_mlp_ln_kernel<Env>, the
// kernel nig_rollout_mlp launches when the handle's actor slot holds a LayerNorm actor (nig_set_mlp_policy_ln).  A family of its own:
// rollout_mlp_body, rollout_mlp_shape_kernel and their kernels are not touched by it.
//
// THE LAW "nig-mlp-ln-v1" (stated here once; restated in plain C by tests/mlp_ln_ref.c).  The actor is S -> 256 -> 256 -> A, the
// reference's MLP with use_layer_norm=True (agents/networks.py: Dense -> LayerNorm -> ReLU per hidden layer, tanh head), all float32.
// rho_h(t) = (t & 3) + 8 (t >> 2) + 4 h is the row of a 32-row tile that register t of lane half h holds (mfma_row).  For hidden layer
// i in {1, 2} with weights W_i, bias b_i, scale gamma_i, shift beta_i:
//   1. z[r], r = 0 .. 255, is the Dense pre-activation in the 256 x 256 law's fma chain, from c = 0:
//        layer 1:  c = fma(W1[k + 1][r], x[k + 1], fma(W1[k][r], x[k], c)) for k = 0, 2, .. , S - 2 (natural k order; S is even),
//        layer 2:  for kt = 0 .. 7, t = 0 .. 15:  c = fma(W2[k1][r], h[k1], fma(W2[k0][r], h[k0], c)), k0 = 32 kt + rho_0(t), k1 = k0 + 4,
//        then the bias as the last k-step: z[r] = fma(0, 0, fma(b_i[r], 1, c))   (v_mfma_f32_32x32x2_f32 = fma(a1, b1, fma(a0, b0, c))).
//   2. The mean.  Lane half h owns the 128 rows 32 mm + rho_h(t) of its env; p_h is their float32 sum as ONE chain from 0, tile
//      ascending, register ascending: p = p + z[32 mm + rho_h(t)] for mm = 0 .. 7, t = 0 .. 15.  mean = (p_0 + p_1) * 2^-8.
//   3. The variance, two passes: d[r] = z[r] - mean; q_h the chain q = fma(d, d, q) from 0 in the same order; var = (q_0 + q_1) * 2^-8.
//   4. rs = det_rsqrtf(var + eps) (nig_detmath.hpp), eps a float32 argument.
//   5. y[r] = fma(d[r], rs * gamma_i[r], beta_i[r]);  h[r] = max(y[r], 0).
// The head is the 256 x 256 law's on h of layer 2: two chains, one per lane half, over m = 0 .. 7, t = 0 .. 15 -- c_h = fma(W3[32 m +
// rho_h(t)][j], h[32 m + rho_h(t)], c_h) -- then the bias (c_0 = fma(b3[j], 1, c_0), c_1 = fma(b3[j], 0, c_1)), pre[j] = c_0 + c_1,
// action[j] = det_tanhf(pre[j]).  The join of the two lane halves in 2 and 3 is one add of the same two numbers on both halves
// (addition commutes), so both halves hold the same bits and step their env identically.  The two-pass variance is the law on
// purpose: the one-pass form E[z^2] - E[z]^2 loses the layer when the mean is large beside the spread.
// The law says nothing about non-finite inputs.
#pragma once
#include "nig_mlp.hpp"
#include "nig_mlp_ln_stream.hpp"     // the image's chunk plan and the gamma / beta table (shared with the host's builder)

namespace nig {

struct MlpLnArgs {
    MlpArgs m;                  // m.wstream: the image built by nig_set_mlp_policy_ln (put_ln_network)
    float eps;
};

// rollout_mlp_shape_kernel's scheme (nig_mlp_shape.hpp: rollout_mlp_body's transposed layout, the weights through LDS buffers filled by
// LDS-DMA along one cyclic chunk sequence, a counter naming the chunk filled next) on the plan of nig_mlp_ln_stream.hpp:
//   * BOTH hidden layers are held whole in registers (128 + 128: the unified 512-entry file, one wave per SIMD, one block per CU) and
//     normalised in place -- z, then d, then h in the same register;
//   * the two lane halves' partial sums meet in v_permlane32_swap_b32 (no LDS round trip): swapping a register with itself leaves half
//     0's value in every lane of one result and half 1's in every lane of the other;
//   * gamma and beta (4 KiB, in mfma_row order) are staged into LDS once per launch; a lane reads its tile's sixteen values as four
//     16-byte vectors, and the 32 lanes of a half read the same address: a broadcast;
//   * the head cannot ride with layer 2's tiles (it reads the normalised layer): its 128 records and bias are a chunk of their own.
template <class Env>
__global__ void __launch_bounds__(BLOCK, 1) rollout_mlp_ln_kernel(const MlpLnArgs qq)
{
    constexpr int S = Env::S, A = Env::A, KS = Env::KS, KR = Env::KR;
    constexpr int KSN = KS > 0 ? KS : 1;
    static_assert(has_mlp_actor<Env>, "MFMA actor needs an even state dim and at most 16 actions");
    constexpr LnPlan P = ln_plan(S);
    static_assert(P.l1.fits(), "a layer-1 chunk must fit the chunk slot");
    constexpr int NBUF = 2, RING = 8;
    __shared__ __attribute__((aligned(16))) float s_w[NBUF][MLP_CHREC * 64];
    __shared__ __attribute__((aligned(16))) float s_tab[LN_TABLE_FLOATS];
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

    // ---------------- the fill chain (rollout_mlp_shape_kernel's): chunk `f_chunk` of the cyclic sequence into buffer `f_buf` ----------------
    int f_chunk = 0, f_buf = 0, f_left = q.n_steps * P.chunks;
    auto fill_next = [&]() __attribute__((always_inline)) {
        if (f_left <= 0) return;
        const int pieces = f_chunk < P.l1.chunks ? P.l1.pieces : f_chunk < P.head_chunk ? P.l2_pieces : P.head_pieces;
        const float *src = q.wstream + (size_t)f_chunk * (MLP_CHREC * 64) + lane * 4u;
        for (int pc = (int)wave; pc < pieces; pc += BLOCK / 64)
            __builtin_amdgcn_global_load_lds((nig_glb_void *)(src + pc * 256), (nig_lds_void *)(&s_w[f_buf][pc * 256]), 16, 0, 0);
        --f_left;
        f_chunk = f_chunk + 1 == P.chunks ? 0 : f_chunk + 1;
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
    {                                                        // gamma / beta of both layers: 256 threads x 16 bytes, once per launch
        static_assert(LN_TABLE_FLOATS == BLOCK * 4);
        const float4 v = reinterpret_cast<const float4 *>(q.wstream + P.table())[tid];
        reinterpret_cast<float4 *>(s_tab)[tid] = v;
        __syncthreads();
    }

    const float one = half ? 0.0f : 1.0f;                    // the bias records' B operand
    // the other lane half's partial sum joins this one's: the same add of the same two numbers on both halves
    auto join = [&](float x) __attribute__((always_inline)) {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
        return __uint_as_float(r[0]) + __uint_as_float(r[1]);
    };
    // steps 2 .. 5 of the law on a whole layer in place: z -> d -> h
    auto layer_norm = [&](f32x16 (&h)[MLP_MT], int layer) __attribute__((always_inline)) {
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
        const float rs = det_rsqrtf(var + qq.eps);
        const float4 *g = reinterpret_cast<const float4 *>(&s_tab[ln_table_at(layer, 0, (int)half, 0, 0)]);
        const float4 *b = reinterpret_cast<const float4 *>(&s_tab[ln_table_at(layer, 1, (int)half, 0, 0)]);
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
    // One chunk of 129 records (in s_w[c_buf]): HEAD = 0: output tile of layer 2 -- the 128 weight records on h1 and the bias record
    // into `acc`; HEAD = 1: the head -- 128 records on the lane's own h2 values and the bias record into `out`.  LDS reads run RING
    // records ahead of their MFMA, the source order pinned (rollout_mlp_body's layer2_chunk).
    auto chunk129 = [&](auto head_, const f32x16 *hin, auto &acc) __attribute__((always_inline)) {
        constexpr bool HEAD = decltype(head_)::value != 0;
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
            if constexpr (!HEAD) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aop, bop, acc, 0, 0, 0);
            else if constexpr (mlp_head4<Env>) acc = __builtin_amdgcn_mfma_f32_4x4x1f32(aop, bop, acc, 0, 0, 0);
            else acc = __builtin_amdgcn_mfma_f32_16x16x1f32(aop, bop, acc, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    for (int it = 0; it < q.n_steps; ++it) {
        // ---------------- actor: two normalised hidden layers and the head of f32 MFMA, whole wave (EXEC all ones) ----------------
        f32x16 ha[MLP_MT], hb[MLP_MT];
#pragma unroll
        for (int c1 = 0; c1 < P.l1.chunks; ++c1) {           // layer 1: natural k order, two inputs per record
            next_chunk();
            const float *wb = &s_w[c_buf][lane];
#pragma unroll
            for (int mm = 0; mm < P.l1.tiles; ++mm) {
                f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int ks = 0; ks < P.l1.records - 1; ++ks) {
                    const float b = half ? s[2 * ks + 1] : s[2 * ks];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wb[(mm * P.l1.records + ks) * 64], b, acc, 0, 0, 0);
                }
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wb[(mm * P.l1.records + P.l1.records - 1) * 64], one, acc, 0, 0, 0);   // + bias
                ha[c1 * P.l1.tiles + mm] = acc;
            }
            done_chunk();
        }
        layer_norm(ha, 0);
#pragma unroll
        for (int m = 0; m < MLP_MT; ++m) {                   // layer 2: held whole beside h1 (unrolled: a register array takes no run-time index)
            f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            next_chunk();
            chunk129(mlp_int<0>{}, ha, acc);
            done_chunk();
            hb[m] = acc;
        }
        layer_norm(hb, 1);
        std::conditional_t<mlp_head4<Env>, f32x4, f32x16> out = {};     // this lane half's partial sums of the head rows
        next_chunk();
        chunk129(mlp_int<1>{}, hb, out);
        done_chunk();
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
