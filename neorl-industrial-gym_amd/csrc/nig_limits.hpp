// nig_limits.hpp -- box constraints added by the user, on the device ("nig-limits-v1", include/nig.h nig_set_limits; device
// code only): the table of bounds, IndustrialEnv.step for one lane under it (step_core_limited) and the one-step kernel
// step_limited_kernel (nig_step_limited / nig_step64_limited).  The closed-loop twins are rollout_policy_limited_kernel
// (nig_rollout_policy.hpp) and rollout_mlp_limited_kernel (nig_mlp.hpp): the parents' bodies with step_core_limited at their
// one step_core site.  step_core, post_finish and every parent kernel stay as they are.
#pragma once
#include "nig_step.hpp"

namespace nig {

// The handle's device copy of the installed constraints.  It is wave-uniform and never written by a kernel: the kernels read
// it through the constant address space, i.e. with scalar loads at compile-time offsets.
struct LimitTable {
    nig_limit c[NIG_MAX_LIMITS];
    int32_t n;                 // installed constraints, 1 .. NIG_MAX_LIMITS
    int32_t reserved;
};
typedef const __attribute__((address_space(4))) LimitTable *limit_table_ptr;

// what a _limited kernel takes beside its parent's arguments
struct LimitArgs {
    const LimitTable *table;
    uint32_t *xflags;          // [n_steps][>= B], row k at + k * out_stride of the launch (the step kernel: one row); may be NULL
};

// the second per-step word (include/nig.h): bit c: added constraint c violated; bits 4-6: how many; bits 8-10: how many critical
__device__ __forceinline__ uint32_t pack_xflags(uint32_t xb, uint32_t xcrit_bits)
{
    return xb | ((uint32_t)__popc(xb) << NIG_XFLAG_NVIOL_SHIFT) | ((uint32_t)__popc(xcrit_bits) << NIG_XFLAG_NCRIT_SHIFT);
}

// The main flag word of a limited step.  step_core_limited leaves the counts of ALL constraints in the result (what the episode
// bookkeeping takes), so pack_flags' count fields hold totals; the word's VIOL / NVIOL / NCRIT fields describe the built-ins
// (include/nig.h): the two count fields are put back from the built-ins' violation bits.  A body calls this in a block of its
// LIMITS form alone, behind its own pack_flags line, which stays as it is for every other form.
template <class Env>
__device__ __forceinline__ uint32_t limited_flag_counts(uint32_t fl, uint32_t vb, bool shutdown)
{
    // pack_flags shifts the critical count in unmasked: a count of 4 .. 7 (built-in + added) reaches the bit above the two-bit
    // field, which is the SHUTDOWN bit -- cleared with the fields here and set again from `shutdown` -- and nothing beyond it
    static_assert(NIG_FLAG_SHUTDOWN == 4u << NIG_FLAG_NCRIT_SHIFT && NIG_MAX_LIMITS + 3 <= 7 && NIG_FLAG_NCRIT_SHIFT == NIG_FLAG_NVIOL_SHIFT + 2,
                  "limited_flag_counts: the total critical count stays inside the NCRIT field and the SHUTDOWN bit");
    constexpr uint32_t FIELDS = (3u << NIG_FLAG_NVIOL_SHIFT) | (3u << NIG_FLAG_NCRIT_SHIFT) | NIG_FLAG_SHUTDOWN;
    return (fl & ~FIELDS) | ((uint32_t)__popc(vb) << NIG_FLAG_NVIOL_SHIFT) | ((uint32_t)__popc(vb & Env::CRIT_MASK) << NIG_FLAG_NCRIT_SHIFT) |
           (shutdown ? NIG_FLAG_SHUTDOWN : 0u);
}

// Bit c: added constraint c is violated on (pre-state s, clipped action a): some LISTED row x has !(lo <= x && x <= hi) -- a NaN
// in a listed row violates, an unlisted row is never looked at.  The lanes' s[] and a[] are register arrays: they are indexed
// by the unrolled loops' compile-time rows only (a run-time index would send the state to scratch); whether a row is listed is
// a scalar bit of the table.  A float64 action is compared against the float32 bound widened to double.
template <class Env, class AT>
__device__ __forceinline__ uint32_t limits_violated(limit_table_ptr T, const float (&s)[Env::S], const AT (&a)[Env::A])
{
    constexpr int S = Env::S, A = Env::A;
    static_assert(S + A <= NIG_LIMIT_ROWS, "a constraint's bounds have a row for every state and action row");
    const int n = T->n;
    uint32_t xb = 0u;
#pragma unroll
    for (int c = 0; c < NIG_MAX_LIMITS; ++c) {
        if (c < n) {                               // wave-uniform
            const uint64_t m = T->c[c].mask;
            bool bad = false;
#pragma unroll
            for (int r = 0; r < S; ++r) {
                const bool listed = ((m >> r) & 1ull) != 0ull;
                const float x = s[r];
                bad |= listed & !((T->c[c].lo[r] <= x) & (x <= T->c[c].hi[r]));
            }
#pragma unroll
            for (int j = 0; j < A; ++j) {
                const bool listed = ((m >> (S + j)) & 1ull) != 0ull;
                const AT x = a[j];
                bad |= listed & !(((AT)T->c[c].lo[S + j] <= x) & (x <= (AT)T->c[c].hi[S + j]));
            }
            xb |= bad ? (1u << c) : 0u;
        }
    }
    return xb;
}

// IndustrialEnv.step for one lane under the added constraints (base.py:157-213): step_core's clip, built-in check and dynamics,
// then the reward in the reference's order -- Env::reward, the violated built-ins' penalties, the violated added constraints'
// penalties in installation order, each add rounded to the reward's type, and ONE -1000 with `terminated` if any critical
// constraint of either kind was violated.  `out`: viol_bits are the built-ins' as step_core's; nviol and ncrit count the
// constraints of BOTH kinds (what the episode's violation count and the tally take; limited_flag_counts gives the flag word its
// built-in fields); terminated / shutdown are also set by an added critical violation.  The return value is the xflags word.
template <class Env, class NZ, class AT>
__device__ __forceinline__ uint32_t step_core_limited(limit_table_ptr T, const float (&s)[Env::S], AT (&a)[Env::A],
                                                      const NZ (&nz)[Env::KS > 0 ? Env::KS : 1], int step_pre, int max_steps,
                                                      float dt32, double dt, uint32_t cmask, float (&n)[Env::S],
                                                      StepResult<Env, reward_of<Env, AT>> &out)
{
    static_assert(!Env::CUSTOM_STEP, "the Advanced envs override step() wholesale: no added constraints (NIG_ERR_UNSUPPORTED)");
    using R = reward_of<Env, AT>;
    clip_action<Env, AT>(a);                                     // base.py:167
    const uint32_t vb = Env::violated(s, a) & cmask;             // base.py:170, the built-ins
    const uint32_t xb = limits_violated<Env, AT>(T, s, a);       // base.py:170, the added ones: same inputs
    Env::dynamics(s, a, nz, dt32, dt, n);                        // base.py:173
    R r = Env::reward(n, a);                                     // base.py:176
    bool term = Env::done(n);                                    // base.py:190
#pragma unroll
    for (int k = 0; k < 3; ++k)                                  // base.py:179-183, constraint order: the built-ins first
        r = (vb & (1u << k)) ? (R)(r + (R)Env::penalty(k)) : r;
    uint32_t xcrit = 0u;
#pragma unroll
    for (int c = 0; c < NIG_MAX_LIMITS; ++c) {
        if (c < T->n) {
            r = (xb & (1u << c)) ? (R)(r + (R)T->c[c].penalty) : r;
            xcrit |= (T->c[c].critical != 0) ? (xb & (1u << c)) : 0u;
        }
    }
    const int ncrit = __popc(vb & Env::CRIT_MASK) + __popc(xcrit);
    const bool shutdown = ncrit > 0;
    if (shutdown) { term = true; r = r - (R)1000; }              // base.py:195-198, once
    out.reward = r; out.viol_bits = vb; out.nviol = __popc(vb) + __popc(xb); out.ncrit = ncrit;
    out.terminated = term; out.truncated = (step_pre + 1) >= max_steps; out.shutdown = shutdown;
    return pack_xflags(xb, xcrit);
}

struct StepLimArgs {
    StepArgs p;
    LimitArgs l;
};

// One launch = IndustrialEnv.step for every lane under the added constraints: one lane per env, 256-thread blocks, injected
// (PARITY) or generated draws, the generator's table read from global memory.  A finishing lane of an auto-reset handle restarts
// in place, from the draws the parent's reset paths take (draw_init + init of the lane's key, or the injected reset row); the
// tally is kept through flush_tally, whose rows hold the bits of the parent's atomic form (nig_episode.hpp).  p.n_en counts the
// added constraints (host side).  ACT64: float64 action rows, the three NumPy envs.
template <class Env, bool PARITY, bool ACT64 = false>
__global__ void __launch_bounds__(BLOCK) step_limited_kernel(const StepLimArgs q)
{
    constexpr int S = Env::S, A = Env::A, KS = Env::KS, KR = Env::KR;
    constexpr int KSN = KS > 0 ? KS : 1;
    using act_t = std::conditional_t<ACT64, double, float>;
    using nz_t = std::conditional_t<PARITY, double, typename Env::fast_noise_t>;
    const StepArgs &p = q.p;
    const limit_table_ptr T = (limit_table_ptr)q.l.table;
    const unsigned tid = threadIdx.x;
    const uint32_t base = blockIdx.x * BLOCK;
    if (base + tid >= p.B) return;
    const uint32_t t_now = launch_counter(p.t_ptr, p.t_off);
    const uint32_t ctr = (p.ctr + base)[tid];
    if (ctr & NIG_CTR_DONE) {                      // base.py:159-160: a finished lane waits for its reset
        if (p.flags) (p.flags + base)[tid] = frozen_flag_word(ctr);
        if (q.l.xflags) (q.l.xflags + base)[tid] = 0u;
        if (p.reward) (p.reward + base)[tid] = 0.0f;
        if (p.reward64) (p.reward64 + base)[tid] = 0.0;
        return;
    }
    float s[S], n[S];
    act_t a[A];
    nz_t nz[KSN];
#pragma unroll
    for (int k = 0; k < S; ++k) s[k] = (p.state + base + k * p.ld_state)[tid];
#pragma unroll
    for (int k = 0; k < A; ++k) {
        if constexpr (ACT64) a[k] = (p.actions64 + base + k * p.ld_act)[tid];
        else a[k] = (p.actions + base + k * p.ld_act)[tid];
    }
    const RngKey key = make_key(p.env0 + (uint64_t)(base + tid), t_now, p.seed_lo, p.seed_hi, NIG_PROBIT);
    if constexpr (KS > 0) {
        if constexpr (PARITY) {
#pragma unroll
            for (int k = 0; k < KS; ++k) nz[k] = (p.step_noise + base + k * p.ld_noise)[tid];
        } else {
            Env::draw_step(key, nz);
        }
    } else {
        nz[0] = (nz_t)0;
    }
    const int step_pre = (int)(ctr & NIG_CTR_STEP_MASK);
    StepResult<Env, reward_of<Env, act_t>> res;
    const uint32_t xf = step_core_limited<Env>(T, s, a, nz, step_pre, p.max_steps, p.dt32, p.dt, p.cmask, n, res);
    const int step = step_pre + 1;
    const uint32_t viol_ep = episode_violations(ctr, res.nviol);
    const bool done = res.terminated || res.truncated;
    const bool autoreset = (p.hflags & NIG_F_AUTORESET) != 0;
    const uint32_t fl = limited_flag_counts<Env>(pack_flags<Env>(res, step), res.viol_bits, res.shutdown) | did_reset_flag(done && autoreset);
    uint32_t nctr = counter_word(step, viol_ep);
    if (p.tally) {
        double ret = add_reward<Env, ACT64>((p.ep_ret + base)[tid], res.reward);        // utils.py:99
        if (done) {
            flush_tally(p.tally + base + tid, p.ld, ret, step, viol_ep, res.ncrit, p.n_en);
            ret = 0.0;
        }
        (p.ep_ret + base)[tid] = ret;
    }
    if (done) {
        (p.life_viol + base)[tid] += (long long)viol_ep;         // base.py:183 total_violations (the lane's own word)
        if (p.final_obs) {
#pragma unroll
            for (int k = 0; k < S; ++k) (p.final_obs + base + k * p.ld_obs)[tid] = n[k];
        }
        if (autoreset) {                                         // IndustrialEnv.reset (base.py:133-155), in place
            double rn[KR > 0 ? KR : 1];
            if constexpr (PARITY) {
#pragma unroll
                for (int k = 0; k < KR; ++k) rn[k] = (p.reset_noise + base + k * p.ld_noise)[tid];
            } else {
                Env::draw_init(key, rn);
            }
            Env::init(rn, n);
            nctr = 0u;
        } else {
            nctr |= NIG_CTR_DONE;
        }
    }
#pragma unroll
    for (int k = 0; k < S; ++k) (p.state + base + k * p.ld_state)[tid] = n[k];
    (p.ctr + base)[tid] = nctr;
    if (p.reward) (p.reward + base)[tid] = (float)res.reward;
    if (p.reward64) (p.reward64 + base)[tid] = (double)res.reward;
    if (p.flags) (p.flags + base)[tid] = fl;
    if (q.l.xflags) (q.l.xflags + base)[tid] = xf;
}

}  // namespace nig
