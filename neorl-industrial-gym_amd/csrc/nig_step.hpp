// nig_step.hpp -- IndustrialEnv.step for one lane and the generator glue around it (device code only): what every kernel body
// that steps an env calls -- clip, post_core / post_finish, step_core, the flag word, generator keys, the sampled action, the
// env hooks of the paired forms and the wave-cooperative reset.
#pragma once
#include "nig_device.hpp"
#include "nig_episode.hpp"

namespace nig {

// IndustrialEnv.step for one lane, entirely in registers (base.py:157-213): action clip, constraint
// check on the pre-state and dynamics, then post_core = reward / penalties / termination on the
// finished transition.
// AT = float, or double when the caller hands float64 actions over (nig_step64): base.py:167 clips a float64 array
// against the float32 bounds without casting, and the envs' arithmetic follows NumPy's promotion from there.
template <class Env, class AT>
__device__ __forceinline__ void clip_action(AT (&a)[Env::A])
{
#pragma unroll
    for (int k = 0; k < Env::A; ++k) {            // base.py:167 np.clip(action, -1, 1) == min(max(x,lo),hi)
        AT x = a[k];
        if constexpr (std::is_same<AT, float>::value) {
            // NumPy's maximum / minimum hand a NaN on, and so do gfx950's v_maximum3_f32 / v_minimum3_f32 (IEEE 754-2019
            // maximum / minimum): two instructions where compare + select pairs are four.  (Neither limit is a zero,
            // so the sign of a zero result never comes from a limit; an action inside the limits is returned as it is.)
            x = __builtin_elementwise_maximum(x, -1.0f);
            x = __builtin_elementwise_minimum(x, 1.0f);
        } else {
            x = (x < (AT)-1) ? (AT)-1 : x;
            x = (x > (AT)1) ? (AT)1 : x;
        }
        a[k] = x;
    }
}

// the reward's type at the end of the reference's arithmetic: float64 as soon as the action is float64
template <class Env, class AT> using reward_of = std::conditional_t<std::is_same<AT, double>::value, double, typename Env::reward_t>;

template <class Env, class R>
__device__ __forceinline__ void post_finish(R r, bool term, uint32_t vb, int step_pre, int max_steps, StepResult<Env, R> &out);

template <class Env, class AT>
__device__ __forceinline__ void post_core(const float (&n)[Env::S], const AT (&a)[Env::A], uint32_t vb,
                                          int step_pre, int max_steps, StepResult<Env, reward_of<Env, AT>> &out)
{
    post_finish<Env, reward_of<Env, AT>>(Env::reward(n, a) /* base.py:176 */, Env::done(n) /* base.py:190 */, vb, step_pre, max_steps, out);
}

// the env-independent rest of IndustrialEnv.step once the reward and the env's own termination test are known
template <class Env, class R>
__device__ __forceinline__ void post_finish(R r, bool term, uint32_t vb, int step_pre, int max_steps, StepResult<Env, R> &out)
{
#pragma unroll
    for (int k = 0; k < 3; ++k)                   // base.py:179-183, constraint order
        r = (vb & (1u << k)) ? (R)(r + (R)Env::penalty(k)) : r;
    const int nviol = __popc(vb);
    const int ncrit = __popc(vb & Env::CRIT_MASK);
    const bool trunc = (step_pre + 1) >= max_steps;   // base.py:191
    if (ncrit > 0) { term = true; r = r - (R)1000; }  // base.py:195-198
    out.reward = r; out.viol_bits = vb; out.nviol = nviol; out.ncrit = ncrit;
    out.terminated = term; out.truncated = trunc; out.shutdown = ncrit > 0;   // info['critical_shutdown'], base.py:210
}

template <class Env, class NZ, class AT>
__device__ __forceinline__ void step_core(const float (&s)[Env::S], AT (&a)[Env::A],
                                          const NZ (&nz)[Env::KS > 0 ? Env::KS : 1], int step_pre,
                                          int max_steps, float dt32, double dt, uint32_t cmask,
                                          float (&n)[Env::S], StepResult<Env, reward_of<Env, AT>> &out)
{
    if constexpr (Env::CUSTOM_STEP) {             // the Advanced envs override step() wholesale
        Env::custom_step(s, a, step_pre, max_steps, dt32, n, out);
        out.viol_bits &= cmask;
        out.nviol = __popc(out.viol_bits);
        return;
    } else {
        clip_action<Env, AT>(a);
        const uint32_t vb = Env::violated(s, a) & cmask;   // base.py:170 (and again :180, same inputs); cmask: base.py:224-228
        Env::dynamics(s, a, nz, dt32, dt, n);         // base.py:173
        post_core<Env, AT>(n, a, vb, step_pre, max_steps, out);
    }
}

// The per-lane flag word of one step (include/nig.h NIG_FLAG_*).
template <class Env, class R>
__device__ __forceinline__ constexpr uint32_t pack_flags(const StepResult<Env, R> &res, int step)
{
    uint32_t f = (res.terminated ? NIG_FLAG_TERMINATED : 0u) | (res.truncated ? NIG_FLAG_TRUNCATED : 0u) |
                 ((res.viol_bits & 7u) << NIG_FLAG_VIOL_SHIFT) | (((uint32_t)res.nviol & 3u) << NIG_FLAG_NVIOL_SHIFT) |
                 ((uint32_t)res.ncrit << NIG_FLAG_NCRIT_SHIFT) | (res.shutdown ? NIG_FLAG_SHUTDOWN : 0u) |
                 ((uint32_t)step << NIG_FLAG_STEP_SHIFT);
    if constexpr (Env::CUSTOM_STEP)                // only the Advanced envs carry a 4th condition / a count of 4
        f |= ((res.viol_bits & 8u) ? NIG_FLAG_VIOL3 : 0u) | (((uint32_t)res.nviol & 4u) ? NIG_FLAG_NVIOL_HI : 0u);
    return f;
}

// ---- a step's outcome decided once, by the wave that needs it first (the three-wave form, nig_split_body.inc) ----------------
// The integrator learns `terminated` and `truncated` from its own post_core call (it needs them for the reset) and hands them to
// the recorder with the violation bits of the pre-state, in the one word it writes into its ring slot anyway:
//   violation bits (0-2) | terminated << 8 | truncated << 9
// -- bits 8-9 are NIG_FLAG_TERMINATED | NIG_FLAG_TRUNCATED eight places up.  The recorder no longer runs Env::done, the critical
// test and the step compare on the same values again (post_record below).
constexpr int OUTCOME_SHIFT = 8;
__device__ __forceinline__ uint32_t outcome_word(uint32_t vb, bool terminated, bool truncated)
{
    return vb | (terminated ? NIG_FLAG_TERMINATED << OUTCOME_SHIFT : 0u) | (truncated ? NIG_FLAG_TRUNCATED << OUTCOME_SHIFT : 0u);
}

// Bits 2-9 of the flag word -- violation bits, violation count, critical count, shutdown -- are a function of the three violation
// bits alone for an env that goes through post_finish: eight bytes in one 64-bit constant, byte vb = those bits for vb, from the
// fields' own definitions (include/nig.h).  Two bit counts, three shifts, three ands, a select and three ors per step become a
// shift of the constant.
template <class Env>
__device__ constexpr uint64_t violation_flag_table()
{
    uint64_t t = 0;
    for (uint32_t vb = 0; vb < 8u; ++vb) {
        const uint32_t nviol = (uint32_t)__builtin_popcount(vb), ncrit = (uint32_t)__builtin_popcount(vb & Env::CRIT_MASK);
        const uint32_t f = (vb << NIG_FLAG_VIOL_SHIFT) | (nviol << NIG_FLAG_NVIOL_SHIFT) | (ncrit << NIG_FLAG_NCRIT_SHIFT) |
                           (ncrit > 0u ? NIG_FLAG_SHUTDOWN : 0u);
        t |= (uint64_t)(f >> NIG_FLAG_VIOL_SHIFT) << (8u * vb);
    }
    return t;
}
// the table against pack_flags on what post_finish makes of vb, all eight values: every bit of the word but the two outcome bits
template <class Env>
__device__ constexpr bool violation_flag_table_is_pack_flags(uint64_t table)
{
    for (uint32_t vb = 0; vb < 8u; ++vb) {
        StepResult<Env> r{};
        r.viol_bits = vb; r.nviol = __builtin_popcount(vb); r.ncrit = __builtin_popcount(vb & Env::CRIT_MASK);
        r.terminated = false; r.truncated = false; r.shutdown = r.ncrit > 0;
        if (pack_flags<Env>(r, 0) != (((uint32_t)(table >> (8u * vb)) & 0xFFu) << NIG_FLAG_VIOL_SHIFT)) return false;
    }
    return true;
}

// What the recorder makes of a step whose outcome is decided: the reward (base.py:176-183,195-198: post_finish's penalty and
// shutdown adds, in its order, on Env::reward), the flag word, the two counts the episode bookkeeping takes.
template <class Env>
struct StepRecord {
    typename Env::reward_t reward;
    uint32_t flags;            // the whole word of pack_flags | did_reset_flag
    int nviol, ncrit;
    bool done;
};
template <class Env>
__device__ __forceinline__ StepRecord<Env> post_record(const float (&n)[Env::S], const float (&a)[Env::A], uint32_t word, int step)
{
    using R = typename Env::reward_t;
    constexpr uint64_t TABLE = violation_flag_table<Env>();
    static_assert(!Env::CUSTOM_STEP && NIG_FLAG_SHUTDOWN >> NIG_FLAG_VIOL_SHIFT < 256u && violation_flag_table_is_pack_flags<Env>(TABLE),
                  "the table is pack_flags' bits 2-9 for the eight values of the violation bits");
    static_assert(NIG_FLAG_TERMINATED == 1u && NIG_FLAG_TRUNCATED == 2u, "outcome_word: the two bits as the flag word has them");
    StepRecord<Env> out;
    R r = Env::reward(n, a);                       // base.py:176
#pragma unroll
    for (int k = 0; k < 3; ++k)                   // base.py:179-183, constraint order
        r = (word & (1u << k)) ? (R)(r + (R)Env::penalty(k)) : r;
    if ((word & Env::CRIT_MASK) != 0u) r = r - (R)1000;     // base.py:195-198
    out.reward = r;
    // (a 64-bit shift takes the low six bits of its count: the outcome bits above them fall away)
    const uint32_t fields = (uint32_t)(TABLE >> ((word << 3) & 63u)) & 0xFFu;
    const uint32_t outcome = (word >> OUTCOME_SHIFT) & (NIG_FLAG_TERMINATED | NIG_FLAG_TRUNCATED);
    out.done = outcome != 0u;
    out.flags = outcome | (fields << NIG_FLAG_VIOL_SHIFT) | did_reset_flag(out.done) | ((uint32_t)step << NIG_FLAG_STEP_SHIFT);
    out.nviol = (int)((fields >> (NIG_FLAG_NVIOL_SHIFT - NIG_FLAG_VIOL_SHIFT)) & 3u);
    out.ncrit = (int)((fields >> (NIG_FLAG_NCRIT_SHIFT - NIG_FLAG_VIOL_SHIFT)) & 3u);
    return out;
}

// Per-lane key of the counter-based generator: (global env index, launch counter t).
__device__ __forceinline__ RngKey make_key(uint64_t gi, uint32_t t, uint32_t seed_lo, uint32_t seed_hi,
                                           const float4 *tab = nullptr)
{
    RngKey k;
    k.env_lo = (uint32_t)gi; k.env_hi = (uint32_t)(gi >> 32);
    k.t = t; k.seed_lo = seed_lo; k.seed_hi = seed_hi; k.tab = tab;
    return k;
}

// One uniform action of the env's Box from one generator word (nig_rollout_sampled: the fused rollout draws what
// nig_fill_actions writes).  fill_actions_kernel's definition is (float)(low + (high - low) * u) in float64 with u = m * 2^-24,
// m the word's top 24 bits; the forms below give the same float32 for every m (tests/test_rollout_sampled_host.py runs all 2^24
// for every Box of nig_envs.hpp) without float64, whose every operation is in the slow issue class:
//   [-1, 1):  -1 + m * 2^-23 is a multiple of 2^-23 below 1 in magnitude, i.e. a float32: one fused multiply-add of the
//             (exact) conversion of m rounds nothing;
//   [0, high): high * (m * 2^-24) in float32 -- m * 2^-24 is exact, so float32 and float64 both round the one product high * u
//             (the float64 product of two 24-bit significands is exact, its narrowing is the float32 product's rounding);
//   any other Box (AdvancedChemicalReactor's 273.15 .. 473.15, AdvancedPowerGrid's dispatch and tap ranges): the float64 form
//             itself -- the float32 sum rounds twice and differs on up to 14 % of the words.
__device__ __forceinline__ float action_from_word(uint32_t word, float low, float high)
{
    const float mf = (float)(word >> 8);
    if (low == -1.0f && high == 1.0f) return __builtin_fmaf(mf, 1.0f / 8388608.0f, -1.0f);
    if (low == 0.0f) return high * (mf * (1.0f / 16777216.0f));
    return (float)((double)low + ((double)high - (double)low) * u01(word));
}

// The action nig_fill_actions(t) writes for the key's lane: blocks STREAM_ACTION + j of the key's counter, words in order.
template <class Env>
__device__ __forceinline__ void sample_action(const RngKey &k, float (&a)[Env::A])
{
#pragma unroll
    for (int j = 0; 4 * j < Env::A; ++j) {
        const u32x4 x = k.block(STREAM_ACTION + (uint32_t)j);
        const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (4 * j + c < Env::A) a[4 * j + c] = action_from_word(w[c], Env::act_low(4 * j + c), Env::act_high(4 * j + c));
    }
}

// Env hooks that only some envs have, callable from generic lambdas (where a discarded
// `if constexpr` branch is still name-checked because Env is not the lambda's own parameter).
template <class Env>
__device__ __forceinline__ u32x4 pair_block(const RngKey &k)
{
    if constexpr (Env::SHARED_STEP_BLOCK) return Env::step_block(k);
    else return u32x4{0u, 0u, 0u, 0u};
}
template <class Env, class NZ>
__device__ __forceinline__ void pair_noise(uint32_t w0, uint32_t w1, const float4 *tab, NZ (&n)[Env::KS > 0 ? Env::KS : 1])
{
    if constexpr (Env::SHARED_STEP_BLOCK) Env::step_noise(w0, w1, tab, n);
}
template <class Env>
__device__ __forceinline__ void pair_fetch(uint32_t w0, uint32_t w1, const float4 *tab, ProbitFetch (&f)[Env::KS > 0 ? Env::KS : 1])
{
    if constexpr (Env::SHARED_STEP_BLOCK) Env::step_noise_fetch(w0, w1, tab, f);
}
template <class Env, class NZ>
__device__ __forceinline__ void pair_eval(const ProbitFetch (&f)[Env::KS > 0 ? Env::KS : 1], NZ (&n)[Env::KS > 0 ? Env::KS : 1])
{
    if constexpr (Env::SHARED_STEP_BLOCK) Env::step_noise_eval(f, n);
}
template <class Env, class NZ>
__device__ __forceinline__ void draw_one(const RngKey &k, NZ (&n)[Env::KS > 0 ? Env::KS : 1])
{
    if constexpr (Env::KS > 0) Env::draw_step(k, n);
}

// Wave-cooperative reset (envs with COOP_RESET): the lanes of `m` (ballot of the finishing lanes of this wave)
// get their initial states from work items (finishing lane, generator block) spread over all 64 lanes; an item
// writes the state rows its block feeds into column `owner` of the wave-private LDS image img[RESET_ROWS][64], the owners
// read their column back.  No block barrier.  DS operations of one wave execute in order, so the reads see the
// writes issued before them without a wait in between; the fences only pin the compiler's ordering.
// `lane_gi0` = global env index of the wave's lane 0, `t` = launch counter of the step that finished.
// QUICK (compile-time; the three-wave forms of an env with QUICK_RESET, whose integrator wave has nothing to overlap a
// restart with): (1) a step with exactly ONE finishing lane -- nearly every restart of a wave whose lanes finish once in a
// few hundred steps -- skips the work list.  `m` is wave-uniform, so its population count, the owner ctz(m) and the branch
// live on the scalar unit; lanes 0 .. ITEMS-1 run the owner's items directly: no list write, no list read, no wait between
// the ballot and the generator.  Two or more finishers take the list.  (2) The items are Env::reset_item_quick: the same
// values by the same operations, scheduled for latency.
template <class Env, class = void>
struct quick_reset : std::false_type {};
template <class Env>
struct quick_reset<Env, std::enable_if_t<Env::QUICK_RESET>> : std::true_type {};

template <class Env, bool QUICK = false>
__device__ __forceinline__ void coop_reset(unsigned long long m, bool mine, unsigned lane, float *img, unsigned char *lst,
                                           uint64_t lane_gi0, uint32_t t, uint32_t seed_lo, uint32_t seed_hi,
                                           const float4 *tab, float (&n)[Env::S])
{
    constexpr int ITEMS = Env::RESET_ITEMS;                   // work items per finishing lane (a power of two, or 6)
    static_assert((ITEMS & (ITEMS - 1)) == 0 || ITEMS == 6, "item index -> (lane, item): shift, or the divide-by-6 below");
    if constexpr (QUICK) {
        static_assert(ITEMS <= 64, "one pass of the wave covers a lone finisher's items");
        if (__popc((uint32_t)m) + __popc((uint32_t)(m >> 32)) == 1) {      // (two 32-bit counts: hipcc compares a 64-bit count on the vector unit)
            const unsigned owner = (unsigned)__builtin_ctzll(m);
            if (lane < (unsigned)ITEMS) {
                unsigned item = lane;                      // laundered like the list path's item index below, for the same reason
                asm volatile("" : "+v"(item));
                Env::reset_item_quick(make_key(lane_gi0 + owner, t, seed_lo, seed_hi, tab), item, img, owner);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            if (mine) Env::reset_readback(img, lane, n);
            return;
        }
    }
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));   // finishing lanes below this one (v_mbcnt: no per-lane mask register)
    if (mine) lst[rank] = (unsigned char)lane;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    const int total = __popcll(m) * ITEMS;
    for (int i = (int)lane; i < total; i += 64) {
        // The item index is laundered: in the first pass it equals the lane index, a loop invariant of the ROLLOUT loop
        // around this call, and hipcc then hoists every per-block constant select of reset_item (standard deviations,
        // offsets, row numbers: ~30 registers for PowerGrid) out of that loop and keeps them alive across the whole step.
        int ii = i;
        asm volatile("" : "+v"(ii));
        unsigned li, item;                     // ii = li * ITEMS + item (ii < 64 * ITEMS)
        if constexpr (ITEMS == 6) { li = ((unsigned)ii * 171u) >> 10; item = (unsigned)ii - 6u * li; }     // exact for ii < 515
        else { li = (unsigned)ii / (unsigned)ITEMS; item = (unsigned)ii % (unsigned)ITEMS; }
        const unsigned owner = lst[li];
        if constexpr (QUICK) Env::reset_item_quick(make_key(lane_gi0 + owner, t, seed_lo, seed_hi, tab), item, img, owner);
        else Env::reset_item(make_key(lane_gi0 + owner, t, seed_lo, seed_hi, tab), item, img, owner);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (mine) Env::reset_readback(img, lane, n);
}

}  // namespace nig
