// nig_episode.hpp -- the episode bookkeeping of the fused kernels, stated once (device code only; included by nig_kernels.hpp
// once StepArgs is defined).
//
// The rule is the reference's IndustrialEnv.step / reset / utils.py accounting: the per-lane counter word (step count, violations
// of the running episode, "finished" bit), the running return, the lifetime violation count and the 13-row episode tally.  Every
// kernel body that steps an env -- step_kernel, rollout_body, rollout_policy_kernel, rollout_mlp_body, the recorders of the
// three-wave forms, the PowerGrid bodies of nig_pg_lds.hpp -- calls what is here instead of restating it, wherever the call
// leaves the kernel's instructions as they were (profiles/episode/isa_diff.txt lists the sites that still spell a piece out,
// and what moved when they did not).
//
// What keeps a call free: every helper is __forceinline__, takes the fields it reads BY VALUE (pointers, pitches, `base` and
// `tid` apart) -- never the kernel's argument struct: a __global__ function's argument block lives in the constant address
// space, and a reference to it changes code generation -- and RETURNS scalars instead of writing them
// through references: hipcc runs its first simplification passes before it inlines, and a scalar whose address has been
// taken, or a branch hidden in a callee, leaves them a function of another shape.  Address expressions keep the form
// (ptr + base)[tid]: the uniform part stays in scalar registers.  The helpers wrap straight-line runs only; fences,
// sched_barriers, the asm pins and the prologue s_waitcnt stay where the bodies have them.
#pragma once
#include "nig_device.hpp"

namespace nig {

// ---- generator table --------------------------------------------------------------------------------------------------------
// Stage the 12 KiB probit table (normal transform of the generator) in LDS with `nthreads` threads.  The block barrier that
// publishes it is the caller's line -- several callers publish other LDS data with the same barrier -- and every thread of the
// block must pass through both before any early exit.
__device__ __forceinline__ void stage_probit(float4 *dst, unsigned tid, int nthreads)
{
    for (int i_ = (int)tid; i_ < 768; i_ += nthreads) dst[i_] = NIG_PROBIT[i_];
}

// ---- launch counter ---------------------------------------------------------------------------------------------------------
// t = (t_ptr ? *t_ptr : 0) + t_off (graph replay keeps t on the device); step k of a launch uses the generator key t + k + 1
__device__ __forceinline__ uint32_t launch_counter(const uint32_t *t_ptr, uint32_t t_off) { return (t_ptr ? *t_ptr : 0u) + t_off; }

// ---- the words of one step (include/nig.h NIG_CTR_*, NIG_FLAG_*) --------------------------------------------------------------
// violations of the running episode after a step with `nviol` of them (base.py:182)
__device__ __forceinline__ uint32_t episode_violations(uint32_t ctr, int nviol) { return (ctr >> NIG_CTR_VIOL_SHIFT) + (uint32_t)nviol; }
// the counter word of a lane that has taken `step` steps of its episode
__device__ __forceinline__ uint32_t counter_word(int step, uint32_t viol_ep) { return (uint32_t)step | (viol_ep << NIG_CTR_VIOL_SHIFT); }
// the flag word of a frozen lane (finished and waiting for reset, base.py:159-160): its step count stands
__device__ __forceinline__ uint32_t frozen_flag_word(uint32_t ctr) { return NIG_FLAG_INACTIVE | ((ctr & NIG_CTR_STEP_MASK) << NIG_FLAG_STEP_SHIFT); }
// the flag bit of a lane that finished and restarted in this step
__device__ __forceinline__ uint32_t did_reset_flag(bool restarted) { return restarted ? NIG_FLAG_DID_RESET : 0u; }

// utils.py:99 episode_return += reward, in the precision the reference accumulates it in: float32 for an env with RET_F32
// (ChemicalReactor, float32 rewards) unless the action -- and with it the reward -- is float64 (ACT64).  A float `ret` is that
// float32 sum itself (widened only when an episode ends); a double `ret` of such an env holds exactly that float.
template <class Env, bool ACT64 = false, class RT, class R>
__device__ __forceinline__ RT add_reward(RT ret, R reward)
{
    if constexpr (std::is_same<RT, float>::value) return ret + (float)reward;
    else if constexpr (Env::RET_F32 && !ACT64) return (double)((float)ret + reward);
    else return ret + (double)reward;
}

// ---- episode tally ------------------------------------------------------------------------------------------------------------
// Episode bookkeeping of one finished episode (utils.py:120-125), lane-private column of the tally.
// All 11 rows are loaded before any is stored: one memory round trip instead of eleven dependent ones.
__device__ __forceinline__ void flush_tally(double *T, uint32_t ld, double ret, int step, uint32_t viol_ep, int ncrit, int n_en)
{
    double v[NIG_T_ROWS];
#pragma unroll
    for (int r = 0; r < NIG_T_ROWS; ++r) v[r] = T[(size_t)r * ld];
    const double len = (double)step;
    v[NIG_T_EPISODES] += 1.0;
    v[NIG_T_RET_SUM] += ret;
    v[NIG_T_RET_SQ] += ret * ret;
    v[NIG_T_RET_MIN] = fmin(v[NIG_T_RET_MIN], ret);
    v[NIG_T_RET_MAX] = fmax(v[NIG_T_RET_MAX], ret);
    v[NIG_T_LEN_SUM] += len;
    v[NIG_T_LEN_SQ] += len * len;
    v[NIG_T_VIOL] += (double)viol_ep;
    v[NIG_T_CRIT] += (double)ncrit;            // a critical step always ends the episode
    v[NIG_T_SHUTDOWN] += (ncrit > 0) ? 1.0 : 0.0;
    v[NIG_T_SUCCESS] += (ret > 0.0) ? 1.0 : 0.0;
    v[NIG_T_SATISFIED] += (double)(n_en * step - (int)viol_ep);   // sum over the episode's steps of constraints_satisfied
    v[NIG_T_CONSTRAINTS] += (double)(n_en * step);
#pragma unroll
    for (int r = 0; r < NIG_T_ROWS; ++r) T[(size_t)r * ld] = v[r];
}

// The same bookkeeping as no-return float64 atomics into the lane's own column (global_atomic_add / min / max_f64,
// executed at the memory side): nothing is loaded, nothing is waited for.  The step kernel used flush_tally, i.e. 13
// loads, a wait and 13 stores behind the step of every finishing lane -- a third dependent memory round trip on the
// critical path of a launch that is latency-bound at the headline batch (profiles/r03/step_api_probe.py: the tally cost
// 0.8 us of a 5.1 us launch).  Each row is one IEEE operation on the same operands as in flush_tally, and a lane's column
// is touched by that lane only (a kernel boundary orders consecutive steps), so the rows hold the same bits.
__device__ __forceinline__ void flush_tally_atomic(double *T, uint32_t ld, double ret, int step, uint32_t viol_ep, int ncrit, int n_en)
{
    typedef __attribute__((address_space(1))) double gdouble;
    auto add = [&](int r, double x) { (void)__builtin_amdgcn_global_atomic_fadd_f64((gdouble *)(T + (size_t)r * ld), x); };
    const double len = (double)step;
    add(NIG_T_EPISODES, 1.0);
    add(NIG_T_RET_SUM, ret);
    add(NIG_T_RET_SQ, ret * ret);
    (void)__builtin_amdgcn_global_atomic_fmin_f64((gdouble *)(T + (size_t)NIG_T_RET_MIN * ld), ret);
    (void)__builtin_amdgcn_global_atomic_fmax_f64((gdouble *)(T + (size_t)NIG_T_RET_MAX * ld), ret);
    add(NIG_T_LEN_SUM, len);
    add(NIG_T_LEN_SQ, len * len);
    add(NIG_T_VIOL, (double)viol_ep);
    add(NIG_T_CRIT, (double)ncrit);
    add(NIG_T_SHUTDOWN, (ncrit > 0) ? 1.0 : 0.0);
    add(NIG_T_SUCCESS, (ret > 0.0) ? 1.0 : 0.0);
    add(NIG_T_SATISFIED, (double)(n_en * step - (int)viol_ep));
    add(NIG_T_CONSTRAINTS, (double)(n_en * step));
}

// Which of the two the step kernel uses: the atomics unless the env says otherwise.  They execute at the memory side at
// ~1.3 TB/s chip-wide (MI355X_MICROARCH.md "Global float atomics"): nothing for an env whose lanes finish rarely
// (ChemicalReactor 0.3 % per step, RobotAssembly 2.4 %), but PowerGrid finishes 18 % of its lanes every step -- 19 bytes
// of atomic traffic per env-step, ~16 % of its step launch at 262 144 lanes -- so it keeps the load / store flush.
template <class E, class = void> struct tally_atomic : std::true_type {};
template <class E> struct tally_atomic<E, std::void_t<decltype(E::TALLY_ATOMIC)>> : std::bool_constant<E::TALLY_ATOMIC> {};

// Register-resident partial tally of one lane for the duration of a fused rollout.
struct LaneTally {
    double ret_sum, ret_sq, ret_min, ret_max, len_sq;
    int episodes, len_sum, viol, crit, shutdown, success;
    long long life;
    __device__ __forceinline__ void clear()
    {
        ret_sum = 0.0; ret_sq = 0.0; ret_min = __builtin_inf(); ret_max = -__builtin_inf(); len_sq = 0.0;
        episodes = 0; len_sum = 0; viol = 0; crit = 0; shutdown = 0; success = 0; life = 0;
    }
    __device__ __forceinline__ void episode(double ret, int step, uint32_t viol_ep, int ncrit)
    {
        const double len = (double)step;
        episodes += 1; ret_sum += ret; ret_sq += ret * ret;
        ret_min = fmin(ret_min, ret); ret_max = fmax(ret_max, ret);
        len_sum += step; len_sq += len * len;
        viol += (int)viol_ep; crit += ncrit; shutdown += (ncrit > 0) ? 1 : 0; success += (ret > 0.0) ? 1 : 0;
    }
    // The episode that ended with this step: base.py:183 total_violations (never reset) takes its violations, the tally -- if
    // the handle keeps one -- the episode, and the running return starts over.  What becomes of the counter word (0 for a lane
    // that restarts, NIG_CTR_DONE for one that waits) is the caller's: the kernels differ in where the restart happens.
    // Returns the running return to go on with.
    template <class RT>
    __device__ __forceinline__ RT finish(bool tally, RT ret, int step, uint32_t viol_ep, int ncrit)
    {
        life += (long long)viol_ep;
        if (tally) { episode((double)ret, step, viol_ep, ncrit); ret = (RT)0; }
        return ret;
    }
    // merge into the lane's column of the global tally (same fp64 operation order per row as
    // flush_tally would have produced when at most one episode finished; sums of several
    // episodes are added as one partial -- integer rows exact, fp rows within 1 ulp of fp64)
    __device__ __forceinline__ void merge(double *T, uint32_t ld, int n_en) const
    {
        double v[NIG_T_ROWS];
#pragma unroll
        for (int r = 0; r < NIG_T_ROWS; ++r) v[r] = T[(size_t)r * ld];
        v[NIG_T_EPISODES] += (double)episodes;
        v[NIG_T_RET_SUM] += ret_sum;
        v[NIG_T_RET_SQ] += ret_sq;
        v[NIG_T_RET_MIN] = fmin(v[NIG_T_RET_MIN], ret_min);
        v[NIG_T_RET_MAX] = fmax(v[NIG_T_RET_MAX], ret_max);
        v[NIG_T_LEN_SUM] += (double)len_sum;
        v[NIG_T_LEN_SQ] += len_sq;
        v[NIG_T_VIOL] += (double)viol;
        v[NIG_T_CRIT] += (double)crit;
        v[NIG_T_SHUTDOWN] += (double)shutdown;
        v[NIG_T_SUCCESS] += (double)success;
        v[NIG_T_SATISFIED] += (double)((long long)n_en * len_sum - viol);   // every step of a finished episode has n_en constraints
        v[NIG_T_CONSTRAINTS] += (double)((long long)n_en * len_sum);
#pragma unroll
        for (int r = 0; r < NIG_T_ROWS; ++r) T[(size_t)r * ld] = v[r];
    }
};

// ---- the end of a fused launch ------------------------------------------------------------------------------------------------
// A lane's bookkeeping goes back to the handle (lanes of the batch only; the state rows are the body's own lines before this):
// the counter word, the lifetime violations of the episodes that finished in this launch (`life`: LaneTally::life, or whatever
// else the body counted them in -- PowerGrid's LDS-resident body uses the tally's own `viol`), the running return, and the
// partial tally if an episode ended.  `life` and `ret` keep the caller's types: they are widened where they are stored.
template <class LT, class RT>
__device__ __forceinline__ void store_episode(uint32_t *ctr_rows, long long *life_viol, double *ep_ret, double *tally_rows, uint32_t ld, int n_en,
                                              uint32_t base, unsigned tid, bool tally, uint32_t ctr, LT life, RT ret, const LaneTally &lt)
{
    (ctr_rows + base)[tid] = ctr;
    if (life != 0) (life_viol + base)[tid] += (long long)life;
    if (tally) {
        (ep_ret + base)[tid] = (double)ret;
        if (lt.episodes > 0) lt.merge(tally_rows + base + tid, ld, n_en);
    }
}

// ---- row-major observation rows -----------------------------------------------------------------------------------------------
// The fence pair between a wave's writes of its 64 rows into its LDS image and the transposed reads that turn them into whole-line
// streaming stores (rollout_body and rollout_policy_kernel: image [64][S]; nig_pg_lds.hpp: PowerGrid's state image).
// The image reads are OTHER lanes' writes.  The compiler reasons per thread: a lane's own piece 48 l + 16 can
// never be the address 16 l + 1024 k it reads, so without the fence it may sink that store out of the loop (it did, in the
// injected-draw variant -- the only one whose loop holds no other fence).  Wavefront scope: pins the compiler's order, emits no
// wait (the LDS pipeline executes a wave's operations in order, so the reads see the writes issued before them).
__device__ __forceinline__ void image_rows_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace nig
