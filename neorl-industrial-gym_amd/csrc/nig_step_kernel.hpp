// nig_step_kernel.hpp -- the one-step kernels (device code only): step_kernel (nig_step and its variants), reset_kernel
// (nig_reset) and fill_actions_kernel (nig_fill_actions).
#pragma once
#include "nig_step.hpp"

namespace nig {

// One launch = IndustrialEnv.step for every lane.
//
// Memory shape: every row pointer is block-uniform (SGPR base) and the lane adds a 32-bit offset,
// so each access is "global_load_dword v, v_off, s[base]" over one contiguous 1 KiB row segment
// per block.  All loads (counter, state rows, action rows, injected noise) are issued up front in
// one batch -- a lane that turns out to be finished just discards them -- so the kernel has one
// memory round trip before the arithmetic, not two.
//
// Auto-reset: lanes that finish are COMPACTED across the 256-lane block through LDS and their
// initial states are produced by the first ceil(n/64) waves at full lane utilisation (with 18 % of
// PowerGrid lanes finishing per step every wave would otherwise run the whole reset path for a
// handful of active lanes).
// ACT64: the action rows are float64 (nig_step64; CR / PG / RA only: the envs whose NumPy arithmetic then changes).
// BLK: threads per block.  256, or Env::STEP_BLOCK for big fast-mode batches (PowerGrid: 512 -- the 12 KiB generator
// table is then shared by eight waves and two blocks = 16 waves fit a CU next to their reset images, so a
// 262 144-lane batch is resident in ONE round instead of 1.33: 30 -> 24 us per step; small batches keep 256 to
// spread over all CUs).
// HELP (auto-reset handles of COOP_RESET envs in fast mode, batches that leave one wave per SIMD: launch_step): the block
// is launched with 2 BLK threads.  Threads BLK .. 2 BLK - 1 are HELPER waves: helper h draws and builds the initial state
// lane h would restart from if it finished in this step -- it depends on the lane's generator key only, not on the state
// -- into LDS while the lane's own wave is still waiting for its loads and stepping; one block barrier later a finishing
// lane just picks its row up.  At 65 536 lanes every launch has some wave with a finishing lane, so the launch always
// paid the reset path behind its step (ballot, work list, two to eight generator blocks, their table look-ups -- a
// third dependent memory round trip -- and the read-back: 1.6 of ChemicalReactor's 4.9 us per replayed launch,
// profiles/r03/step_api_probe.txt); now that path runs beside the step instead of behind it, on issue slots the lone
// wave of a SIMD leaves empty.  Same draw_init + init as reset_kernel and as the cooperative reset: same values.
template <class Env, bool PARITY, bool ACT64 = false, int BLK = 256, bool HELP = false>
__global__ void __launch_bounds__(HELP ? 2 * BLK : BLK, (ACT64 || HELP ? 2 : (BLK / 256) * Env::STEP_WAVES)) step_kernel(const StepArgs p)
{
    constexpr int BLOCK = BLK;             // shadows the file-wide constant inside this kernel: LANES per block
    constexpr int S = Env::S, A = Env::A, KS = Env::KS, KR = Env::KR;
    constexpr int KSN = KS > 0 ? KS : 1;
    constexpr int NWAVE = BLOCK / 64;
    constexpr bool COOP = Env::COOP_RESET && !PARITY;          // wave-cooperative auto-reset (fast mode): coop_reset above
    static_assert(!HELP || (COOP && !ACT64), "helper waves: fast-mode float32 steps of envs with a cooperative reset");
    using act_t = std::conditional_t<ACT64, double, float>;
    __shared__ unsigned short s_list[COOP ? 1 : BLOCK];
    __shared__ int s_cnt[COOP ? 1 : NWAVE];
    __shared__ float s_img[COOP && !HELP ? NWAVE * Env::RESET_ROWS * 64 : 1];
    __shared__ unsigned char s_wlist[COOP && !HELP ? BLOCK : 1];
    __shared__ float s_new[HELP ? S * BLOCK : 1];              // [S][BLOCK]: the initial states the helpers prepared
    constexpr bool HELP_TALLY = HELP && !tally_atomic<Env>::value;
    __shared__ double s_fin_ret[HELP_TALLY ? BLOCK : 1];       // what a finished episode leaves for the tally when the helpers flush it
    __shared__ uint32_t s_fin_viol[HELP_TALLY ? BLOCK : 1], s_fin_word[HELP_TALLY ? BLOCK : 1];   // word: step | ncrit << 20 | finished << 31

    const bool helper = HELP && threadIdx.x >= (unsigned)BLOCK;
    const unsigned tid = HELP ? (threadIdx.x & (unsigned)(BLOCK - 1)) : threadIdx.x;    // lane of the block (helper: the lane it works for)
    const uint32_t base = blockIdx.x * BLOCK;                  // block-uniform
    const bool in_range = base + tid < p.B;
    const uint32_t t_now = launch_counter(p.t_ptr, p.t_off);        // (the pointer chase costs 0.03-0.05 us of the launch: measured with a build that skipped it)
    // The generator's table: staged in LDS when a lane looks up many normals per launch; an env with a couple of draws
    // per step reads its entries straight from the 12 KiB global table (L2-resident) -- staging 12 KiB per block plus a
    // block barrier costs more than two or three 16-byte loads per lane.  With helper waves THEY stage it, first thing.
    constexpr bool STAGE_TABLE = PARITY ? false : (KS > 4 || (HELP && KS > 0));
    __shared__ float4 s_probit_[STAGE_TABLE ? 768 : 1];
    const float4 *const s_probit = STAGE_TABLE ? s_probit_ : NIG_PROBIT;
    if constexpr (HELP) {
        if (helper) {
            __builtin_amdgcn_s_setprio(0);
            if constexpr (STAGE_TABLE) {
                for (int i_ = (int)tid; i_ < 768; i_ += BLOCK) s_probit_[i_] = NIG_PROBIT[i_];
                __syncthreads();
            }
#ifdef NIG_DIAG_HELP_SKIP              // (diagnostic builds only, wrong restart states: what is left when the helpers cost nothing?)
            if (false) {
#else
            if (in_range) {
#endif
                double rn[KR > 0 ? KR : 1];
                Env::draw_init(make_key(p.env0 + (uint64_t)(base + tid), t_now, p.seed_lo, p.seed_hi, s_probit), rn);
                float r0[S];
                Env::init(rn, r0);
#pragma unroll
                for (int k = 0; k < S; ++k) s_new[k * BLOCK + tid] = r0[k];
            }
            __syncthreads();
            // ... and, for an env whose tally is not kept with atomics (PowerGrid), takes the episode tally of the lanes that
            // finished off their waves after the barrier: 13 loads, a wait and 13 stores the stepping wave no longer sits
            // through (8.84 -> 8.57 us per launch).  No-return atomics stay with the stepping wave, which issues them earlier
            // than a helper could (ChemicalReactor: 4.05 us there, 4.23 us from the helper).
            if constexpr (HELP_TALLY) {
                if (p.tally != nullptr && in_range) {
                    const uint32_t w = s_fin_word[tid];
                    if (w >> 31)
                        flush_tally(p.tally + base + tid, p.ld, s_fin_ret[tid], (int)(w & 0xFFFFFu), s_fin_viol[tid], (int)((w >> 20) & 0x7FFu), p.n_en);
                }
            }
            return;
        }
        __builtin_amdgcn_s_setprio(2);
    }

    // ---- one batch of loads -------------------------------------------------------------
    const uint32_t *ctr_row = p.ctr + base;
    const float *st_row = p.state + base;
    const act_t *act_row;
    if constexpr (ACT64) act_row = p.actions64 + base; else act_row = p.actions + base;
    uint32_t ctr = NIG_CTR_DONE;
    float s[S], n[S];
    act_t a[A];
    using nz_t = std::conditional_t<PARITY, double, typename Env::fast_noise_t>;   // injected draws are fp64
    nz_t nz[KSN];
    double ret_prev = 0.0;                 // the running episode return (utils.py:99), read with the batch: a load behind the
                                           // step's arithmetic would be one more memory round trip on the launch's critical path
    // No branch around the loads: a lane beyond the batch reads lane 0's rows of its block (which exist) and is masked out
    // below.  Loads inside a conditional block make the waitcnt pass wait for them where the block ends -- before the
    // generator's arithmetic, which needs none of them -- instead of at their first use.
    const unsigned li = in_range ? tid : 0u;
    {
        const uint32_t c_ld = ctr_row[li];
        ctr = in_range ? c_ld : NIG_CTR_DONE;
        // (the running return without a branch as well.  A handle without the tally has no return row; the always-present
        // lifetime-violation row stands in, its value unused)
        ret_prev = (p.tally ? p.ep_ret + base : reinterpret_cast<const double *>(p.life_viol + base))[li];
#pragma unroll
        for (int k = 0; k < S; ++k) s[k] = (st_row + k * p.ld_state)[li];
#pragma unroll
        for (int k = 0; k < A; ++k) a[k] = (act_row + k * p.ld_act)[li];
        if constexpr (PARITY && KS > 0) {
            const double *nz_row = p.step_noise + base;
#pragma unroll
            for (int k = 0; k < KS; ++k) nz[k] = (nz_row + k * p.ld_noise)[li];
        }
    }
    // the table is staged only now: the state / action loads above are already in flight
    if constexpr (STAGE_TABLE) {
        if constexpr (!HELP) {
            for (int i_ = (int)threadIdx.x; i_ < 768; i_ += BLOCK) s_probit_[i_] = NIG_PROBIT[i_];
        }
        __syncthreads();
    }
    const bool active = in_range && !(ctr & NIG_CTR_DONE);     // base.py:159-160: finished lanes wait for reset

    const RngKey key = make_key(p.env0 + (uint64_t)(base + tid), t_now, p.seed_lo, p.seed_hi, s_probit);
    if constexpr (KS > 0) {
        if constexpr (!PARITY) Env::draw_step(key, nz);
    } else {
        nz[0] = (nz_t)0;
    }

    // ---- IndustrialEnv.step in registers --------------------------------------------------
    const int step_pre = (int)(ctr & NIG_CTR_STEP_MASK);
    StepResult<Env, reward_of<Env, act_t>> res;
    step_core<Env>(s, a, nz, step_pre, p.max_steps, p.dt32, p.dt, p.cmask, n, res);

    const int step = step_pre + 1;
    const uint32_t viol_ep = episode_violations(ctr, res.nviol);
    const bool done = res.terminated || res.truncated;
    uint32_t fl = pack_flags<Env>(res, step);
    uint32_t nctr = counter_word(step, viol_ep);
    const bool autoreset = (p.hflags & NIG_F_AUTORESET) != 0;
    const bool need_reset = active && done && autoreset;

    // utils.py:99  episode_return += reward.  Computed for every lane, used by the tally's: a use inside the conditional
    // blocks below would let the compiler sink the LOAD of the running return down there, behind the step (one more round trip)
    double ret = add_reward<Env, ACT64>(ret_prev, res.reward);
    asm volatile("" :: "v"(ret));                 // (a use the sinking pass cannot move the load past)
    if (active) {
        if (done) {
            // base.py:183 total_violations (never reset): the lane's own counter, added to with a no-return atomic -- a
            // load + add + store would put a dependent memory round trip behind the step in every launch that finishes a lane
            __hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(p.life_viol + base) + tid, (unsigned long long)viol_ep,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (p.tally) {
                if constexpr (HELP_TALLY) { s_fin_ret[tid] = ret; s_fin_viol[tid] = viol_ep; }      // flushed by the lane's helper, after the barrier
                else if constexpr (tally_atomic<Env>::value) flush_tally_atomic(p.tally + base + tid, p.ld, ret, step, viol_ep, res.ncrit, p.n_en);
                else flush_tally(p.tally + base + tid, p.ld, ret, step, viol_ep, res.ncrit, p.n_en);
                ret = 0.0;
            }
            if (p.final_obs) {
                float *fo = p.final_obs + base;
#pragma unroll
                for (int k = 0; k < S; ++k) (fo + k * p.ld_obs)[tid] = n[k];
            }
            if (autoreset) { nctr = 0u; fl |= did_reset_flag(true); }
            else nctr |= NIG_CTR_DONE;
        }
        if constexpr (!COOP) {
            if (!need_reset) {                    // a resetting lane's state is written by the compacted pass below
                float *so = p.state + base;
#pragma unroll
                for (int k = 0; k < S; ++k) (so + k * p.ld_state)[tid] = n[k];
                if (p.mirror) {
#pragma unroll
                    for (int k = 0; k < S; ++k) (p.mirror + base + k * p.ld_mirror)[tid] = n[k];
                }
            }
        }
        (p.ctr + base)[tid] = nctr;
        if (p.tally) (p.ep_ret + base)[tid] = ret;
        if (p.reward) (p.reward + base)[tid] = (float)res.reward;
        if (p.reward64) (p.reward64 + base)[tid] = (double)res.reward;
        if (p.flags) (p.flags + base)[tid] = fl;
    } else if (in_range) {
        if (p.flags) (p.flags + base)[tid] = NIG_FLAG_INACTIVE | ((ctr & NIG_CTR_STEP_MASK) << NIG_FLAG_STEP_SHIFT);
        if (p.reward) (p.reward + base)[tid] = 0.0f;
        if (p.reward64) (p.reward64 + base)[tid] = 0.0;
        if (p.mirror) {                           // a frozen lane: its state as it stands
#pragma unroll
            for (int k = 0; k < S; ++k) (p.mirror + base + k * p.ld_mirror)[tid] = s[k];
        }
    }

    if constexpr (COOP) {
        if constexpr (HELP) {
            if constexpr (HELP_TALLY) {
                if (in_range) s_fin_word[tid] = (uint32_t)step | ((uint32_t)res.ncrit << 20) | ((active && done) ? 0x80000000u : 0u);
            }
            __syncthreads();                      // the helpers' rows are in LDS
            if (need_reset) {
#pragma unroll
                for (int k = 0; k < S; ++k) n[k] = s_new[k * BLOCK + tid];
            }
        } else {
        // every wave renews its own finishing lanes (all 64 lanes work, whatever their own state), then stores
        const unsigned long long m = __ballot(need_reset);
        if (m != 0ull)
            coop_reset<Env>(m, need_reset, tid & 63u, s_img + (tid >> 6) * (Env::RESET_ROWS * 64), s_wlist + (tid >> 6) * 64,
                            p.env0 + (uint64_t)(base + (tid & ~63u)), t_now, p.seed_lo, p.seed_hi, s_probit, n);
        }
        if (active) {
            float *so = p.state + base;
#pragma unroll
            for (int k = 0; k < S; ++k) (so + k * p.ld_state)[tid] = n[k];
            if (p.mirror) {
#pragma unroll
                for (int k = 0; k < S; ++k) (p.mirror + base + k * p.ld_mirror)[tid] = n[k];
            }
        }
        return;
    }
    // ---- compacted auto-reset: IndustrialEnv.reset (base.py:133-155) for the finished lanes ----
    if (!autoreset) return;                       // block-uniform
    const unsigned wave = tid >> 6, lane = tid & 63u;
    const unsigned long long m = __ballot(need_reset);
    if (lane == 0) s_cnt[wave] = __popcll(m);
    if (need_reset) s_list[wave * 64 + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)tid;
    __syncthreads();
    int cnt[NWAVE], total = 0;
#pragma unroll
    for (int w = 0; w < NWAVE; ++w) { cnt[w] = s_cnt[w]; total += cnt[w]; }
    for (int j = (int)tid; j < total; j += BLOCK) {
        int w = 0, r = j;
#pragma unroll
        for (int q = 0; q < NWAVE - 1; ++q) { const bool nxt = (w == q) && (r >= cnt[q]); r = nxt ? r - cnt[q] : r; w = nxt ? q + 1 : w; }
        const unsigned tl = s_list[w * 64 + r];   // block-local index of the lane being reset
        double rn[KR > 0 ? KR : 1];
        if constexpr (PARITY) {
            const double *rn_row = p.reset_noise + base;
#pragma unroll
            for (int k = 0; k < KR; ++k) rn[k] = (rn_row + k * p.ld_noise)[tl];
        } else {
            Env::draw_init(make_key(p.env0 + (uint64_t)(base + tl), t_now, p.seed_lo, p.seed_hi, s_probit), rn);
        }
        float r0[S];
        Env::init(rn, r0);
        float *so = p.state + base;
#pragma unroll
        for (int k = 0; k < S; ++k) (so + k * p.ld_state)[tl] = r0[k];
        if (p.mirror) {
#pragma unroll
            for (int k = 0; k < S; ++k) (p.mirror + base + k * p.ld_mirror)[tl] = r0[k];
        }
    }
}

struct ResetArgs {
    float *state; uint32_t *ctr; long long *life_viol; double *ep_ret;
    int64_t ld; int64_t B; int64_t ld_state;
    const uint8_t *mask; const double *noise; int64_t ld_noise;
    uint64_t env0; uint32_t seed_lo, seed_hi, t;
};

template <class Env, bool PARITY>
__global__ void __launch_bounds__(BLOCK) reset_kernel(const ResetArgs p)
{
    constexpr int S = Env::S, KR = Env::KR;
    __shared__ float4 s_probit[768];
    stage_probit(s_probit, threadIdx.x, BLOCK);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= p.B) return;
    if (p.mask && !p.mask[i]) return;
    double rn[KR > 0 ? KR : 1];
    if constexpr (PARITY) {
#pragma unroll
        for (int k = 0; k < KR; ++k) rn[k] = p.noise[(int64_t)k * p.ld_noise + i];
    } else {
        Env::draw_init(make_key(p.env0 + (uint64_t)i, p.t, p.seed_lo, p.seed_hi, s_probit), rn);
    }
    float s[S];
    Env::init(rn, s);
#pragma unroll
    for (int k = 0; k < S; ++k) p.state[(int64_t)k * p.ld_state + i] = s[k];
    const uint32_t ctr = p.ctr[i];
    // violations of an abandoned (not finished) episode still belong to total_violations
    if (!(ctr & NIG_CTR_DONE)) p.life_viol[i] += (long long)(ctr >> NIG_CTR_VIOL_SHIFT);
    p.ctr[i] = 0u;                                // base.py:137-139
    if (p.ep_ret) p.ep_ret[i] = 0.0;
}

template <class Env>
__global__ void __launch_bounds__(BLOCK) fill_actions_kernel(float *act, int64_t ld_act, int64_t B, uint64_t env0,
                                                             uint32_t seed_lo, uint32_t seed_hi, uint32_t t)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= B) return;
    const RngKey key = make_key(env0 + (uint64_t)i, t, seed_lo, seed_hi);
    double u[Env::A];
    gen_uniforms<Env::A>(key, STREAM_ACTION, u);
#pragma unroll
    for (int k = 0; k < Env::A; ++k)      // uniform in the env's action Box: low + (high - low) * u
        act[(int64_t)k * ld_act + i] = (float)((double)Env::act_low(k) + ((double)Env::act_high(k) - (double)Env::act_low(k)) * u[k]);
}

}  // namespace nig
