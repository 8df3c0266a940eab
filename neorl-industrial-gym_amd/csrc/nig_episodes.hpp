// nig_episodes.hpp -- per-episode records from the reward / flag rows every rollout entry point writes (include/nig.h
// nig_episode_log_*, nig_collect_episodes, nig_reduce_episodes).
//
// Three pieces:
//   (a) the per-lane state machine that turns step rows into records, stated ONCE as plain C++17 (no HIP types; NIG_HD is
//       __host__ __device__ under hipcc and nothing under a host compiler): collect_episodes_kernel runs it on the device,
//       tests/episodes_probe.cpp on the host, and episodes.episodes_from_rows restates it in NumPy;
//   (b) the record layout (episode_log_layout: what nig_episode_log_query answers) and the counting rule of a reduction;
//   (c) the two kernels (device builds only): collect_episodes_kernel and episode_tally_kernel.
//
// The log never looks into a handle's workspace: it consumes rows, so it serves the ring-fed, sampled, policy, MLP, shielded,
// ensemble and disturbed rollouts, in every kernel form, without a twin of any of them.
#pragma once
#include <stdint.h>

#include "../../include/nig.h"
#ifdef __HIPCC__
#include "nig_device.hpp"
#include "nig_episode.hpp"
#define NIG_HD __host__ __device__
#else
#define NIG_HD
#endif

namespace nig {

// ---- (a) the state machine ----------------------------------------------------------------------------------------------------
// What a lane carries from one step row to the next, and from one nig_collect_episodes call to the next.  The packed words use
// the records' own formats (w2, w3, w4 below), so a finished episode's words are the carry's words.
struct EpisodeCarry {
    double ret;        // running return (an env that accumulates in float32 holds exactly that float)
    uint32_t viol;     // violations of the running episode (sum of the per-step violation counts, base.py:182)
    uint32_t c01, c23; // steps on which constraint 0 / 1 (2 / 3) was violated: low / high 16 bits
    uint32_t su;       // NIG_FLAG_SHIELDED steps (low 16 bits), NIG_FLAG_UNCERTAIN steps (high 16 bits)
};

// One finished episode: a column entry of the six record rows.
struct EpisodeRecord {
    double ret;        // episode return
    uint32_t w0;       // NIG_CTR_* format: length | NIG_CTR_DONE | violations << NIG_CTR_VIOL_SHIFT
    uint32_t w1;       // the done step's flag word masked to EPISODE_END_MASK
    uint32_t w2, w3;   // EpisodeCarry::c01, c23
    uint32_t w4;       // EpisodeCarry::su
};

constexpr uint32_t EPISODE_END_MASK = NIG_FLAG_TERMINATED | NIG_FLAG_TRUNCATED | (3u << NIG_FLAG_NCRIT_SHIFT) | NIG_FLAG_SHUTDOWN;

// SafetyMetrics.violation_count of a step's flag word (bits 5-6, plus 4 with NIG_FLAG_NVIOL_HI)
NIG_HD constexpr uint32_t flag_violations(uint32_t f) { return ((f >> NIG_FLAG_NVIOL_SHIFT) & 3u) + ((f & NIG_FLAG_NVIOL_HI) ? 4u : 0u); }

// One step row of one lane.  A frozen lane's row (NIG_FLAG_INACTIVE) is skipped entirely.  Otherwise the reward is added in the
// precision the env accumulates its return in (add_reward, nig_episode.hpp: float32 for a RET_F32 env, float64 over the float
// rows for every other), the step's counts are added, and on TERMINATED | TRUNCATED the episode becomes record number `count`
// -- written through store(count, record) only while count < capacity; `count` moves on regardless, so a caller sees an
// overflow -- and the running values start over.  The length is the done step's own step field.
template <class Store>
NIG_HD inline void episode_row(EpisodeCarry &c, uint32_t &count, uint32_t capacity, float reward, uint32_t f, bool ret_f32, Store &&store)
{
    if (f & NIG_FLAG_INACTIVE) return;
    c.ret = ret_f32 ? (double)((float)c.ret + reward) : c.ret + (double)reward;
    c.viol += flag_violations(f);
    c.c01 += ((f >> NIG_FLAG_VIOL_SHIFT) & 1u) + (((f >> (NIG_FLAG_VIOL_SHIFT + 1)) & 1u) << 16);
    c.c23 += ((f >> (NIG_FLAG_VIOL_SHIFT + 2)) & 1u) + ((f & NIG_FLAG_VIOL3) ? 0x10000u : 0u);
    c.su += ((f & NIG_FLAG_SHIELDED) ? 1u : 0u) + ((f & NIG_FLAG_UNCERTAIN) ? 0x10000u : 0u);
    if (f & (NIG_FLAG_TERMINATED | NIG_FLAG_TRUNCATED)) {
        if (count < capacity) {
            EpisodeRecord r;
            r.ret = c.ret;
            r.w0 = ((f >> NIG_FLAG_STEP_SHIFT) & NIG_CTR_STEP_MASK) | NIG_CTR_DONE | (c.viol << NIG_CTR_VIOL_SHIFT);
            r.w1 = f & EPISODE_END_MASK;
            r.w2 = c.c01; r.w3 = c.c23; r.w4 = c.su;
            store(count, r);
        }
        count += 1u;
        c.ret = 0.0; c.viol = 0u; c.c01 = 0u; c.c23 = 0u; c.su = 0u;
    }
}

// ---- (b) layout and counting rule ---------------------------------------------------------------------------------------------
// Record (k, i) -- episode k of lane i -- takes part in a reduction over n_episodes iff k * B + i < n_episodes: a pure rule of
// the indices.  n_episodes = q * B + r counts the first q episodes of every lane and one more of lanes [0, r): a fixed episode
// count per lane (the unbiased sample), and exactly the episodes the rounds of evaluate_with_safety play.
NIG_HD constexpr bool episode_counts(int64_t k, int64_t i, int64_t B, int64_t n_episodes) { return k * B + i < n_episodes; }

constexpr int EPISODE_CARRY_WORDS = 4;      // uint32 rows of the carry: viol, c01, c23, su

NIG_HD constexpr int64_t episodes_align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

// byte offsets of a log's arrays for (batch, capacity, ld); ld == 0 asks for the default pitch, batch rounded up to 64
NIG_HD inline nig_episode_log_layout episode_log_layout(int64_t batch, int64_t capacity, int64_t ld)
{
    nig_episode_log_layout L = {};
    L.batch = batch; L.capacity = capacity; L.ld = ld ? ld : episodes_align_up(batch, 64);
    int64_t off = 0;
    L.off_ret = off;        off = episodes_align_up(off + capacity * L.ld * 8, 256);
    for (int w = 0; w < 5; ++w) { L.off_w[w] = off; off = episodes_align_up(off + capacity * L.ld * 4, 256); }
    L.off_count = off;      off = episodes_align_up(off + L.ld * 4, 256);
    L.off_carry_ret = off;  off = episodes_align_up(off + L.ld * 8, 256);
    L.off_carry_w = off;    off = episodes_align_up(off + (int64_t)EPISODE_CARRY_WORDS * L.ld * 4, 256);
    L.off_tally = off;      off = episodes_align_up(off + (int64_t)(NIG_T_ROWS + 1) * L.ld * 8, 256);
    L.off_scratch = off;    off = episodes_align_up(off + (int64_t)256 * NIG_T_ROWS * 8, 256);
    L.bytes = off;
    return L;
}

#ifdef __HIPCC__
// ---- (c) the kernels ----------------------------------------------------------------------------------------------------------
// (templates on the block size, all of them: the umbrella brings this header into every translation unit, and only nig_api.hip,
// which launches them, instantiates -- and so emits -- them)
static_assert(REDUCE_BLOCKS == 256, "episode_log_layout sizes the reduce scratch for 256 block partials");

struct EpisodeLogArgs {
    double *ret; uint32_t *w[5];             // records [capacity][ld]
    uint32_t *count; double *carry_ret; uint32_t *carry_w;     // [ld], [ld], [EPISODE_CARRY_WORDS][ld]
    double *tally;                           // [NIG_T_ROWS + 1][ld]
    int64_t ld, B; uint32_t capacity;
};

// nig_episode_log_init: no episode finished, nothing running (columns [0, B) only)
template <int NT = BLOCK>
__global__ void __launch_bounds__(NT) episode_log_init_kernel(EpisodeLogArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= a.B) return;
    a.count[i] = 0u;
    a.carry_ret[i] = 0.0;
#pragma unroll
    for (int r = 0; r < EPISODE_CARRY_WORDS; ++r) a.carry_w[(int64_t)r * a.ld + i] = 0u;
}

// One lane per thread.  A lane's loads of consecutive step rows do not depend on its carry: they are issued EPISODE_GROUP rows
// at a time, ahead of the state machine.  At 65 536 lanes the launch is one wave per SIMD, and n_steps dependent round trips
// would make it latency-bound; in groups it is n_steps / EPISODE_GROUP trips with 2 x EPISODE_GROUP
// loads in flight per lane.  Record stores are rare and go to the lane's own column: plain stores.
constexpr int EPISODE_GROUP = 16;

template <bool RET_F32>
__global__ void __launch_bounds__(BLOCK) collect_episodes_kernel(EpisodeLogArgs a, const float *reward, const uint32_t *flags, int64_t out_stride, int n_steps)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.B) return;
    EpisodeCarry c;
    c.ret = a.carry_ret[i];
    c.viol = a.carry_w[i]; c.c01 = a.carry_w[a.ld + i]; c.c23 = a.carry_w[2 * a.ld + i]; c.su = a.carry_w[3 * a.ld + i];
    uint32_t count = a.count[i];
    auto store = [&](uint32_t k, const EpisodeRecord &r) {
        const int64_t at = (int64_t)k * a.ld + i;
        a.ret[at] = r.ret; a.w[0][at] = r.w0; a.w[1][at] = r.w1; a.w[2][at] = r.w2; a.w[3][at] = r.w3; a.w[4][at] = r.w4;
    };
    const float *rw = reward + i;
    const uint32_t *fl = flags + i;
    int k = 0;
    for (; k + EPISODE_GROUP <= n_steps; k += EPISODE_GROUP) {
        float r[EPISODE_GROUP]; uint32_t f[EPISODE_GROUP];
#pragma unroll
        for (int g = 0; g < EPISODE_GROUP; ++g) { r[g] = rw[(int64_t)(k + g) * out_stride]; f[g] = fl[(int64_t)(k + g) * out_stride]; }
#pragma unroll
        for (int g = 0; g < EPISODE_GROUP; ++g) episode_row(c, count, a.capacity, r[g], f[g], RET_F32, store);
    }
    for (; k < n_steps; ++k) episode_row(c, count, a.capacity, rw[(int64_t)k * out_stride], fl[(int64_t)k * out_stride], RET_F32, store);
    a.carry_ret[i] = c.ret;
    a.carry_w[i] = c.viol; a.carry_w[a.ld + i] = c.c01; a.carry_w[2 * a.ld + i] = c.c23; a.carry_w[3 * a.ld + i] = c.su;
    a.count[i] = count;
}

// nig_reduce_episodes, first step: the lane's counted records, in order, through flush_tally -- the arithmetic every kernel
// that keeps a tally uses -- into the lane's column of a tally image; row NIG_T_ROWS of the image: the lane's counted episodes
// with a non-zero violation count.  The image is then reduced by reduce_tally_stage1 / stage2 as a handle's own tally is.
template <int NT = BLOCK>
__global__ void __launch_bounds__(NT) episode_tally_kernel(EpisodeLogArgs a, int64_t n_episodes, int n_en)
{
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= a.B) return;
    double *T = a.tally + i;
#pragma unroll
    for (int r = 0; r < NIG_T_ROWS; ++r) T[(int64_t)r * a.ld] = 0.0;
    T[(int64_t)NIG_T_RET_MIN * a.ld] = __builtin_inf();
    T[(int64_t)NIG_T_RET_MAX * a.ld] = -__builtin_inf();
    const uint32_t have = a.count[i] < a.capacity ? a.count[i] : a.capacity;
    double with_violation = 0.0;
    for (uint32_t k = 0; k < have && episode_counts(k, i, a.B, n_episodes); ++k) {
        const int64_t at = (int64_t)k * a.ld + i;
        const uint32_t w0 = a.w[0][at], w1 = a.w[1][at];
        const uint32_t viol = w0 >> NIG_CTR_VIOL_SHIFT;
        flush_tally(T, (uint32_t)a.ld, a.ret[at], (int)(w0 & NIG_CTR_STEP_MASK), viol, (int)((w1 >> NIG_FLAG_NCRIT_SHIFT) & 3u), n_en);
        with_violation += viol != 0u ? 1.0 : 0.0;
    }
    T[(int64_t)NIG_T_ROWS * a.ld] = with_violation;
}

// the extra sum of nig_reduce_episodes: one block adds a row of integer-valued doubles (exact in any order) into *out
template <int NT = BLOCK>
__global__ void __launch_bounds__(NT) episode_row_sum_kernel(const double *row, int64_t B, double *out)
{
    __shared__ double sh[NT];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < B; i += NT) acc += row[i];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = sh[0];
}
#endif  // __HIPCC__

}  // namespace nig
