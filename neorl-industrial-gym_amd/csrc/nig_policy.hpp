// nig_policy.hpp -- the on-device feedback policy (device code only; spec: include/nig.h "nig-policy-v1"): PolicyArgs, the
// policy's draws, its register / dense-LDS copies and the law itself (policy_switches ... policy_action).  The kernels that run
// it: nig_rollout_policy.hpp, nig_split_policy.hpp and the closed-loop PowerGrid forms of nig_pg_lds.hpp.
#pragma once
#include "nig_step.hpp"

namespace nig {

// ------------------------------------------------------------------------------------------
// Closed-loop fused rollout: action = on-device policy(observation) -> IndustrialEnv.step, n steps
// per launch, state / counters / tallies / PID memory in registers.  No loads inside the loop
// (the policy struct is staged in LDS), so the optional outputs can stay
// run-time switches.  Spec of the policy arithmetic: include/nig.h "nig-policy-v1".
struct PolicyArgs {
    StepArgs s;
    const nig_policy *pol;      // device copy
    float *pid;                 // PID policies: per-lane controller memory [2*A][ld] (integral rows, then previous-error rows)
    int n_steps;
    uint32_t out_stride;
    float *obs_out; uint64_t obs_step_stride;                        // row-major [B][S] per step, pre-step obs
    float *act_out; uint32_t ld_act_out; uint64_t act_step_stride;   // [A][ld] per step
    uint32_t block0;            // first 256-lane block of this launch (whole blocks and a ragged last block are separate launches)
    int32_t pol_kind;           // host copy of pol->kind (NIG_POLICY_*): selects the kernel form, never read on the device
};

// The policy's random draws of one step: they depend on the lane's key only, not on the observation, so the
// cooperating-wave forms (nig_split_policy.hpp, nig_pg_lds.hpp) produce them ahead of the step that consumes them.
template <int A>
struct PolicyDraws { float z[A], h[A], ra[A], wmix; };

// Register copy of the policy fields a closed-loop form reads every step besides the feedback matrix (same field names as
// nig_policy: policy_finish / policy_switches take either).  Read in place from LDS, every field was an exposed ds_read round
// trip per step on the wave that evaluates the law.
template <int A>
struct PolicyHead {
    int32_t kind; uint32_t colmask;
    float b[A], sigma[A], half_range[A], setpoint[A], p_uniform, uniform_range, clip_lo, clip_hi, kp, ki, kd;
    __device__ __forceinline__ void load(const nig_policy &P)
    {
        kind = (int32_t)__builtin_amdgcn_readfirstlane((uint32_t)P.kind);
        colmask = __builtin_amdgcn_readfirstlane(P.colmask);
#pragma unroll
        for (int j = 0; j < A; ++j) { b[j] = P.b[j]; sigma[j] = P.sigma[j]; half_range[j] = P.half_range[j]; setpoint[j] = P.setpoint[j]; }
        p_uniform = P.p_uniform; uniform_range = P.uniform_range; clip_lo = P.clip_lo; clip_hi = P.clip_hi;
        kp = P.kp; ki = P.ki; kd = P.kd;
    }
};

// policy_affine for envs whose feedback matrix does not fit registers (PowerGrid 32 x 8, RobotAssembly 24 x 7): u_j = b_j +
// sum_k Wt[k][j] obs[k], ascending k, zero columns skipped -- the same operations on the same values as policy_affine -- with
// the matrix read from a dense 16-byte-aligned LDS copy [S rounded up to 8][8 actions] EIGHT COLUMNS AHEAD: sixteen
// ds_read_b128 in flight, one wait, then the columns' multiply-adds behind wave-uniform tests of the column mask.  (Read
// column by column inside those tests, every active column cost two exposed LDS round trips: 34 per step for PowerGrid's
// "expert" law -- +1.9 us per step, which made the paired closed loop no faster than the one-wave kernel.)
// (COLS: columns read ahead per batch -- eight where the wave has registers to spare, four on RobotAssembly's integrator)
template <class Env, int COLS = 8, class PV = PolicyHead<Env::A>>
__device__ __forceinline__ void policy_affine_dense(const PV &H, const v4f *__restrict__ wd, const float (&obs)[Env::S], float (&u)[Env::A])
{
    constexpr int S = Env::S, A = Env::A;
    static_assert(A <= 8, "dense copy holds eight actions per column");
#pragma unroll
    for (int j = 0; j < A; ++j) u[j] = H.b[j];
    const uint32_t cm = H.colmask;
#pragma unroll
    for (int q8 = 0; COLS * q8 < S; ++q8) {
        if ((cm >> (COLS * q8)) & ((1u << COLS) - 1u)) {      // wave-uniform: any column of this batch in use?
            v4f c[COLS][2];
#pragma unroll
            for (int k = 0; k < COLS; ++k) {
                if (COLS * q8 + k < S) { c[k][0] = wd[(COLS * q8 + k) * 2]; c[k][1] = wd[(COLS * q8 + k) * 2 + 1]; }
            }
#pragma unroll
            for (int k = 0; k < COLS; ++k) {
                if (COLS * q8 + k < S) {
                    if (cm & (1u << (COLS * q8 + k))) {   // wave-uniform: whole zero columns are skipped (as policy_affine)
                        const float o = obs[COLS * q8 + k];
                        const float w[8] = {c[k][0].x, c[k][0].y, c[k][0].z, c[k][0].w, c[k][1].x, c[k][1].y, c[k][1].z, c[k][1].w};
#pragma unroll
                        for (int j = 0; j < A; ++j) u[j] = u[j] + w[j] * o;
                    }
                }
            }
        }
    }
}

// fills the dense copy (every thread of the block calls it before the block barrier): wd[k][j] = Wt[k][j], j < 8
template <class Env>
__device__ __forceinline__ void policy_stage_dense(const nig_policy *gpol, float *wd, unsigned tid, unsigned nthreads)
{
    constexpr int SP = (Env::S + 7) / 8 * 8;
    for (unsigned i = tid; i < (unsigned)SP * 8u; i += nthreads)
        wd[i] = ((int)(i >> 3) < Env::S && (int)(i & 7u) < Env::A) ? gpol->Wt[i >> 3][i & 7u] : 0.0f;
}

// Register copy of the policy fields an env of this size reads, for a wave that evaluates the feedback law on its
// critical path (the integrator of nig_split_policy.hpp): read in place from LDS, every observation column is one
// exposed ds_read round trip per step.  Same field names as nig_policy: policy_apply takes either.
template <class Env>
struct PolicyRegs {
    static constexpr int S = Env::S, A = Env::A;
    int32_t kind; uint32_t colmask;
    float Wt[S][A], b[A], sigma[A], half_range[A], setpoint[A];
    float p_uniform, uniform_range, clip_lo, clip_hi, kp, ki, kd;
    // (vector registers: as scalars they spill -- 36 weights + 19 other fields against ~100 SGPRs -- and every use of a
    // spilled one costs a v_readlane; the kernel's three waves per SIMD leave each 168 VGPRs)
    __device__ static float sreg(float v) { return v; }
    __device__ __forceinline__ void load(const nig_policy &P)
    {
        kind = (int32_t)__builtin_amdgcn_readfirstlane((uint32_t)P.kind);
        colmask = __builtin_amdgcn_readfirstlane(P.colmask);
#pragma unroll
        for (int k = 0; k < S; ++k)
#pragma unroll
            for (int j = 0; j < A; ++j) Wt[k][j] = sreg(P.Wt[k][j]);
#pragma unroll
        for (int j = 0; j < A; ++j) { b[j] = sreg(P.b[j]); sigma[j] = sreg(P.sigma[j]); half_range[j] = sreg(P.half_range[j]); setpoint[j] = sreg(P.setpoint[j]); }
        p_uniform = sreg(P.p_uniform); uniform_range = sreg(P.uniform_range); clip_lo = sreg(P.clip_lo); clip_hi = sreg(P.clip_hi);
        kp = sreg(P.kp); ki = sreg(P.ki); kd = sreg(P.kd);
    }
};

template <int A, class PV>
__device__ __forceinline__ void policy_switches(const PV *__restrict__ P, bool &any_sigma, bool &any_half, bool &mix)
{
    any_sigma = false; any_half = false;
#pragma unroll
    for (int j = 0; j < A; ++j) { any_sigma = any_sigma || (P->sigma[j] != 0.0f); any_half = any_half || (P->half_range[j] != 0.0f); }
    mix = P->p_uniform > 0.0f;
}

template <class Env>
__device__ __forceinline__ void policy_draws(const nig_policy *__restrict__ P, const RngKey &key, PolicyDraws<Env::A> &d)
{
    constexpr int A = Env::A;
    bool any_sigma, any_half, mix;
    policy_switches<A>(P, any_sigma, any_half, mix);
    if (any_sigma) gen_normals<A>(key, STREAM_POLICY + 1u, d.z);
    if (any_half) {
#pragma unroll
        for (int b4 = 0; 4 * b4 < A; ++b4) {
            const u32x4 x = key.block(STREAM_POLICY + 8u + (uint32_t)b4);
            const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (4 * b4 + i < A) d.h[4 * b4 + i] = 2.0f * u01f(w[i]) - 1.0f;
        }
    }
    if (mix) {
        d.wmix = u01f(key.block(STREAM_POLICY).x);
        const float r = P->uniform_range;
#pragma unroll
        for (int b4 = 0; 4 * b4 < A; ++b4) {
            const u32x4 x = key.block(STREAM_POLICY + 16u + (uint32_t)b4);
            const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (4 * b4 + i < A) d.ra[4 * b4 + i] = r * (2.0f * u01f(w[i]) - 1.0f);
        }
    }
}

// feedback law on the observation + the draws + the policy's own clip (include/nig.h "nig-policy-v1"), in its two halves:
// policy_affine = u_j = b_j + sum_k Wt[k][j] obs[k] (ascending k, zero columns skipped), policy_finish = exploration
// noise, epsilon-mix and the policy's clip.  policy_apply composes them (PID: its own law, then policy_finish).
template <class Env, class PV>
__device__ __forceinline__ void policy_affine(const PV *__restrict__ P, const float (&obs)[Env::S], float (&u)[Env::A])
{
    constexpr int S = Env::S, A = Env::A;
#pragma unroll
    for (int j = 0; j < A; ++j) u[j] = P->b[j];
    const uint32_t cm = P->colmask;
#pragma unroll
    for (int k = 0; k < S; ++k) {
        if (cm & (1u << k)) {                  // wave-uniform: whole zero columns are skipped
#pragma unroll
            for (int j = 0; j < A; ++j) u[j] = u[j] + P->Wt[k][j] * obs[k];
        }
    }
}

// (the switches and the clip bounds handed in: a caller that keeps them in registers across its loop spares the wave that
// evaluates the law ~16 LDS reads and a round trip per step)
template <class Env, class PV>
__device__ __forceinline__ void policy_finish_sw(const PV *__restrict__ P, bool any_sigma, bool any_half, bool mix, float lo, float hi,
                                                 const PolicyDraws<Env::A> &d, float (&u)[Env::A])
{
    constexpr int A = Env::A;
    if (any_sigma) {
#pragma unroll
        for (int j = 0; j < A; ++j) u[j] = u[j] + P->sigma[j] * d.z[j];
    }
    if (any_half) {
#pragma unroll
        for (int j = 0; j < A; ++j) u[j] = u[j] + P->half_range[j] * d.h[j];
    }
    if (mix) {
        const bool rnd = d.wmix < P->p_uniform;
#pragma unroll
        for (int j = 0; j < A; ++j) u[j] = rnd ? d.ra[j] : u[j];
    }
#pragma unroll
    for (int j = 0; j < A; ++j) {                  // np.clip == minimum(maximum(x, lo), hi)
        float x = u[j];
        x = (x < lo) ? lo : x;
        x = (x > hi) ? hi : x;
        u[j] = x;
    }
}

template <class Env, class PV>
__device__ __forceinline__ void policy_finish(const PV *__restrict__ P, const PolicyDraws<Env::A> &d, float (&u)[Env::A])
{
    bool any_sigma, any_half, mix;
    policy_switches<Env::A>(P, any_sigma, any_half, mix);
    policy_finish_sw<Env>(P, any_sigma, any_half, mix, P->clip_lo, P->clip_hi, d, u);
}

template <class Env, class PV>
__device__ __forceinline__ void policy_apply(const PV *__restrict__ P, const float (&obs)[Env::S],
                                             const PolicyDraws<Env::A> &d, float (&integ)[Env::A], float (&eprev)[Env::A],
                                             float (&u)[Env::A])
{
    constexpr int A = Env::A;
    if (P->kind == NIG_POLICY_PID) {               // baseline_agents.py:61-80
        const float kp = P->kp, ki = P->ki, kd = P->kd;
#pragma unroll
        for (int j = 0; j < A; ++j) {
            const float e = P->setpoint[j] - obs[j];
            integ[j] = integ[j] + e;
            u[j] = (kp * e + ki * integ[j]) + kd * (e - eprev[j]);
            eprev[j] = e;
        }
    } else {
        policy_affine<Env>(P, obs, u);
    }
    policy_finish<Env>(P, d, u);
}

// The one-wave kernel's form of the same policy: draws interleaved with their use (shorter live ranges than
// policy_draws + policy_apply; the two forms are pinned against each other by tests/test_gpu_split.py).
template <class Env>
__device__ __forceinline__ void policy_action(const nig_policy *__restrict__ P, const float (&obs)[Env::S],
                                              const RngKey &key, float (&integ)[Env::A], float (&eprev)[Env::A],
                                              float (&u)[Env::A])
{
    constexpr int S = Env::S, A = Env::A;
    if (P->kind == NIG_POLICY_PID) {               // baseline_agents.py:61-80
        const float kp = P->kp, ki = P->ki, kd = P->kd;
#pragma unroll
        for (int j = 0; j < A; ++j) {
            const float e = P->setpoint[j] - obs[j];
            integ[j] = integ[j] + e;
            u[j] = (kp * e + ki * integ[j]) + kd * (e - eprev[j]);
            eprev[j] = e;
        }
    } else {
#pragma unroll
        for (int j = 0; j < A; ++j) u[j] = P->b[j];
        const uint32_t cm = P->colmask;
#pragma unroll
        for (int k = 0; k < S; ++k) {
            if (cm & (1u << k)) {                  // wave-uniform: whole zero columns are skipped
#pragma unroll
                for (int j = 0; j < A; ++j) u[j] = u[j] + P->Wt[k][j] * obs[k];
            }
        }
    }
    bool any_sigma = false, any_half = false;
#pragma unroll
    for (int j = 0; j < A; ++j) { any_sigma = any_sigma || (P->sigma[j] != 0.0f); any_half = any_half || (P->half_range[j] != 0.0f); }
    if (any_sigma) {
        float z[A];
        gen_normals<A>(key, STREAM_POLICY + 1u, z);
#pragma unroll
        for (int j = 0; j < A; ++j) u[j] = u[j] + P->sigma[j] * z[j];
    }
    if (any_half) {
#pragma unroll
        for (int b4 = 0; 4 * b4 < A; ++b4) {
            const u32x4 x = key.block(STREAM_POLICY + 8u + (uint32_t)b4);
            const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (4 * b4 + i < A) u[4 * b4 + i] = u[4 * b4 + i] + P->half_range[4 * b4 + i] * (2.0f * u01f(w[i]) - 1.0f);
        }
    }
    if (P->p_uniform > 0.0f) {
        const float wmix = u01f(key.block(STREAM_POLICY).x);
        const bool rnd = wmix < P->p_uniform;
        const float r = P->uniform_range;
#pragma unroll
        for (int b4 = 0; 4 * b4 < A; ++b4) {
            const u32x4 x = key.block(STREAM_POLICY + 16u + (uint32_t)b4);
            const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (4 * b4 + i < A) { const float ra = r * (2.0f * u01f(w[i]) - 1.0f); u[4 * b4 + i] = rnd ? ra : u[4 * b4 + i]; }
        }
    }
    const float lo = P->clip_lo, hi = P->clip_hi;
#pragma unroll
    for (int j = 0; j < A; ++j) {                  // np.clip == minimum(maximum(x, lo), hi)
        float x = u[j];
        x = (x < lo) ? lo : x;
        x = (x > hi) ? hi : x;
        u[j] = x;
    }
}

}  // namespace nig
