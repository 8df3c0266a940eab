// nig_disturb.hpp -- sensor / actuator noise of the closed-loop kernels (device code only; spec: include/nig.h
// "nig-disturb-v1"): DisturbArgs as the kernels receive it, its switches, and the law in three parts -- disturb_draws,
// disturb_obs, disturb_act.  The kernels that run it: rollout_policy_disturbed_kernel (nig_rollout_policy.hpp) and
// rollout_mlp_disturbed_kernel (nig_mlp.hpp).
#pragma once
#include "nig_step.hpp"

namespace nig {

// Passed by value inside the kernel arguments: every field is wave-uniform and read through the scalar cache.
struct DisturbArgs {
    float sigma_obs[NIG_MAX_STATE_DIM];
    float sigma_act[NIG_MAX_ACTION_DIM];
    float clip_lo, clip_hi;
    int32_t hold;               // NIG_HOLD_STEP / NIG_HOLD_EPISODE
    float *seen_out; uint64_t seen_step_stride;      // row-major [B][S] per step: the observation the policy acted on
};

// wave-uniform: is any observation / action dimension disturbed at all?  (the switch idiom of policy_switches)
template <int S, int A>
__device__ __forceinline__ void disturb_switches(const DisturbArgs &d, bool &any_obs, bool &any_act)
{
    any_obs = false; any_act = false;
#pragma unroll
    for (int k = 0; k < S; ++k) any_obs = any_obs || (d.sigma_obs[k] != 0.0f);
#pragma unroll
    for (int j = 0; j < A; ++j) any_act = any_act || (d.sigma_act[j] != 0.0f);
}

// The step's draws.  They depend on the lane's key only -- (g, td, seed), td = t, or the counter the episode's first step had
// when the draws are held for the episode: t - step_pre, so no per-lane memory is needed -- not on the observation: a kernel
// issues them wherever they overlap other work.  Blocks STREAM_POLICY + 32.. (observation) and + 48.. (action).
template <int S, int A>
__device__ __forceinline__ void disturb_draws(const DisturbArgs &d, bool any_obs, bool any_act, uint64_t gi, uint32_t t, uint32_t step_pre,
                                              uint32_t seed_lo, uint32_t seed_hi, const float4 *tab, float (&zo)[S], float (&za)[A])
{
    static_assert(S <= 4 * 16 && A <= 4 * 16, "sixteen generator blocks per draw vector");
    const uint32_t td = d.hold == NIG_HOLD_EPISODE ? t - step_pre : t;
    const RngKey key = make_key(gi, td, seed_lo, seed_hi, tab);
    if (any_obs) gen_normals<S>(key, STREAM_POLICY + 32u, zo);
    if (any_act) gen_normals<A>(key, STREAM_POLICY + 48u, za);
}

// o_k = s_k + sigma_obs[k] * zo_k on every dimension when any is disturbed, else o = s
template <int S>
__device__ __forceinline__ void disturb_obs(const DisturbArgs &d, bool any_obs, const float (&s)[S], const float (&zo)[S], float (&o)[S])
{
#pragma unroll
    for (int k = 0; k < S; ++k) o[k] = any_obs ? s[k] + d.sigma_obs[k] * zo[k] : s[k];
}

// u_j += sigma_act[j] * za_j when any dimension is disturbed, then the disturbance's clip (policy_finish_sw's form)
template <int A>
__device__ __forceinline__ void disturb_act(const DisturbArgs &d, bool any_act, const float (&za)[A], float (&u)[A])
{
    const float lo = d.clip_lo, hi = d.clip_hi;
#pragma unroll
    for (int j = 0; j < A; ++j) {
        float x = any_act ? u[j] + d.sigma_act[j] * za[j] : u[j];
        x = (x < lo) ? lo : x;
        x = (x > hi) ? hi : x;
        u[j] = x;
    }
}

// the row of a live lane in seen_out: plain row stores (a diagnostic output)
template <int S>
__device__ __forceinline__ void disturb_store_seen(const DisturbArgs &d, int it, size_t lane, const float (&o)[S])
{
    float *oo = d.seen_out + (size_t)it * d.seen_step_stride + lane * S;
    if constexpr (S % 4 == 0) {
#pragma unroll
        for (int k = 0; k < S / 4; ++k) store16(oo + 4 * k, o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
    } else {
#pragma unroll
        for (int k = 0; k < S; ++k) oo[k] = o[k];
    }
}

}  // namespace nig
