// nig_rollout_policy.hpp -- the closed-loop fused rollout, one wave per 64 lanes (device code only): rollout_policy_kernel,
// under sensor / actuator noise rollout_policy_disturbed_kernel, under added box constraints rollout_policy_limited_kernel, and
// under both rollout_policy_disturbed_limited_kernel.
// Its three-wave form is nig_split_policy.hpp.
#pragma once
#include "nig_policy.hpp"
#include "nig_disturb.hpp"
#include "nig_limits.hpp"

namespace nig {

// The body is written once (nig_rollout_policy_body.inc) and compiled into four kernels by textual inclusion, as the three-wave
// kernels are (nig_split.hpp says why: through a __device__ function taking the arguments by reference hipcc generates different
// code for the existing kernel, which is required not to change: profiles/isa_diff.py).
template <class Env>
__global__ void __launch_bounds__(BLOCK) rollout_policy_kernel(const PolicyArgs q)
{
    constexpr bool DIST = false, LIM = false;
    [[maybe_unused]] constexpr const DisturbArgs *dq = nullptr;
    [[maybe_unused]] constexpr const LimitArgs *lq = nullptr;
#include "nig_rollout_policy_body.inc"
}

struct PolicyDistArgs {
    PolicyArgs p;
    DisturbArgs d;
};

// DIST: the policy acts on a disturbed observation and the plant receives a disturbed action (include/nig.h "nig-disturb-v1").
// Instantiated in the env's disturbed_*.hip translation unit only (launch_policy_family on PolicyDistArgs).
template <class Env>
__global__ void __launch_bounds__(BLOCK) rollout_policy_disturbed_kernel(const PolicyDistArgs qd)
{
    constexpr bool DIST = true, LIM = false;
    const PolicyArgs &q = qd.p;
    const DisturbArgs *const dq = &qd.d;
    [[maybe_unused]] constexpr const LimitArgs *lq = nullptr;
#include "nig_rollout_policy_body.inc"
}

struct PolicyLimArgs {
    PolicyArgs p;
    LimitArgs l;
};

// LIM: the step law is step_core_limited -- the user's added box constraints beside the built-ins (include/nig.h "nig-limits-v1")
// -- and a second word per step, xflags, says which of them fired.  The one-wave form only, like the disturbed twin.
// Instantiated in the env's limited_*.hip translation unit only (launch_policy_family on PolicyLimArgs).
template <class Env>
__global__ void __launch_bounds__(BLOCK) rollout_policy_limited_kernel(const PolicyLimArgs ql)
{
    constexpr bool DIST = false, LIM = true;
    const PolicyArgs &q = ql.p;
    [[maybe_unused]] constexpr const DisturbArgs *dq = nullptr;
    const LimitArgs *const lq = &ql.l;
#include "nig_rollout_policy_body.inc"
}

struct PolicyDistLimArgs {
    PolicyArgs p;
    DisturbArgs d;
    LimitArgs l;
};

// DIST and LIM together: the disturbed and clipped action is the one step_core_limited checks.
// Instantiated in the env's limited_disturbed_*.hip translation unit only (launch_policy_family on PolicyDistLimArgs).
template <class Env>
__global__ void __launch_bounds__(BLOCK) rollout_policy_disturbed_limited_kernel(const PolicyDistLimArgs qx)
{
    constexpr bool DIST = true, LIM = true;
    const PolicyArgs &q = qx.p;
    const DisturbArgs *const dq = &qx.d;
    const LimitArgs *const lq = &qx.l;
#include "nig_rollout_policy_body.inc"
}

}  // namespace nig
