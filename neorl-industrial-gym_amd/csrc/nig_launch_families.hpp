// nig_launch_families.hpp -- the definitions of the family launchers nig_launch.hpp declares: the kernels of nig_rollout_sampled,
// nig_rollout_mlp_ensemble, nig_rollout_policy_disturbed / nig_rollout_mlp_disturbed, nig_rollout_mlp_search, nig_rollout_mlp_gated,
// nig_rollout_mlp_projected, nig_rollout_mlp_bf16 and the _limited entry points (nig_step_limited, nig_step64_limited, nig_rollout_policy_limited,
// nig_rollout_mlp_limited) with the other families' _limited twins.
// Included by the family translation units alone (sampled_, ensemble_, disturbed_, search_, gated_, projected_, bf16_, limited_, limited_<family>_<key>.hip).  A template that is defined but not
// instantiated emits nothing: each unit explicitly instantiates the launcher of its own family for its own env, and with it that
// family's kernels and no other's.
#pragma once
#include "nig_launch.hpp"

namespace nig {

// nig_rollout_sampled: launch_rollout_env's selection on the twin kernels that draw their actions
template <class Env>
void launch_rollout_sampled_env(int out_mode, const RolloutArgs &q, uint32_t t0, unsigned grid, hipStream_t st)
{
    launch_rollout_paired<Env, true>(out_mode, q, t0, grid, st);
}

// nig_rollout_mlp_ensemble: one kernel per combination rule
template <class Env>
void launch_mlp_ensemble_env(int ens, const MlpEnsArgs &q, unsigned grid, hipStream_t st)
{
    if constexpr (has_mlp_actor<Env>) {
        if (ens == ENS_AVERAGE) hipLaunchKernelGGL((rollout_mlp_ensemble_kernel<Env, ENS_AVERAGE>), dim3(grid), dim3(BLOCK), 0, st, q);
        else hipLaunchKernelGGL((rollout_mlp_ensemble_kernel<Env, ENS_VOTING>), dim3(grid), dim3(BLOCK), 0, st, q);
    }
}

// nig_rollout_policy_disturbed.  The closed loop under a disturbance has the one-wave form only (plan_policy_disturbed): the
// three-wave and paired PowerGrid closed loops have no disturbed twin.
template <class Env>
void launch_policy_disturbed_env(const PolicyDistArgs &q, unsigned /*grid*/, hipStream_t st)
{
    const LaunchPlan plan = plan_policy_disturbed(q.p.s.B);
    PolicyDistArgs r = q;
    for (const Segment &s : plan) {
        r.p.block0 = s.block0;
        hipLaunchKernelGGL((rollout_policy_disturbed_kernel<Env>), dim3(s.grid), dim3(BLOCK), 0, st, r);
    }
}

// nig_rollout_mlp_disturbed, nig_rollout_mlp_search, nig_rollout_mlp_gated, nig_rollout_mlp_projected
template <class Env>
void launch_mlp_disturbed_env(const MlpDistArgs &q, unsigned grid, hipStream_t st) { launch_mlp<Env>(q, grid, st); }

template <class Env>
void launch_mlp_search_env(const MlpSearchArgs &q, unsigned grid, hipStream_t st) { launch_mlp<Env>(q, grid, st); }

template <class Env>
void launch_mlp_gated_env(const MlpGateArgs &q, unsigned grid, hipStream_t st) { launch_mlp<Env>(q, grid, st); }

template <class Env>
void launch_mlp_projected_env(const MlpProjectArgs &q, unsigned grid, hipStream_t st) { launch_mlp<Env>(q, grid, st); }

// nig_rollout_mlp_bf16: the actor on the bf16 matrix unit (nig_mlp_bf16.hpp)
template <class Env>
void launch_mlp_bf16_env(const MlpBf16Args &q, unsigned grid, hipStream_t st)
{
    if constexpr (has_mlp_actor<Env>) hipLaunchKernelGGL((rollout_mlp_bf16_kernel<Env>), dim3(grid), dim3(BLOCK), 0, st, q);
}

// nig_step_limited / nig_step64_limited: one plain kernel form each (injected or generated draws)
template <class Env>
void launch_step_limited_env(const StepLimArgs &q, bool parity, unsigned grid, hipStream_t st)
{
    if (parity) hipLaunchKernelGGL((step_limited_kernel<Env, true>), dim3(grid), dim3(BLOCK), 0, st, q);
    else hipLaunchKernelGGL((step_limited_kernel<Env, false>), dim3(grid), dim3(BLOCK), 0, st, q);
}
template <class Env>
void launch_step64_limited_env(const StepLimArgs &q, bool parity, unsigned grid, hipStream_t st)
{
    if constexpr (Env::HAS_ACT64) {
        if (parity) hipLaunchKernelGGL((step_limited_kernel<Env, true, true>), dim3(grid), dim3(BLOCK), 0, st, q);
        else hipLaunchKernelGGL((step_limited_kernel<Env, false, true>), dim3(grid), dim3(BLOCK), 0, st, q);
    }
}

// nig_rollout_policy_limited: the one-wave form only, as the disturbed twin (plan_policy_disturbed: whole blocks and a ragged last one)
template <class Env>
void launch_policy_limited_env(const PolicyLimArgs &q, unsigned /*grid*/, hipStream_t st)
{
    const LaunchPlan plan = plan_policy_disturbed(q.p.s.B);
    PolicyLimArgs r = q;
    for (const Segment &s : plan) {
        r.p.block0 = s.block0;
        hipLaunchKernelGGL((rollout_policy_limited_kernel<Env>), dim3(s.grid), dim3(BLOCK), 0, st, r);
    }
}

// nig_rollout_mlp_limited
template <class Env>
void launch_mlp_limited_env(const MlpLimArgs &q, unsigned grid, hipStream_t st) { launch_mlp<Env>(q, grid, st); }

// the other families' _limited twins (limited_<family>_<key>.hip): each the launcher of its parent on the twin kernel
template <class Env>
void launch_mlp_shield_limited_env(const MlpLimited<MlpShieldArgs> &q, unsigned grid, hipStream_t st) { launch_mlp<Env>(q, grid, st); }
template <class Env>
void launch_mlp_search_limited_env(const MlpLimited<MlpSearchArgs> &q, unsigned grid, hipStream_t st) { launch_mlp<Env>(q, grid, st); }
template <class Env>
void launch_mlp_gated_limited_env(const MlpLimited<MlpGateArgs> &q, unsigned grid, hipStream_t st) { launch_mlp<Env>(q, grid, st); }
template <class Env>
void launch_mlp_projected_limited_env(const MlpLimited<MlpProjectArgs> &q, unsigned grid, hipStream_t st) { launch_mlp<Env>(q, grid, st); }
template <class Env>
void launch_mlp_disturbed_limited_env(const MlpLimited<MlpDistArgs> &q, unsigned grid, hipStream_t st) { launch_mlp<Env>(q, grid, st); }
template <class Env>
void launch_mlp_ensemble_limited_env(int ens, const MlpLimited<MlpEnsArgs> &q, unsigned grid, hipStream_t st)
{
    if constexpr (has_mlp_actor<Env>) {
        if (ens == ENS_AVERAGE) hipLaunchKernelGGL((rollout_mlp_ensemble_limited_kernel<Env, ENS_AVERAGE>), dim3(grid), dim3(BLOCK), 0, st, q);
        else hipLaunchKernelGGL((rollout_mlp_ensemble_limited_kernel<Env, ENS_VOTING>), dim3(grid), dim3(BLOCK), 0, st, q);
    }
}
template <class Env>
void launch_policy_disturbed_limited_env(const PolicyDistLimArgs &q, unsigned /*grid*/, hipStream_t st)
{
    const LaunchPlan plan = plan_policy_disturbed(q.p.s.B);
    PolicyDistLimArgs r = q;
    for (const Segment &s : plan) {
        r.p.block0 = s.block0;
        hipLaunchKernelGGL((rollout_policy_disturbed_limited_kernel<Env>), dim3(s.grid), dim3(BLOCK), 0, st, r);
    }
}

}  // namespace nig

// the one line of a family translation unit: the explicit instantiation of its env's launcher(s)
#define NIG_DEFINE_ENV_SAMPLED(EnvType) \
    template void nig::launch_rollout_sampled_env<nig::EnvType>(int, const nig::RolloutArgs &, uint32_t, unsigned, hipStream_t);
#define NIG_DEFINE_ENV_ENSEMBLE(EnvType) \
    template void nig::launch_mlp_ensemble_env<nig::EnvType>(int, const nig::MlpEnsArgs &, unsigned, hipStream_t);
#define NIG_DEFINE_ENV_DISTURBED(EnvType) \
    template void nig::launch_policy_disturbed_env<nig::EnvType>(const nig::PolicyDistArgs &, unsigned, hipStream_t); \
    template void nig::launch_mlp_disturbed_env<nig::EnvType>(const nig::MlpDistArgs &, unsigned, hipStream_t);
#define NIG_DEFINE_ENV_SEARCH(EnvType) \
    template void nig::launch_mlp_search_env<nig::EnvType>(const nig::MlpSearchArgs &, unsigned, hipStream_t);
#define NIG_DEFINE_ENV_GATED(EnvType) \
    template void nig::launch_mlp_gated_env<nig::EnvType>(const nig::MlpGateArgs &, unsigned, hipStream_t);
#define NIG_DEFINE_ENV_PROJECTED(EnvType) \
    template void nig::launch_mlp_projected_env<nig::EnvType>(const nig::MlpProjectArgs &, unsigned, hipStream_t);
#define NIG_DEFINE_ENV_BF16(EnvType) \
    template void nig::launch_mlp_bf16_env<nig::EnvType>(const nig::MlpBf16Args &, unsigned, hipStream_t);
#define NIG_DEFINE_ENV_LIMITED(EnvType) \
    template void nig::launch_step_limited_env<nig::EnvType>(const nig::StepLimArgs &, bool, unsigned, hipStream_t); \
    template void nig::launch_step64_limited_env<nig::EnvType>(const nig::StepLimArgs &, bool, unsigned, hipStream_t); \
    template void nig::launch_policy_limited_env<nig::EnvType>(const nig::PolicyLimArgs &, unsigned, hipStream_t); \
    template void nig::launch_mlp_limited_env<nig::EnvType>(const nig::MlpLimArgs &, unsigned, hipStream_t);
#define NIG_DEFINE_ENV_SHIELD_LIMITED(EnvType) \
    template void nig::launch_mlp_shield_limited_env<nig::EnvType>(const nig::MlpLimited<nig::MlpShieldArgs> &, unsigned, hipStream_t);
#define NIG_DEFINE_ENV_SEARCH_LIMITED(EnvType) \
    template void nig::launch_mlp_search_limited_env<nig::EnvType>(const nig::MlpLimited<nig::MlpSearchArgs> &, unsigned, hipStream_t);
#define NIG_DEFINE_ENV_GATED_LIMITED(EnvType) \
    template void nig::launch_mlp_gated_limited_env<nig::EnvType>(const nig::MlpLimited<nig::MlpGateArgs> &, unsigned, hipStream_t);
#define NIG_DEFINE_ENV_PROJECTED_LIMITED(EnvType) \
    template void nig::launch_mlp_projected_limited_env<nig::EnvType>(const nig::MlpLimited<nig::MlpProjectArgs> &, unsigned, hipStream_t);
#define NIG_DEFINE_ENV_ENSEMBLE_LIMITED(EnvType) \
    template void nig::launch_mlp_ensemble_limited_env<nig::EnvType>(int, const nig::MlpLimited<nig::MlpEnsArgs> &, unsigned, hipStream_t);
#define NIG_DEFINE_ENV_DISTURBED_LIMITED(EnvType) \
    template void nig::launch_policy_disturbed_limited_env<nig::EnvType>(const nig::PolicyDistLimArgs &, unsigned, hipStream_t); \
    template void nig::launch_mlp_disturbed_limited_env<nig::EnvType>(const nig::MlpLimited<nig::MlpDistArgs> &, unsigned, hipStream_t);
