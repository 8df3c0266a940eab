// nig_launch_families.hpp -- the definitions of the family launchers nig_launch.hpp declares: the kernels of nig_rollout_sampled,
// nig_rollout_mlp_ensemble, nig_rollout_policy_disturbed / nig_rollout_mlp_disturbed, nig_rollout_mlp_search, nig_rollout_mlp_gated,
// nig_rollout_mlp_projected, nig_rollout_mlp_bf16, the shaped and the LayerNorm actor of nig_rollout_mlp, the LayerNorm and the shaped shield of nig_rollout_mlp_safe, and of every _limited entry point.  A launcher is stated once per kind of family,
// on the argument-block type: a family's parent and its _limited twin are two instantiations of it.
// Included by the family translation units alone (sampled_, ensemble_, disturbed_, search_, gated_, projected_, bf16_, categorical_, shape*_, shape*_shield_, ln_, ln_shield_, limited_,
// limited_<family>_<key>.hip).  A template that is defined but not instantiated emits nothing: each unit explicitly instantiates the
// launcher of its own family for its own env (the macros at the end), and with it that family's kernels and no other's.
#pragma once
#include "nig_launch.hpp"

namespace nig {

// nig_rollout_sampled: launch_rollout_env's selection on the twin kernels that draw their actions
template <class Env>
void launch_rollout_sampled_env(int out_mode, const RolloutArgs &q, uint32_t t0, unsigned grid, hipStream_t st)
{
    launch_rollout_paired<Env, true>(out_mode, q, t0, grid, st);
}

// the MFMA families (nig_launch.hpp: launch_mlp on the kernel mlp_kernel names for the argument block)
template <class Env, class Args>
void launch_mlp_family(const Args &q, unsigned grid, hipStream_t st) { launch_mlp<Env>(q, grid, st); }

// The policy loops beside nig_rollout_policy, by their argument block.  They have the one-wave form only (plan_policy_disturbed:
// whole blocks and a ragged last one): the three-wave and paired PowerGrid closed loops have no disturbed or limited twin.
template <class Env> constexpr auto policy_kernel(const PolicyDistArgs &) { return rollout_policy_disturbed_kernel<Env>; }
template <class Env> constexpr auto policy_kernel(const PolicyLimArgs &) { return rollout_policy_limited_kernel<Env>; }
template <class Env> constexpr auto policy_kernel(const PolicyDistLimArgs &) { return rollout_policy_disturbed_limited_kernel<Env>; }

template <class Env, class Args>
void launch_policy_family(const Args &q, unsigned /*grid*/, hipStream_t st)
{
    const LaunchPlan plan = plan_policy_disturbed(q.p.s.B);
    Args r = q;
    for (const Segment &s : plan) {
        r.p.block0 = s.block0;
        hipLaunchKernelGGL(policy_kernel<Env>(r), dim3(s.grid), dim3(BLOCK), 0, st, r);
    }
}

// nig_rollout_mlp_ensemble and its twin: one kernel per combination rule, chosen at run time
template <class Env, int ENS> constexpr auto ensemble_kernel(const MlpEnsArgs &) { return rollout_mlp_ensemble_kernel<Env, ENS>; }
template <class Env, int ENS> constexpr auto ensemble_kernel(const MlpLimited<MlpEnsArgs> &) { return rollout_mlp_ensemble_limited_kernel<Env, ENS>; }

template <class Env, class Args>
void launch_ensemble_family(int ens, const Args &q, unsigned grid, hipStream_t st)
{
    if constexpr (has_mlp_actor<Env>) {
        if (ens == ENS_AVERAGE) hipLaunchKernelGGL((ensemble_kernel<Env, ENS_AVERAGE>(q)), dim3(grid), dim3(BLOCK), 0, st, q);
        else hipLaunchKernelGGL((ensemble_kernel<Env, ENS_VOTING>(q)), dim3(grid), dim3(BLOCK), 0, st, q);
    }
}

// nig_step_limited / nig_step64_limited (ACT64: float64 action rows): one plain kernel form each (injected or generated draws)
template <class Env, bool ACT64>
void launch_step_limited(const StepLimArgs &q, bool parity, unsigned grid, hipStream_t st)
{
    if constexpr (!ACT64 || Env::HAS_ACT64) {
        if (parity) hipLaunchKernelGGL((step_limited_kernel<Env, true, ACT64>), dim3(grid), dim3(BLOCK), 0, st, q);
        else hipLaunchKernelGGL((step_limited_kernel<Env, false, ACT64>), dim3(grid), dim3(BLOCK), 0, st, q);
    }
}

}  // namespace nig

// The one line of a family translation unit: the explicit instantiation of its env's launcher(s), NIG_FAMILY(launcher, env, argument
// block) under the unit's name for it.
#define NIG_FAMILY(launcher, EnvType, Args) \
    namespace nig { template void launcher<EnvType, Args>(const Args &, unsigned, hipStream_t); }
#define NIG_FAMILY_ENSEMBLE(EnvType, Args) \
    namespace nig { template void launch_ensemble_family<EnvType, Args>(int, const Args &, unsigned, hipStream_t); }
#define NIG_DEFINE_ENV_SAMPLED(EnvType) \
    template void nig::launch_rollout_sampled_env<nig::EnvType>(int, const nig::RolloutArgs &, uint32_t, unsigned, hipStream_t);
#define NIG_DEFINE_ENV_ENSEMBLE(EnvType) NIG_FAMILY_ENSEMBLE(EnvType, MlpEnsArgs)
#define NIG_DEFINE_ENV_ENSEMBLE_LIMITED(EnvType) NIG_FAMILY_ENSEMBLE(EnvType, MlpLimited<MlpEnsArgs>)
#define NIG_DEFINE_ENV_DISTURBED(EnvType) \
    NIG_FAMILY(launch_policy_family, EnvType, PolicyDistArgs) NIG_FAMILY(launch_mlp_family, EnvType, MlpDistArgs)
#define NIG_DEFINE_ENV_DISTURBED_LIMITED(EnvType) \
    NIG_FAMILY(launch_policy_family, EnvType, PolicyDistLimArgs) NIG_FAMILY(launch_mlp_family, EnvType, MlpLimited<MlpDistArgs>)
#define NIG_DEFINE_ENV_SEARCH(EnvType) NIG_FAMILY(launch_mlp_family, EnvType, MlpSearchArgs)
#define NIG_DEFINE_ENV_SEARCH_LIMITED(EnvType) NIG_FAMILY(launch_mlp_family, EnvType, MlpLimited<MlpSearchArgs>)
#define NIG_DEFINE_ENV_GATED(EnvType) NIG_FAMILY(launch_mlp_family, EnvType, MlpGateArgs)
#define NIG_DEFINE_ENV_GATED_LIMITED(EnvType) NIG_FAMILY(launch_mlp_family, EnvType, MlpLimited<MlpGateArgs>)
#define NIG_DEFINE_ENV_PROJECTED(EnvType) NIG_FAMILY(launch_mlp_family, EnvType, MlpProjectArgs)
#define NIG_DEFINE_ENV_PROJECTED_LIMITED(EnvType) NIG_FAMILY(launch_mlp_family, EnvType, MlpLimited<MlpProjectArgs>)
#define NIG_DEFINE_ENV_BF16(EnvType) NIG_FAMILY(launch_mlp_family, EnvType, MlpBf16Args)
#define NIG_DEFINE_ENV_SHAPE(EnvType, Shape) NIG_FAMILY(launch_mlp_family, EnvType, MlpShapeArgs<Shape>)
#define NIG_DEFINE_ENV_SHAPE_SHIELD(EnvType, Shape) NIG_FAMILY(launch_mlp_family, EnvType, MlpShapeShieldArgs<Shape>)
#define NIG_DEFINE_ENV_LN(EnvType) NIG_FAMILY(launch_mlp_family, EnvType, MlpLnArgs)
#define NIG_DEFINE_ENV_LN_SHIELD(EnvType) NIG_FAMILY(launch_mlp_family, EnvType, MlpLnShieldArgs)
#define NIG_DEFINE_ENV_CATEGORICAL(EnvType) \
    NIG_FAMILY(launch_mlp_family, EnvType, MlpCatShieldArgs) NIG_FAMILY(launch_mlp_family, EnvType, MlpCatSearchArgs) \
    NIG_FAMILY(launch_mlp_family, EnvType, MlpCatEvalArgs)
#define NIG_DEFINE_ENV_CATEGORICAL_LIMITED(EnvType) \
    NIG_FAMILY(launch_mlp_family, EnvType, MlpLimited<MlpCatShieldArgs>) NIG_FAMILY(launch_mlp_family, EnvType, MlpLimited<MlpCatSearchArgs>)
#define NIG_DEFINE_ENV_SHIELD_LIMITED(EnvType) NIG_FAMILY(launch_mlp_family, EnvType, MlpLimited<MlpShieldArgs>)
#define NIG_DEFINE_ENV_LIMITED(EnvType) \
    template void nig::launch_step_limited<nig::EnvType, false>(const nig::StepLimArgs &, bool, unsigned, hipStream_t); \
    template void nig::launch_step_limited<nig::EnvType, true>(const nig::StepLimArgs &, bool, unsigned, hipStream_t); \
    NIG_FAMILY(launch_policy_family, EnvType, PolicyLimArgs) NIG_FAMILY(launch_mlp_family, EnvType, MlpLimArgs)
