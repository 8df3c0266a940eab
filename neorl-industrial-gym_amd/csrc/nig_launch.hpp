// nig_launch.hpp -- the host side of libnig.so's kernels: the list of environments and the per-environment launch table.  An
// env_<key>.hip instantiates the env's kernels by defining its table (NIG_DEFINE_ENV_LAUNCH); nig_api.hip reaches them through the
// table's function pointers only.  The launchers of the kernel families with translation units of their own (sampled_, ensemble_,
// disturbed_, search_, gated_, projected_, bf16_, categorical_, shape*_, ln_, ln_shield_, limited_, limited_<family>_<key>.hip) are DECLARED here and defined in
// nig_launch_families.hpp, which those units alone include: one function template per kind of family, keyed by the argument-block
// type, so that a family and its _limited twin are two instantiations of one launcher and two neighbouring slots of the table.
// Which kernel form a rollout launch takes is decided in nig_launch_plan.hpp; the functions here run its plans.
#pragma once
#include "nig_kernels.hpp"
#include "nig_launch_plan.hpp"

// The environments, once, in id order: (type in nig_envs.hpp, key of its translation units and of nig_launch_<key>(), id in nig.h).
// From it: nig_api.hip's spec rows, names ("<type>-v0") and launch tables; the declarations below; tests/launch_plan_probe.hip's dispatch.
#define NIG_ENV_LIST(X)                                                                                         \
    X(ChemicalReactor, cr, NIG_ENV_CHEMICAL_REACTOR) X(PowerGrid, pg, NIG_ENV_POWER_GRID)                       \
    X(RobotAssembly, ra, NIG_ENV_ROBOT_ASSEMBLY) X(AdvancedChemicalReactor, acr, NIG_ENV_ADV_CHEMICAL_REACTOR)  \
    X(AdvancedPowerGrid, apg, NIG_ENV_ADV_POWER_GRID) X(HVACControl, hvac, NIG_ENV_HVAC_CONTROL)                \
    X(WaterTreatment, water, NIG_ENV_WATER_TREATMENT) X(SteelAnnealing, steel, NIG_ENV_STEEL_ANNEALING)         \
    X(SupplyChain, supply, NIG_ENV_SUPPLY_CHAIN)

namespace nig {

// an entry's position in the list is its NIG_ENV_* id and its struct's ID: the tables built from the list are indexed by env id
#define NIG_ENV_POSITION(EnvType, key, id) list_position_##key,
enum { NIG_ENV_LIST(NIG_ENV_POSITION) list_length };
#undef NIG_ENV_POSITION
#define NIG_ENV_CHECK(EnvType, key, id) \
    static_assert(list_position_##key == id && EnvType::ID == id, "NIG_ENV_LIST: " #EnvType " is not at the position of " #id);
NIG_ENV_LIST(NIG_ENV_CHECK)
#undef NIG_ENV_CHECK
static_assert(list_length == NIG_NUM_ENVS);

struct EnvLaunch {
    // the env's own translation unit, env_<key>.hip (defined below)
    void (*step)(const StepArgs &, bool parity, unsigned grid, hipStream_t);
    void (*step64)(const StepArgs &, bool parity, unsigned grid, hipStream_t);   // float64 action rows; nullptr: the env takes float32
    void (*reset)(const ResetArgs &, bool parity, unsigned grid, hipStream_t);
    void (*fill)(float *act, int64_t ld_act, int64_t B, uint64_t env0, uint32_t seed_lo, uint32_t seed_hi, uint32_t t,
                 unsigned grid, hipStream_t);
    void (*rollout)(int out_mode, const RolloutArgs &, uint32_t t0, unsigned grid, hipStream_t);
    // does `rollout` read a ROW-MAJOR action ring ([B][A] slots, RolloutArgs.s.ld_act == 0) natively for this request?
    bool (*rows_native)(int out_mode, const RolloutArgs &);
    void (*policy)(const PolicyArgs &, unsigned grid, hipStream_t);
    void (*mlp)(const MlpArgs &, unsigned grid, hipStream_t);                // nullptr: the env has no MFMA actor (has_mlp_actor)
    void (*mlp_shield)(const MlpShieldArgs &, unsigned grid, hipStream_t);   // the same with the safety-critic shield; nullptr as `mlp`
    // sampled_<key>.hip (nig_launch_families.hpp): nig_rollout_sampled
    void (*rollout_sampled)(int out_mode, const RolloutArgs &, uint32_t t0, unsigned grid, hipStream_t);
    // The families in units of their own, each beside its twin under the added constraints (nig_<entry point>_limited; the twins
    // of the env's own kernels come first).  An mlp_ slot is nullptr as `mlp`, step64_limited as `step64`; every _limited slot is
    // nullptr for an env that overrides step() wholesale (the Advanced pair).
    // limited_<key>.hip
    void (*step_limited)(const StepLimArgs &, bool parity, unsigned grid, hipStream_t);
    void (*step64_limited)(const StepLimArgs &, bool parity, unsigned grid, hipStream_t);
    void (*policy_limited)(const PolicyLimArgs &, unsigned grid, hipStream_t);
    void (*mlp_limited)(const MlpLimArgs &, unsigned grid, hipStream_t);
    // limited_shield_<key>.hip
    void (*mlp_shield_limited)(const MlpLimited<MlpShieldArgs> &, unsigned grid, hipStream_t);
    // ensemble_<key>.hip, limited_ensemble_<key>.hip: nig_rollout_mlp_ensemble
    void (*mlp_ensemble)(int ens, const MlpEnsArgs &, unsigned grid, hipStream_t);
    void (*mlp_ensemble_limited)(int ens, const MlpLimited<MlpEnsArgs> &, unsigned grid, hipStream_t);
    // disturbed_<key>.hip, limited_disturbed_<key>.hip: nig_rollout_policy_disturbed, nig_rollout_mlp_disturbed
    void (*policy_disturbed)(const PolicyDistArgs &, unsigned grid, hipStream_t);
    void (*policy_disturbed_limited)(const PolicyDistLimArgs &, unsigned grid, hipStream_t);
    void (*mlp_disturbed)(const MlpDistArgs &, unsigned grid, hipStream_t);
    void (*mlp_disturbed_limited)(const MlpLimited<MlpDistArgs> &, unsigned grid, hipStream_t);
    // search_<key>.hip, limited_search_<key>.hip: nig_rollout_mlp_search
    void (*mlp_search)(const MlpSearchArgs &, unsigned grid, hipStream_t);
    void (*mlp_search_limited)(const MlpLimited<MlpSearchArgs> &, unsigned grid, hipStream_t);
    // gated_<key>.hip, limited_gated_<key>.hip: nig_rollout_mlp_gated
    void (*mlp_gated)(const MlpGateArgs &, unsigned grid, hipStream_t);
    void (*mlp_gated_limited)(const MlpLimited<MlpGateArgs> &, unsigned grid, hipStream_t);
    // projected_<key>.hip, limited_projected_<key>.hip: nig_rollout_mlp_projected
    void (*mlp_projected)(const MlpProjectArgs &, unsigned grid, hipStream_t);
    void (*mlp_projected_limited)(const MlpLimited<MlpProjectArgs> &, unsigned grid, hipStream_t);
    // bf16_<key>.hip: nig_rollout_mlp_bf16
    void (*mlp_bf16)(const MlpBf16Args &, unsigned grid, hipStream_t);
    // categorical_<key>.hip, limited_categorical_<key>.hip ("nig-categorical-v1"): what nig_rollout_mlp_safe / _search and their
    // twins launch when the handle's critic is the distributional one, and nig_mlp_violation_prob's kernel
    void (*mlp_cat_shield)(const MlpCatShieldArgs &, unsigned grid, hipStream_t);
    void (*mlp_cat_shield_limited)(const MlpLimited<MlpCatShieldArgs> &, unsigned grid, hipStream_t);
    void (*mlp_cat_search)(const MlpCatSearchArgs &, unsigned grid, hipStream_t);
    void (*mlp_cat_search_limited)(const MlpLimited<MlpCatSearchArgs> &, unsigned grid, hipStream_t);
    void (*mlp_cat_eval)(const MlpCatEvalArgs &, unsigned grid, hipStream_t);
    // shape128_<key>.hip, shape512x256_<key>.hip, shape512_<key>.hip, shape3_<key>.hip ("nig-mlp-shape-v1"): what nig_rollout_mlp
    // launches when the handle's actor slot holds a shaped actor of that class
    void (*mlp_shape128)(const MlpShapeArgs<Shape128> &, unsigned grid, hipStream_t);
    void (*mlp_shape512x256)(const MlpShapeArgs<Shape512x256> &, unsigned grid, hipStream_t);
    void (*mlp_shape512)(const MlpShapeArgs<Shape512> &, unsigned grid, hipStream_t);
    void (*mlp_shape3)(const MlpShapeArgs<Shape3> &, unsigned grid, hipStream_t);
    // shape128_shield_<key>.hip .. shape3_shield_<key>.hip ("nig-mlp-shape-shield-v1"): what nig_rollout_mlp_safe launches when the
    // actor slot and the critic slot hold shaped networks of the same class
    void (*mlp_shape128_shield)(const MlpShapeShieldArgs<Shape128> &, unsigned grid, hipStream_t);
    void (*mlp_shape512x256_shield)(const MlpShapeShieldArgs<Shape512x256> &, unsigned grid, hipStream_t);
    void (*mlp_shape512_shield)(const MlpShapeShieldArgs<Shape512> &, unsigned grid, hipStream_t);
    void (*mlp_shape3_shield)(const MlpShapeShieldArgs<Shape3> &, unsigned grid, hipStream_t);
    // ln_<key>.hip ("nig-mlp-ln-v1"): what nig_rollout_mlp launches when the slot holds a LayerNorm actor
    void (*mlp_ln)(const MlpLnArgs &, unsigned grid, hipStream_t);
    // ln_shield_<key>.hip ("nig-mlp-ln-shield-v1"): what nig_rollout_mlp_safe launches when both slots hold LayerNorm networks
    void (*mlp_ln_shield)(const MlpLnShieldArgs &, unsigned grid, hipStream_t);
};

template <class Env>
static void launch_reset(const ResetArgs &a, bool parity, unsigned grid, hipStream_t st)
{
    if (parity) hipLaunchKernelGGL((reset_kernel<Env, true>), dim3(grid), dim3(BLOCK), 0, st, a);
    else hipLaunchKernelGGL((reset_kernel<Env, false>), dim3(grid), dim3(BLOCK), 0, st, a);
}

// The MFMA actor's kernels that differ in their argument type alone, by that type, and their one launcher: the kernel is compiled
// only for an env that has the actor.  (The ensemble's launcher chooses between two kernels at run time: nig_launch_families.hpp.)
template <class Env> constexpr auto mlp_kernel(const MlpArgs &) { return rollout_mlp_kernel<Env>; }
template <class Env> constexpr auto mlp_kernel(const MlpShieldArgs &) { return rollout_mlp_shield_kernel<Env>; }
template <class Env> constexpr auto mlp_kernel(const MlpDistArgs &) { return rollout_mlp_disturbed_kernel<Env>; }
template <class Env> constexpr auto mlp_kernel(const MlpSearchArgs &) { return rollout_mlp_search_kernel<Env>; }
template <class Env> constexpr auto mlp_kernel(const MlpGateArgs &) { return rollout_mlp_gated_kernel<Env>; }
template <class Env> constexpr auto mlp_kernel(const MlpProjectArgs &) { return rollout_mlp_projected_kernel<Env>; }
template <class Env> constexpr auto mlp_kernel(const MlpLimArgs &) { return rollout_mlp_limited_kernel<Env>; }
template <class Env> constexpr auto mlp_kernel(const MlpLimited<MlpShieldArgs> &) { return rollout_mlp_shield_limited_kernel<Env>; }
template <class Env> constexpr auto mlp_kernel(const MlpLimited<MlpSearchArgs> &) { return rollout_mlp_search_limited_kernel<Env>; }
template <class Env> constexpr auto mlp_kernel(const MlpLimited<MlpGateArgs> &) { return rollout_mlp_gated_limited_kernel<Env>; }
template <class Env> constexpr auto mlp_kernel(const MlpLimited<MlpProjectArgs> &) { return rollout_mlp_projected_limited_kernel<Env>; }
template <class Env> constexpr auto mlp_kernel(const MlpLimited<MlpDistArgs> &) { return rollout_mlp_disturbed_limited_kernel<Env>; }
template <class Env> constexpr auto mlp_kernel(const MlpBf16Args &) { return rollout_mlp_bf16_kernel<Env>; }
template <class Env> constexpr auto mlp_kernel(const MlpCatShieldArgs &) { return rollout_mlp_cat_shield_kernel<Env>; }
template <class Env> constexpr auto mlp_kernel(const MlpCatSearchArgs &) { return rollout_mlp_cat_search_kernel<Env>; }
template <class Env> constexpr auto mlp_kernel(const MlpLimited<MlpCatShieldArgs> &) { return rollout_mlp_cat_shield_limited_kernel<Env>; }
template <class Env> constexpr auto mlp_kernel(const MlpLimited<MlpCatSearchArgs> &) { return rollout_mlp_cat_search_limited_kernel<Env>; }
template <class Env> constexpr auto mlp_kernel(const MlpCatEvalArgs &) { return mlp_violation_prob_kernel<Env>; }
template <class Env, class Shape> constexpr auto mlp_kernel(const MlpShapeArgs<Shape> &) { return rollout_mlp_shape_kernel<Env, Shape>; }
template <class Env, class Shape> constexpr auto mlp_kernel(const MlpShapeShieldArgs<Shape> &) { return rollout_mlp_shape_shield_kernel<Env, Shape>; }
template <class Env> constexpr auto mlp_kernel(const MlpLnArgs &) { return rollout_mlp_ln_kernel<Env>; }
template <class Env> constexpr auto mlp_kernel(const MlpLnShieldArgs &) { return rollout_mlp_ln_shield_kernel<Env>; }

template <class Env, class Args>
static void launch_mlp(const Args &q, unsigned grid, hipStream_t st)
{
    if constexpr (has_mlp_actor<Env>) hipLaunchKernelGGL(mlp_kernel<Env>(q), dim3(grid), dim3(BLOCK), 0, st, q);
}

// a table slot of the MFMA actor: null for an env without it, which is how nig_api.hip asks "is this shape supported"
template <class Env, class F>
constexpr F *mlp_slot(F *f) { return has_mlp_actor<Env> ? f : nullptr; }

template <class Env>
static void launch_step(const StepArgs &a, bool parity, unsigned grid, hipStream_t st)
{
    constexpr int FB = Env::STEP_BLOCK;
    if (parity) { hipLaunchKernelGGL((step_kernel<Env, true>), dim3(grid), dim3(BLOCK), 0, st, a); return; }
    if constexpr (Env::COOP_RESET) {
        // auto-reset handles whose batch leaves one wave per SIMD (up to nig_tune(NIG_TUNE_SPLIT_BLOCKS) 256-lane blocks, default
        // one per compute unit -- the knob of the three-wave rollout, the same regime): a helper wave per lane wave prepares
        // the restart states beside the step (step_kernel, HELP)
        if ((a.hflags & NIG_F_AUTORESET) != 0 && a.split_blocks != 0 && grid <= a.split_blocks) {
            hipLaunchKernelGGL((step_kernel<Env, false, false, BLOCK, true>), dim3(grid), dim3(2 * BLOCK), 0, st, a);
            return;
        }
    }
    if (FB != BLOCK && a.B > 768u * BLOCK)            // more 256-thread blocks than are resident at once (3 per CU)
        hipLaunchKernelGGL((step_kernel<Env, false, false, FB>), dim3((a.B + FB - 1) / FB), dim3(FB), 0, st, a);
    else hipLaunchKernelGGL((step_kernel<Env, false>), dim3(grid), dim3(BLOCK), 0, st, a);
}

template <class Env>
static void launch_step64(const StepArgs &a, bool parity, unsigned grid, hipStream_t st)
{
    if constexpr (Env::HAS_ACT64) {
        if (parity) hipLaunchKernelGGL((step_kernel<Env, true, true>), dim3(grid), dim3(BLOCK), 0, st, a);
        else hipLaunchKernelGGL((step_kernel<Env, false, true>), dim3(grid), dim3(BLOCK), 0, st, a);
    }
}

// The output mode as a template argument: the ONE place a run-time out_mode is switched on.  f is a generic callable taking
// std::integral_constant<int, 0..3>.
template <class F>
static void with_out_mode(int out_mode, F &&f)
{
    switch (out_mode) {
    case 0: f(std::integral_constant<int, 0>{}); break;
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    default: f(std::integral_constant<int, 3>{}); break;
    }
}

// (nig_launch_plan.hpp restates these three constants to stay free of HIP headers)
static_assert(PLAN_BLOCK == BLOCK && PLAN_F_AUTORESET == NIG_F_AUTORESET && PLAN_HF_MAY_HOLD_DONE == HF_MAY_HOLD_DONE);

template <class Env>
struct PlanTraits {
    static constexpr bool split_rollout = nig::split_rollout<Env>::value, split_rounds = nig::split_rounds<Env>::value;
    static constexpr bool pair_rollout = nig::pair_rollout<Env>::value, ks0 = Env::KS == 0, shared_step_block = Env::SHARED_STEP_BLOCK;
    static constexpr int wide_rollout = nig::wide_rollout<Env>::value;
    // (read by plan_policy for the three-wave envs only, for which the closed loop's LDS layout exists and fits)
    static constexpr bool split_policy_big = SplitPolicyLds<Env, BLOCK / 64>::BIG;
};

// One segment of a rollout plan.  Every form's kernels stay behind the trait that declares them: no env gains a kernel.
// NOISE: the injected-draw variants of nig_rollout_noise, instantiated for the row-major full-output mode only (OUT 3, what the
// headline configuration runs).  SAMPLED: nig_rollout_sampled -- the twin kernels that draw their actions (rollout_sampled_kernel,
// rollout_sampled_wide_kernel, split_sampled_kernel, pg_pair_sampled_kernel): the same plan, the kernel name is the only thing
// either flag changes.
template <class Env, bool PAIRED, bool NOISE, bool SAMPLED, int OUT>
static void launch_rollout_segment(const Segment &s, const RolloutArgs &r, hipStream_t st)
{
    const dim3 grid(s.grid);
    // (Every form: `if constexpr (SAMPLED) ... else ...`, so a sampled_*.hip unit instantiates the twins alone and each kernel
    // symbol of the library lives in exactly one code object.)
    auto one_wave = [&](auto FULL) {
        if constexpr (SAMPLED) hipLaunchKernelGGL((rollout_sampled_kernel<Env, OUT, PAIRED, FULL()>), grid, dim3(BLOCK), 0, st, r);
        else hipLaunchKernelGGL((rollout_kernel<Env, OUT, PAIRED, FULL(), NOISE>), grid, dim3(BLOCK), 0, st, r);
    };
    auto wide = [&](auto BLK) {
        if constexpr (SAMPLED) hipLaunchKernelGGL((rollout_sampled_wide_kernel<Env, OUT, BLK()>), grid, dim3(BLK()), 0, st, r);
        else hipLaunchKernelGGL((rollout_wide_kernel<Env, OUT, BLK(), NOISE>), grid, dim3(BLK()), 0, st, r);
    };
    constexpr bool WIDE = !PAIRED && wide_rollout<Env>::value != 0;
    switch (s.form) {
    case Form::OneWaveFull: one_wave(std::true_type{}); break;
    case Form::OneWaveRagged: one_wave(std::false_type{}); break;
    case Form::ThreeWave:
        if constexpr ((PAIRED || Env::KS == 0 || NOISE) && split_rollout<Env>::value)
            launch_split_blocks<Env, BLOCK / 64, OUT, NOISE, SAMPLED>(r, s.grid, st);
        break;
    case Form::Wide: if constexpr (WIDE) wide(std::integral_constant<int, wide_rollout<Env>::value>{}); break;
    case Form::Wide256: if constexpr (WIDE) wide(std::integral_constant<int, BLOCK>{}); break;
    case Form::PairedReg:
    case Form::PairedLds:
        if constexpr (WIDE && pair_rollout<Env>::value) {
            constexpr bool REG = paired_stepper_reg(OUT);      // (what the plan's form says: the same function of the same constant)
            if constexpr (SAMPLED) hipLaunchKernelGGL((pg_pair_sampled_kernel<OUT, REG>), grid, dim3(512), 0, st, r);
            else hipLaunchKernelGGL((rollout_pg_pair_kernel<OUT, NOISE, REG>), grid, dim3(512), 0, st, r);
        }
        break;
    }
}

template <class Env, bool PAIRED, bool NOISE = false, bool SAMPLED = false>
static void launch_rollout_form(int out_mode, const RolloutArgs &q, unsigned /*grid*/, hipStream_t st)
{
    const LaunchPlan plan = plan_rollout<PlanTraits<Env>>(PAIRED, NOISE, out_mode, q.s.B, q.s.hflags, q.s.split_blocks, q.s.wide_min_blocks);
    with_out_mode(out_mode, [&](auto MODE) {
        constexpr int OUT = NOISE ? 3 : MODE();    // (nig_rollout_noise accepts out_mode 3 only)
        RolloutArgs r = q;
        for (const Segment &s : plan) { r.block0 = s.block0; launch_rollout_segment<Env, PAIRED, NOISE, SAMPLED, OUT>(s, r, st); }
    });
}

// nig_rollout's row-major action ring (ld_act == 0): true when EVERY kernel launch_rollout_form<Env, false> starts for this
// request reads a lane's actions as contiguous bytes -- asked of the plan itself.  (A == 8: two 16-byte loads per lane.)
template <class Env>
static bool rollout_rows_native(int out_mode, const RolloutArgs &q)
{
    const LaunchPlan plan = plan_rollout<PlanTraits<Env>>(false, false, out_mode, q.s.B, q.s.hflags, q.s.split_blocks, q.s.wide_min_blocks);
    bool native = Env::A == 8 && plan.n > 0;
    for (const Segment &s : plan) native = native && reads_lane_bytes(s.form);
    return native;
}

// the envs the reference can record draws for (ChemicalReactor, PowerGrid, RobotAssembly): nig_rollout_noise
template <class Env> struct noise_rollout : std::bool_constant<(Env::ID <= 2)> {};

// t0 = launch counter of the call's first step (host-known: rollouts are never graph-captured)
template <class Env, bool SAMPLED>
static void launch_rollout_paired(int out_mode, const RolloutArgs &q, uint32_t t0, unsigned grid, hipStream_t st)
{
    if constexpr (Env::SHARED_STEP_BLOCK) {
        RolloutArgs r = q;
        if ((t0 & 1u) == 0u) {                    // starts on the second step of a pair: peel it
            r.n_steps = 1;
            launch_rollout_form<Env, false, false, SAMPLED>(out_mode, r, grid, st);
            if (q.n_steps == 1) return;
            r.n_steps = q.n_steps; r.it0 = 1;
        }
        launch_rollout_form<Env, true, false, SAMPLED>(out_mode, r, grid, st);
    } else {
        launch_rollout_form<Env, false, false, SAMPLED>(out_mode, q, grid, st);
    }
}

template <class Env>
static void launch_rollout_env(int out_mode, const RolloutArgs &q, uint32_t t0, unsigned grid, hipStream_t st)
{
    if (q.s.step_noise != nullptr || q.s.reset_noise != nullptr) {       // injected draws (nig_rollout_noise has validated the request)
        if constexpr (noise_rollout<Env>::value) launch_rollout_form<Env, false, true>(3, q, grid, st);
        return;
    }
    launch_rollout_paired<Env, false>(out_mode, q, t0, grid, st);
}

// The launchers of the kernel families in translation units of their own: declared here, defined in nig_launch_families.hpp.  A
// unit that includes this header alone -- env_*.hip, nig_api.hip, nig_mixed.hip -- can name them (the table below does) but cannot
// instantiate them, so the env_*.hip units hold exactly the instantiations they held before a family existed: their code objects do
// not move by an instruction (profiles/isa_diff.py), each kernel symbol of the library lives in one code object, and the families
// compile beside them in parallel.  A family and its _limited twin are one launcher on two argument-block types: the type names
// the kernel.
template <class Env> void launch_rollout_sampled_env(int out_mode, const RolloutArgs &q, uint32_t t0, unsigned grid, hipStream_t st);
template <class Env, class Args> void launch_mlp_family(const Args &q, unsigned grid, hipStream_t st);         // the MFMA families: mlp_kernel
template <class Env, class Args> void launch_policy_family(const Args &q, unsigned grid, hipStream_t st);      // the planned policy loops
template <class Env, class Args> void launch_ensemble_family(int ens, const Args &q, unsigned grid, hipStream_t st);
template <class Env, bool ACT64> void launch_step_limited(const StepLimArgs &q, bool parity, unsigned grid, hipStream_t st);

template <class Env>
static void launch_policy(const PolicyArgs &q, unsigned /*grid*/, hipStream_t st)
{
    const LaunchPlan plan = plan_policy<PlanTraits<Env>>(q.pol_kind == NIG_POLICY_AFFINE, q.obs_out != nullptr, q.s.B, q.s.hflags, q.s.split_blocks);
    PolicyArgs r = q;
    for (const Segment &s : plan) {
        void (*kernel)(const PolicyArgs) = rollout_policy_kernel<Env>;
        unsigned threads = BLOCK;
        // (RobotAssembly's observations of the transition stream ride in the BIG layout's P -> I slots)
        if constexpr (split_rollout<Env>::value && (Env::SHARED_STEP_BLOCK || Env::KS == 0))
            if (s.form == Form::ThreeWave) { kernel = split_policy_kernel<Env, BLOCK / 64>; threads = 192 * (BLOCK / 64); }
        if constexpr (pair_rollout<Env>::value)
            if (s.form == Form::PairedReg) { kernel = rollout_pg_pair_policy_kernel<PolicyArgs>; threads = 512; }
        r.block0 = s.block0;
        hipLaunchKernelGGL(kernel, dim3(s.grid), dim3(threads), 0, st, r);
    }
}

template <class Env>
static void launch_fill(float *act, int64_t ld_act, int64_t B, uint64_t env0, uint32_t seed_lo, uint32_t seed_hi, uint32_t t,
                        unsigned grid, hipStream_t st)
{
    hipLaunchKernelGGL((fill_actions_kernel<Env>), dim3(grid), dim3(BLOCK), 0, st, act, ld_act, B, env0, seed_lo, seed_hi, t);
}

// Filled by name: a member added to EnvLaunch moves no other.
template <class Env>
static const EnvLaunch *env_launch_table()
{
    static const EnvLaunch T = [] {
        EnvLaunch t = {};
        t.step = launch_step<Env>;
        t.step64 = Env::HAS_ACT64 ? launch_step64<Env> : nullptr;
        t.reset = launch_reset<Env>;
        t.fill = launch_fill<Env>;
        t.rollout = launch_rollout_env<Env>;
        t.rows_native = rollout_rows_native<Env>;
        t.policy = launch_policy<Env>;
        t.mlp = mlp_slot<Env>(launch_mlp<Env, MlpArgs>);
        t.mlp_shield = mlp_slot<Env>(launch_mlp<Env, MlpShieldArgs>);
        t.rollout_sampled = launch_rollout_sampled_env<Env>;
        t.mlp_ensemble = mlp_slot<Env>(launch_ensemble_family<Env, MlpEnsArgs>);
        t.policy_disturbed = launch_policy_family<Env, PolicyDistArgs>;
        t.mlp_disturbed = mlp_slot<Env>(launch_mlp_family<Env, MlpDistArgs>);
        t.mlp_search = mlp_slot<Env>(launch_mlp_family<Env, MlpSearchArgs>);
        t.mlp_gated = mlp_slot<Env>(launch_mlp_family<Env, MlpGateArgs>);
        t.mlp_projected = mlp_slot<Env>(launch_mlp_family<Env, MlpProjectArgs>);
        t.mlp_bf16 = mlp_slot<Env>(launch_mlp_family<Env, MlpBf16Args>);
        t.mlp_cat_shield = mlp_slot<Env>(launch_mlp_family<Env, MlpCatShieldArgs>);
        t.mlp_cat_search = mlp_slot<Env>(launch_mlp_family<Env, MlpCatSearchArgs>);
        t.mlp_cat_eval = mlp_slot<Env>(launch_mlp_family<Env, MlpCatEvalArgs>);
        t.mlp_ln = mlp_slot<Env>(launch_mlp_family<Env, MlpLnArgs>);
        t.mlp_ln_shield = mlp_slot<Env>(launch_mlp_family<Env, MlpLnShieldArgs>);
        if constexpr (has_mlp_actor<Env>) {           // (the shape units exist for the envs with the actor alone)
            t.mlp_shape128 = launch_mlp_family<Env, MlpShapeArgs<Shape128>>;
            t.mlp_shape512x256 = launch_mlp_family<Env, MlpShapeArgs<Shape512x256>>;
            t.mlp_shape512 = launch_mlp_family<Env, MlpShapeArgs<Shape512>>;
            t.mlp_shape3 = launch_mlp_family<Env, MlpShapeArgs<Shape3>>;
            t.mlp_shape128_shield = launch_mlp_family<Env, MlpShapeShieldArgs<Shape128>>;
            t.mlp_shape512x256_shield = launch_mlp_family<Env, MlpShapeShieldArgs<Shape512x256>>;
            t.mlp_shape512_shield = launch_mlp_family<Env, MlpShapeShieldArgs<Shape512>>;
            t.mlp_shape3_shield = launch_mlp_family<Env, MlpShapeShieldArgs<Shape3>>;
        }
        if constexpr (!Env::CUSTOM_STEP) {            // the twins: the same lines on the twin's argument block
            t.step_limited = launch_step_limited<Env, false>;
            t.step64_limited = Env::HAS_ACT64 ? launch_step_limited<Env, true> : nullptr;
            t.policy_limited = launch_policy_family<Env, PolicyLimArgs>;
            t.mlp_limited = mlp_slot<Env>(launch_mlp_family<Env, MlpLimArgs>);
            t.mlp_shield_limited = mlp_slot<Env>(launch_mlp_family<Env, MlpLimited<MlpShieldArgs>>);
            t.mlp_ensemble_limited = mlp_slot<Env>(launch_ensemble_family<Env, MlpLimited<MlpEnsArgs>>);
            t.policy_disturbed_limited = launch_policy_family<Env, PolicyDistLimArgs>;
            t.mlp_disturbed_limited = mlp_slot<Env>(launch_mlp_family<Env, MlpLimited<MlpDistArgs>>);
            t.mlp_search_limited = mlp_slot<Env>(launch_mlp_family<Env, MlpLimited<MlpSearchArgs>>);
            t.mlp_gated_limited = mlp_slot<Env>(launch_mlp_family<Env, MlpLimited<MlpGateArgs>>);
            t.mlp_projected_limited = mlp_slot<Env>(launch_mlp_family<Env, MlpLimited<MlpProjectArgs>>);
            t.mlp_cat_shield_limited = mlp_slot<Env>(launch_mlp_family<Env, MlpLimited<MlpCatShieldArgs>>);
            t.mlp_cat_search_limited = mlp_slot<Env>(launch_mlp_family<Env, MlpLimited<MlpCatSearchArgs>>);
        }
        return t;
    }();
    return &T;
}

// Mixed-batch launch (nig_mixed.hip): per-segment rollout arguments + the block -> segment table, in launch order.
constexpr int MIXED_MAX_SEG = NIG_MIXED_MAX_SEGMENTS;
struct MixedArgs {
    RolloutArgs seg[MIXED_MAX_SEG];
    uint32_t blk_end[MIXED_MAX_SEG];     // cumulative block count up to and including segment k
    int env[MIXED_MAX_SEG];
    int n_seg;
};
static_assert(sizeof(MixedArgs) <= 4000, "kernel argument segment is 4 KiB");

}  // namespace nig

// nig_mixed.hip
void nig_launch_mixed_rollout(int out_mode, const nig::MixedArgs &m, unsigned grid, hipStream_t st);

// the launch table of every environment, nig_launch_<key>(): defined by env_<key>.hip
#define NIG_ENV_DECLARE(EnvType, key, id) const nig::EnvLaunch *nig_launch_##key();
NIG_ENV_LIST(NIG_ENV_DECLARE)
#undef NIG_ENV_DECLARE
#define NIG_DEFINE_ENV_LAUNCH(EnvType, fn_name) \
    const nig::EnvLaunch *fn_name() { return nig::env_launch_table<nig::EnvType>(); }
