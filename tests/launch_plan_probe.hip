// launch_plan_probe.hip -- TEST ONLY (tests/test_launch_plan.py): the library's own launch planner on the host.  Compiled
// host-only (hipcc --cuda-host-only), runs without a device and launches nothing.  Reads one case per line from stdin and
// prints, with the traits and the wrappers nig_launch.hpp itself uses, the plan's segments and the row-major-ring answer:
//   R <env> <out_mode> <B> <plain|noreset|held> <split_blocks> <wide_min_blocks>
//       -> "<rows_native> <256-lane blocks covered> <form>:<block0>:<grid> ..."    (planned as launch_rollout_paired's main launch)
//   P <env> <affine 0|1> <obs stream 0|1> <B> <plain|noreset|held> <split_blocks>
//       -> "- <256-lane blocks covered> <form>:<block0>:<grid> ..."
//   T <env>
//       -> "<WIDE_ROLLOUT_BLOCK or 0> <A> <pair_rollout> <pair_reg>"
#include <iostream>
#include <string>

#include "nig_launch.hpp"

using namespace nig;

static const char *form_name(Form f)
{
    switch (f) {
    case Form::OneWaveFull: return "one_wave_full";
    case Form::OneWaveRagged: return "one_wave_ragged";
    case Form::ThreeWave: return "three_wave";
    case Form::Wide: return "wide";
    case Form::Wide256: return "wide_256";
    case Form::PairedReg: return "paired_reg";
    case Form::PairedLds: return "paired_lds";
    }
    return "?";
}

static uint32_t handle_flags(const std::string &kind)
{
    if (kind == "plain") return NIG_F_AUTORESET;
    if (kind == "held") return NIG_F_AUTORESET | HF_MAY_HOLD_DONE;
    return 0u;
}

static void print_plan(const LaunchPlan &plan)
{
    std::cout << ' ' << plan.next;
    for (const Segment &s : plan) std::cout << ' ' << form_name(s.form) << ':' << s.block0 << ':' << s.grid;
    std::cout << '\n';
}

// RobotAssembly as a -DNIG_RA_SPLIT_ROUNDS=true diagnostic build sees it ("rar"): the closed loop's BIG layout must still keep it
// to a single round
struct RobotAssemblyRounds : PlanTraits<RobotAssembly> { static constexpr bool split_rounds = true; };

template <class Env, class E = PlanTraits<Env>>
static void one_case(char what)
{
    std::string kind;
    if (what == 'T') {
        std::cout << E::wide_rollout << ' ' << Env::A << ' ' << E::pair_rollout << ' ' << paired_stepper_reg(0) << '\n';
    } else if (what == 'R') {
        int out_mode;
        RolloutArgs q = {};
        std::cin >> out_mode >> q.s.B >> kind >> q.s.split_blocks >> q.s.wide_min_blocks;
        q.s.hflags = handle_flags(kind);
        std::cout << rollout_rows_native<Env>(out_mode, q);
        print_plan(plan_rollout<E>(Env::SHARED_STEP_BLOCK, false, out_mode, q.s.B, q.s.hflags, q.s.split_blocks, q.s.wide_min_blocks));
    } else {
        int affine, obs;
        uint32_t B, split_blocks;
        std::cin >> affine >> obs >> B >> kind >> split_blocks;
        std::cout << '-';
        print_plan(plan_policy<E>(affine != 0, obs != 0, B, handle_flags(kind), split_blocks));
    }
}

int main()
{
    char what;
    std::string env;
    while (std::cin >> what >> env) {
        if (env == "rar") one_case<RobotAssembly, RobotAssemblyRounds>(what);
#define NIG_PROBE_CASE(EnvType, key, id) else if (env == #key) one_case<EnvType>(what);
        NIG_ENV_LIST(NIG_PROBE_CASE)       // the library's own list of environments, by the key of their translation units
#undef NIG_PROBE_CASE
        else return 2;
    }
    return 0;
}
