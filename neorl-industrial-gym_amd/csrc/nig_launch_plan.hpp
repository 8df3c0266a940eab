// nig_launch_plan.hpp -- which kernel form every 256-lane block of a rollout launch runs: the ONE statement of that policy.
//
// Plain C++17, no HIP: nig_launch.hpp fills the traits from the Env structs and launches the plan's segments, its
// rollout_rows_native asks the plan which action layout the kernels read, and tests/launch_plan_probe.hip calls the same
// functions on the host (tests/test_launch_plan.py).  A threshold lives in exactly one function here, with the measurement
// that sets it.
#pragma once
#include <cstdint>

namespace nig {

enum class Form : uint8_t {
    OneWaveFull,      // rollout_kernel FULL: whole blocks without lane predication
    OneWaveRagged,    // rollout_kernel with lane predication: a ragged last block; rollout_policy_kernel, which has that form only
    ThreeWave,        // producer / integrator / recorder wave per 64 lanes (nig_split.hpp, nig_split_policy.hpp)
    Wide,             // the LDS-resident body in blocks of WIDE_ROLLOUT_BLOCK lanes (nig_pg_lds.hpp)
    Wide256,          // the same body in 256-lane blocks
    PairedReg,        // stepping + producer wave per 64 lanes, register-resident stepper (reads [A][ld] action rows)
    PairedLds,        // ... LDS-resident stepper
};

// the forms that read a lane's actions as contiguous bytes (a row-major action ring in place)
constexpr bool reads_lane_bytes(Form f) { return f == Form::Wide || f == Form::Wide256 || f == Form::PairedLds; }

// What the plan reads of an environment: a traits type E with the static constexpr members
//   bool split_rollout, split_rounds, pair_rollout;  int wide_rollout (WIDE_ROLLOUT_BLOCK, 0: the env has no wide form);
//   bool ks0 (no step noise), shared_step_block (steps 2k-1, 2k share one generator block), split_policy_big (SplitPolicyLds::BIG)
// -- nig_launch.hpp PlanTraits<Env> fills them from the Env structs.

struct Segment {
    Form form;
    uint32_t block0, grid;        // first 256-lane block; thread blocks of the form's own size
};

struct LaunchPlan {
    Segment seg[4] = {};
    int n = 0;
    uint32_t next = 0;            // first 256-lane block no segment covers yet
    constexpr void add(Form f, uint32_t grid, uint32_t blocks) { seg[n++] = Segment{f, next, grid}; next += blocks; }
    constexpr const Segment *begin() const { return seg; }
    constexpr const Segment *end() const { return seg + n; }
};

constexpr uint32_t PLAN_BLOCK = 256;
constexpr uint32_t PLAN_F_AUTORESET = 0x1u, PLAN_HF_MAY_HOLD_DONE = 0x10000u;     // NIG_F_AUTORESET, HF_MAY_HOLD_DONE (nig_launch.hpp asserts)

// an auto-reset handle on which no lane can be frozen: every form but the one-wave kernels needs it
constexpr bool plain_handle(uint32_t hflags) { return (hflags & PLAN_F_AUTORESET) != 0 && (hflags & PLAN_HF_MAY_HOLD_DONE) == 0; }

// Up to nig_tune(NIG_TUNE_SPLIT_BLOCKS) whole 256-lane blocks (default: one per compute unit, all resident at once) the batch
// leaves a single wave on every SIMD: producer / integrator / recorder wave per 64 lanes instead, or PowerGrid's paired form.
// Larger batches run the three-wave form in ROUNDS of one block per CU where the caller
// allows it (`rounds`), which beats the one-wave form (lanes filling the SIMDs) by 4-12 % when the rounds come out even --
// measured at 2, 3, 4, 8 and 16 rounds, profiles/r02/rounds_probe.txt -- and loses when the last round is mostly empty
// (1.5 rounds: -8 %): used when the last round is at least 3/4 full.
constexpr bool fits_rounds(uint32_t n_full, uint32_t per_round, bool rounds)
{
    if (n_full == 0 || per_round == 0) return false;
    if (n_full <= per_round) return true;
    const uint32_t last_round = n_full % per_round;
    return rounds && (last_round == 0 || 4u * last_round >= 3u * per_round);
}

#ifdef NIG_DIAG_PG_PAIR_LDS            // (diagnostic builds only: round 3's LDS-resident stepping waves, for same-box A/Bs)
constexpr bool PG_PAIR_REG = false;
#else
constexpr bool PG_PAIR_REG = true;
#endif
// The paired form's stepper per output mode -- the plan names it in the segment's form, the launcher instantiates that kernel.
// With an observation trajectory the LDS-resident stepping body stays: its state
// image IS the transposing image of the row-major rows; the register body pays an extra LDS round trip for them -- same box,
// 65 536 lanes x 250 steps: reward + flags 665 -> 582 us, no outputs 643 -> 557 us with registers, but full outputs
// 687 -> 774 us: profiles/r04/pg_pair_reg_ab.txt
constexpr bool paired_stepper_reg(int out_mode) { return PG_PAIR_REG && out_mode <= 1; }

// nig_rollout / nig_rollout_sampled / nig_rollout_noise.  paired: the launch starts on an odd counter of an env whose step pairs
// share a generator block; noise: injected draws; out_mode 0 none, 1 reward + flags, 2 / 3 + the observation trajectory.
// The batch's whole 256-lane blocks without lane predication, a ragged last block in a launch of its own.
template <class E>
constexpr LaunchPlan plan_rollout(bool paired, bool noise, int out_mode, uint32_t B, uint32_t hflags, uint32_t split_blocks,
                                  uint32_t wide_min_blocks)
{
    LaunchPlan p;
    const uint32_t n_full = B / PLAN_BLOCK;
    const bool plain = plain_handle(hflags);
    // Three-wave rounds beyond the first only for launches that write an observation trajectory (out_mode >= 2).  A round takes
    // the three-wave pipeline's ~142 us per 250 steps whatever it writes, so with reward + flags or no outputs the rounds LOSE to
    // lanes filling the SIMDs -- 131 072 lanes 280 vs 214-231 us, 262 144 lanes 555 vs 384-409 us, 1 048 576 lanes 2.20 vs
    // 1.31-1.46 ms -- while with the trajectory (HBM-bound either way) they win by 6-15 % (335 vs 378 us, 680 vs 726 us,
    // 3.30 vs 3.72 ms; profiles/r05/cr_rounds_by_output_mode.txt).
    // (Not for the LAST, partial residency round of a RobotAssembly batch either -- 262 144 lanes = 768 blocks one-wave + 256
    // three-wave, two launches: slower, full outputs 1 857-1 877 vs 1 842-1 863 us, reward + flags 1 590 vs 1 464, none 1 559 vs
    // 1 427 (profiles/r05/ra_tail_round_three_wave_ab.txt): one launch lets the tail's blocks start as compute units free up, two
    // launches drain the chip in between.)
    if (E::split_rollout && (paired || E::ks0 || noise) && plain &&
        fits_rounds(n_full, split_blocks, E::split_rounds && (out_mode >= 2 || noise))) {
        p.add(Form::ThreeWave, n_full, n_full);
    } else if (!paired && E::wide_rollout != 0 && plain && wide_min_blocks < (1u << 30)) {
        // Envs with an LDS-resident rollout body (PowerGrid): from nig_tune(NIG_TUNE_WIDE_MIN_BLOCKS) wide blocks up, the batch's
        // whole 512-lane blocks in the wide form (four waves per SIMD); a remaining whole 256-lane block, and every whole block of
        // a smaller batch, in the same body with 256-thread blocks (three blocks per CU by LDS: 262 144 lanes would need 1.33
        // rounds, which is why big batches take the wide form; small ones spread over more CUs this way and still run ~7 % fewer
        // instructions than the register-resident kernel, without its spills: 65 536 lanes 927 -> 858 us, 98 304 lanes
        // 1.29 -> 1.08 ms per 250 steps, profiles/r03/pg_small.txt).  A knob value of 2^30 or more keeps everything on rollout_kernel.
        const uint32_t n_wide = B / (uint32_t)E::wide_rollout;
        if (n_wide > 0 && n_wide >= wide_min_blocks) p.add(Form::Wide, n_wide, n_wide * ((uint32_t)E::wide_rollout / PLAN_BLOCK));
        // below the wide form, one round: a producer wave draws the step's normals beside every stepping wave
        if (E::pair_rollout && p.next == 0 && fits_rounds(n_full, split_blocks, false))
            p.add(paired_stepper_reg(out_mode) ? Form::PairedReg : Form::PairedLds, n_full, n_full);
        if (n_full > p.next) p.add(Form::Wide256, n_full - p.next, n_full - p.next);
    }
    if (n_full > p.next) p.add(Form::OneWaveFull, n_full - p.next, n_full - p.next);
    if (B % PLAN_BLOCK) p.add(Form::OneWaveRagged, 1u, 1u);
    return p;
}

// nig_rollout_policy.  The one-wave closed-loop kernel has the predicated form only.
template <class E>
constexpr LaunchPlan plan_policy(bool affine, bool obs_stream, uint32_t B, uint32_t hflags, uint32_t split_blocks)
{
    LaunchPlan p;
    const uint32_t n_full = B / PLAN_BLOCK;
    const bool plain = plain_handle(hflags);
    // The three-wave closed loop for the batch's whole 256-lane blocks: beyond one round only for calls that write the observation
    // stream, as in the open loop, and only up to TWO rounds: a closed-loop round takes ~1 us per step whatever it writes, lanes
    // filling the SIMDs take 1.75 / 2.5 us per step at 131 072 / 262 144 lanes without the stream and 1.97 / 3.25 with it -- two
    // rounds 1.84, four rounds 3.72: profiles/r05/policy_rounds_cr.txt.  The BIG layout (RobotAssembly, S = 24): a single round
    // only, as in the open loop.
    if constexpr (E::split_rollout && (E::shared_step_block || E::ks0)) {
        const bool rounds = !E::split_policy_big && E::split_rounds && obs_stream && n_full <= 2u * split_blocks;
        if (plain && fits_rounds(n_full, split_blocks, rounds)) p.add(Form::ThreeWave, n_full, n_full);
    }
    // PowerGrid, affine policies, the open loop's paired-form regime.  PID policies keep their memory in registers: one-wave kernel.
    if (p.n == 0 && E::pair_rollout && plain && affine && fits_rounds(n_full, split_blocks, false))
        p.add(Form::PairedReg, n_full, n_full);
    const uint32_t all = (B + PLAN_BLOCK - 1) / PLAN_BLOCK;    // everything else in one launch; after the forms above, a ragged block
    if (all > p.next) p.add(Form::OneWaveRagged, all - p.next, all - p.next);
    return p;
}

// nig_rollout_policy_disturbed: always the one-wave closed-loop kernel, at every batch size -- whole blocks and the ragged last
// block in one launch, as plan_policy's last segment.  The three-wave and paired PowerGrid closed loops have no disturbed twin.
constexpr LaunchPlan plan_policy_disturbed(uint32_t B)
{
    LaunchPlan p;
    const uint32_t all = (B + PLAN_BLOCK - 1) / PLAN_BLOCK;
    if (all > 0) p.add(Form::OneWaveRagged, all, all);
    return p;
}

}  // namespace nig
