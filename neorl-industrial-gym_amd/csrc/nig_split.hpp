// nig_split.hpp -- the fused rollout for batches that leave ONE wave per SIMD (included by nig_kernels.hpp).
//
// At BASELINE.json's headline size (65 536 lanes = 1024 waves on 1024 SIMDs) the rollout kernel is bound by what a
// single wave can issue: a lone wave gets one VALU instruction issued every 5-7 cycles where the SIMD could take
// one every ~2.5 (profiles/ubench/valu_rate.hip), and the lane-count probe (profiles/r02/scale_probe.txt) shows
// the same thing on the kernel itself -- twice the lanes cost 1.25x the time.  More lanes per SIMD are not
// available at that batch size, so this kernel puts THREE waves on every SIMD that work on the SAME 64
// environments, each with a third of IndustrialEnv.step:
//
//   producer   (P): what a step consumes.  Philox + normal transform of the process noise, action load + clip.
//                   Runs ahead of the integrator by up to the ring length.  Loads only, no stores.
//   integrator (I): owns the state.  Constraint check on the pre-state, dynamics, done / truncation, in-kernel
//                   reset.  Touches no global memory inside the loop.  The critical path of the three.
//   recorder   (C): what a step leaves behind.  Reward, penalties, flag word, episode tally, the transposed
//                   trajectory rows and ALL the stores.  Stores only, no loads: it never waits on vmcnt.
//
// They exchange through two rings of K slots in LDS, each guarded by a monotonically increasing counter (slots
// produced so far), plus the recorder's count of slots it is done with.  P -> I slot: the KS noise values and A
// clipped actions of one step, [row][lane].  I -> C slot: the S post-dynamics state values row-major [lane][S]
// (this IS the transposing image of the row-major trajectory) plus one word with the violation bits of the pre-state and
// how the step ended (terminated, truncated: outcome_word, nig_step.hpp -- I decides it once, C takes it); C also
// reads the clipped action back from the P -> I slot.  DS operations of one wave execute in order, so "write data,
// then write counter" / "read counter, then read data" needs no wait in between; the wavefront-scope fences only
// pin the compiler's order.  No block barrier inside the loop.  Flow control: P writes slot j only after C is
// done with slot j - K; I needs P's slot j before it writes its own slot j, so it cannot overrun C either.
//
// The arithmetic is the other kernels': same clip, violated, dynamics, post_core (I; C adds post_finish's penalties to the
// same reward and reads pack_flags' bits off a table checked against it at compile time: post_record), tally and reset
// calls on the same values with the same generator keys -- the results are bit-identical to rollout_kernel's
// (tests/test_gpu_parity.py, tests/test_spec_envs.py: the fused-rollout tests run this form wherever it applies,
// tests/test_gpu_split.py pins it against the one-wave form).
#pragma once
#include <utility>
#include "nig_ring.hpp"
#include "nig_rollout.hpp"

namespace nig {

template <class E, class = void> struct split_rollout : std::false_type {};
template <class E> struct split_rollout<E, std::void_t<decltype(E::SPLIT_ROLLOUT)>> : std::bool_constant<E::SPLIT_ROLLOUT> {};
// batches of more blocks than are resident at once: run the three-wave form in rounds (ChemicalReactor: measured faster,
// profiles/r02/rounds_probe.txt), or leave them to the form that fills the SIMDs with lanes (SPLIT_ROUNDS = false)
template <class E, class = void> struct split_rounds : std::true_type {};
template <class E> struct split_rounds<E, std::void_t<decltype(E::SPLIT_ROUNDS)>> : std::bool_constant<E::SPLIT_ROUNDS> {};

template <class Env, int NP>
struct SplitLds {
    // ring slots: as many as the CU's LDS holds for NP triples (ChemicalReactor, S = 12: six; RobotAssembly, S = 24, whose
    // producer and recorder are light next to the integrator and never need to run far ahead / behind: three)
    static constexpr int K = Env::S > 16 ? 3 : 6;
    static constexpr int HI_ROWS = Env::KS + Env::A;
    static constexpr int HI_SLOT = HI_ROWS * 64;             // floats
    static constexpr int IH_SLOT = (Env::S + 1) * 64;        // floats: [64][S] state rows, then [64] violation words
    static constexpr int OFF_PROBIT = 16 * PROBIT_BIAS;                        // (probit_fetch: the bias rides in the DS offset field)
    static constexpr int OFF_IMG = OFF_PROBIT + 768 * 16;                                   // float [NP][RESET_ROWS][64]
    static constexpr int OFF_WLIST = OFF_IMG + NP * Env::RESET_ROWS * 64 * 4;  // uchar [NP][64]
    static constexpr int OFF_SYNC = OFF_WLIST + NP * 64;                       // uint32 [NP][4]: {P produced, I produced, C done}
    static constexpr int OFF_HI = OFF_SYNC + NP * 16;
    static constexpr int OFF_IH = OFF_HI + NP * K * HI_SLOT * 4;
    static constexpr int BYTES = OFF_IH + NP * K * IH_SLOT * 4;
    static_assert(BYTES <= 160 * 1024, "LDS of one CU");
};

// (ring counters, waits, posts and the ordering assumption they rest on: nig_ring.hpp)

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>) in order: the step loops of the three roles are unrolled
// with it over their static positions (ring slot, register set) -- nig_split_body.inc
template <class F, int... R>
__device__ __forceinline__ void split_unrolled_seq(F &&f, std::integer_sequence<int, R...>) { (f(std::integral_constant<int, R>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void split_unrolled(F &&f) { split_unrolled_seq(f, std::make_integer_sequence<int, N>{}); }
constexpr int split_lcm(int a, int b)
{
    int m = a;
    while (m % b != 0) m += a;
    return m;
}

// NP wave triples per block: wave w < NP integrates lanes base + 64 w .. + 63, wave NP + w is their producer and
// wave 2 NP + w their recorder (a block's waves go to the CU's four SIMDs round-robin: with NP = 4 the three
// share one).  Whole 64*NP-lane blocks only, auto-reset handles without frozen lanes only, and for an env with step
// noise a launch starting on an odd counter (PAIRED form): the host keeps every other case on rollout_kernel.
// NOISE (nig_rollout_noise): the reference's recorded draws instead of the generator's -- the producer LOADS the step's
// process noise (float64 rows, handed on as the float the fast-mode ring carries: ChemicalReactor's dynamics round the
// draw to float32 before they use it, chemical_reactor.py:149,159 under NEP 50, so nothing is lost) and a finishing lane
// restarts from Env::init(recorded draws), per lane, in place of the cooperative reset.  Ring protocol, roles, clip,
// constraint check, dynamics, reward, flags, tally and stores are the timed kernel's, instruction for instruction.
// SAMPLED (nig_rollout_sampled, split_sampled_kernel): no action ring -- the PRODUCER draws the step's action (sample_action:
// blocks STREAM_ACTION + j of the lane's key at the step's own launch counter; the action stream is keyed per counter, so unlike
// the step noise's block it is not shared by the two steps of a pair) where it used to take a prefetched register set.  The LA
// register sets and their look-ahead existed to hide a global load's latency: nothing is loaded now, so the sampled producer
// holds ONE action set and draws it in the step that hands it on; what keeps it ahead of the integrator is the K-slot LDS ring,
// as before.  Integrator and recorder are the ring-fed form's, instruction for instruction.
// The body is written once (nig_split_body.inc) and compiled into two kernels under names of their own, so that nothing that picks
// kernels by name confuses the sampled form with the ring-fed one.  (Textual inclusion, not a __device__ function taking the
// arguments by reference: the kernel's by-value argument block lives in the constant address space, and through a reference
// hipcc generates different -- a few instructions shorter, differently allocated -- code for the ring-fed kernels, which are
// required not to change: profiles/isa_diff.py.)
template <class Env, int OUT, int NP, bool NOISE = false>
__global__ void __launch_bounds__(192 * NP, 1) split_rollout_kernel(const RolloutArgs q)
{
    constexpr bool SAMPLED = false;
#include "nig_split_body.inc"
}
template <class Env, int OUT, int NP>             // nig_rollout_sampled's twin
__global__ void __launch_bounds__(192 * NP, 1) split_sampled_kernel(const RolloutArgs q)
{
    constexpr bool SAMPLED = true, NOISE = false;
#include "nig_split_body.inc"
}

// whole blocks of 64*NP lanes, PAIRED start; the caller (nig_launch.hpp, from the launch plan) has checked that the form applies
// (NOISE, injected draws: the row-major full-output variant only -- OUT == 3)
template <class Env, int NP, int OUT, bool NOISE = false, bool SAMPLED = false>
static void launch_split_blocks(const RolloutArgs &q, unsigned grid, hipStream_t st)
{
    if constexpr (SAMPLED) hipLaunchKernelGGL((split_sampled_kernel<Env, OUT, NP>), dim3(grid), dim3(192 * NP), 0, st, q);
    else hipLaunchKernelGGL((split_rollout_kernel<Env, OUT, NP, NOISE>), dim3(grid), dim3(192 * NP), 0, st, q);
}

}  // namespace nig
