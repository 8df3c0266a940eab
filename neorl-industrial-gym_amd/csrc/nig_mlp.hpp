// nig_mlp.hpp -- the fused MLP actor on MFMA with its safety-critic shield and its ensemble (device code only): MlpArgs,
// MlpShieldArgs, MlpEnsArgs, MlpDistArgs, MlpSearchArgs, MlpGateArgs, MlpProjectArgs, MlpCatArgs, MlpLimArgs, MlpLimited<>,
// rollout_mlp_body and its eight kernels with their _limited twins, the distributional critic's kernels (the shield and the search on a
// 64-row softmax head, and the stand-alone evaluator).
#pragma once
#include <type_traits>
#include "nig_step.hpp"
#include "nig_disturb.hpp"
#include "nig_limits.hpp"
#include "nig_mlp_stream.hpp"        // the operand stream's constants and layer-1 shape (shared with the host's builder)

namespace nig {

// ------------------------------------------------------------------------------------------
// Fused MLP actor + env step (the one contraction on this path, so the one place for MFMA).
//
// One wavefront = 32 env instances.  Everything is computed TRANSPOSED, h^T = W^T x^T, so that
//   * the A operand is the weight matrix (one float per lane, streamed from a pre-ordered
//     array: record r = 64 floats = one 256-byte coalesced load),
//   * the B operand has the env on the lane (l & 31) and the k index on the lane half (l >> 5),
//   * the 32x32 result tile has the env on the lane again and the hidden unit in the register,
// which makes an accumulator register of layer n directly usable as a B operand of layer n+1
// (register t of a tile holds hidden rows rho_h(t) = (t&3) + 8(t>>2) + 4h of that tile for lane
// half h; the weight stream is ordered to match).  No LDS, no transposes, no conversion.
// v_mfma_f32_32x32x2_f32 is bit-for-bit fma(a1,b1, fma(a0,b0, c)) (k0 = lane half 0, then k1), so
// the CPU oracle reproduces the actor exactly.  Biases ride along as one extra k-step per tile
// (A = bias on half 0 / 0 on half 1, B = 1 / 0).
// Both lane halves carry the full env state and run the env step redundantly (it is ~3 % of the
// MFMA time); lanes 32-63 never store.
using f32x16 = __attribute__((ext_vector_type(16))) float;

struct MlpArgs {
    StepArgs s;
    const float *wstream;       // MFMA operand stream built by nig_set_mlp_policy
    int n_steps;
    uint32_t out_stride;
    float *obs_out; uint64_t obs_step_stride;
    float *act_out; uint32_t ld_act_out; uint64_t act_step_stride;
};

typedef __attribute__((address_space(3))) void nig_lds_void;
typedef __attribute__((address_space(1))) const void nig_glb_void;

// Two blocks per CU: the double-buffered weight image is 74 KiB per block, so two blocks fit a CU's 160 KiB as long as nothing
// else of size lives in LDS -- the generator's 12 KiB table does not: every env reads its table entries from global memory
// (L2-resident, as step_kernel does; PowerGrid's 23 + 31 reads per step / reset are noise beside 1 217 MFMAs).  The kernels are
// compiled for two waves per SIMD (__launch_bounds__(BLOCK, 2)), so a second block's waves fill the bubbles of the first: with
// one block per CU every chunk barrier and ring refill was exposed MFMA idle time (duty cycle 0.78 against 0.875,
// profiles/r04/mlp_cr65536_sq.txt, mlp_two_blocks.txt).
// The head (layer 3) of an env with at most FOUR actions runs on v_mfma_f32_4x4x1_16B_f32 (round 5): sixteen 4 x 4 blocks of
// four lanes, K = 1 -- lane l multiplies ITS OWN h2 value (B) with the four head weights held by the four lanes of its block
// (A: lane 4 b + r holds W3[k][r]) into four accumulators, out[r] += W3[k][r] h2[k]: exactly a head of <= 4 rows, 8 cycles an
// instruction, where the 32 x 32 x 2 tile spent 64 cycles on 32 rows of which 29 were zero padding (11 % of the step's MFMA
// time).  Each lane half accumulates the hidden rows ITS accumulator registers hold (rho_h(t)), the two
// partial sums meet in one v_add_f32 across the halves: a different summation order from the 32 x 32 x 2 head (k0, k1
// interleaved), restated by the oracle (mlp_actor).
// Heads of FIVE TO SIXTEEN actions take the same route on v_mfma_f32_16x16x1_4B_f32: four 16 x 16 blocks of sixteen lanes, K = 1,
// 32 cycles.  Block b = lane >> 4 multiplies its lanes' own h2 values (B: hidden row rho_{b>>1}(t), envs 16 (b & 1) ..) with the
// sixteen head weights its lanes hold (A: lane 16 b + r holds W3[k_b][r]) into registers 4 b .. 4 b + 3 (row r of env column c in
// register 4 b + (r & 3) of lane 16 (r >> 2) + c): blocks 0 / 1 are lane half 0's fma chain for envs 0-15 / 16-31, blocks 2 / 3
// lane half 1's -- the SAME two chains and the same joining add as the 4 x 4 x 1 head, so the oracle has one head for every env.
// The 32 x 32 x 2 head (64 cycles for 32 rows, 24 of them padding with eight actions) is gone.
// The one statement of which envs have the MFMA actor: an even state dim (layer 1 takes the state two rows per k-step) and a head of
// at most 16 rows.  The body asserts it, the launchers (nig_launch.hpp) compile a kernel only where it holds and leave the env's
// table slot null elsewhere, which is what the C ABI asks.
template <class Env> constexpr bool has_mlp_actor = Env::S % 2 == 0 && Env::A <= 16;
template <class Env> constexpr bool mlp_head4 = Env::A <= 4;
using f32x4 = __attribute__((ext_vector_type(4))) float;
template <int N> using mlp_int = std::integral_constant<int, N>;      // a compile-time count handed to a lambda

// Safety-critic shield (rollout_mlp_shield_kernel, agents/cql.py predict_with_safety): after the actor, a second pass of the
// same routines evaluates p = sigmoid(critic([s, a])), and the env receives a * 0.5 unless p < threshold.  The critic is the
// network (S + A, 1) of nig_mlp_stream.hpp: layer 1 on x = [s (S), a (A), 0-pad to even] in mlp_layer1(S + A).chunks chunks
// (two of four tiles each for PowerGrid, AdvancedPowerGrid, SupplyChain), a one-row head on v_mfma_f32_4x4x1 (the actor's
// mlp_head4 form).  Its chunks are consumed through the same double-buffered LDS image, so the fill of the next chunk stays in
// flight across actor -> critic and critic -> next step's actor.
struct MlpShieldArgs {
    MlpArgs m;
    const float *cstream;       // critic operand stream built by nig_set_mlp_safety
    float *prob_out;            // [n_steps][>= B] p of the unshielded action (row k at prob_out + k * m.out_stride), may be NULL
    float threshold;            // shield when !(p < threshold)
};

// Ensemble actor (rollout_mlp_ensemble_kernel, agents/ensemble.py EnsembleAgent.predict / predict_with_uncertainty): ENS != 0 runs
// n_members actor passes per step through the same double-buffered LDS image -- member k + 1's layer-1 chunk is in flight while
// member k's last hidden tile is consumed, the next step's member 0 behind the last member -- and reduces the members' actions
// p_k (float32, each bit for bit the single actor's) as they arrive, in registers that do not grow with the member count:
//   action, ENS_AVERAGE ("mean" / "weighted"; float64, the env steps with step_core<Env, NZ, double> where the env has it):
//       acc = (double)p_0 * w_0;  acc = acc + (double)p_k * w_k  (k = 1 .. K-1, products rounded);  action = acc / wsum
//   action, ENS_VOTING (np.mean of a float32 array; float32):  acc = p_0;  acc = acc + p_k;  action = acc / (float)K
//   uncertainty (float32), per action dimension about member 0, d_k = p_k - p_0:
//       s1 = sum_k d_k,  s2 = sum_k d_k * d_k  (k = 1 .. K-1 in order, from 0),  v = max(s2 - (s1 * s1) / (float)K, 0),
//       sd = sqrt(v / (float)K);   uncertainty = (sd_0 + sd_1 + ... + sd_{A-1}) / (float)A, summed in index order.
//   The shifted form needs p_0, s1, s2 and the action's accumulator: 5 A registers (4 A for voting) whatever K is, where the
//   reference's two-pass np.std needs all K A member actions at once.  It is exactly 0 for identical members, and because member
//   0's own deviation from the mean is part of v, s2 <= (1 + K) v: the subtraction loses at most a factor 1 + K <= 9 of float32's
//   precision (measured against np.std: tests/test_ensemble_host.py, 1e-5 relative).
// Every division and the square root are IEEE correctly rounded: plain `/` and __builtin_sqrtf, which hipcc expands to the
// v_div_scale / v_div_fmas / v_div_fixup sequences (float32: -fhip-fp32-correctly-rounded-divide-sqrt, the compiler's default,
// denormals kept) -- the translation unit is compiled with -ffp-contract=off, so no product above fuses into a sum.
constexpr int ENS_NONE = 0, ENS_AVERAGE = 1, ENS_VOTING = 2;
struct MlpEnsArgs {
    MlpArgs m;                  // m.wstream: the members' operand streams, MLP_STREAM_FLOATS floats apart, in member order
    int n_members;
    const double *w;            // device [n_members]: the active weights (ENS_AVERAGE)
    double wsum;                // np.sum of the active weights, computed by the host
    float kf;                   // (float)n_members
    float threshold;            // NIG_FLAG_UNCERTAIN when uncertainty > threshold
    float *unc_out;             // [n_steps][>= B], row k at unc_out + k * m.out_stride, may be NULL
    float *member_out;          // member k of step it: [A][m.ld_act_out] at member_out + (it * n_members + k) * m.act_step_stride, may be NULL
};

// Disturbed actor (rollout_mlp_disturbed_kernel, include/nig.h "nig-disturb-v1"): DIST feeds layer 1 the noisy observation
// o = s + sigma_obs * zo instead of s and adds sigma_act * za to the tanh head's action before the disturbance's clip.  The draws
// depend on the lane's key only, so they are made at the top of the step, ahead of the first chunk barrier, while the LDS-DMA
// fill of layer 1 is in flight; both lane halves compute the same o from the same key.  o[] is dead after layer 1.
struct MlpDistArgs {
    MlpArgs m;
    DisturbArgs d;
};

// Safe-action search (rollout_mlp_search_kernel, agents/safety_critical.py RiskAwareCQLAgent.get_safe_action; include/nig.h
// "nig-search-v1"): SEARCH is the shield's form with another correction.  Where the critic's p0 of the actor's action is not below
// the threshold, n_candidates uniform actions of [-1, 1) are scored by the same critic pass -- through the same double-buffered LDS
// image, the critic's stream cycled once per pass, candidate c + 1's layer-1 chunk in flight while candidate c's last hidden tile is
// consumed, the next step's actor behind the last -- and the env receives the first one of least p.  MFMA passes and chunk
// barriers are block-wide, so the block votes (__syncthreads_or) and runs no candidate pass when none of its live lanes asks
// for one; the fill that follows p0's pass is issued after the vote (one exposed fill per step).  A lane that keeps its action
// ignores the candidates, so no lane's result depends on its block's vote.  A candidate is a function of (lane key, c) alone: it is
// drawn ahead of its pass's first chunk barrier, is dead after layer 1, and the winner is drawn again from its number at the end --
// the running best is (p_best, choice): two registers, whatever n_candidates and A are.
constexpr uint32_t SEARCH_BLOCK0 = 0x100u;       // candidate c, action j: word j & 3 of block STREAM_POLICY + SEARCH_BLOCK0 + 4 c + (j >> 2)
struct MlpSearchArgs {
    MlpShieldArgs sh;           // sh.prob_out: p0, the actor's action's p
    int n_candidates;           // 1 .. NIG_MAX_CANDIDATES
    float *risk_out;            // [n_steps][>= B] p of the action the env received, row k at risk_out + k * m.out_stride, may be NULL
    int32_t *choice_out;        // [n_steps][>= B] the candidate's number, -1 where the actor's action was kept, may be NULL
};

// candidate c of the key's lane and step (action_from_word's [-1, 1) form, whatever the env's Box)
template <int A>
__device__ __forceinline__ void search_candidate(const RngKey &key, int c, float (&u)[A])
{
#pragma unroll
    for (int j4 = 0; 4 * j4 < A; ++j4) {
        const u32x4 x = key.block(STREAM_POLICY + SEARCH_BLOCK0 + 4u * (uint32_t)c + (uint32_t)j4);
        const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * j4 + k < A) u[4 * j4 + k] = action_from_word(w[k], -1.0f, 1.0f);
    }
}

// Safety-ensemble gate (rollout_mlp_gated_kernel, agents/safety_critical.py SafeEnsembleAgent.get_safe_action; include/nig.h
// "nig-gate-v1"): GATE is the shield's form with n_members critics of n_outputs <= 4 head rows each.  The members' passes run through
// the same double-buffered LDS image, member m's stream at cstreams + m * MLP_CSTREAM_FLOATS -- the ensemble actor's fill chain on
// the critic's two layer-1 shapes: member m + 1's layer-1 chunk is in flight while member m's last hidden tile is consumed, the
// next step's actor layer 1 behind the last member.  The head stays f32x4 on v_mfma_f32_4x4x1: row c of a member is the shield's
// one-row head on column c (rows do not interact), rows >= n_outputs carry zero weights and stay out of the vote and of every
// output.  The members' logits are reduced as they arrive by the ensemble actor's shifted sums about member 0 -- z_0, s1, s2 and
// the running sum: 16 registers whatever K is -- except that the variance's clamp keeps a NaN (v < 0 ? 0 : v): a member whose
// logit is -inf must reject.  Every pass is needed by every block: there is no vote.  As the search, the form keeps nothing across
// the passes that a step can form again from the lane index.
struct MlpGateArgs {
    MlpArgs m;
    const float *cstreams;      // the members' operand streams built by nig_set_mlp_safety_ensemble, MLP_CSTREAM_FLOATS floats apart
    int n_members;              // K, 1 .. NIG_MAX_ENSEMBLE
    int n_outputs;              // C, 1 .. 4: the head rows that vote
    float kf;                   // (float)n_members
    float temperature;          // T
    float threshold;            // reject unless p[c] < threshold for every c
    float umax;                 // reject (NIG_FLAG_UNCERTAIN) unless sd[c] < umax for every c
    float *prob_out;            // p: row c of step k at prob_out + k * c_step_stride + c * ld_c, may be NULL
    float *unc_out;             // sd: the same layout, may be NULL
    float *logit_out;           // z: member m of step k is [C][ld_c] at logit_out + (k * n_members + m) * c_step_stride, may be NULL
    uint32_t ld_c; uint64_t c_step_stride;
};

// Constraint projection (rollout_mlp_projected_kernel, agents/safety_critical.py ConstrainedIQLAgent.get_safe_action; include/nig.h
// "nig-project-v1"): PROJECT is the shield's form with a gradient descent on the action.  The constraint predictor f (S + A -> 256 ->
// 256 -> C, C <= 4 head rows on v_mfma_f32_4x4x1: the gate's member) scores the actor's action; where some p0[c] is not below the
// threshold the lane walks a <- clip(a - step * dG/da, -1, 1), G = sum_c relu(f_c), until every logit is below the tolerance or
// max_iters steps are taken.  In this kernel's transposed layout a backward pass IS a forward pass of the transposed network
// C -> 256 -> 256 -> A (weights W3^T zero-padded to four rows, W2^T, W1[S:S+A, :]^T, zero biases: an operand stream of put_network
// like any other, at `bstream`) whose "activation" is a select on the forward pass's ReLU mask: output tile m of either hidden layer
// holds unit 32 m + mfma_row(t, half) in register t in both directions, so the mask bit a backward tile needs sits in the lane that
// recorded it -- 128 bits per lane and hidden layer, eight registers, alive from a forward pass to the backward pass behind it.  The
// backward head has A rows: the actor's head instruction and decode, without the tanh.  Passes go through the same double-buffered
// LDS image; behind every forward pass the block votes (__syncthreads_or over "live, projected, not yet satisfied, steps left") and
// runs a backward + forward pair or leaves, the fill behind the vote exposed as in the search.  A lane that has stopped holds its
// action: the further forward passes of its block recompute its logits from the same (s, a), bit for bit, so no lane's result
// depends on its block's vote.  As the search and the gate, the form keeps nothing across the passes that a step can form again from
// the lane index.
constexpr int ACT_RELU = 0, ACT_RELU_RECORD = 1, ACT_SELECT = 2;   // a hidden layer's activation: ReLU; ReLU that records the lane's mask bits; select on a recorded bit
struct MlpProjectArgs {
    MlpArgs m;
    const float *cstream;       // the predictor's operand stream (S + A, C) built by nig_set_mlp_constraint
    const float *bstream;       // the backward network's operand stream (4, A), MLP_STREAM_FLOATS floats
    int n_outputs;              // C, 1 .. 4
    int max_iters;              // 1 .. NIG_MAX_PROJECT_ITERS
    float threshold;            // project unless sigmoid(z[c]) < threshold for every c
    float tolerance;            // stop once z[c] < tolerance for every c
    float step;                 // the gradient step
    float *prob_out;            // p0: row c of step k at prob_out + k * c_step_stride + c * ld_c, may be NULL
    float *viol_out;            // sigmoid(z) of the action the env received: the same layout, may be NULL
    int32_t *iters_out;         // [n_steps][>= B] gradient steps taken, -1 where the actor's action was kept, row k at iters_out + k * m.out_stride, may be NULL
    float *grad_out;            // the first gradient of the step, act_out's layout; untouched where iters < 1, may be NULL
    uint32_t ld_c; uint64_t c_step_stride;
};

// Distributional safety critic (agents/safety_critical.py RiskAwareCQLAgent.compute_safety_violation_probability; include/nig.h
// "nig-categorical-v1"): CAT is the shield's (and the search's) form with a head of up to 64 rows and a softmax across them in
// place of the sigmoid.  Layers 1 and 2 are the critic pass as it stands.  The head is four 16-row passes of v_mfma_f32_16x16x1
// per hidden register, their four accumulators (MlpCatHead) held across the eight layer-2 tiles: every column keeps the one-row
// head's two fma chains and joining add.  Pass 0's operands are the chunk's 16 head records (put_network's 16-row head), so the
// chunk slot, the double buffer and two blocks per CU stay as they are; the operands of passes 1 .. 3 come from the image's tail
// in global memory (put_network_wide: 16 bytes per lane and hidden register, 129 KiB a network, L2-resident and shared by every
// block), through a ring of MLP_CAT_RING entries whose first loads are issued ahead of the tile's 129 layer-2 MFMAs.  No chunk
// barrier is added and the fill chain is the shield's.
// After the last tile lane 16 q + c holds, for the two env columns 16 beta + c, the 16 logits of rows 16 P + 4 q + i (P: pass,
// i: register) -- the softmax runs where they lie (categorical_prob): the lane's own 16 rows in row order, then the four lanes
// of a column by two butterfly steps (xor 16, xor 32), which is the law's fixed order ((q0 + q1) + (q2 + q3)).
constexpr int CAT_NONE = 0, CAT_LOOP = 1, CAT_EVAL = 2;   // no categorical critic; in the closed loop; the stand-alone evaluator (nig_mlp_violation_prob)
constexpr int MLP_CAT_RING = 4;
// Experiment builds only (profiles/mkvariant.sh, profiles/categorical/parts.txt; never libnig.so): -DNIG_CAT_PARTS=1 replaces the tail's
// global loads by zero operands (the MFMAs stay), 2 replaces the softmax by a plain sum of the 64 accumulator registers, 3 both -- what each part costs.
#ifndef NIG_CAT_PARTS
#define NIG_CAT_PARTS 0
#endif
struct MlpCatHead { f32x16 p[MLP_WIDE_PASSES]; };
struct MlpCatArgs {
    const float *tail;          // put_network_wide's tail: rows 16 .. 63 of the head
    uint64_t below_mask;        // bit j: atom j counts as a violation
    int atoms;                  // N, 2 .. 64
    // the evaluator alone (the closed loops leave them zero):
    const float *act;           // [A][ld_act] the actions as given
    float *logit_out;           // [atoms][ld_logit], may be NULL
    uint32_t ld_act, ld_logit;
};
struct MlpCatShieldArgs { MlpShieldArgs sh; MlpCatArgs c; };
struct MlpCatSearchArgs { MlpSearchArgs sr; MlpCatArgs c; };
struct MlpCatEvalArgs { MlpShieldArgs sh; MlpCatArgs c; };     // sh.m.s.state / ld_state / B: the observations [S][ld_obs] and n; sh.prob_out: [n]

// p of "nig-categorical-v1" from the four head accumulators, for the env of this lane (both lane halves).  Whole wave, EXEC all
// ones.  STORE: the logits leave from the lanes that hold them (env column lane0 + 16 beta + c, where it is below n).
template <bool STORE>
__device__ __forceinline__ float categorical_prob(const MlpCatHead &h, const MlpCatArgs &cq, unsigned lane, [[maybe_unused]] uint32_t lane0, [[maybe_unused]] uint32_t n)
{
    const int q4 = 4 * (int)(lane >> 4);
    if constexpr ((NIG_CAT_PARTS & 2) != 0) {                // (every accumulator register stays live, so no head MFMA is removed with the softmax)
        float sum = 0.0f;
#pragma unroll
        for (int k = 0; k < 64; ++k) sum = sum + h.p[k >> 4][k & 15];
        return sum;
    }
    float pb[2];
#pragma unroll
    for (int beta = 0; beta < 2; ++beta) {
        float z[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) z[k] = h.p[k >> 2][4 * beta + (k & 3)] + h.p[k >> 2][8 + 4 * beta + (k & 3)];    // the two chains' joining add
        float m = -__builtin_inff();
#pragma unroll
        for (int k = 0; k < 16; ++k) m = (16 * (k >> 2) + q4 + (k & 3)) < cq.atoms ? fmaxf(m, z[k]) : m;
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        float t = 0.0f, v = 0.0f;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int j = 16 * (k >> 2) + q4 + (k & 3);
            const float ej = det_expf(z[k] - m);
            t = t + (j < cq.atoms ? ej : 0.0f);
            v = v + ((j < cq.atoms && ((cq.below_mask >> j) & 1ull)) ? ej : 0.0f);
        }
        t = t + __shfl_xor(t, 16);
        v = v + __shfl_xor(v, 16);
        t = t + __shfl_xor(t, 32);
        v = v + __shfl_xor(v, 32);
        pb[beta] = v / t;
        if constexpr (STORE) {
            const uint32_t col = lane0 + 16u * (uint32_t)beta + (lane & 15u);
            if (cq.logit_out && col < n) {
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int j = 16 * (k >> 2) + q4 + (k & 3);
                    if (j < cq.atoms) (cq.logit_out + (size_t)j * cq.ld_logit)[col] = z[k];
                }
            }
        }
    }
    // (after the two butterfly steps every lane 16 q + c holds p of both columns c and 16 + c: the lane's own env is one of them)
    return ((lane >> 4) & 1u) ? pb[1] : pb[0];
}

template <class Env, bool SHIELD, int ENS = ENS_NONE, bool DIST = false, bool SEARCH = false, bool GATE = false, bool PROJECT = false, bool LIMITS = false, int CAT = CAT_NONE>
__device__ __attribute__((always_inline)) inline void rollout_mlp_body(const MlpArgs &q, const float *cstream, float *prob_out, float threshold,
                                                                       [[maybe_unused]] const MlpEnsArgs *eq = nullptr,
                                                                       [[maybe_unused]] const DisturbArgs *dq = nullptr,
                                                                       [[maybe_unused]] const MlpSearchArgs *sq = nullptr,
                                                                       [[maybe_unused]] const MlpGateArgs *gq = nullptr,
                                                                       [[maybe_unused]] const MlpProjectArgs *jq = nullptr,
                                                                       [[maybe_unused]] const LimitArgs *lq = nullptr,
                                                                       [[maybe_unused]] const MlpCatArgs *cq = nullptr)
{
    // LIMITS combines with every other form (the _limited twins at the end of this header): the added constraints live at the one step site
    static_assert(!PROJECT || (SHIELD && !SEARCH && !GATE), "the projection is a form of the shield; it excludes the search and the gate");
    static_assert(!(SHIELD && ENS != ENS_NONE), "the ensemble has no shield");
    static_assert(!SEARCH || SHIELD, "the search is a form of the shield");
    static_assert(!GATE || (SHIELD && !SEARCH), "the gate is a form of the shield; it has no searching twin");
    static_assert(!DIST || (!SHIELD && ENS == ENS_NONE), "the shield and the ensemble have no disturbed form");
    static_assert(CAT == CAT_NONE || (SHIELD && !GATE && !PROJECT), "the categorical critic is a form of the shield and of the search");
    static_assert(CAT != CAT_EVAL || (!SEARCH && !LIMITS), "the evaluator steps no env");
    // the env steps on the ensemble's float64 action where its NumPy arithmetic follows the action's type (nig_step64's rule)
    constexpr bool ACT64 = ENS == ENS_AVERAGE && Env::HAS_ACT64;
    using act_t = std::conditional_t<ACT64, double, float>;
    constexpr int S = Env::S, A = Env::A, KS = Env::KS, KR = Env::KR;
    constexpr int KSN = KS > 0 ? KS : 1;
    static_assert(has_mlp_actor<Env>, "MFMA actor needs an even state dim and at most 16 actions");
    // Weight records are shared by the four waves of the block through LDS: round 1 let every wave stream all
    // ~1 200 records of a step from L2 on its own (the same 256-byte lines requested by every wave of the chip at
    // about the same time: 96 TFLOP/s of 155).  Now the block fills a double-buffered LDS image chunk by chunk with
    // LDS-DMA (global_load_lds_dwordx4: 1 KiB per wave-instruction, no registers), nine fills per step, each wave a
    // quarter of the pieces, the fill of chunk c+1 in flight while chunk c is consumed; an MFMA's A operand is one
    // ds_read_b32.  L2 traffic per block and step: 311 KB instead of 4 x 311 KB.
    __shared__ __attribute__((aligned(16))) float s_w[2][MLP_CHREC * 64];
    const float4 *const s_probit = NIG_PROBIT;               // the generator's table stays in global memory: two blocks per CU
    const StepArgs &p = q.s;
    const unsigned tid = threadIdx.x, lane = tid & 63u, half = lane >> 5, e = lane & 31u, wave = tid >> 6;
    const uint32_t lane0 = blockIdx.x * (BLOCK / 2) + (tid >> 6) * 32u;     // first env of this wave
    const uint32_t li = lane0 + e;
    const bool in_range = li < p.B;
    const bool writer = in_range && half == 0;
    const uint32_t t_base = (p.t_ptr ? *p.t_ptr : 0u) + p.t_off;
    const uint64_t gi = p.env0 + (uint64_t)li;
    // the lane's global index where a step needs it; the search forms it anew each time (as its output addresses, below: nothing
    // that a step can form from the lane index is kept in registers across the candidate passes)
    auto lane_gi = [&]() __attribute__((always_inline)) {
        if constexpr (SEARCH || GATE || PROJECT) { uint32_t l = li; asm volatile("" : "+v"(l)); return p.env0 + (uint64_t)l; }
        else return gi;
    };
    const bool autoreset = (p.hflags & NIG_F_AUTORESET) != 0;
    const bool tally = p.tally != nullptr;

    uint32_t ctr;
    if constexpr (CAT == CAT_EVAL) ctr = in_range ? 0u : (uint32_t)NIG_CTR_DONE;      // (the evaluator has no handle state: p.state is the caller's obs)
    else ctr = in_range ? p.ctr[li] : (uint32_t)NIG_CTR_DONE;
    float s[S], a[A], n[S];
    typename Env::fast_noise_t nz[KSN];
#pragma unroll
    for (int k = 0; k < S; ++k) s[k] = in_range ? (p.state + k * p.ld_state)[li] : 0.0f;
    double ret = (tally && in_range) ? p.ep_ret[li] : 0.0;
    LaneTally lt;
    lt.clear();
    // fill LDS buffer `buf` with chunk `c` of the operand stream: this wave's quarter of the KiB pieces
    const float *wsrc = q.wstream;                           // operand stream of the actor (ensemble: of the member) being filled from
    auto fill_from = [&](const float *stream, int c, int buf, int pieces) __attribute__((always_inline)) {
        const float *src = stream + (size_t)c * (MLP_CHREC * 64) + lane * 4u;
        for (int pc = (int)wave; pc < pieces; pc += BLOCK / 64)
            __builtin_amdgcn_global_load_lds((nig_glb_void *)(src + pc * 256), (nig_lds_void *)(&s_w[buf][pc * 256]), 16, 0, 0);
    };
    auto fill = [&](int c, int buf, int pieces) __attribute__((always_inline)) { fill_from(ENS != ENS_NONE ? wsrc : q.wstream, c, buf, pieces); };
    [[maybe_unused]] const float *gsrc = cstream;            // gate: operand stream of the member being filled from
    [[maybe_unused]] auto cfill = [&](int c, int buf, int pieces) __attribute__((always_inline)) { fill_from(GATE ? gsrc : cstream, c, buf, pieces); };
    constexpr MlpLayer1 L1 = mlp_layer1(S), C1 = mlp_layer1(S + A);   // layer 1 of the actor (S, A) and of the critic (S + A, 1)
    static_assert(L1.chunks == 1, "the actor's layer 1 must fit one chunk");
    static_assert(C1.fits(), "a critic layer-1 chunk must fit one chunk slot");
    // ---------------- one network = layer 1, then MLP_MT chunks of layer 2 + head; the two routines every pass is made of ----------------
    // Both consume the chunk that is in s_w[gbuf] and are straight-line code: the chunk barrier, the fill of the chunk that
    // follows (the one thing that differs between actor, critic, ensemble member and step) and the loop over chunks stay in
    // the body, where the compiler saw them before there were routines (nig_episode.hpp's rule; profiles/mlp_network/isa_diff.txt).
    // Layer 1, one chunk of it: TILES hidden tiles of REC records each on the input x(k) -> ReLU'd tiles h[0 .. TILES).
    // The activation `act_` is ReLU, ReLU that also records the lane's mask bits (tile mm, register r: bit 16 (mm & 1) + r of
    // mk[mm >> 1]), or the backward pass's select on such a recorded bit; mk is unused with plain ReLU.
    auto layer1_chunk = [&](auto tiles_, auto rec_, const auto &x, f32x16 *h, int gbuf, auto act_, [[maybe_unused]] uint32_t *mk) __attribute__((always_inline)) {
        constexpr int TILES = decltype(tiles_)::value, REC = decltype(rec_)::value, ACT = decltype(act_)::value;
        const float *wb = &s_w[gbuf][lane];
#pragma unroll
        for (int mm = 0; mm < TILES; ++mm) {
            f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int ks = 0; ks < REC - 1; ++ks) {
                const float b = half ? x(2 * ks + 1) : x(2 * ks);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wb[(mm * REC + ks) * 64], b, acc, 0, 0, 0);
            }
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wb[(mm * REC + REC - 1) * 64], half ? 0.0f : 1.0f, acc, 0, 0, 0);   // + bias
            if constexpr (ACT == ACT_SELECT) {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = ((mk[mm >> 1] >> (16 * (mm & 1) + r)) & 1u) ? acc[r] : 0.0f;
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = fmaxf(acc[r], 0.0f);                               // ReLU
            }
            if constexpr (ACT == ACT_RELU_RECORD) {
                uint32_t bits = 0u;
#pragma unroll
                for (int r = 0; r < 16; ++r) bits |= (acc[r] > 0.0f ? 1u : 0u) << (16 * (mm & 1) + r);
                mk[mm >> 1] = (mm & 1) ? (mk[mm >> 1] | bits) : bits;
                // the word is formed HERE: hipcc otherwise sinks the compares to the word's first use, behind the block's vote, and
                // keeps the tiles they read alive until then (the backward pass's tiles on top of them: 500 B of spills per lane)
                asm volatile("" : "+v"(mk[mm >> 1]));
            }
            h[mm] = acc;
        }
    };
    // Layer 2, hidden tile number `tiles` (counted from 1) on the layer-1 tiles h, consumed at once by its slice of the head:
    // returns the head's accumulator `out` (this lane half's partial sums; its type names the instruction, f32x4: 4 x 4 x 1,
    // f32x16: 16 x 16 x 1) with the tile's 16 hidden rows added, and the head's bias behind the last tile.  (The count and not
    // a `bool last`: the caller would evaluate that ahead of the first sched_barrier, and the parent compares after the last.)
    // `act_` as in layer1_chunk: the tile's bits are bits 16 ((tiles - 1) & 1) .. of mk[(tiles - 1) >> 1]; the word is picked by a
    // chain of selects, since `tiles` is a run-time count and a register array takes no run-time index.
    auto layer2_chunk = [&](const f32x16 *h, auto out, int tiles, int gbuf, auto act_, [[maybe_unused]] uint32_t *mk) __attribute__((always_inline)) {
        constexpr int RING = 8;                             // LDS reads in flight ahead of their MFMA (~64 cycles apart)
        constexpr int ACT = decltype(act_)::value;
        [[maybe_unused]] uint32_t bits = 0u;                // ACT_RELU_RECORD: gathered here; ACT_SELECT: the tile's recorded bits
        if constexpr (ACT == ACT_SELECT) {
            const int tw = (tiles - 1) >> 1;
            bits = (tw == 0 ? mk[0] : tw == 1 ? mk[1] : tw == 2 ? mk[2] : mk[3]) >> (16 * ((tiles - 1) & 1));
        }
        // the head's B operand: register t of the tile through the activation
        auto hidden = [&](const f32x16 &acc, int t) __attribute__((always_inline)) {
            if constexpr (ACT == ACT_SELECT) return ((bits >> t) & 1u) ? acc[t] : 0.0f;
            else {
                if constexpr (ACT == ACT_RELU_RECORD) bits |= (acc[t] > 0.0f ? 1u : 0u) << t;
                return fmaxf(acc[t], 0.0f);
            }
        };
        const float *wb = &s_w[gbuf][lane];
        f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        float ring[RING];
#pragma unroll
        for (int j = 0; j < RING; ++j) ring[j] = wb[j * 64];
        // the 64-row head: this tile's entries of the tail (rows 16 .. 63), from global memory ahead of the layer-2 MFMAs
        constexpr bool WIDE = std::is_same_v<decltype(out), MlpCatHead>;
        [[maybe_unused]] f32x4 gring[MLP_CAT_RING];
        [[maybe_unused]] const f32x4 *gt = nullptr;
        if constexpr (WIDE) {
            gt = (const f32x4 *)cq->tail + (size_t)(tiles - 1) * (16 * 64) + lane;
#pragma unroll
            for (int j = 0; j < MLP_CAT_RING; ++j) {
                if constexpr ((NIG_CAT_PARTS & 1) != 0) gring[j] = f32x4{0, 0, 0, 0}; else gring[j] = gt[j * 64];
            }
        }
#pragma unroll
        for (int i = 0; i < MLP_PER; ++i) {
            const float aop = ring[i % RING];
            if (i + RING < MLP_PER + 1) ring[i % RING] = wb[(i + RING) * 64];       // (+1: the head's bias record of the last chunk)
            // pin the source order: hipcc's scheduler otherwise sinks every read to just before its use
            __builtin_amdgcn_sched_barrier(0);
            if (i < MLP_MT * 16) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aop, h[i / 16][i % 16], acc, 0, 0, 0);
            } else if (i == MLP_MT * 16) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aop, half ? 0.0f : 1.0f, acc, 0, 0, 0);      // + bias
            } else if constexpr (std::is_same_v<decltype(out), f32x4>) {      // own value x the weights of the lane's block
                out = __builtin_amdgcn_mfma_f32_4x4x1f32(aop, hidden(acc, i - MLP_MT * 16 - 1), out, 0, 0, 0);
            } else if constexpr (WIDE) {                    // four 16-row passes on the one hidden value
                const int t = i - MLP_MT * 16 - 1;
                const float hv = hidden(acc, t);
                const f32x4 g = gring[t % MLP_CAT_RING];
                if constexpr ((NIG_CAT_PARTS & 1) == 0)
                    if (t + MLP_CAT_RING < 16 + 1) gring[t % MLP_CAT_RING] = gt[(t + MLP_CAT_RING) * 64];   // (+1: the bias entry behind the last tile)
                out.p[0] = __builtin_amdgcn_mfma_f32_16x16x1f32(aop, hv, out.p[0], 0, 0, 0);
                out.p[1] = __builtin_amdgcn_mfma_f32_16x16x1f32(g[0], hv, out.p[1], 0, 0, 0);
                out.p[2] = __builtin_amdgcn_mfma_f32_16x16x1f32(g[1], hv, out.p[2], 0, 0, 0);
                out.p[3] = __builtin_amdgcn_mfma_f32_16x16x1f32(g[2], hv, out.p[3], 0, 0, 0);
            } else {
                out = __builtin_amdgcn_mfma_f32_16x16x1f32(aop, hidden(acc, i - MLP_MT * 16 - 1), out, 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (ACT == ACT_RELU_RECORD) {
            const int tw = (tiles - 1) >> 1;
            const bool hi = ((tiles - 1) & 1) != 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                mk[w] = tw == w ? (hi ? (mk[w] | (bits << 16)) : bits) : mk[w];
                asm volatile("" : "+v"(mk[w]));             // (formed here, as in layer1_chunk)
            }
        }
        if (tiles == MLP_MT) {                              // record 145 of the last chunk: + the head's bias
            if constexpr (std::is_same_v<decltype(out), f32x4>) out = __builtin_amdgcn_mfma_f32_4x4x1f32(ring[MLP_PER % RING], half ? 0.0f : 1.0f, out, 0, 0, 0);
            else if constexpr (WIDE) {
                const f32x4 g = gring[16 % MLP_CAT_RING];
                const float one = half ? 0.0f : 1.0f;
                out.p[0] = __builtin_amdgcn_mfma_f32_16x16x1f32(ring[MLP_PER % RING], one, out.p[0], 0, 0, 0);
                out.p[1] = __builtin_amdgcn_mfma_f32_16x16x1f32(g[0], one, out.p[1], 0, 0, 0);
                out.p[2] = __builtin_amdgcn_mfma_f32_16x16x1f32(g[1], one, out.p[2], 0, 0, 0);
                out.p[3] = __builtin_amdgcn_mfma_f32_16x16x1f32(g[2], one, out.p[3], 0, 0, 0);
            }
            else out = __builtin_amdgcn_mfma_f32_16x16x1f32(ring[MLP_PER % RING], half ? 0.0f : 1.0f, out, 0, 0, 0);
        }
        return out;
    };
    if constexpr (CAT == CAT_EVAL) cfill(0, 0, C1.pieces);   // the evaluator has no actor: the critic's layer 1
    else fill(0, 0, L1.pieces);
    int gbuf = 0;                                            // buffer that holds (or receives) the chunk consumed next
    // The categorical critic's pass on x = [s, a, 0] -> p of "nig-categorical-v1": the shield's critic pass with the 64-row head,
    // stated once for the closed loops and the evaluator.  `next_fill` issues what follows the last chunk (the caller's business,
    // as in the shield); store_: the logits leave too.  (The closure exists in the categorical kernels alone: one that captures
    // gbuf in every kernel reorders two scalar moves in all of them -- profiles/categorical/isa_diff.txt.)
    [[maybe_unused]] auto cat_pass = [&]() __attribute__((always_inline)) { if constexpr (CAT == CAT_NONE) return 0; else
    return [&](const auto &x, auto &&next_fill, auto store_) __attribute__((always_inline)) {
        f32x16 g1[MLP_MT];
        if constexpr (C1.chunks == 1) {
            __syncthreads();                                // the critic's layer 1 is in s_w[gbuf]
            cfill(1, gbuf ^ 1, MLP_PIECES);
            layer1_chunk(mlp_int<MLP_MT>{}, mlp_int<C1.records>{}, x, g1, gbuf, mlp_int<ACT_RELU>{}, nullptr);
            gbuf ^= 1;
        } else {
#pragma unroll
            for (int c1 = 0; c1 < C1.chunks; ++c1) {
                __syncthreads();                            // critic layer-1 chunk c1 is in s_w[gbuf]
                if (c1 + 1 < C1.chunks) cfill(c1 + 1, gbuf ^ 1, C1.pieces);
                else cfill(C1.chunks, gbuf ^ 1, MLP_PIECES);
                layer1_chunk(mlp_int<C1.tiles>{}, mlp_int<C1.records>{}, x, g1 + c1 * C1.tiles, gbuf, mlp_int<ACT_RELU>{}, nullptr);
                gbuf ^= 1;
            }
        }
        MlpCatHead zc = {};
        for (int m2 = 0; m2 < MLP_MT; ++m2) {
            __syncthreads();                                // critic chunk C1.chunks + m2 is in s_w[gbuf]
            if (m2 + 1 < MLP_MT) cfill(C1.chunks + 1 + m2, gbuf ^ 1, MLP_PIECES);
            else next_fill();
            zc = layer2_chunk(g1, zc, m2 + 1, gbuf, mlp_int<ACT_RELU>{}, nullptr);
            gbuf ^= 1;
        }
        return categorical_prob<decltype(store_)::value != 0>(zc, *cq, lane, lane0, p.B);
    }; }();
    if constexpr (CAT == CAT_EVAL) {
        // ---------------- nig_mlp_violation_prob: one pass on the caller's (state, action) columns, no env ----------------
#pragma unroll
        for (int j = 0; j < A; ++j) a[j] = in_range ? (cq->act + (size_t)j * cq->ld_act)[li] : 0.0f;
        auto x = [&](int k) __attribute__((always_inline)) { return k < S ? s[k] : (k < S + A ? a[k - S] : 0.0f); };
        const float pv = cat_pass(x, [] {}, mlp_int<1>{});
        if (writer && prob_out) prob_out[li] = pv;
        return;
    }
    const int n_members = ENS != ENS_NONE ? eq->n_members : 1;
    [[maybe_unused]] bool d_obs = false, d_act = false;
    if constexpr (DIST) disturb_switches<S, A>(*dq, d_obs, d_act);
    for (int it = 0; it < q.n_steps; ++it) {
        [[maybe_unused]] float d_o[DIST ? S : 1], d_za[DIST ? A : 1];
        if constexpr (DIST) {                                      // (before the chunk barrier: beside the fill of layer 1)
            float zo[S];
            disturb_draws<S, A>(*dq, d_obs, d_act, gi, t_base + (uint32_t)it + 1u, ctr & NIG_CTR_STEP_MASK, p.seed_lo, p.seed_hi, s_probit, zo, d_za);
            disturb_obs<S>(*dq, d_obs, s, zo, d_o);
            // seen_out's row leaves here, so that o[] is dead once layer 1 has read it
            if (writer && !(ctr & NIG_CTR_DONE) && dq->seen_out) disturb_store_seen<S>(*dq, it, (size_t)li, d_o);
        }
        auto xin = [&](int k) __attribute__((always_inline)) { if constexpr (DIST) return d_o[k]; else return s[k]; };   // layer 1's input
        [[maybe_unused]] float e_p0[A], e_s1[A], e_s2[A], e_f[A];   // ensemble: member 0, sum d, sum d^2, float32 action sum
        [[maybe_unused]] double e_d[A];                            // ensemble: float64 weighted action sum
        [[maybe_unused]] float g_z0[GATE ? 4 : 1], g_s1[GATE ? 4 : 1], g_s2[GATE ? 4 : 1], g_acc[GATE ? 4 : 1];   // gate: member 0, sum d, sum d^2, logit sum
        [[maybe_unused]] int j_iters = -1;                         // projection: gradient steps taken, -1 where the actor's action is kept
        [[maybe_unused]] float j_z[PROJECT ? 4 : 1];               // projection: the logits of the last forward pass
        [[maybe_unused]] int g_mem = 0;                            // gate: this pass's member
        [[maybe_unused]] bool g_uncertain = false;
        int mem = 0;
        do {                                                       // (one pass unless ENS)
        // ---------------- actor: 3 layers of f32 MFMA, whole wave (EXEC all ones) ----------------
        f32x16 h1[MLP_MT];
        // chunk boundary: every wave's share of the fill has landed (the compiler drains vmcnt before the barrier)
        // and every wave is done with the buffer the next fill overwrites
        __syncthreads();
        fill(1, gbuf ^ 1, MLP_PIECES);
        layer1_chunk(mlp_int<MLP_MT>{}, mlp_int<L1.records>{}, xin, h1, gbuf, mlp_int<ACT_RELU>{}, nullptr);
        gbuf ^= 1;
        std::conditional_t<mlp_head4<Env>, f32x4, f32x16> out = {};     // this lane half's partial sums of the head rows
        for (int m2 = 0; m2 < MLP_MT; ++m2) {               // a real loop: the body is 145 MFMAs of straight-line code
            __syncthreads();                                // chunk 1 + m2 is in s_w[gbuf]; s_w[gbuf ^ 1] is free
            if (m2 + 1 < MLP_MT) fill(2 + m2, gbuf ^ 1, MLP_PIECES);
            else if constexpr (SHIELD) cfill(0, gbuf ^ 1, C1.pieces);  // the critic's layer 1 follows the actor
            else if constexpr (ENS != ENS_NONE) {                     // layer 1 of the next member, or of member 0 for the next step
                const bool more = mem + 1 < n_members;
                wsrc = more ? wsrc + MLP_STREAM_FLOATS : q.wstream;
                if (more || it + 1 < q.n_steps) fill(0, gbuf ^ 1, L1.pieces);
            }
            else if (it + 1 < q.n_steps) fill(0, gbuf ^ 1, L1.pieces);   // layer 1 of the NEXT step (the weights do not change)
            out = layer2_chunk(h1, out, m2 + 1, gbuf, mlp_int<ACT_RELU>{}, nullptr);
            gbuf ^= 1;
        }
        if constexpr (mlp_head4<Env>) {
            // action r = this half's partial sum + the other half's (lane l and l + 32 carry the same env)
#pragma unroll
            for (int r = 0; r < A; ++r) a[r] = det_tanhf(out[r] + __shfl_xor(out[r], 32));
        } else {
            // head row r of env column c (env 16 beta + c, beta = block parity): lane 16 (r >> 2) + c, registers 4 beta + (r & 3)
            // (lane half 0's chain) and 8 + 4 beta + (r & 3) (lane half 1's); hand every lane all A rows of its env
            const int beta = (int)(e >> 4);
#pragma unroll
            for (int r = 0; r < A; ++r) {
                const int src = 16 * (r >> 2) + (int)(e & 15u);
                const float v0 = __shfl(out[r & 3] + out[8 + (r & 3)], src);
                const float v1 = __shfl(out[4 + (r & 3)] + out[12 + (r & 3)], src);
                a[r] = det_tanhf(beta ? v1 : v0);
            }
        }
        if constexpr (ENS != ENS_NONE) {                     // fold member `mem` into the running sums (the law above)
            if (writer && !(ctr & NIG_CTR_DONE) && eq->member_out) {
                float *mo = eq->member_out + ((size_t)it * (size_t)n_members + (size_t)mem) * q.act_step_stride;
#pragma unroll
                for (int j = 0; j < A; ++j) (mo + j * q.ld_act_out)[li] = a[j];
            }
            if (mem == 0) {
#pragma unroll
                for (int j = 0; j < A; ++j) {
                    e_p0[j] = a[j]; e_s1[j] = 0.0f; e_s2[j] = 0.0f;
                    if constexpr (ENS == ENS_AVERAGE) e_d[j] = (double)a[j] * eq->w[0]; else e_f[j] = a[j];
                }
            } else {
                [[maybe_unused]] const double wk = ENS == ENS_AVERAGE ? eq->w[mem] : 0.0;
#pragma unroll
                for (int j = 0; j < A; ++j) {
                    const float d = a[j] - e_p0[j];
                    e_s1[j] = e_s1[j] + d; e_s2[j] = e_s2[j] + d * d;
                    if constexpr (ENS == ENS_AVERAGE) e_d[j] = e_d[j] + (double)a[j] * wk; else e_f[j] = e_f[j] + a[j];
                }
            }
        }
        } while (ENS != ENS_NONE && ++mem < n_members);
        if constexpr (DIST) disturb_act<A>(*dq, d_act, d_za, a);
        [[maybe_unused]] float unc = 0.0f;
        [[maybe_unused]] bool uncertain = false;
        [[maybe_unused]] double a64[ACT64 ? A : 1];
        if constexpr (ENS != ENS_NONE) {                     // once per step: the ensemble's action, its uncertainty, the flag bit
            const float kf = eq->kf;
            float usum = 0.0f;
#pragma unroll
            for (int j = 0; j < A; ++j) {
                float v = e_s2[j] - (e_s1[j] * e_s1[j]) / kf;
                v = v > 0.0f ? v : 0.0f;
                usum = usum + __builtin_sqrtf(v / kf);
                if constexpr (ENS == ENS_AVERAGE) {
                    const double x = e_d[j] / eq->wsum;
                    if constexpr (ACT64) a64[j] = x;
                    a[j] = (float)x;                         // act_out's word; the action itself for envs that take float32 (nig_step64's rule)
                } else a[j] = e_f[j] / kf;
            }
            unc = usum / (float)A;
            uncertain = unc > eq->threshold;
        }
        [[maybe_unused]] bool shield = false;
        [[maybe_unused]] float prob = 0.0f;
        [[maybe_unused]] float s_best = 0.0f;                      // search: p of the action the env receives, as far as the passes have come
        [[maybe_unused]] int s_choice = -1, s_cand = -1, s_passes = 0;   // search: the best's number; this pass (-1: the actor's action); how many
        [[maybe_unused]] float s_u[SEARCH ? A : 1];                // search: this pass's candidate (dead after layer 1)
        if constexpr (PROJECT) {
            // ---------------- constraint projection: forward pass, vote, backward + forward pairs (the law, include/nig.h) ----------------
            constexpr MlpLayer1 B1 = mlp_layer1(4);                // the backward network's layer 1: C <= 4 inputs, whatever C is
            static_assert(B1.chunks == 1 && B1.tiles == MLP_MT, "the backward layer 1 is one chunk");
            auto bfill = [&](int c, int buf, int pieces) __attribute__((always_inline)) { fill_from(jq->bstream, c, buf, pieces); };
            auto x = [&](int k) __attribute__((always_inline)) { return k < S ? s[k] : (k < S + A ? a[k - S] : 0.0f); };
            bool active = false;                                   // this lane is projected and has neither met the tolerance nor run out of steps
            for (int pk = 0;; ++pk) {                              // pk: the gradient steps taken so far by the lanes still walking (block-uniform)
                uint32_t m1[4], m2[4];                             // ReLU masks of the forward pass's two hidden layers (dead behind the backward pass)
                f32x16 g1[MLP_MT];
                if constexpr (C1.chunks == 1) {
                    __syncthreads();                        // the predictor's layer 1 is in s_w[gbuf]
                    cfill(1, gbuf ^ 1, MLP_PIECES);
                    layer1_chunk(mlp_int<MLP_MT>{}, mlp_int<C1.records>{}, x, g1, gbuf, mlp_int<ACT_RELU_RECORD>{}, m1);
                    gbuf ^= 1;
                } else {
#pragma unroll
                    for (int c1 = 0; c1 < C1.chunks; ++c1) {
                        __syncthreads();                    // predictor layer-1 chunk c1 is in s_w[gbuf]
                        if (c1 + 1 < C1.chunks) cfill(c1 + 1, gbuf ^ 1, C1.pieces);
                        else cfill(C1.chunks, gbuf ^ 1, MLP_PIECES);
                        static_assert(C1.tiles % 2 == 0, "a layer-1 chunk's tiles fill whole mask words");
                        layer1_chunk(mlp_int<C1.tiles>{}, mlp_int<C1.records>{}, x, g1 + c1 * C1.tiles, gbuf, mlp_int<ACT_RELU_RECORD>{}, m1 + c1 * (C1.tiles / 2));
                        gbuf ^= 1;
                    }
                }
                f32x4 z4 = {0, 0, 0, 0};
                for (int t2 = 0; t2 < MLP_MT; ++t2) {
                    __syncthreads();                        // predictor chunk C1.chunks + t2 is in s_w[gbuf]
                    if (t2 + 1 < MLP_MT) cfill(C1.chunks + 1 + t2, gbuf ^ 1, MLP_PIECES);      // (behind the last chunk the fill waits for the block's vote)
                    z4 = layer2_chunk(g1, z4, t2 + 1, gbuf, mlp_int<ACT_RELU_RECORD>{}, m2);
                    gbuf ^= 1;
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) j_z[c] = z4[c] + __shfl_xor(z4[c], 32);
                if (pk == 0) {                                     // the acceptance test on the actor's action
                    const bool live_writer = writer && !(ctr & NIG_CTR_DONE);
                    uint32_t lo = li;
                    asm volatile("" : "+v"(lo));
                    bool keep = true;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        if (c < jq->n_outputs) {
                            const float p0 = det_sigmoidf(j_z[c]);
                            keep = keep && p0 < threshold;
                            // p0 leaves here, so that it is dead during the gradient passes
                            if (live_writer && jq->prob_out) (jq->prob_out + (size_t)it * jq->c_step_stride + lo)[(size_t)c * jq->ld_c] = p0;
                        }
                    }
                    shield = !keep && !(ctr & NIG_CTR_DONE);       // (lanes past the batch are frozen: they never ask)
                    active = shield;
                }
                if (active) {                                      // the reference's loop head: the raw logits against the tolerance, then the step count
                    bool met = true;
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (c < jq->n_outputs) met = met && j_z[c] < jq->tolerance;
                    if (met || pk >= jq->max_iters) { active = false; j_iters = pk; }
                }
                // every wave is past the barrier behind which s_w[gbuf] was last read: it takes the chunk consumed next
                if (!__syncthreads_or(active)) {
                    if (it + 1 < q.n_steps) fill(0, gbuf, L1.pieces);
                    break;
                }
                bfill(0, gbuf, B1.pieces);
                // ---- backward: dG/da on d_c = (z_c > 0), the transposed network with the masks' selects ----
                auto xd = [&](int k) __attribute__((always_inline)) { return (k < jq->n_outputs && j_z[k] > 0.0f) ? 1.0f : 0.0f; };
                __syncthreads();                            // the backward layer 1 is in s_w[gbuf]
                bfill(1, gbuf ^ 1, MLP_PIECES);
                f32x16 q1[MLP_MT];
                layer1_chunk(mlp_int<MLP_MT>{}, mlp_int<B1.records>{}, xd, q1, gbuf, mlp_int<ACT_SELECT>{}, m2);
                gbuf ^= 1;
                std::conditional_t<mlp_head4<Env>, f32x4, f32x16> gout = {};
                for (int t2 = 0; t2 < MLP_MT; ++t2) {
                    __syncthreads();                        // backward chunk 1 + t2 is in s_w[gbuf]
                    if (t2 + 1 < MLP_MT) bfill(2 + t2, gbuf ^ 1, MLP_PIECES);
                    else cfill(0, gbuf ^ 1, C1.pieces);            // a forward pass follows every backward pass
                    gout = layer2_chunk(q1, gout, t2 + 1, gbuf, mlp_int<ACT_SELECT>{}, m1);
                    gbuf ^= 1;
                }
                float g[A];                                        // the actor's head decode, without the tanh
                if constexpr (mlp_head4<Env>) {
#pragma unroll
                    for (int r = 0; r < A; ++r) g[r] = gout[r] + __shfl_xor(gout[r], 32);
                } else {
                    const int beta = (int)(e >> 4);
#pragma unroll
                    for (int r = 0; r < A; ++r) {
                        const int src = 16 * (r >> 2) + (int)(e & 15u);
                        const float v0 = __shfl(gout[r & 3] + gout[8 + (r & 3)], src);
                        const float v1 = __shfl(gout[4 + (r & 3)] + gout[12 + (r & 3)], src);
                        g[r] = beta ? v1 : v0;
                    }
                }
                if (pk == 0 && writer && active && jq->grad_out) {   // the first gradient leaves here
                    uint32_t lo = li;
                    asm volatile("" : "+v"(lo));
                    float *go = jq->grad_out + (size_t)it * q.act_step_stride;
#pragma unroll
                    for (int j = 0; j < A; ++j) (go + j * q.ld_act_out)[lo] = g[j];
                }
                if (active) {
#pragma unroll
                    for (int r = 0; r < A; ++r) {
                        const float v = a[r] - jq->step * g[r];
                        a[r] = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);      // (the select form: a NaN stays a NaN)
                    }
                }
            }
        } else if constexpr (SHIELD) {
            do {                                                   // (one pass unless SEARCH or GATE)
            // ---------------- safety critic on x = [s, a, 0]: the network (S + A, 1) ----------------
            auto x = [&](int k) __attribute__((always_inline)) {
                if constexpr (SEARCH) return k < S ? s[k] : (k < S + A ? (s_cand < 0 ? a[k - S] : s_u[k - S]) : 0.0f);
                else return k < S ? s[k] : (k < S + A ? a[k - S] : 0.0f);
            };
            if constexpr (CAT != CAT_NONE) {                       // the distributional critic: the same pass, p from the softmax of its 64-row head
                prob = cat_pass(x, [&]() __attribute__((always_inline)) {
                    if constexpr (SEARCH) {                        // (the search's fill chain, below)
                        if (s_cand >= 0) {
                            if (s_cand + 1 < s_passes) cfill(0, gbuf ^ 1, C1.pieces);
                            else if (it + 1 < q.n_steps) fill(0, gbuf ^ 1, L1.pieces);
                        }
                    }
                    else if (it + 1 < q.n_steps) fill(0, gbuf ^ 1, L1.pieces);
                }, mlp_int<0>{});
            } else {
            // (The sigmoid critic's pass.  cat_pass above restates its layer-1 and layer-2 loops on purpose -- moving these lines into a
            // routine both share changes the existing kernels' instructions -- so the two must change together.)
            f32x16 g1[MLP_MT];
            // (one chunk: the actor's lines; two: a loop.  Only so do all eight shield kernels keep the parent's registers and
            // scratch -- with a one-trip loop, or with the two chunks spelled out, some spill more: profiles/mlp_network/isa_diff.txt)
            if constexpr (C1.chunks == 1) {
                __syncthreads();                            // the critic's layer 1 is in s_w[gbuf]
                cfill(1, gbuf ^ 1, MLP_PIECES);
                layer1_chunk(mlp_int<MLP_MT>{}, mlp_int<C1.records>{}, x, g1, gbuf, mlp_int<ACT_RELU>{}, nullptr);
                gbuf ^= 1;
            } else {
#pragma unroll
                for (int c1 = 0; c1 < C1.chunks; ++c1) {
                    __syncthreads();                        // critic layer-1 chunk c1 is in s_w[gbuf]
                    if (c1 + 1 < C1.chunks) cfill(c1 + 1, gbuf ^ 1, C1.pieces);
                    else cfill(C1.chunks, gbuf ^ 1, MLP_PIECES);
                    layer1_chunk(mlp_int<C1.tiles>{}, mlp_int<C1.records>{}, x, g1 + c1 * C1.tiles, gbuf, mlp_int<ACT_RELU>{}, nullptr);
                    gbuf ^= 1;
                }
            }
            f32x4 z4 = {0, 0, 0, 0};
            for (int m2 = 0; m2 < MLP_MT; ++m2) {
                __syncthreads();                            // critic chunk C1.chunks + m2 is in s_w[gbuf]
                if (m2 + 1 < MLP_MT) cfill(C1.chunks + 1 + m2, gbuf ^ 1, MLP_PIECES);
                else if constexpr (SEARCH) {                       // (behind p0's pass the fill waits for the block's vote, below)
                    if (s_cand >= 0) {
                        if (s_cand + 1 < s_passes) cfill(0, gbuf ^ 1, C1.pieces);      // the next candidate's layer 1
                        else if (it + 1 < q.n_steps) fill(0, gbuf ^ 1, L1.pieces);
                    }
                }
                else if constexpr (GATE) {                         // layer 1 of the next member, or of the actor for the next step
                    const bool more = g_mem + 1 < gq->n_members;
                    gsrc = more ? gsrc + MLP_CSTREAM_FLOATS : cstream;
                    if (more) cfill(0, gbuf ^ 1, C1.pieces);
                    else if (it + 1 < q.n_steps) fill(0, gbuf ^ 1, L1.pieces);
                }
                else if (it + 1 < q.n_steps) fill(0, gbuf ^ 1, L1.pieces);   // the actor's layer 1 of the NEXT step
                z4 = layer2_chunk(g1, z4, m2 + 1, gbuf, mlp_int<ACT_RELU>{}, nullptr);
                gbuf ^= 1;
            }
            if constexpr (GATE) {                                  // fold member `g_mem` into the running sums (the law, include/nig.h)
                float z[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) z[c] = z4[c] + __shfl_xor(z4[c], 32);
                if (writer && !(ctr & NIG_CTR_DONE) && gq->logit_out) {   // the logits leave here
                    uint32_t lo = li;
                    asm volatile("" : "+v"(lo));
                    float *zo = gq->logit_out + ((size_t)it * (size_t)gq->n_members + (size_t)g_mem) * gq->c_step_stride;
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (c < gq->n_outputs) (zo + c * gq->ld_c)[lo] = z[c];
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (g_mem == 0) { g_z0[c] = z[c]; g_acc[c] = z[c]; g_s1[c] = 0.0f; g_s2[c] = 0.0f; }
                    else {
                        const float d = z[c] - g_z0[c];
                        g_s1[c] = g_s1[c] + d; g_s2[c] = g_s2[c] + d * d;
                        g_acc[c] = g_acc[c] + z[c];
                    }
                }
            }
            else prob = det_sigmoidf(z4[0] + __shfl_xor(z4[0], 32));
            }
            if constexpr (SEARCH) {
                if (s_cand < 0) {
                    s_best = prob;
                    shield = !(prob < threshold) && !(ctr & NIG_CTR_DONE);     // (lanes past the batch are frozen: they never ask)
                    // p0 leaves here, so that it is dead during the candidate passes
                    if (writer && !(ctr & NIG_CTR_DONE) && prob_out) {
                        uint32_t lo = li;
                        asm volatile("" : "+v"(lo));
                        (prob_out + (uint32_t)it * q.out_stride)[lo] = prob;
                    }
                    s_passes = __syncthreads_or(shield) ? sq->n_candidates : 0;
                    // every wave is past the barrier behind which s_w[gbuf] was last read: it takes the chunk consumed next
                    if (s_passes > 0) cfill(0, gbuf, C1.pieces);
                    else if (it + 1 < q.n_steps) fill(0, gbuf, L1.pieces);
                } else if (shield && (s_cand == 0 || prob < s_best || (s_best != s_best && prob == prob))) {   // the first of least p; a NaN never wins
                    s_best = prob; s_choice = s_cand;
                }
                if (++s_cand < s_passes)                           // (beside the fill of its layer 1, ahead of the chunk barrier)
                    search_candidate<A>(make_key(lane_gi(), t_base + (uint32_t)it + 1u, p.seed_lo, p.seed_hi, s_probit), s_cand, s_u);
            }
            } while (GATE ? ++g_mem < gq->n_members : (SEARCH && s_cand < s_passes));
            if constexpr (SEARCH) {
                if (shield) search_candidate<A>(make_key(lane_gi(), t_base + (uint32_t)it + 1u, p.seed_lo, p.seed_hi, s_probit), s_choice, a);
            } else if constexpr (GATE) {                           // once per step: p and sd of every row, the vote, the zero action
                const float kf = gq->kf;
                const bool live_writer = writer && !(ctr & NIG_CTR_DONE);
                uint32_t lo = li;
                asm volatile("" : "+v"(lo));
                const size_t crow = (size_t)it * gq->c_step_stride + lo;
                bool safe = true, certain = true;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    float v = g_s2[c] - (g_s1[c] * g_s1[c]) / kf;
                    v = v < 0.0f ? 0.0f : v;                       // (a NaN stays a NaN)
                    const float sd = __builtin_sqrtf(v / kf);
                    const float pen = sd > 1.0f ? 1.0f : sd;
                    float pc = det_sigmoidf((g_acc[c] / kf) / gq->temperature) + 0.5f * pen;
                    pc = pc < 0.0f ? 0.0f : (pc > 1.0f ? 1.0f : pc);
                    if (c < gq->n_outputs) {
                        safe = safe && pc < gq->threshold;
                        certain = certain && sd < gq->umax;
                        if (live_writer && gq->prob_out) (gq->prob_out + crow)[(size_t)c * gq->ld_c] = pc;
                        if (live_writer && gq->unc_out) (gq->unc_out + crow)[(size_t)c * gq->ld_c] = sd;
                    }
                }
                g_uncertain = !certain;
                shield = !(safe && certain);
#pragma unroll
                for (int r = 0; r < A; ++r) a[r] = shield ? 0.0f : a[r];     // "reject_conservative"
            } else {
                shield = !(prob < threshold);
#pragma unroll
                for (int r = 0; r < A; ++r) a[r] = shield ? a[r] * 0.5f : a[r];
            }
        }

        // ---------------- IndustrialEnv.step (both lane halves, identical results) ----------------
        const uint32_t orow = (uint32_t)it * q.out_stride;
        uint32_t lo = li;                                          // the lane's index in this step's output addresses
        if constexpr (SEARCH || GATE || PROJECT || LIMITS) asm volatile("" : "+v"(lo)); // (formed here, step by step: no address is kept in registers across the passes; LIMITS: the per-lane xflags address, hoisted out of the step loop, was one more spilled register pair at the 256-register cap)
        const bool frozen = (ctr & NIG_CTR_DONE) != 0;
        if (writer && !frozen) {
            if (q.obs_out) {
                float *oo = q.obs_out + (size_t)it * q.obs_step_stride + (size_t)lo * S;
                if constexpr (S % 4 == 0) {
#pragma unroll
                    for (int k = 0; k < S / 4; ++k) store16(oo + 4 * k, s[4 * k], s[4 * k + 1], s[4 * k + 2], s[4 * k + 3]);
                } else {
#pragma unroll
                    for (int k = 0; k < S; ++k) oo[k] = s[k];
                }
            }
            if (q.act_out) {
                float *ao = q.act_out + (size_t)it * q.act_step_stride;
#pragma unroll
                for (int j = 0; j < A; ++j) (ao + j * q.ld_act_out)[lo] = a[j];
            }
            if constexpr (PROJECT) {
                if (jq->viol_out) {
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (c < jq->n_outputs) (jq->viol_out + (size_t)it * jq->c_step_stride + lo)[(size_t)c * jq->ld_c] = det_sigmoidf(j_z[c]);
                }
                if (jq->iters_out) (jq->iters_out + (uint32_t)it * q.out_stride)[lo] = j_iters;
            }
            if constexpr (SHIELD && !SEARCH && !GATE && !PROJECT) {
                if (prob_out) (prob_out + (uint32_t)it * q.out_stride)[lo] = prob;
            }
            if constexpr (SEARCH) {
                if (sq->risk_out) (sq->risk_out + (uint32_t)it * q.out_stride)[lo] = s_best;
                if (sq->choice_out) (sq->choice_out + (uint32_t)it * q.out_stride)[lo] = s_choice;
            }
            if constexpr (ENS != ENS_NONE) {
                if (eq->unc_out) (eq->unc_out + (uint32_t)it * q.out_stride)[lo] = unc;
            }
        }
        const RngKey key = make_key(lane_gi(), t_base + (uint32_t)it + 1u, p.seed_lo, p.seed_hi, s_probit);
        if constexpr (KS > 0) Env::draw_step(key, nz); else nz[0] = 0;
        const int step_pre = (int)(ctr & NIG_CTR_STEP_MASK);
        StepResult<Env, reward_of<Env, act_t>> res;
        if constexpr (LIMITS) {                    // the added constraints beside the built-ins (nig_limits.hpp): res counts both kinds
            // (the action the env receives: halved, chosen, zeroed, projected, disturbed; the ensemble's float64 one where the env steps on it)
            uint32_t xf;
            if constexpr (ACT64) xf = step_core_limited<Env>((limit_table_ptr)lq->table, s, a64, nz, step_pre, p.max_steps, p.dt32, p.dt, p.cmask, n, res);
            else xf = step_core_limited<Env>((limit_table_ptr)lq->table, s, a, nz, step_pre, p.max_steps, p.dt32, p.dt, p.cmask, n, res);
            if (writer && lq->xflags) (lq->xflags + orow)[lo] = frozen ? 0u : xf;
        }
        else if constexpr (ACT64) step_core<Env>(s, a64, nz, step_pre, p.max_steps, p.dt32, p.dt, p.cmask, n, res);
        else step_core<Env>(s, a, nz, step_pre, p.max_steps, p.dt32, p.dt, p.cmask, n, res);
        const int step = step_pre + 1;
        const uint32_t viol_ep = episode_violations(ctr, res.nviol);
        const bool done = (res.terminated || res.truncated) && !frozen;
        uint32_t fl = pack_flags<Env>(res, step) | did_reset_flag(done && autoreset);
        if constexpr (LIMITS) fl = limited_flag_counts<Env>(fl, res.viol_bits, res.shutdown);
        if constexpr (SHIELD) fl |= shield ? NIG_FLAG_SHIELDED : 0u;
        if constexpr (ENS != ENS_NONE) fl |= uncertain ? NIG_FLAG_UNCERTAIN : 0u;
        if constexpr (GATE) fl |= g_uncertain ? NIG_FLAG_UNCERTAIN : 0u;
        float rew = (float)res.reward;
        if (frozen) {
            fl = NIG_FLAG_INACTIVE | ((ctr & NIG_CTR_STEP_MASK) << NIG_FLAG_STEP_SHIFT);
            rew = 0.0f;
#pragma unroll
            for (int k = 0; k < S; ++k) n[k] = s[k];
        } else {
            ctr = counter_word(step, viol_ep);
            if (tally) ret = add_reward<Env, ACT64>(ret, res.reward);
        }
        if (writer) {
            if (p.reward) (p.reward + orow)[lo] = rew;
            if (p.flags) (p.flags + orow)[lo] = fl;
        }
        if (done) {
            ret = lt.finish(tally, ret, step, viol_ep, res.ncrit);
            if (autoreset) {
                double rn[KR > 0 ? KR : 1];
                Env::draw_init(key, rn);
                Env::init(rn, n);
                ctr = 0u;
            } else {
                ctr |= NIG_CTR_DONE;
            }
        }
#pragma unroll
        for (int k = 0; k < S; ++k) s[k] = n[k];
    }
    if (!writer) return;
#pragma unroll
    for (int k = 0; k < S; ++k) (p.state + k * p.ld_state)[li] = s[k];
    store_episode(p.ctr, p.life_viol, p.ep_ret, p.tally, p.ld, p.n_en, 0u, li, tally, ctr, lt.life, ret, lt);   // (row offset 0: `li` counts from the batch's first lane)
}

template <class Env>
__global__ void __launch_bounds__(BLOCK, 2) rollout_mlp_kernel(const MlpArgs q)
{
    rollout_mlp_body<Env, false>(q, nullptr, nullptr, 0.0f);
}

template <class Env>
__global__ void __launch_bounds__(BLOCK, 2) rollout_mlp_shield_kernel(const MlpShieldArgs q)
{
    rollout_mlp_body<Env, true>(q.m, q.cstream, q.prob_out, q.threshold);
}

// Instantiated in the env's search_*.hip translation unit only (launch_mlp_family).
template <class Env>
__global__ void __launch_bounds__(BLOCK, 2) rollout_mlp_search_kernel(const MlpSearchArgs q)
{
    rollout_mlp_body<Env, true, ENS_NONE, false, true>(q.sh.m, q.sh.cstream, q.sh.prob_out, q.sh.threshold, nullptr, nullptr, &q);
}

// Instantiated in the env's gated_*.hip translation unit only (launch_mlp_family).
template <class Env>
__global__ void __launch_bounds__(BLOCK, 2) rollout_mlp_gated_kernel(const MlpGateArgs q)
{
    rollout_mlp_body<Env, true, ENS_NONE, false, false, true>(q.m, q.cstreams, nullptr, q.threshold, nullptr, nullptr, nullptr, &q);
}

// Instantiated in the env's projected_*.hip translation unit only (launch_mlp_family).
template <class Env>
__global__ void __launch_bounds__(BLOCK, 2) rollout_mlp_projected_kernel(const MlpProjectArgs q)
{
    rollout_mlp_body<Env, true, ENS_NONE, false, false, false, true>(q.m, q.cstream, nullptr, q.threshold, nullptr, nullptr, nullptr, nullptr, &q);
}

// ENS = ENS_AVERAGE / ENS_VOTING.  Instantiated in the env's ensemble_*.hip translation unit only (launch_ensemble_family).
template <class Env, int ENS>
__global__ void __launch_bounds__(BLOCK, 2) rollout_mlp_ensemble_kernel(const MlpEnsArgs q)
{
    rollout_mlp_body<Env, false, ENS>(q.m, nullptr, nullptr, 0.0f, &q);
}

// Instantiated in the env's disturbed_*.hip translation unit only (launch_mlp_family).
template <class Env>
__global__ void __launch_bounds__(BLOCK, 2) rollout_mlp_disturbed_kernel(const MlpDistArgs q)
{
    rollout_mlp_body<Env, false, ENS_NONE, true>(q.m, nullptr, nullptr, 0.0f, nullptr, &q.d);
}

struct MlpLimArgs {
    MlpArgs m;
    LimitArgs l;
};

// The plain actor under the user's added box constraints (include/nig.h "nig-limits-v1"): step_core_limited at the body's one step
// site, a second word per step.  Instantiated in the env's limited_*.hip translation unit only (launch_mlp_family).
template <class Env>
__global__ void __launch_bounds__(BLOCK, 2) rollout_mlp_limited_kernel(const MlpLimArgs q)
{
    rollout_mlp_body<Env, false, ENS_NONE, false, false, false, false, true>(q.m, nullptr, nullptr, 0.0f, nullptr, nullptr, nullptr, nullptr, nullptr, &q.l);
}

// The other families under the added constraints: a parent's argument block with the limits behind it, and the parent's body with
// LIMITS on -- step_core_limited on the action the env receives, limited_flag_counts behind pack_flags (SHIELDED / UNCERTAIN are
// OR-ed in after it), the xflags row.  Each is instantiated in the env's limited_<family>_*.hip translation unit only.
template <class Parent>
struct MlpLimited {
    Parent a;
    LimitArgs l;
};

template <class Env>
__global__ void __launch_bounds__(BLOCK, 2) rollout_mlp_shield_limited_kernel(const MlpLimited<MlpShieldArgs> q)
{
    rollout_mlp_body<Env, true, ENS_NONE, false, false, false, false, true>(q.a.m, q.a.cstream, q.a.prob_out, q.a.threshold, nullptr, nullptr, nullptr, nullptr, nullptr, &q.l);
}

template <class Env>
__global__ void __launch_bounds__(BLOCK, 2) rollout_mlp_search_limited_kernel(const MlpLimited<MlpSearchArgs> q)
{
    rollout_mlp_body<Env, true, ENS_NONE, false, true, false, false, true>(q.a.sh.m, q.a.sh.cstream, q.a.sh.prob_out, q.a.sh.threshold, nullptr, nullptr, &q.a, nullptr, nullptr, &q.l);
}

template <class Env>
__global__ void __launch_bounds__(BLOCK, 2) rollout_mlp_gated_limited_kernel(const MlpLimited<MlpGateArgs> q)
{
    rollout_mlp_body<Env, true, ENS_NONE, false, false, true, false, true>(q.a.m, q.a.cstreams, nullptr, q.a.threshold, nullptr, nullptr, nullptr, &q.a, nullptr, &q.l);
}

template <class Env>
__global__ void __launch_bounds__(BLOCK, 2) rollout_mlp_projected_limited_kernel(const MlpLimited<MlpProjectArgs> q)
{
    rollout_mlp_body<Env, true, ENS_NONE, false, false, false, true, true>(q.a.m, q.a.cstream, nullptr, q.a.threshold, nullptr, nullptr, nullptr, nullptr, &q.a, &q.l);
}

// (ENS_AVERAGE on an HAS_ACT64 env: step_core_limited on the float64 action, as step_limited_kernel<Env, *, true>)
template <class Env, int ENS>
__global__ void __launch_bounds__(BLOCK, 2) rollout_mlp_ensemble_limited_kernel(const MlpLimited<MlpEnsArgs> q)
{
    rollout_mlp_body<Env, false, ENS, false, false, false, false, true>(q.a.m, nullptr, nullptr, 0.0f, &q.a, nullptr, nullptr, nullptr, nullptr, &q.l);
}

template <class Env>
__global__ void __launch_bounds__(BLOCK, 2) rollout_mlp_disturbed_limited_kernel(const MlpLimited<MlpDistArgs> q)
{
    rollout_mlp_body<Env, false, ENS_NONE, true, false, false, false, true>(q.a.m, nullptr, nullptr, 0.0f, nullptr, &q.a.d, nullptr, nullptr, nullptr, &q.l);
}

// The distributional critic's kernels ("nig-categorical-v1").  Instantiated in the env's categorical_*.hip /
// limited_categorical_*.hip translation units only (launch_mlp_family).
template <class Env>
__global__ void __launch_bounds__(BLOCK, 2) rollout_mlp_cat_shield_kernel(const MlpCatShieldArgs q)
{
    rollout_mlp_body<Env, true, ENS_NONE, false, false, false, false, false, CAT_LOOP>(q.sh.m, q.sh.cstream, q.sh.prob_out, q.sh.threshold, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &q.c);
}

template <class Env>
__global__ void __launch_bounds__(BLOCK, 2) rollout_mlp_cat_search_kernel(const MlpCatSearchArgs q)
{
    rollout_mlp_body<Env, true, ENS_NONE, false, true, false, false, false, CAT_LOOP>(q.sr.sh.m, q.sr.sh.cstream, q.sr.sh.prob_out, q.sr.sh.threshold, nullptr, nullptr, &q.sr, nullptr, nullptr, nullptr, &q.c);
}

template <class Env>
__global__ void __launch_bounds__(BLOCK, 2) rollout_mlp_cat_shield_limited_kernel(const MlpLimited<MlpCatShieldArgs> q)
{
    rollout_mlp_body<Env, true, ENS_NONE, false, false, false, false, true, CAT_LOOP>(q.a.sh.m, q.a.sh.cstream, q.a.sh.prob_out, q.a.sh.threshold, nullptr, nullptr, nullptr, nullptr, nullptr, &q.l, &q.a.c);
}

template <class Env>
__global__ void __launch_bounds__(BLOCK, 2) rollout_mlp_cat_search_limited_kernel(const MlpLimited<MlpCatSearchArgs> q)
{
    rollout_mlp_body<Env, true, ENS_NONE, false, true, false, false, true, CAT_LOOP>(q.a.sr.sh.m, q.a.sr.sh.cstream, q.a.sr.sh.prob_out, q.a.sr.sh.threshold, nullptr, nullptr, &q.a.sr, nullptr, nullptr, &q.l, &q.a.c);
}

// nig_mlp_violation_prob: the pass alone, on the caller's columns
template <class Env>
__global__ void __launch_bounds__(BLOCK, 2) mlp_violation_prob_kernel(const MlpCatEvalArgs q)
{
    rollout_mlp_body<Env, true, ENS_NONE, false, false, false, false, false, CAT_EVAL>(q.sh.m, q.sh.cstream, q.sh.prob_out, q.sh.threshold, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &q.c);
}

}  // namespace nig
