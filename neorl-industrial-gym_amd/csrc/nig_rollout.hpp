// nig_rollout.hpp -- the open-loop fused rollout (device code only): RolloutArgs, the LDS plan of a rollout block, rollout_body
// and its one-wave kernels (ring-fed and sampled).  The wide kernels are nig_rollout_wide.hpp, the three-wave form nig_split.hpp.
#pragma once
#include "nig_ring.hpp"
#include "nig_step.hpp"

namespace nig {

// ------------------------------------------------------------------------------------------
// Fused multi-step rollout: n_steps consecutive IndustrialEnv.step calls per lane in ONE launch.
// State, counter word and running return live in registers for the whole launch; per step a
// lane reads only its action (ring slot k % ring_len) and writes only what the caller asked
// for (reward / flag word / observation of that step).  Lanes are independent, so there is no
// barrier between steps: waves drift apart and the divergent reset path costs its average,
// not its maximum.  The arithmetic, the generator keys (t = t_base + k + 1) and the
// bookkeeping are those of step_kernel: n_steps launches of step_kernel and one launch of
// this kernel leave bit-identical state, counters and tallies.
// This is the loop of the reference's own measurement / data-generation harnesses
// (performance_benchmark.py:106-133; chemical_reactor.py:364-405) with the policy replaced by
// a pre-filled action ring.
struct RolloutArgs {
    StepArgs s;                 // actions = ring base; reward/flags = per-step output bases (optional)
    int n_steps;                // steps [it0, n_steps) of the call are run by this launch
    int it0;
    int ring_len; uint32_t slot_stride;          // elements between ring slots
    uint32_t out_stride;                         // elements between per-step reward/flag rows (0: overwrite)
    float *obs_out; uint32_t ld_obs_out; uint64_t obs_step_stride;   // optional trajectory, [n_steps][S][ld] ...
    int obs_aos;                                                     // ... or row-major transitions [n_steps][B][S]
    uint32_t block0;            // first 256-lane block of this launch (the ragged last block is a launch of its own)
    // Injected draws (nig_rollout_noise; the NOISE kernel variants): s.step_noise = [n_steps][KS][ld_noise] float64, the
    // values the reference's np.random calls inside _dynamics returned for call step k (chemical_reactor.py:149,159,
    // power_grid.py:136-144), s.reset_noise = [n_steps][KR][ld_noise], the draws of _get_initial_state for a lane that
    // finishes its episode in call step k (base.py:133-155) -- nig_step's parity convention, one row set per step.
    uint64_t nz_step_stride, nz_reset_stride;   // elements between the row sets of consecutive steps
};

// OUT: 0 = no per-step outputs, 1 = reward + flag word, 2 = + observation rows [S][ld],
//      3 = + observation row-major [B][S].  Compile-time so that the number of stores per
// iteration is static and the wait for the prefetched action is a counted vmcnt(N), not a
// full drain of the iteration's stores.
// FULL: every lane of every block of the launch exists (the host launches the batch's whole 256-lane blocks with
// FULL = true and a ragged last block on its own with FULL = false).  Without lane predication the loop's loads
// and stores sit in one basic block, so the waits for the prefetched actions stay counted vmcnt(N) instead of
// the vmcnt(0) drains the waitcnt pass has to place behind exec-masked memory operations.
// LDS of one rollout block, carved from ONE buffer the kernel declares (the per-env kernels size it for their own
// env and output mode, the mixed-batch kernel for the largest of its envs): generator table, then the env's
// reset scratch, then the per-wave transpose image of the row-major trajectory.
template <class Env, int OUT, int BLK = 256>
struct RolloutLds {
    static constexpr int BLOCK = BLK;            // shadows the file-wide constant
    static constexpr int NWAVE = BLOCK / 64;
    static constexpr int OFF_PROBIT = 16 * PROBIT_BIAS;     // (nig_detmath.hpp probit_fetch: the piece number's bias rides in the DS offset field)
    // Per-wave scratch: the cooperative reset's image [RESET_ROWS][64] and, for the row-major trajectory, the transpose
    // image [16 S] float4 -- ONE region for both (a wave uses them at different points of its step, and its DS
    // operations execute in order).  Separate regions put RobotAssembly's row-major kernel at 66 KB per block, two
    // blocks per CU instead of the three its registers allow.
    static constexpr int IMG_BYTES = Env::COOP_RESET ? Env::RESET_ROWS * 64 * 4 : 0;
    static constexpr int TR_BYTES = OUT == 3 ? 16 * Env::S * 16 : 0;
    static constexpr bool SHARE_SCRATCH = Env::COOP_RESET && OUT == 3;
    static constexpr int WAVE_SCRATCH = SHARE_SCRATCH ? (IMG_BYTES > TR_BYTES ? IMG_BYTES : TR_BYTES) : IMG_BYTES;   // bytes per wave at OFF_IMG
    static constexpr int OFF_IMG = OFF_PROBIT + 768 * 16;                                          // [NWAVE][WAVE_SCRATCH]
    static constexpr int OFF_WLIST = OFF_IMG + NWAVE * WAVE_SCRATCH;                                // uchar [BLOCK]
    static constexpr int OFF_INIT = OFF_WLIST + (Env::COOP_RESET ? BLOCK : 0);                      // float [S][BLOCK]
    static constexpr int OFF_LIST = OFF_INIT + (Env::COMPACT_RESET ? Env::S * BLOCK * 4 : 0);       // ushort [BLOCK]
    static constexpr int OFF_CNT = OFF_LIST + (Env::COMPACT_RESET ? BLOCK * 2 : 0);                 // int [NWAVE]
    static constexpr int OFF_TR = SHARE_SCRATCH ? OFF_IMG : OFF_CNT + (Env::COMPACT_RESET ? 16 : 0);   // v4f [NWAVE][TR_STRIDE]
    static constexpr int TR_STRIDE = (SHARE_SCRATCH ? WAVE_SCRATCH : TR_BYTES) / 16;                // float4 per wave
    static constexpr int IMG_STRIDE = WAVE_SCRATCH / 4;                                             // floats per wave
    static constexpr int BYTES = SHARE_SCRATCH ? OFF_CNT + (Env::COMPACT_RESET ? 16 : 0) : OFF_TR + NWAVE * TR_BYTES;
};

// NOFREEZE (only with FULL): the host has checked that no lane of the handle can be frozen (auto-reset handle, no lane
// holding NIG_CTR_DONE), so the pre-step state is dead once the dynamics have read it -- with the run-time flag the
// "discard the speculative step" path keeps all S pre-step values alive next to the S new ones through the whole step
// (PowerGrid: 32 of the registers that capped it at two waves per SIMD).
// BLK: threads per block (256; 512 for the wide form of envs with a big per-wave LDS scratch: the 12 KiB generator
// table is then shared by eight waves and two blocks = four waves per SIMD fit a CU).
// NOISE: the reference's recorded draws are injected instead of the generator's (RolloutArgs::nz_*): the step's process
// noise is loaded as the float64 values the dynamics' parity branch takes, and a finishing lane restarts from
// Env::init(recorded draws) -- _get_initial_state itself, per lane, in place of the cooperative / compacted schemes
// (whose work items contain the generator).  Every other instruction of the step is the timed kernel's.
// RING (the paired form of an env with many draws per step, PowerGrid: rollout_pg_pair_kernel<.., REG>): the step's normals
// come from a PRODUCER wave through an LDS ring (nig_pg_lds.hpp pg_pair_producer: [generator block][lane] float4 slots of raw
// normals, two slots, counters at ring_sync) instead of this wave's own generator; the caller has staged the generator's table
// and passed the block barrier.  State, counters and tallies stay in REGISTERS: at the two waves per SIMD of that form the
// register file has room for them, and the step is then one dependent chain of arithmetic instead of a chain of LDS round trips.
// SAMPLED (nig_rollout_sampled): there is no action ring -- the action of the step with launch counter t is drawn here, blocks
// STREAM_ACTION + j of the lane's key at t (sample_action: what nig_fill_actions(t) writes for the lane), at the point of the step
// where the ring-fed form issues the refill load of the same register set, DEPTH steps ahead of its use: the rounds of those one
// or two generator blocks run in the shadow of the step's stores, and the loop holds no global load at all.
template <class Env, int OUT, bool PAIRED, bool FULL, bool NOFREEZE = false, int BLK = 256, bool NOISE = false, bool RING = false,
          bool SAMPLED = false>
__device__ __forceinline__ void rollout_body(const RolloutArgs &q, const uint32_t base, unsigned char *smem,
                                             const v4f *ring_slots = nullptr, lds_u32_t *ring_sync = nullptr)
{
    static_assert(!NOFREEZE || FULL, "NOFREEZE is a property of whole-block launches");
    static_assert(!NOISE || !PAIRED, "injected draws: nothing to share between the steps of a pair");
    static_assert(!SAMPLED || !NOISE, "recorded draws come with recorded actions");
    static_assert(!RING || (!NOISE && !PAIRED && FULL && NOFREEZE && Env::KS > 4 && std::is_same<typename Env::fast_noise_t, float>::value),
                  "ring-fed form: whole blocks of an env with float32 step noise");
    static_assert(BLK == 256 || (Env::COOP_RESET && !Env::COMPACT_RESET), "wide blocks: no block barrier inside the loop");
    constexpr int BLOCK = BLK;                   // shadows the file-wide constant
    constexpr int S = Env::S, A = Env::A, KS = Env::KS, KR = Env::KR;
    constexpr int KSN = KS > 0 ? KS : 1;
    // Envs whose episodes are short (PowerGrid ~6 steps, RobotAssembly: most waves see a reset
    // every step) compact the finishing lanes of the 256-lane block through LDS each step and let
    // ONE wave produce all their initial states at full lane utilisation; the owners read them
    // back from LDS.  Costs two block barriers per step, saves running the whole reset path in
    // every wave for a few active lanes.  ChemicalReactor (0.3 % of lanes per step) keeps the
    // barrier-free divergent form.
    constexpr bool COMPACT = Env::COMPACT_RESET && !NOISE;
    // COOP (PowerGrid: ~11 lanes of every wave finish in every step): each WAVE produces the initial states of
    // its own finishing lanes cooperatively -- work item = (finishing lane, generator block) -> a few state rows,
    // spread over all 64 lanes through a wave-private LDS image.  No block barrier (waves keep drifting), the
    // generator runs at ~70 % lane utilisation instead of one wave carrying the whole block's resets while three
    // wait (53 % of the wave cycles of round 1's kernel were spent at those barriers).
    constexpr bool COOP = Env::COOP_RESET && !NOISE;
    static_assert(!(COMPACT && COOP), "one reset scheme per env");
    constexpr int NWAVE = BLOCK / 64;
    using Lds = RolloutLds<Env, OUT, BLK>;
    float4 *const s_probit = reinterpret_cast<float4 *>(smem + Lds::OFF_PROBIT);
    float *const s_img = reinterpret_cast<float *>(smem + Lds::OFF_IMG);         // per wave: [RESET_ROWS][64] initial states, column = owner lane
    unsigned char *const s_wlist = smem + Lds::OFF_WLIST;                        // per wave: lanes that finished, in lane order
    float *const s_init = reinterpret_cast<float *>(smem + Lds::OFF_INIT);
    unsigned short *const s_list = reinterpret_cast<unsigned short *>(smem + Lds::OFF_LIST);
    int *const s_cnt = reinterpret_cast<int *>(smem + Lds::OFF_CNT);
    v4f *const s_tr = reinterpret_cast<v4f *>(smem + Lds::OFF_TR);               // per wave: [16 S] transpose image of the row-major observation rows (64 x S floats)
    if constexpr (!RING) {                 // (ring-fed form: the kernel staged the table with all its waves)
        for (int i_ = (int)threadIdx.x; i_ < 768; i_ += BLOCK) s_probit[i_] = NIG_PROBIT[i_];
        __syncthreads();                   // every thread of the block passes here before any early exit
    }
    [[maybe_unused]] uint32_t ring_seen = 0u;
    const StepArgs &p = q.s;
    const unsigned tid = threadIdx.x;
    const bool in_range = FULL ? true : (base + tid < p.B);
    if constexpr (FULL) {
    } else if constexpr (COOP) {
        if (base + (tid & ~63u) >= p.B) return;   // whole wave out of range; a partial wave keeps all 64 lanes as workers
    } else if constexpr (!COMPACT) {
        if (!in_range) return;       // compacting blocks keep every thread for the barriers.  (From here on the
    }                                // compiler knows in_range: no exec masking around the loop's loads and stores.)
    const uint32_t t_base = (p.t_ptr ? *p.t_ptr : 0u) + p.t_off;      // step k uses t_base + k + 1
    const uint64_t gi = p.env0 + (uint64_t)(base + tid);
    const bool autoreset = (p.hflags & NIG_F_AUTORESET) != 0;
    const bool tally = p.tally != nullptr;

    uint32_t ctr = in_range ? (p.ctr + base)[tid] : (uint32_t)NIG_CTR_DONE;   // out-of-range lanes idle as "frozen"
    float s[S], a[A], n[S];
#pragma unroll
    for (int k = 0; k < S; ++k) s[k] = in_range ? (p.state + base + k * p.ld_state)[tid] : 0.0f;
    // running episode return in the precision the reference accumulates it in (float32 for ChemicalReactor:
    // the stored double is exactly that float), widened only when an episode ends
    using ret_t = std::conditional_t<Env::RET_F32, float, double>;
    ret_t ret = (tally && in_range) ? (ret_t)(p.ep_ret + base)[tid] : (ret_t)0;
    LaneTally lt;
    lt.clear();
    // Actions are prefetched TWO steps ahead into two ping-pong register sets (the loop is unrolled
    // by two so no register copy sits between load and use).  vmcnt retires in issue order, so the
    // wait for a prefetched action also waits for every store issued before it; at distance 2 those
    // are the stores of two steps ago, acknowledged long before (a distance-1 prefetch stalled ~20 %
    // of the wave's cycles on the previous step's store acknowledgements).
    //
    // PAIRED (envs that share one Philox block between the two steps of a pair of launch counters
    // 2k-1, 2k: ChemicalReactor; the launch must start on an odd counter, the host peels a misaligned
    // first step into a launch of the unpaired form): process noise is produced one step AHEAD, in the
    // shadow of the current step's stores -- the tail of a pair's second step runs the Philox rounds of
    // the next pair and the normal transform of its first step, the tail of the first step transforms
    // the two words kept for the second.  One block per two steps, LDS table latency off the critical
    // path.
    constexpr bool SHARE = PAIRED;
    static_assert(!PAIRED || (Env::SHARED_STEP_BLOCK && KS > 0 && KS <= 2), "a shared step block holds two steps");
    [[maybe_unused]] const float *ring = p.actions + base;
    // DEPTH = steps of slack between an action load and its use = ring of register sets = loop unroll.
    // The wait for a prefetched action is in-order with the stores issued before it; at the headline
    // size a step is ~1.2 us and a streaming store takes longer than two of them to be acknowledged.
    // Four steps for the envs whose step is short enough that four copies stay inside the I-cache.
    constexpr int DEPTH = PAIRED ? 4 : 2;
    float buf[DEPTH][A];
    using nz_t = std::conditional_t<NOISE, double, typename Env::fast_noise_t>;   // injected draws are fp64
    nz_t nzA[KSN], nzB[KSN];
    nzA[0] = (nz_t)0; nzB[0] = (nz_t)0;
    uint32_t kept0 = 0u, kept1 = 0u;          // words 2-3 of the current pair's block
    int slot = 0;
    // Wave-uniform running pointers instead of it * stride products: the per-step 64-bit scalar
    // multiplies and adds of the address arithmetic were ~40 of the step's ~80 SALU issue slots.
    const float *act_next = ring;              // ring slot of the step whose action is fetched next
    float *rew_row = p.reward ? p.reward + base + (size_t)q.it0 * q.out_stride : nullptr;
    uint32_t *fl_row = p.flags ? p.flags + base + (size_t)q.it0 * q.out_stride : nullptr;
    float *obs_row = nullptr;                  // this step's observation block / rows
    // (OUT == 3: the wave's first lane through readfirstlane -- the block pointer is wave-uniform, and only then does the
    // compiler keep it in scalar registers: the KiB stores within the instruction's 4 KiB immediate range are issued as
    // "scalar base + 32-bit lane offset", one 64-bit address computation less per step.  No measurable effect on the
    // launch time, profiles/r03/store_addr.txt and the A/B beside it.)
    if constexpr (OUT == 3)
        obs_row = q.obs_out + (size_t)q.it0 * q.obs_step_stride + (size_t)(base + __builtin_amdgcn_readfirstlane(tid & ~63u)) * S;
    if constexpr (OUT == 2) obs_row = q.obs_out + (size_t)q.it0 * q.obs_step_stride + base;
    // block-uniform: lanes can be frozen (finished and waiting for reset -- also on an auto-reset handle whose lanes
    // were never reset, left out by reset(mask) or marked done by set_state: base.py:159-160 -- or out of range)
    const bool may_freeze = NOFREEZE ? false : (!autoreset || (p.hflags & HF_MAY_HOLD_DONE) != 0 || (!FULL && base + BLOCK > p.B));

    auto one_step = [&](auto pos_tag, float (&abuf)[A], nz_t (&nz)[KSN], const int it) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < A; ++k) a[k] = abuf[k];
        const bool frozen = may_freeze && (ctr & NIG_CTR_DONE) != 0;   // no auto-reset: base.py:159-160
        const RngKey key = make_key(gi, t_base + (uint32_t)it + 1u, p.seed_lo, p.seed_hi, s_probit);
        const int step_pre = (int)(ctr & NIG_CTR_STEP_MASK);
        StepResult<Env> res;
        if constexpr (NOISE) {
            if constexpr (KS > 0) {
                const double *nzr = p.step_noise + (size_t)it * q.nz_step_stride + base;
#pragma unroll
                for (int k = 0; k < KS; ++k) nz[k] = in_range ? (nzr + (size_t)k * p.ld_noise)[tid] : 0.0;
            }
        } else if constexpr (RING) {
            // the producer's slot of this step: raw normals, [generator block][lane]; scaled here exactly as Env::draw_step does
            const int itl = it - q.it0;
            if (ring_seen < (uint32_t)itl + 1u) ring_seen = split_wait(ring_sync + 0, (uint32_t)itl + 1u);
            constexpr int NB = (KS + 3) / 4;
            const v4f *slot = ring_slots + (itl & 1) * (NB * 64) + (tid & 63u);
            float z[4 * NB];
#pragma unroll
            for (int j = 0; j < NB; ++j) { const v4f w = slot[64 * j]; z[4 * j] = w.x; z[4 * j + 1] = w.y; z[4 * j + 2] = w.z; z[4 * j + 3] = w.w; }
            split_post(ring_sync + 1, (uint32_t)itl + 1u, tid & 63u);     // (DS order: the reads above execute before this write)
            Env::scale_step_normals(z, nz);
        } else if constexpr (KS > 0 && !SHARE) draw_one<Env>(key, nz);
        step_core<Env>(s, a, nz, step_pre, p.max_steps, p.dt32, p.dt, p.cmask, n, res);
        const int step = step_pre + 1;
        const uint32_t viol_ep = episode_violations(ctr, res.nviol);
        const bool done = (res.terminated || res.truncated) && !frozen;
        uint32_t fl = pack_flags<Env>(res, step);
        float rew = (float)res.reward;
        if (may_freeze) {                          // skipped wholesale (scalar branch) when no lane can be frozen
            if (frozen) {                          // untouched lane: discard the speculative step
                fl = frozen_flag_word(ctr);
                rew = 0.0f;
#pragma unroll
                for (int k = 0; k < S; ++k) n[k] = s[k];
            }
        }
        if (!frozen) {
            ctr = counter_word(step, viol_ep);
            if (tally) ret = add_reward<Env>(ret, res.reward);
        }
        // Next step's process noise, first half: (second step of a pair) the Philox rounds of the next
        // pair, then the index arithmetic and the LDS table reads of the two draws.  The cubic that
        // consumes them runs after this step's stores: the reads' latency is covered by the store traffic
        // instead of a wait.
        ProbitFetch pf[KSN];
        if constexpr (decltype(pos_tag)::value == 2) {         // next pair: counters t+1, t+2
            const u32x4 x = pair_block<Env>(make_key(gi, t_base + (uint32_t)it + 2u, p.seed_lo, p.seed_hi, s_probit));
            pair_fetch<Env>(x.x, x.y, s_probit, pf);
            kept0 = x.z; kept1 = x.w;
            __builtin_amdgcn_sched_barrier(0);     // keep it here: hipcc would sink it back to its consumer
        } else if constexpr (decltype(pos_tag)::value == 1) {  // this pair's second step
            pair_fetch<Env>(kept0, kept1, s_probit, pf);
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (OUT == 3) {                  // stage this lane's row; read back transposed below
            if constexpr (S % 4 == 0) {
                v4f *tr = s_tr + (tid >> 6) * Lds::TR_STRIDE + (tid & 63u) * (S / 4);
#pragma unroll
                for (int k = 0; k < S / 4; ++k) { v4f v = {n[4 * k], n[4 * k + 1], n[4 * k + 2], n[4 * k + 3]}; tr[k] = v; }
            } else {
                float *tr = reinterpret_cast<float *>(s_tr + (tid >> 6) * Lds::TR_STRIDE) + (tid & 63u) * S;
#pragma unroll
                for (int k = 0; k < S; ++k) tr[k] = n[k];
            }
        }
        // Refill this buffer with the action of step it+DEPTH, issued BEFORE this step's stores: the
        // registers of `a` are dead by now (the load lands in place, no rotation of register sets),
        // and the in-order vmcnt wait at the top of step it+DEPTH then only needs the stores of step
        // it-1 and older to have been acknowledged -- DEPTH full steps of slack.
        if constexpr (SAMPLED) {
            sample_action<Env>(make_key(gi, t_base + (uint32_t)(it + DEPTH) + 1u, p.seed_lo, p.seed_hi), abuf);
        } else {
#pragma unroll
            for (int k = 0; k < A; ++k) abuf[k] = in_range ? (act_next + k * p.ld_act)[tid] : 0.0f;
            slot = (slot + 1 == q.ring_len) ? 0 : slot + 1;
            act_next = (slot == 0) ? ring : act_next + q.slot_stride;
        }
        if constexpr (OUT == 3) {
            // row-major transitions [step][lane][S] (the D4RL "observations[N,S]" layout).  A lane's row is
            // 4*S contiguous bytes, but written lane by lane every store instruction would scatter 64
            // 16-byte pieces at a 4*S-byte stride (partial lines: -15 % against the [S][lane] layout, -45 %
            // with streaming stores).  The wave's 64 rows are one contiguous 256*S-byte block, so they go
            // through a wave-private LDS image and leave in lane-contiguous order: S/4 stores of one
            // contiguous KiB each.  (DS operations of one wave execute in order: the reads see the writes
            // issued above without a wait in between.)
            const unsigned lane = tid & 63u, wave_env0 = base + (tid & ~63u);
            const v4f *tr = s_tr + (tid >> 6) * Lds::TR_STRIDE;
            image_rows_fence();                    // the reads below are OTHER lanes' writes
            v4f *oo = reinterpret_cast<v4f *>(obs_row);
            constexpr int NV = (16 * S + 63) / 64;  // float4 pieces per lane: the wave's block is 64*S floats = 16*S float4
            v4f v[NV];
#pragma unroll
            for (int k = 0; k < NV; ++k) v[k] = tr[(16 * S % 64 == 0 || lane + 64u * k < 16u * S) ? lane + 64u * k : 0u];
            if (FULL || wave_env0 + 64u <= p.B) {  // wave-uniform: the whole wave exists
#pragma unroll
                for (int k = 0; k < NV; ++k)
                    if (16 * S % 64 == 0 || lane + 64u * k < 16u * S) stream_store(oo + lane + 64u * k, v[k]);
            } else if (in_range) {                 // the batch's last, partial wave (its other lanes may have exited):
                float *row = obs_row + (size_t)lane * S;       // every live lane writes its own row
                if constexpr (S % 4 == 0) {
#pragma unroll
                    for (int k = 0; k < S / 4; ++k) store16(row + 4 * k, n[4 * k], n[4 * k + 1], n[4 * k + 2], n[4 * k + 3]);
                } else {
#pragma unroll
                    for (int k = 0; k < S; ++k) row[k] = n[k];
                }
            }
        }
        if (in_range) {
        if constexpr (OUT == 2) {
#pragma unroll
            for (int k = 0; k < S; ++k) stream_store(obs_row + k * q.ld_obs_out + tid, n[k]);
        }
        if constexpr (OUT >= 1) {
            stream_store(rew_row + tid, rew);
            stream_store(fl_row + tid, fl | did_reset_flag(done && autoreset));
        }
        }   // in_range
        if constexpr (OUT >= 1) { rew_row += q.out_stride; fl_row += q.out_stride; }
        if constexpr (OUT >= 2) obs_row += q.obs_step_stride;
        if constexpr (decltype(pos_tag)::value == 2) {         // second half: the normals themselves
            __builtin_amdgcn_sched_barrier(0);
            pair_eval<Env>(pf, nzA);
        } else if constexpr (decltype(pos_tag)::value == 1) {
            __builtin_amdgcn_sched_barrier(0);
            pair_eval<Env>(pf, nzB);
        }
        if (done) {
            lt.life += (long long)viol_ep;
            if (tally) { lt.episode((double)ret, step, viol_ep, res.ncrit); ret = (ret_t)0; }
            if (!autoreset) ctr |= NIG_CTR_DONE;
        }
        if constexpr (COOP) {
            const unsigned long long m = __ballot(done && autoreset);
            if (m != 0ull) {                       // wave-uniform
                const unsigned lane = tid & 63u, wave = tid >> 6;
                coop_reset<Env>(m, done, lane, s_img + wave * Lds::IMG_STRIDE, s_wlist + wave * 64,
                                p.env0 + (uint64_t)(base + (tid & ~63u)), t_base + (uint32_t)it + 1u, p.seed_lo, p.seed_hi,
                                s_probit, n);
                if (done) ctr = 0u;
            }
        } else if constexpr (!COMPACT) {
            if (done && autoreset) {               // divergent per-lane reset (base.py:133-155)
                double rn[KR > 0 ? KR : 1];
                if constexpr (NOISE) {             // _get_initial_state on the recorded draws of this step's row set
                    const double *rnr = p.reset_noise + (size_t)it * q.nz_reset_stride + base;
#pragma unroll
                    for (int k = 0; k < KR; ++k) rn[k] = (rnr + (size_t)k * p.ld_noise)[tid];
                } else {
                    Env::draw_init(key, rn);
                }
                Env::init(rn, n);
                ctr = 0u;
            }
        } else if (autoreset) {                    // block-uniform
            const unsigned wave = tid >> 6, lane = tid & 63u;
            const unsigned long long m = __ballot(done);
            const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));   // finishing lanes below this one (v_mbcnt: no per-lane mask register)
            if (lane == 0) s_cnt[wave] = __popcll(m);
            if (done) s_list[wave * 64 + rank] = (unsigned short)tid;
            __syncthreads();
            int cnt[NWAVE], total = 0, mine = rank;
#pragma unroll
            for (int w = 0; w < NWAVE; ++w) { cnt[w] = s_cnt[w]; mine += ((unsigned)w < wave) ? cnt[w] : 0; total += cnt[w]; }
            // the worker role rotates over the block's waves so no SIMD carries it every step
            const unsigned widx = (tid + BLOCK - 64u * ((unsigned)it & (NWAVE - 1))) & (BLOCK - 1);
            for (int j = (int)widx; j < total; j += BLOCK) {
                int w = 0, r = j;
#pragma unroll
                for (int qq = 0; qq < NWAVE - 1; ++qq) { const bool nxt = (w == qq) && (r >= cnt[qq]); r = nxt ? r - cnt[qq] : r; w = nxt ? qq + 1 : w; }
                const unsigned tl = s_list[w * 64 + r];
                double rn[KR > 0 ? KR : 1];
                Env::draw_init(make_key(p.env0 + (uint64_t)(base + tl), t_base + (uint32_t)it + 1u, p.seed_lo, p.seed_hi, s_probit), rn);
                float r0[S];
                Env::init(rn, r0);
#pragma unroll
                for (int k = 0; k < S; ++k) s_init[k * BLOCK + j] = r0[k];
            }
            __syncthreads();
            if (done) {
#pragma unroll
                for (int k = 0; k < S; ++k) n[k] = s_init[k * BLOCK + mine];
                ctr = 0u;
            }
        }
#pragma unroll
        for (int k = 0; k < S; ++k) s[k] = n[k];
    };

    int it = q.it0;
    if constexpr (!SAMPLED) slot = it % q.ring_len;
    if constexpr (SHARE) {
        const u32x4 x = pair_block<Env>(make_key(gi, t_base + (uint32_t)it + 1u, p.seed_lo, p.seed_hi, s_probit));
        pair_noise<Env>(x.x, x.y, s_probit, nzA);
        kept0 = x.z; kept1 = x.w;
    }
    if constexpr (SAMPLED) {
#pragma unroll
        for (int j = 0; j < DEPTH; ++j) sample_action<Env>(make_key(gi, t_base + (uint32_t)(it + j) + 1u, p.seed_lo, p.seed_hi), buf[j]);
    } else {
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) {                                  // steps it .. it + DEPTH - 1
        const float *nx = ring + (size_t)slot * q.slot_stride;
#pragma unroll
        for (int k = 0; k < A; ++k) buf[j][k] = in_range ? (nx + k * p.ld_act)[tid] : 0.0f;
        slot = (slot + 1 == q.ring_len) ? 0 : slot + 1;
    }
    act_next = ring + (size_t)slot * q.slot_stride;                   // step it + DEPTH: the first refill
    }
    // Drain the prologue loads HERE (vmcnt(0); expcnt/lgkmcnt untouched).  Otherwise hipcc's waitcnt
    // pass merges "prologue loads still in flight" into the loop header and every iteration inherits
    // waits sized for the first one.
    __builtin_amdgcn_s_waitcnt(0x0F70);

    // no conditional inside the loop: a phi on the action registers would put register copies (and
    // with them the wait for the freshest loads) on the back edge
    using first = std::integral_constant<int, SHARE ? 1 : 0>;      // position in the pair (0: unpaired env)
    using second = std::integral_constant<int, SHARE ? 2 : 0>;
    for (; it + DEPTH <= q.n_steps; it += DEPTH) {
#pragma unroll
        for (int j = 0; j < DEPTH; j += 2) {
            one_step(first{}, buf[j], nzA, it + j);
            one_step(second{}, buf[j + 1], nzB, it + j + 1);
        }
    }
    // tail: at most DEPTH - 1 steps (noise drawn past the last step is simply not used)
    static_assert(DEPTH == 2 || DEPTH == 4, "tail written out for these depths");
    if (it < q.n_steps) one_step(first{}, buf[0], nzA, it);
    if constexpr (DEPTH == 4) {
        if (it + 1 < q.n_steps) one_step(second{}, buf[1], nzB, it + 1);
        if (it + 2 < q.n_steps) one_step(first{}, buf[2], nzA, it + 2);
    }
    if (!in_range) return;
#pragma unroll
    for (int k = 0; k < S; ++k) (p.state + base + k * p.ld_state)[tid] = s[k];
    store_episode(p.ctr, p.life_viol, p.ep_ret, p.tally, p.ld, p.n_en, base, tid, tally, ctr, lt.life, ret, lt);
}

template <class Env, int OUT, bool PAIRED, bool FULL, bool NOISE = false>
__global__ void __launch_bounds__(BLOCK, Env::ROLLOUT_WAVES) rollout_kernel(const RolloutArgs q)
{
    __shared__ __attribute__((aligned(16))) unsigned char smem[RolloutLds<Env, OUT>::BYTES];
    rollout_body<Env, OUT, PAIRED, FULL, false, 256, NOISE>(q, (blockIdx.x + q.block0) * BLOCK, smem);
}
// nig_rollout_sampled's twin (a kernel name of its own: tools that pick kernels by name never confuse the two)
template <class Env, int OUT, bool PAIRED, bool FULL>
__global__ void __launch_bounds__(BLOCK, Env::ROLLOUT_WAVES) rollout_sampled_kernel(const RolloutArgs q)
{
    __shared__ __attribute__((aligned(16))) unsigned char smem[RolloutLds<Env, OUT>::BYTES];
    rollout_body<Env, OUT, PAIRED, FULL, false, 256, false, false, true>(q, (blockIdx.x + q.block0) * BLOCK, smem);
}

// The wide form (envs that declare WIDE_ROLLOUT_BLOCK): whole blocks of BLK lanes of a handle on which no lane can be
// frozen.  q.block0 counts 256-lane blocks.
template <class E, class = void> struct wide_rollout : std::integral_constant<int, 0> {};
template <class E> struct wide_rollout<E, std::void_t<decltype(E::WIDE_ROLLOUT_BLOCK)>> : std::integral_constant<int, E::WIDE_ROLLOUT_BLOCK> {};

}  // namespace nig
