/*
 * nig.h -- C ABI of libnig.so: the MI355X-native batched simulator for the
 * IndustrialEnv.step() hot path of neoRL-industrial-gym.
 *
 * The reference has NO native/FFI layer: its boundary is the
 * Python class surface IndustrialEnv.reset/step (environments/base.py:133-213),
 * utils.make (utils.py:12-39) and utils.evaluate_with_safety (utils.py:42-154).
 * Each entry point below names the reference interface it stands in for.  The
 * Python mirror of that surface (neorl-industrial-gym_amd/) is a thin ctypes shim
 * over exactly these symbols; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every function returns an int status, 0 = NIG_OK; nig_last_error() explains
 *     the last failure on the calling thread;
 *   - all data pointers are DEVICE pointers unless a parameter says "host";
 *   - batch arrays are structure-of-arrays: row k of a [R][B] array starts at
 *     element k*ld, where ld = nig_layout.ld (B rounded up to 64) for library-owned
 *     arrays and ld = the ld_* argument for caller-owned arrays;
 *   - every launch goes to the caller-supplied hipStream_t (passed as void*), no
 *     hidden synchronisation; a handle is not thread-safe, distinct handles are;
 *   - there is no CPU fallback: without a HIP device nig_create fails.
 *
 * Memory footprint (pinned by tests/test_gpu_footprint.py for every entry point and kernel form)
 *   - a call writes only the documented words of the documented rows of its output arguments: columns [0, batch) of a
 *     row, rows [0, n_steps) of a per-step output (one row / one block where a stride of 0 means "overwrite": it ends
 *     holding the last step's values).  It never writes the pad columns [batch, pitch) of a row, the gap between the end
 *     of a row set and the next step's (any stride above the stated minimum is legal, odd ones included), or anything
 *     before or behind a buffer; in the workspace it never writes the pad columns [batch, ld) of the library-owned arrays;
 *   - input arguments are never written, and the pad columns and stride gaps of an input (action rings, noise rows) never
 *     influence a result: they may hold anything, NaN and infinities included;
 *   - a pitch or stride below its stated minimum is NIG_ERR_INVALID and nothing is written;
 *   - no alignment beyond the element size (4 bytes for float / uint32 / int32, 8 for double) is required of a caller
 *     buffer unless the argument's text says so (the workspace: 256 bytes; row-major observation trajectories: 16 bytes),
 *     and results do not depend on the alignment or pitch chosen.
 */
#ifndef NIG_H
#define NIG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NIG_OK 0
#define NIG_ERR_INVALID 1      /* bad argument                                   */
#define NIG_ERR_HIP 2          /* a HIP runtime call failed                      */
#define NIG_ERR_NODEVICE 3     /* no usable HIP device                           */
#define NIG_ERR_UNSUPPORTED 4

/* environment ids: the registry of utils.py:26-32 (working environments) */
#define NIG_ENV_CHEMICAL_REACTOR 0   /* 'ChemicalReactor-v0'  environments/chemical_reactor.py */
#define NIG_ENV_POWER_GRID 1         /* 'PowerGrid-v0'        environments/power_grid.py       */
#define NIG_ENV_ROBOT_ASSEMBLY 2     /* 'RobotAssembly-v0'    environments/robot_assembly.py   */
/* Candidate rows: registered upstream (utils.py:30-31) but NOT instantiable there;
 * restated from the source text, no reference output exists to pin them. */
#define NIG_ENV_ADV_CHEMICAL_REACTOR 3   /* 'AdvancedChemicalReactor-v0'  environments/advanced_chemical_reactor.py */
#define NIG_ENV_ADV_POWER_GRID 4         /* 'AdvancedPowerGrid-v0'        environments/advanced_power_grid.py       */
/* BUILD-SPECIFIED environments: the reference's README lists them (README.md:28-32: name, dims,
 * constraint names) and ships no implementation -- no reference output exists, parity is undefined.
 * Plants: neorl-industrial-gym_amd/spec_plants.py.  They complete BASELINE's "all 7 envs" mixed batch. */
#define NIG_ENV_HVAC_CONTROL 5       /* 'HVACControl-v0'      18 / 5  */
#define NIG_ENV_WATER_TREATMENT 6    /* 'WaterTreatment-v0'   15 / 4  */
#define NIG_ENV_STEEL_ANNEALING 7    /* 'SteelAnnealing-v0'   20 / 6  */
#define NIG_ENV_SUPPLY_CHAIN 8       /* 'SupplyChain-v0'      28 / 10 */
#define NIG_NUM_ENVS 9

/* nig_create flags */
#define NIG_F_AUTORESET 0x1u   /* finished lanes re-sample their initial state inside the step kernel   */
#define NIG_F_TALLY 0x2u       /* keep per-lane episode tallies (what evaluate_with_safety aggregates)   */

/* per-lane flag word written by nig_step (one uint32 per env instance per step) */
#define NIG_FLAG_TERMINATED 0x1u        /* base.py:190,195-197                               */
#define NIG_FLAG_TRUNCATED 0x2u         /* base.py:191                                       */
#define NIG_FLAG_VIOL0 0x4u             /* constraint k violated on the pre-state: bit 2+k   */
#define NIG_FLAG_VIOL_SHIFT 2
#define NIG_FLAG_NVIOL_SHIFT 5          /* bits 5-6: SafetyMetrics.violation_count (0..3)    */
#define NIG_FLAG_NCRIT_SHIFT 7          /* bits 7-8: SafetyMetrics.critical_violations       */
#define NIG_FLAG_SHUTDOWN 0x200u        /* info['critical_shutdown'], base.py:210            */
#define NIG_FLAG_DID_RESET 0x400u       /* lane auto-reset in this call (state = new episode)*/
#define NIG_FLAG_INACTIVE 0x800u        /* lane was already done (no auto-reset): untouched  */
#define NIG_FLAG_VIOL3 0x1000u          /* 4th safety condition violated (Advanced envs)     */
#define NIG_FLAG_NVIOL_HI 0x2000u       /* adds 4 to the violation count field (Advanced envs) */
#define NIG_FLAG_SHIELDED 0x4000u       /* nig_rollout_mlp_safe: the safety critic halved the action (nig_rollout_mlp_search: replaced it; nig_rollout_mlp_gated: the gate replaced it by zero; nig_rollout_mlp_projected: the lane was projected) */
#define NIG_FLAG_UNCERTAIN 0x8000u      /* nig_rollout_mlp_ensemble: uncertainty > threshold on this live step (nig_rollout_mlp_gated: some sd[c] is not below the spread limit) */
#define NIG_FLAG_STEP_SHIFT 16          /* bits 16-31: current_step after this call          */

/* per-lane counter word kept by the library */
#define NIG_CTR_STEP_MASK 0x7fffu       /* current_step (base.py:187)                        */
#define NIG_CTR_DONE 0x8000u            /* self.done (base.py:192,197)                       */
#define NIG_CTR_VIOL_SHIFT 16           /* violation_count of the running episode (base.py:182) */
#define NIG_MAX_EPISODE_STEPS 21845     /* keeps 3*steps inside 16 bits                      */
#define NIG_MAX_BATCH (1 << 24)         /* lanes per handle: row offsets stay 32-bit scalars */
#define NIG_MAX_PITCH (1 << 26)         /* largest caller row pitch (elements)               */

/* rows of the tally array (NIG_F_TALLY), all stored as double, one column per lane.
 * Count rows (EPISODES, LEN_SUM, VIOL, CRIT, SHUTDOWN, SUCCESS, SATISFIED, CONSTRAINTS) hold integers and every add to them is
 * an integer-valued float64 add: EXACT while a sum stays below 2^53 = 9.0e15 -- per lane, per GPU after nig_reduce_tally, and
 * across ranks after the rank-order combine ("counts must be reduced as integers, never fp32": no float32 is ever
 * involved; at the headline's 6.7e9 violations per 0.6 s a single GPU would need ~9 days of continuous stepping to reach the
 * bound).  A host that needs more sums the partial vectors of shorter runs (fresh handles) in integers itself;
 * parallel.metrics_from_partial rounds the float64 sums to int, which is the identity below 2^53. */
enum {
    NIG_T_EPISODES = 0,   /* finished episodes                                   utils.py:120 */
    NIG_T_RET_SUM,        /* sum of episode returns                              utils.py:130 */
    NIG_T_RET_SQ,         /* sum of squared episode returns                      utils.py:131 */
    NIG_T_RET_MIN,        /*                                                     utils.py:132 */
    NIG_T_RET_MAX,        /*                                                     utils.py:133 */
    NIG_T_LEN_SUM,        /* sum of episode lengths (= steps in finished eps)    utils.py:136 */
    NIG_T_LEN_SQ,         /*                                                     utils.py:137 */
    NIG_T_VIOL,           /* sum of SafetyMetrics.violation_count                utils.py:140 */
    NIG_T_CRIT,           /* sum of SafetyMetrics.critical_violations            utils.py:142 */
    NIG_T_SHUTDOWN,       /* steps with info['critical_shutdown']                utils.py:143 */
    NIG_T_SUCCESS,        /* episodes with return > 0                            utils.py:150 */
    NIG_T_SATISFIED,      /* sum over steps of SafetyMetrics.constraints_satisfied  utils.py:109 (numerator)   */
    NIG_T_CONSTRAINTS,    /* sum over steps of SafetyMetrics.total_constraints      utils.py:109 (denominator):
                             constraint_satisfaction_rate (utils.py:144-147) = SATISFIED / CONSTRAINTS, 1.0 if 0 */
    NIG_T_ROWS
};

/* static description of an environment: base.py:22-72 plus each env's ctor */
typedef struct nig_env_spec {
    int32_t state_dim;          /* base.py:41  */
    int32_t action_dim;         /* base.py:42  */
    int32_t n_constraints;      /* len(self.safety_constraints)              */
    int32_t max_episode_steps;  /* default: CR 500 (chemical_reactor.py:66), PG/RA 1000 (base.py:27) */
    int32_t k_step;             /* RNG values drawn per step, reference call order  */
    int32_t k_reset;            /* RNG values drawn per reset                       */
    double dt;                  /* base.py:28 */
    double penalty[3];          /* SafetyConstraint.penalty  */
    int32_t critical[3];        /* SafetyConstraint.critical */
    int32_t reward_is_f32;      /* 1: reward accumulates in float32 (CR, NumPy>=2), 0: fp64 */
} nig_env_spec;

/* byte offsets of the library-owned arrays inside the handle's workspace */
typedef struct nig_layout {
    int64_t batch;          /* B                                              */
    int64_t ld;             /* row pitch in elements of every [R][B] array    */
    int64_t bytes;          /* total workspace size                           */
    int64_t off_state;      /* float  [S][ld]  current state == observation   */
    int64_t off_ctr;        /* uint32 [ld]     counter word (NIG_CTR_*)       */
    int64_t off_life_viol;  /* int64  [ld]     total_violations of FINISHED episodes (base.py:57,183) */
    int64_t off_ep_return;  /* double [ld]     return of the running episode (NIG_F_TALLY only, else -1) */
    int64_t off_tally;      /* double [NIG_T_ROWS][ld]  (NIG_F_TALLY only, else -1) */
} nig_layout;

typedef struct nig_handle nig_handle;

/* "nig <major.minor.patch> (gfx950; generator <id>)".  The generator id names the fast-mode random stream: trajectories of a
 * given (seed, lane, launch counter) are reproducible only under the same id ("nig-philox-v1" up to 0.1.0; "nig-philox-v2":
 * Philox4x32-7, float32 reset draws, 0.2.0; "nig-philox-v3", since 0.3.0: v2 with PowerGrid's eight reset load factors taken as
 * 16-bit uniforms from the low bytes of its reset normals' words -- only PowerGrid trajectories differ from v2). */
const char *nig_version(void);
const char *nig_last_error(void);

/* Process-wide tuning knobs.  Results never depend on them: every kernel form a knob selects between is
 * bit-identical (tests/test_gpu_split.py).  No counterpart upstream.
 *   NIG_TUNE_SPLIT_BLOCKS   256-lane blocks per ROUND of the three-wave form of nig_rollout / nig_rollout_policy
 *                           (csrc/nig_split.hpp: producer / integrator / recorder wave per 64 ChemicalReactor or
 *                           RobotAssembly lanes, one block resident per compute unit); default = the compute units of the HANDLE's
 *                           device, read at nig_create (256 on an MI355X; nig_tune_get reports it for the device of
 *                           the latest handle), 0 = never use that form.  An explicit value is process-wide and atomic.  nig_rollout
 *                           uses it for batches of at most one round and (ChemicalReactor) for larger ones whose
 *                           last round is at least 3/4 full WHEN the launch writes an observation trajectory (without one the
 *                           rounds lose to lanes filling the SIMDs, measured in round 5), nig_rollout_policy (ChemicalReactor)
 *                           likewise.  The same
 *                           "one wave per SIMD" threshold selects PowerGrid's paired rollout form (a producer wave per
 *                           stepping wave, csrc/nig_pg_lds.hpp) and the step kernel's helper waves (nig_step / nig_plan_*
 *                           on auto-reset handles of ChemicalReactor, PowerGrid, RobotAssembly).  The environment variable
 *                           NIG_SPLIT_BLOCKS sets the initial value.
 *   NIG_TUNE_WIDE_MIN_BLOCKS  smallest batch, in 512-lane blocks, that nig_rollout runs in the WIDE form (csrc/nig_kernels.hpp
 *                           rollout_wide_kernel: PowerGrid, 512-thread blocks at four waves per SIMD,
 *                           handles on which no lane can be frozen); default = 1.5 x the compute units of the handle's
 *                           device + 1 (the first batch that no longer fits one round of the 256-lane form at three
 *                           blocks per compute unit); smaller batches run the same LDS-resident
 *                           body in 256-lane blocks; 2^30 or more = never use that body (rollout_kernel only).  Environment variable NIG_WIDE_MIN_BLOCKS sets the initial value.
 * A value of -1 removes an explicit setting: every handle is back on its own device's default (tests restore with it).
 * nig_tune returns NIG_OK or NIG_ERR_INVALID (unknown key / value below -1); nig_tune_get returns the value in effect
 * for the device of the latest handle, or -1 for an unknown key. */
/* NIG_TUNE_DIAG_RING_FAULT: exists in the TEST-ONLY library variant built with -DNIG_RING_SPIN_LIMIT=<polls>
 * (profiles/mkvariant.sh; csrc/nig_ring.hpp) -- there the cooperating-wave kernels' ring waits are bounded and a
 * time-out makes nig_rollout / nig_rollout_policy return NIG_ERR_HIP naming the ring (they synchronise the stream in that
 * build); a non-zero value makes the producing waves stop posting after 7 steps, which is how tests/test_gpu_ring_limit.py
 * shows the error path.  The production library returns NIG_ERR_UNSUPPORTED for this key. */
enum { NIG_TUNE_SPLIT_BLOCKS = 0, NIG_TUNE_WIDE_MIN_BLOCKS = 1, NIG_TUNE_DIAG_RING_FAULT = 2 };
int nig_tune(int32_t key, int64_t value);
int64_t nig_tune_get(int32_t key);
/* the value in effect for THIS handle (its own device's default unless an explicit setting exists); -1: NULL handle / unknown key */
int64_t nig_handle_tune_get(const nig_handle *h, int32_t key);

/* Measurement aid (no counterpart upstream: performance_benchmark.py:106-133 times its loop with time.time()).  Enqueues a
 * small kernel on `stream` of the CURRENT device that stamps, per compute unit, the shader-clock counter and the constant
 * 100 MHz counter into the caller's DEVICE buffer of NIG_CLOCK_STAMP_WORDS uint64: slot = XCD (HW_REG_XCC_ID, 0-7) x 256 +
 * HW_REG_HW_ID bits 15:8 (se_id, sh_id, cu_id); out[2 slot] = s_memtime, out[2 slot + 1] = s_memrealtime; a compute unit no
 * block landed on keeps its old words (zero the buffer first).  Two stamps around a run of launches give the clock the chip
 * held over that run: (memtime1 - memtime0) / (memrealtime1 - memrealtime0) x 100 MHz for every slot stamped both times --
 * bench.py records the median next to every timed region so that box-to-box spread of a line can be attributed (VERDICT r04
 * next #6).  Never part of a timed kernel. */
#define NIG_CLOCK_STAMP_WORDS 4096
int nig_clock_stamp(void *stream, uint64_t *out);

/* utils.make registry lookup (utils.py:26-35): name -> id, or -1 */
int nig_env_id(const char *name);
const char *nig_env_name(int env);
int nig_env_spec_get(int env, nig_env_spec *out);

/* Workspace size/layout for a batch; `flags` as for nig_create. */
int nig_layout_query(int env, int64_t batch, uint32_t flags, nig_layout *out);

/*
 * Construct a batch of `batch` independent env instances of one type on `device`
 * (stands in for B calls of utils.make / IndustrialEnv.__init__, base.py:22-72).
 *   env_index0         global index of lane 0 (keys the counter-based RNG so results do
 *                      not depend on how a job is sharded over GPUs)
 *   max_episode_steps  0 = the env's default; CR ignores overrides upstream
 *                      (chemical_reactor.py:62-69 hard-codes 500 / 0.1), here it is honoured
 *   dt                 0 = default
 *   workspace          device memory of nig_layout.bytes (256-byte aligned) owned by the
 *                      caller, or NULL to let the library hipMalloc it.  It must be ordinary
 *                      device-local memory of `device` (hipMalloc / a torch CUDA tensor), not
 *                      host-pinned or fine-grained memory: with NIG_F_TALLY the step kernel
 *                      updates the episode tally with float64 hardware atomics
 * States are undefined until nig_reset.
 */
int nig_create(int env, int64_t batch, int device, uint64_t seed, uint64_t env_index0,
               int32_t max_episode_steps, double dt, uint32_t flags, void *workspace,
               nig_handle **out);
int nig_destroy(nig_handle *h);
int nig_get_layout(const nig_handle *h, nig_layout *out);
void *nig_workspace(const nig_handle *h);

/* RNG launch counter t ("nig-philox-v2"): nig_reset draws with the current
 * t, nig_step increments t first; every draw is a pure function of (seed, global lane index, t),
 * whatever the launch shape (ChemicalReactor's two step draws come from the Philox block with
 * counter word (t+1)/2: words 0-1 for odd t, 2-3 for even t).  Exposed so a caller can
 * checkpoint / replay. */
int nig_get_counter(const nig_handle *h, uint32_t *t);
int nig_set_counter(nig_handle *h, uint32_t t);

/*
 * Keep this handle's state rows in a caller-owned SoA array instead of the workspace: row k
 * of lane i lives at state[k*ld + i].  Lets several handles of different env types share one
 * padded observation matrix [S_max][total lanes] (BASELINE config "all envs mixed-batch,
 * heterogeneous state dims, padded SoA"): bind each handle at its column offset.  The current
 * contents are not copied; call before nig_reset.  state == NULL restores the internal array.
 */
int nig_bind_state(nig_handle *h, float *state, int64_t ld);

/* env.remove_safety_constraint(name) for a built-in constraint (base.py:224-228): bit k of
 * `mask` keeps constraint k enabled (default 0x7).  A disabled constraint is neither
 * counted nor penalised.  Constraints ADDED by the user (base.py:220-222) are arbitrary
 * Python callables upstream; the declarative ones -- boxes over state and action rows -- run on the device
 * (nig_set_limits below), every other callable stays on the host side of the binding. */
int nig_set_constraint_mask(nig_handle *h, uint32_t mask);

/*
 * env.add_safety_constraint(c) for box constraints ("nig-limits-v1"; base.py:157-213,220-222).
 *
 * An added constraint lists rows of the step's PRE-STATE (bit r < S of `mask`: state row r) and of the CLIPPED action (bit
 * S + j: action row j) -- the inputs the built-in constraints get -- and gives each listed row a closed interval [lo, hi] of
 * float32 bounds (+-inf allowed).  It is violated when some listed row x has !(lo <= x && x <= hi): a NaN in a listed row
 * violates, unlisted rows are never looked at.  Comparisons are exact; a float64 action (nig_step64_limited) is compared
 * against the bound widened to double.
 * Reward, in the reference's order and in the env's reward type R (float32 for ChemicalReactor with float32 actions, double
 * otherwise):  r = reward(next, a);  r = R(r + R(penalty_k)) for each violated enabled built-in k = 0, 1, 2;
 * r = R(r + R(penalty_c)) for each violated added constraint in installation order;  then, if ANY critical constraint (built-in
 * or added) was violated:  terminated = true and r = r - 1000, once.
 * The added constraints count: the episode's violation_count and total_violations, the tally rows VIOL, CRIT and SHUTDOWN,
 * and SATISFIED / CONSTRAINTS, which take (enabled built-ins + added) per step.
 * (The single env's Python path -- envs.py, arbitrary callables -- subtracts the 1000 BEFORE it adds the added constraints'
 * penalties when a built-in critical violation and an added violation fall on the same step; the device follows base.py's
 * order.  The two differ by floating-point rounding of that one reward at most.)
 *
 * The main flag word keeps its meaning: the VIOL bits, NVIOL and NCRIT describe the built-ins; TERMINATED and SHUTDOWN also
 * fire for an added critical violation.  A second word per lane and step, xflags_out, carries the added constraints:
 * bit c (0-3): added constraint c violated; bits 4-6: how many were; bits 8-10: how many critical ones were; 0 for a frozen
 * lane.
 *
 * nig_set_limits copies n <= NIG_MAX_LIMITS constraints from the HOST array `limits` into the handle (it waits for the copy
 * on `stream`); n == 0 removes them.  NIG_ERR_INVALID (the installed set stays): n outside 0 .. NIG_MAX_LIMITS, a mask bit
 * >= S + A, an empty mask, lo > hi or a NaN bound on a listed row, a NaN penalty, or (built-in constraints + n) *
 * max_episode_steps > 65535 (the counter word keeps the episode's violations in 16 bits).  NIG_ERR_UNSUPPORTED: the
 * Advanced envs, which override step() wholesale.
 * While limits are installed, every entry point that steps the env EXCEPT the _limited ones below returns
 * NIG_ERR_UNSUPPORTED before anything is launched or written (nig_step*, nig_rollout*, the MFMA families, nig_plan_*,
 * nig_step_host*, the mixed entry points given such a handle, nig_collect_episodes, which decodes the main flag word only).
 */
#define NIG_MAX_LIMITS 4
#define NIG_LIMIT_ROWS 48              /* row capacity of a constraint's bounds (S + A <= 38) */
typedef struct nig_limit {
    uint64_t mask;                     /* bit r < S: state row r; bit S + j: action row j */
    float lo[NIG_LIMIT_ROWS];          /* bounds of row (bit index) r; read for listed rows only */
    float hi[NIG_LIMIT_ROWS];
    double penalty;                    /* SafetyConstraint.penalty */
    int32_t critical;                  /* SafetyConstraint.critical */
    int32_t reserved;
} nig_limit;
int nig_set_limits(nig_handle *h, int32_t n, const nig_limit *limits /* host */, void *stream);
/* number of installed limits (0 .. NIG_MAX_LIMITS), -1 for a NULL handle */
int nig_get_limit_count(const nig_handle *h);
#define NIG_XFLAG_NVIOL_SHIFT 4
#define NIG_XFLAG_NCRIT_SHIFT 8

/* nig_step / nig_step64 under the installed limits (NIG_ERR_INVALID without any): every argument as there, plus
 * xflags_out uint32 [B] (may be NULL).  One plain 256-lane kernel form; finishing lanes of an auto-reset handle restart in
 * place with the parent's draws. */
int nig_step_limited(nig_handle *h, const float *actions, int64_t ld_act,
                     const double *step_noise, const double *reset_noise, int64_t ld_noise,
                     float *reward_out, double *reward64_out, uint32_t *flags_out, uint32_t *xflags_out,
                     float *final_obs, int64_t ld_obs, void *stream);
int nig_step64_limited(nig_handle *h, const double *actions, int64_t ld_act,
                       const double *step_noise, const double *reset_noise, int64_t ld_noise,
                       float *reward_out, double *reward64_out, uint32_t *flags_out, uint32_t *xflags_out,
                       float *final_obs, int64_t ld_obs, void *stream);

/*
 * IndustrialEnv.reset (base.py:133-155) for the lanes selected by `mask`
 * (uint8 [B], NULL = all): current_step = 0, done = False, violation_count = 0,
 * state = _get_initial_state().
 *   init_noise   double [k_reset][ld_noise]: the values the reference's RNG calls
 *                would have returned, in call order ("parity mode"); NULL = draw
 *                them on device from the counter-based generator ("fast mode").
 */
int nig_reset(nig_handle *h, const uint8_t *mask, const double *init_noise, int64_t ld_noise,
              void *stream);

/*
 * IndustrialEnv.step (base.py:157-213) for every lane, one kernel launch.
 *   actions      float [A][ld_act]   raw actions (clipped to [-1,1] inside, base.py:167)
 *   step_noise   double [k_step][ld_noise] or NULL (fast mode)
 *   reset_noise  double [k_reset][ld_noise] or NULL: initial-state draws for lanes that
 *                auto-reset in this call (NIG_F_AUTORESET)
 *   reward_out   float [B]   reward (rounded to float32 for PG/RA)        may be NULL
 *   reward64_out double [B]  the reference's fp64 Python-float reward      may be NULL
 *   flags_out    uint32 [B]  NIG_FLAG_* word                               may be NULL
 *   final_obs    float [S][ld_obs] terminal observation of lanes that finished in this
 *                call (other lanes' columns untouched)                     may be NULL
 * The new state/observation is the library-owned state array (nig_layout.off_state);
 * with NIG_F_AUTORESET a finished lane already holds the first observation of its next
 * episode.  Without it a finished lane is frozen until nig_reset (the reference raises
 * RuntimeError, base.py:159-160; here its flag word reads NIG_FLAG_INACTIVE).
 */
int nig_step(nig_handle *h, const float *actions, int64_t ld_act,
             const double *step_noise, const double *reset_noise, int64_t ld_noise,
             float *reward_out, double *reward64_out, uint32_t *flags_out,
             float *final_obs, int64_t ld_obs, void *stream);

/*
 * IndustrialEnv.step with FLOAT64 actions: double [A][ld_act], everything else as nig_step.
 * The reference's own callers hand np.float64 arrays to step() -- get_dataset (chemical_reactor.py:364-393,
 * power_grid.py:216-233, robot_assembly.py:266-290) and the baseline agents (benchmarks/baseline_agents.py:28-114)
 * -- and base.py:167 clips without casting, so under NumPy >= 2 every expression that touches an action element is
 * float64 and float64 spreads through what depends on it until a value is stored into the float32 state vector
 * (ChemicalReactor: temperature, pressure, flows, concentration, level and the reward; PowerGrid: generation,
 * frequency deviation, the action penalty; RobotAssembly: the joint update, the action penalty).  This entry point
 * follows that arithmetic for the three NumPy envs (pinned by the reference's outputs, tests/golden/<env>_g5.npz and
 * _g6.npz: state words bit-exact); the other envs convert the action to float32 on entry, as their own code would.
 * reward_out is the float64 reward rounded to float32; ChemicalReactor's reward is float64 here (np.float32 - np.float64).
 */
int nig_step64(nig_handle *h, const double *actions, int64_t ld_act,
               const double *step_noise, const double *reset_noise, int64_t ld_noise,
               float *reward_out, double *reward64_out, uint32_t *flags_out,
               float *final_obs, int64_t ld_obs, void *stream);

/*
 * A plan = n_steps consecutive nig_step launches in fast mode recorded once as a hipGraph
 * and replayed with one call (the per-step launch is otherwise host-bound at small batch).
 * Step k (0-based) of every replay reads its actions from ring slot k % ring_len:
 *   action_ring  float, slot s at action_ring + s*slot_stride, each slot [A][ld_act]
 *   reward_out / flags_out  optional; rings like the actions: step k writes slot s = k % ring_len at
 *                base + s*out_stride (min(n_steps, ring_len) slots are written; out_stride 0 = every
 *                step overwrites the same [B] array)
 * Semantics per step are exactly nig_step's (same kernel); the launch counter advances by
 * n_steps per replay.  This is the shape of the reference's own measurement loop
 * (performance_benchmark.py:106-133: sample action -> step -> reset on done).
 */
typedef struct nig_plan nig_plan;
int nig_plan_create(nig_handle *h, int32_t n_steps, const float *action_ring, int64_t ld_act,
                    int64_t slot_stride, int32_t ring_len, float *reward_out, uint32_t *flags_out,
                    int64_t out_stride, nig_plan **out);
int nig_plan_launch(nig_plan *p, void *stream);
int nig_plan_destroy(nig_plan *p);

/*
 * Fused rollout: n_steps consecutive steps of every lane in ONE kernel launch, state held in
 * registers between steps (fast mode only).  Same per-step semantics, generator keys and
 * bookkeeping as n_steps calls of nig_step -- the resulting state, counters and tallies are
 * bit-identical -- but a lane touches memory per step only for its action and for the outputs
 * requested here:
 *   action_ring / ld_act / slot_stride / ring_len   as for nig_plan_create; or, with ld_act == 0, a ROW-MAJOR ring: slot s =
 *                [batch][A] at action_ring + s*slot_stride (slot_stride >= batch*A) -- the layout of a policy's batched
 *                output (agents/base.py:106-141 predict() returns [n, A]).  Read natively (two 16-byte loads per lane, 2 KiB
 *                contiguous per wave) where every kernel of the launch is PowerGrid's LDS-resident body (auto-reset handle,
 *                no held lanes, batch a multiple of 256, 16-byte aligned slots; not the small-batch launches without an
 *                observation trajectory, whose stepping waves keep the state in registers); every
 *                other launch reads rows, so the library first transposes the slots this call reads (the first
 *                min(ring_len, n_steps): step k takes slot k % ring_len) into a buffer the handle owns (that many times
 *                A*ld floats, grown on demand, on the caller's stream, EVERY call: prefer rows for a ring that is
 *                replayed).  Same values either way (tests/test_gpu_action_layout.py).
 *   reward_out, flags_out   optional (both or neither), row of step k at base + k*out_stride
 *                (0 = overwrite)
 *   obs_out      optional (needs reward_out/flags_out) float trajectory: observation returned by step k (the terminal one for
 *                a lane that finishes) at obs_out + k*obs_step_stride, laid out [S][ld_obs], or
 *                -- with ld_obs == 0 -- row-major [B][S] (the D4RL observations[N,S] layout; obs_out
 *                16-byte aligned and obs_step_stride a multiple of 4 floats, i.e. B*S % 4 == 0 for a
 *                dense trajectory: each wave's 64 rows leave as whole-line 16-byte streaming stores).
 *                obs_step_stride == 0: every step overwrites the same block (as out_stride == 0 does for the
 *                reward / flag rows) -- the caller keeps the observations the last step returned
 * A frozen lane (finished on a handle without NIG_F_AUTORESET, or done before the call) still gets its rows written in every
 * step: flags_out = NIG_FLAG_INACTIVE | its step count, reward_out = 0.0f, and obs_out = the state the lane holds (the
 * closed-loop entry points below leave a frozen lane's observation / action rows untouched instead).
 * Stands in for the step loops of the reference's harnesses: benchmark_environment_steps
 * (performance_benchmark.py:106-133) and the get_dataset episode loops
 * (chemical_reactor.py:364-405, power_grid.py:209-237, robot_assembly.py:259-296).
 */
int nig_rollout(nig_handle *h, int32_t n_steps, const float *action_ring, int64_t ld_act,
                int64_t slot_stride, int32_t ring_len, float *reward_out, uint32_t *flags_out,
                int64_t out_stride, float *obs_out, int64_t ld_obs, int64_t obs_step_stride,
                void *stream);

/*
 * nig_rollout WITHOUT an action ring: every step draws its own uniform action in the kernel -- the reference's measurement
 * loop as it is written (performance_benchmark.py:106-133: a fresh action_space.sample() on every step, step, reset on done).
 * The step with launch counter t takes, for lane i, exactly the action nig_fill_actions(h, t, ...) writes for that lane:
 * uniforms of the generator's action stream at key (env_index0 + i, t, seed), mapped into the env's action Box.  A call is
 * therefore bit-identical -- outputs, state, counters, tallies -- to nig_rollout on a ring of n_steps slots filled with
 * nig_fill_actions(t0 + 1 + s) (tests/test_gpu_rollout_sampled.py), with no ring in memory, no fill launches and no action
 * reads: a finite ring repeats a lane's actions, one slot per step costs memory and traffic.
 * Everything else is nig_rollout's: the output modes and their arguments, the rows of a frozen lane, auto-reset, tallies,
 * the launch-counter advance (n_steps), the argument checks and their error texts (a refused call launches nothing), and the
 * kernel form -- the same rule, thresholds, nig_tune knobs and launch shapes for the same handle, batch and output mode;
 * the kernels are twins of the ring-fed ones under names of their own (rollout_sampled_kernel, rollout_sampled_wide_kernel,
 * split_sampled_kernel, pg_pair_sampled_kernel).
 * There is deliberately no act_out: the action of (lane, t) is a pure function of (seed, env index, t), so a caller who
 * needs the actions of a call regenerates them with nig_fill_actions(t) for t = counter before the call + 1 ... + n_steps.
 * Ring-fed only, as before: nig_rollout_noise (recorded draws come with recorded actions), nig_plan_create and the mixed
 * launches (nig_rollout_mixed*, nig_mixed_rollout*).
 */
int nig_rollout_sampled(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out,
                        int64_t out_stride, float *obs_out, int64_t ld_obs, int64_t obs_step_stride,
                        void *stream);

/*
 * nig_rollout with the reference's RECORDED random draws in place of the generator's -- parity mode of the fused
 * kernels: the same kernel forms nig_rollout selects for the handle and batch (three-wave, LDS-resident wide / paired,
 * one-wave; same thresholds, same launch shapes) run base.py:157-213 end to end on the values np.random returned
 * inside _dynamics (chemical_reactor.py:149,159; power_grid.py:136-144) and _get_initial_state
 * (chemical_reactor.py:89-107, power_grid.py:90-110, robot_assembly.py:113-137).  One row set per call step, as
 * nig_step's parity arguments:
 *   step_noise   double, row set of call step k at step_noise + k*step_noise_stride, laid out [k_step][ld_noise]
 *                (NULL for an env without step noise)
 *   reset_noise  double, row set of call step k at reset_noise + k*reset_noise_stride, laid out [k_reset][ld_noise]:
 *                the initial-state draws of a lane whose episode ends in call step k (auto-reset handles; a finishing
 *                lane restarts from _get_initial_state on them, evaluated per lane)
 * action_ring must hold every step of the call (ring_len >= n_steps).  Outputs as nig_rollout with the row-major
 * trajectory (obs_out float [n_steps][B][S], obs_step_stride 0 or >= S*B): reward_out, flags_out and obs_out are all
 * required.  ChemicalReactor, PowerGrid, RobotAssembly only (NIG_ERR_UNSUPPORTED otherwise): the envs upstream can run.
 * Exists for tests/test_gpu_noise_rollout.py (tests/golden/<env>_g3.npz through every form); the arithmetic outside
 * the replaced draws is the code nig_rollout runs.
 */
int nig_rollout_noise(nig_handle *h, int32_t n_steps, const float *action_ring, int64_t ld_act,
                      int64_t slot_stride, int32_t ring_len, const double *step_noise, int64_t step_noise_stride,
                      const double *reset_noise, int64_t reset_noise_stride, int64_t ld_noise,
                      float *reward_out, uint32_t *flags_out, int64_t out_stride,
                      float *obs_out, int64_t obs_step_stride, void *stream);

/*
 * Closed-loop rollouts with an on-device policy ("nig-policy-v1").  The policy
 * families are the reference's non-neural ones: the baseline agents Constant / "MPC"
 * (proportional) / PID / Random (benchmarks/baseline_agents.py:28-114) and the behaviour
 * policies of get_dataset (chemical_reactor.py:364-393, power_grid.py:216-233,
 * robot_assembly.py:266-290): an affine map of the observation, plus per-dimension Gaussian
 * and uniform noise, an epsilon-mixture with a uniform random action, and a clip.
 * All arithmetic is float32, terms in ascending (k, then j) order, zero columns skipped:
 *     u_j = b_j + sum_k Wt[k][j] * obs[k]                       (kind AFFINE)
 *     e_j = setpoint_j - obs[j]; I_j += e_j; u_j = kp*e_j + ki*I_j + kd*(e_j - eprev_j)   (kind PID)
 *     u_j += sigma_j * z_j + half_range_j * (2*v_j - 1)          z ~ N(0,1), v ~ U[0,1)
 *     if (w < p_uniform) u_j = uniform_range * (2*r_j - 1)       w, r ~ U[0,1)
 *     a_j = min(max(u_j, clip_lo), clip_hi)                      then IndustrialEnv.step clips to [-1,1]
 * Random draws come from generator stream "policy" at (global lane, launch counter t).
 */
#define NIG_POLICY_AFFINE 1
#define NIG_POLICY_PID 2
#define NIG_MAX_STATE_DIM 32
#define NIG_MAX_ACTION_DIM 10
typedef struct nig_policy {
    int32_t kind;
    uint32_t colmask;        /* bit k set: observation column k has a non-zero weight (host-computed) */
    float Wt[NIG_MAX_STATE_DIM][NIG_MAX_ACTION_DIM];   /* Wt[k][j] = weight of obs[k] in action j */
    float b[NIG_MAX_ACTION_DIM];
    float sigma[NIG_MAX_ACTION_DIM];
    float half_range[NIG_MAX_ACTION_DIM];
    float p_uniform, uniform_range;
    float clip_lo, clip_hi;
    float kp, ki, kd;
    float setpoint[NIG_MAX_ACTION_DIM];
} nig_policy;

/* Install the policy used by nig_rollout_policy (copied to device memory owned by the handle).
 * A PID policy owns per-lane controller memory (integral, previous error: float [2*A][ld], device
 * memory of the handle, zeroed when a PID policy is installed = the agent's constructor,
 * baseline_agents.py:55-57).  It persists across launches and across nig_reset -- upstream never
 * resets the integral either (baseline_agents.py:61-80) -- so a rollout cut into several launches
 * equals one launch. */
int nig_set_policy(nig_handle *h, const nig_policy *policy /* host */, void *stream);

/*
 * n_steps closed-loop steps per lane in one launch: action = policy(observation), then
 * IndustrialEnv.step, state in registers.  Optional per-step outputs (any subset):
 *   obs_out   float row-major [n_steps][B][S]: the observation the policy acted on (D4RL
 *             'observations'), step k at obs_out + k*obs_step_stride; obs_out 16-byte aligned,
 *             obs_step_stride >= S*B and a multiple of 4 floats (NIG_ERR_INVALID otherwise; there
 *             is no "overwrite" form: 0 is refused)
 *   act_out   float [n_steps][A][ld_act]: the policy's action (after its own clip, before the
 *             env's), step k at act_out + k*act_step_stride (ld_act >= B, act_step_stride >= A*ld_act)
 *   reward_out / flags_out   row of step k at base + k*out_stride (0 = overwrite)
 * Frozen lanes (finished, no auto-reset) write NIG_FLAG_INACTIVE | their step count and reward 0.0f and leave
 * their obs/act rows untouched in that step (nig_rollout_mlp_safe: their prob_out words too).
 * This is the loop of utils.evaluate_with_safety (utils.py:80-112) and of the get_dataset
 * generators, with the agent on the device.
 */
int nig_rollout_policy(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out,
                       int64_t out_stride, float *obs_out, int64_t obs_step_stride,
                       float *act_out, int64_t ld_act, int64_t act_step_stride, void *stream);

/*
 * Closed-loop rollouts with the reference agents' deterministic ACTOR on the device: a
 * (S -> 256 -> 256 -> A) ReLU MLP with a tanh head (agents/networks.py:47-70,125-144;
 * cql.py:339-343) evaluated with float32-input MFMA (v_mfma_f32_32x32x2_f32: an exact k-ordered
 * float32 fma chain) and fused with IndustrialEnv.step in one kernel: 32 envs per wavefront, the
 * hidden activations never leave the accumulator registers (an accumulator tile is the next
 * layer's B operand as it stands).  Weights are host pointers, row-major [in][out] (the layout of
 * a Flax Dense kernel); the library re-orders them once into the MFMA operand stream and keeps
 * that copy in device memory it owns.  hidden must be 256.  The tanh head runs on K = 1 MFMAs sized
 * to the env's action count (v_mfma_f32_4x4x1 up to four actions, v_mfma_f32_16x16x1 up to sixteen);
 * envs with an odd state dim or more than sixteen actions are refused (NIG_ERR_UNSUPPORTED).
 */
int nig_set_mlp_policy(nig_handle *h, int32_t hidden, const float *W1, const float *b1, const float *W2,
                       const float *b2, const float *W3, const float *b3, void *stream);

/* As nig_rollout_policy (arguments, minima, obs_out alignment, frozen lanes), with the MLP actor installed by nig_set_mlp_policy. */
int nig_rollout_mlp(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out,
                    int64_t out_stride, float *obs_out, int64_t obs_step_stride,
                    float *act_out, int64_t ld_act, int64_t act_step_stride, void *stream);

/*
 * The same actor on the bf16 matrix unit (v_mfma_f32_32x32x16_bf16: a sixteenth of the float32 form's matrix cycles), for
 * throughput-only sweeps: an opt-in family with its own arithmetic, outside the 1e-5 parity bar of nig_rollout_mlp, which it
 * leaves untouched.  The law "nig-mlp-bf16-v1", for one lane and one step on state s[0..S) and the network (S -> 256 -> 256 -> A)
 * of nig_set_mlp_policy:
 *   rounding  bf(x): float32 -> bfloat16, round to nearest even; a NaN stays a NaN.
 *   weights   W1, W2, W3 are rounded once on the host with bf; the biases b1, b2, b3 stay float32.
 *   input     the observation enters as two bf16 parts (16 significant bits): hi_k = bf(s_k), lo_k = bf(s_k - hi_k) (the
 *             subtraction is exact in float32), lo_k = 0 where hi_k is not finite; layer 1 reads
 *             x = [hi_0 .. hi_{S-1}, lo_0 .. lo_{S-1}] against W1's rows used twice (zero-padded to a multiple of 16).
 *   layers    z1_u = b1_u + sum_k W1[k][u] x_k, h1_u = bf(max(z1_u, 0));  z2_u = b2_u + sum_k W2[k][u] h1_k, h2_u = bf(max(z2_u, 0));
 *             z3_j = b3_j + sum_k W3[k][j] h2_k, a_j = det_tanhf(z3_j) (the float32 actor's tanh).
 *   sums      products of two bf16 values are exact; every sum is accumulated in float32 starting from the bias, in the kernel's
 *             own k order.  That order, and the matrix unit's internal order within an instruction, are NOT part of the law: it
 *             fixes the result only up to float32 accumulation error.
 *   determinism  the same inputs give the same bits on the same device; the kernel uses no atomics.
 *   the step  the env then steps on that float32 action exactly as in nig_rollout_mlp: clip, constraints, dynamics, reward,
 *             bookkeeping, auto-reset, tally and generator streams are shared code.
 * Non-finite observations are outside the law, as they are for the float32 loop.
 *
 * nig_set_mlp_policy_bf16: nig_set_mlp_policy's arguments (float32 host arrays); rounds them, builds the bf16 operand image and
 * keeps it on the handle beside the float32 actor's: installing one does not disturb the other.
 * nig_rollout_mlp_bf16: nig_rollout_mlp's arguments and checks, then the debug output hid_out (may be NULL): the lane's h1 and h2
 * as bf16 words, unit u in natural index -- step k, layer L (0: h1, 1: h2), unit u at
 * hid_out + k*hid_step_stride + (L*256 + u)*ld_hid + lane (ld_hid >= B, hid_step_stride >= 512*ld_hid, in uint16 elements;
 * frozen lanes leave their words untouched).  Refusals, before anything is launched or written: limits installed
 * (NIG_ERR_UNSUPPORTED, as every entry point without a _limited twin of its own), an env shape without the MFMA actor
 * (NIG_ERR_UNSUPPORTED), no bf16 actor installed (NIG_ERR_INVALID).
 * nig_bf16_from_f32: bf of n host floats (host only, no device needed): the builder's rounding.
 */
int nig_set_mlp_policy_bf16(nig_handle *h, int32_t hidden, const float *W1, const float *b1, const float *W2,
                            const float *b2, const float *W3, const float *b3, void *stream);
int nig_rollout_mlp_bf16(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out,
                         int64_t out_stride, float *obs_out, int64_t obs_step_stride,
                         float *act_out, int64_t ld_act, int64_t act_step_stride,
                         uint16_t *hid_out, int64_t ld_hid, int64_t hid_step_stride, void *stream);
int nig_bf16_from_f32(const float *x, uint16_t *out, int64_t n);

/*
 * The float32 MFMA actor for the other hidden shapes of the reference's agents (hidden_dims of CQLAgent, IQLAgent, TD3BCAgent; the
 * tuner sweeps (128,128) (256,256) (512,256) (256,256,256) (512,512)): two or three ReLU hidden layers of 1 .. 512 units and the
 * tanh head.  The kernel family "nig-mlp-shape-v1", reached through nig_rollout_mlp, which runs whichever actor the handle holds.
 *
 * Shape classes.  A network is zero-padded (zero weight rows and columns, zero biases) to the class that holds it with the fewest
 * 32x32x2 MFMAs per step; padding changes no value (a padded unit is relu(0), and fma(w, 0, c) == c), only the sign of a zero:
 *   "128x128"      two hidden layers, both <= 128                        4, 4 tiles of 32 units
 *   reference      two hidden layers, both <= 256, not in "128x128"      nig_set_mlp_policy's image and kernel, padded to 256 x 256
 *   "512x256"      two hidden layers, H1 <= 512, H2 <= 256               16, 8 tiles
 *   "512x512"      two hidden layers, both <= 512                        16, 16 tiles
 *   "256x256x256"  three hidden layers, all <= 256                       8, 8, 8 tiles
 * More than three hidden layers and a width above 512 are outside every class; a LayerNorm actor of hidden widths (256, 256) has a
 * kernel family of its own ("nig-mlp-ln-v1", nig_set_mlp_policy_ln below) and so has its shield beside a LayerNorm critic
 * ("nig-mlp-ln-shield-v1", nig_set_mlp_safety_ln), any other LayerNorm network stays on the host.
 *
 * The law, for one lane and one step on state s[0..S) and the PADDED network (the arithmetic of the padded network is the law):
 *   layer 1   z_u = the float32 fma chain over k = 0 .. S-1 in natural order, from 0: c = fma(W1[k][u], s_k, c), two inputs per MFMA
 *             k-step applied as fma(a1, b1, fma(a0, b0, c)); then the bias, c = fma(b1_u, 1, c) (and fma(0, 0, c));
 *             h_u = fmaxf(z_u, 0).
 *   layer n   (every later hidden layer) the same chain over the units of the layer below in the order of the accumulator
 *             registers that hold them: for tile kt = 0, 1, .. and register t = 0 .. 15 the pair (k0, k1) =
 *             (32 kt + rho_0(t), 32 kt + rho_1(t)), rho_h(t) = (t & 3) + 8 (t >> 2) + 4 h, applied as
 *             c = fma(W[k1][u], h_k1, fma(W[k0][u], h_k0, c)); the bias comes last; h_u = fmaxf(z_u, 0).
 *   head      row j is two chains, one per lane half h, each over the units 32 kt + rho_h(t) of the last hidden layer in (kt, t) order
 *             from 0, c_h = fma(W_head[k][j], h_k, c_h); the bias rides behind half 0's chain (c_0 = fma(b_j, 1, c_0), c_1 =
 *             fma(b_j, 0, c_1)); z_j = c_0 + c_1; a_j = det_tanhf(z_j), the project's tanh.
 *   the step  the env then steps on that action exactly as in nig_rollout_mlp: shared code.
 * For (256, 256) this text is what nig_rollout_mlp computes with nig_set_mlp_policy's actor (the oracle's mlp_actor).
 *
 * nig_set_mlp_policy_dims: n_hidden in 2 .. 3 hidden widths `hidden`, and n_hidden + 1 layers W[i] ([in][out] row-major, unpadded)
 * and b[i] as host pointers.  The library pads, builds the image, uploads it and records the class on the handle.  The handle has ONE
 * actor slot with a kind: nig_set_mlp_policy, and a _dims call whose class is the reference, fill it with nig_set_mlp_policy's image
 * (bit for bit the image of the padded arrays); every other class fills it with the shaped image; either call replaces the other's
 * actor.  The critic, ensemble, bf16 and limits slots are untouched.  NIG_ERR_UNSUPPORTED on an env without the MFMA actor;
 * NIG_ERR_INVALID for n_hidden outside 2 .. 3, a width outside 1 .. 512, a shape no class holds, a NULL pointer.
 * nig_rollout_mlp dispatches on the slot's kind: prototype, checks, outputs, frozen lanes, tallies and counter are the same.  While
 * a SHAPED actor is installed every other entry point that reads the actor slot (nig_rollout_mlp_safe, _search, _gated, _projected,
 * _disturbed and every _limited twin, nig_rollout_mlp_limited included) returns NIG_ERR_UNSUPPORTED with nothing launched or
 * written and the handle unchanged: those families on other shapes are later work.
 * nig_get_mlp_policy_dims: n_hidden of the installed actor and its (unpadded) widths in hidden[0 .. n_hidden) (an actor of
 * nig_set_mlp_policy reports 2 and 256, 256); 0 without one; -1 for NULL.
 */
int nig_set_mlp_policy_dims(nig_handle *h, int32_t n_hidden, const int32_t *hidden, const float *const *W,
                            const float *const *b, void *stream);
int nig_get_mlp_policy_dims(const nig_handle *h, int32_t *hidden /* [3] */);

/*
 * The float32 MFMA actor with LayerNorm: the reference's MLP with use_layer_norm=True (agents/networks.py: Dense -> LayerNorm ->
 * ReLU per hidden layer, tanh head), S -> 256 -> 256 -> A with hidden widths exactly (256, 256).  The kernel family "nig-mlp-ln-v1",
 * reached through nig_rollout_mlp.  The law is stated once, in csrc/nig_mlp_ln.hpp's opening comment (tests/mlp_ln_ref.c restates
 * it): the Dense pre-activations are the 256 x 256 law's fma chains; mean and a TWO-PASS variance are float32 sums in one stated
 * order per lane half, joined by one add; 1 / sigma is det_rsqrtf(var + eps) (IEEE sqrt and division); y = fma(z - mean, rs *
 * gamma, beta); the head and det_tanhf are nig_rollout_mlp's.  Non-finite inputs are outside the law.
 *
 * nig_set_mlp_policy_ln: nig_set_mlp_policy's arrays plus g1 / be1 and g2 / be2 [256], the scale and bias of the two LayerNorms,
 * and eps (flax's default: 1e-6), all host pointers.  Fills the ONE actor slot with a kind of its own: nig_set_mlp_policy and
 * nig_set_mlp_policy_dims replace the LayerNorm actor and it replaces theirs; the critic, ensemble, bf16 and limits slots are
 * untouched.  nig_get_mlp_policy_dims reports 2 and 256, 256.  Refusals, before anything is written: NIG_ERR_INVALID for a NULL
 * pointer and for an eps that is not finite and positive; NIG_ERR_UNSUPPORTED for hidden != 256 and for an env shape without the
 * MFMA actor.  While a LayerNorm actor is installed nig_rollout_mlp runs it, nig_rollout_mlp_safe runs it beside a LayerNorm critic
 * ("nig-mlp-ln-shield-v1", nig_set_mlp_safety_ln below), and every other entry point that reads the actor slot (nig_rollout_mlp_safe
 * beside any other critic, _search, _gated, _projected, _disturbed and every _limited twin, nig_rollout_mlp_limited and
 * nig_rollout_mlp_safe_limited included) returns NIG_ERR_UNSUPPORTED with nothing launched or written: the shaped actor's rule.
 * nig_get_mlp_policy_norm: 1 while the actor slot holds a LayerNorm actor, 0 otherwise; -1 for NULL.
 */
int nig_set_mlp_policy_ln(nig_handle *h, int32_t hidden, const float *W1, const float *b1, const float *g1, const float *be1,
                          const float *W2, const float *b2, const float *g2, const float *be2, const float *W3, const float *b3,
                          float eps, void *stream);
int nig_get_mlp_policy_norm(const nig_handle *h);

/*
 * nig_rollout_policy / nig_rollout_mlp under the installed limits ("nig-limits-v1", nig_set_limits): every argument and
 * refusal as the twin's, plus xflags_out uint32 [n_steps][>= B] (row k at xflags_out + k * out_stride; may be NULL; a frozen
 * lane's word is 0).  NIG_ERR_INVALID without installed limits.  With limits that no state can violate (infinite bounds)
 * every output equals the twin's but the tally's SATISFIED / CONSTRAINTS rows.  The policy twin has the one-wave kernel form
 * only.  The kernels are the twins' bodies with the step law of nig_step_limited, so a rollout equals nig_step_limited fed
 * with the rollout's own actions.
 */
int nig_rollout_policy_limited(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out,
                               int64_t out_stride, float *obs_out, int64_t obs_step_stride,
                               float *act_out, int64_t ld_act, int64_t act_step_stride, uint32_t *xflags_out, void *stream);
int nig_rollout_mlp_limited(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out,
                            int64_t out_stride, float *obs_out, int64_t obs_step_stride,
                            float *act_out, int64_t ld_act, int64_t act_step_stride, uint32_t *xflags_out, void *stream);

/*
 * Safety-critic shield of the reference agents' predict_with_safety (agents/cql.py, iql.py, td3bc.py):
 * a = actor(s); p = sigmoid(critic([s, a])); the env receives a if p < threshold, a * 0.5 otherwise.
 * The critic is a (S + A) -> 256 -> 256 -> 1 ReLU MLP (agents/networks.py SafetyCritic), evaluated after
 * the actor in the same kernel by the same f32-MFMA scheme (its weights streamed through the same
 * double-buffered LDS image; the one-row head on v_mfma_f32_4x4x1).
 * Safety critic for the shielded MLP loop: C1 [S+A][hidden], c1 [hidden], C2 [hidden][hidden], c2,
 * C3 [hidden][1], c3 [1]; row-major [in][out] (Flax Dense kernels); hidden must be 256.  The library
 * keeps its own device copy; installing a new actor (nig_set_mlp_policy) keeps the critic.
 */
int nig_set_mlp_safety(nig_handle *h, int32_t hidden, const float *C1, const float *c1, const float *C2,
                       const float *c2, const float *C3, const float *c3, float threshold, void *stream);

/*
 * As nig_rollout_mlp, with the shield: prob_out (optional) float [n_steps][>=B]: p of the UNshielded
 * action, row k at prob_out + k*out_stride (live lanes only, like obs/act); act_out holds the action
 * the env received; flags carry NIG_FLAG_SHIELDED on live steps whose action was halved.  The raw
 * action is bit-identical to nig_rollout_mlp's.  NIG_ERR_INVALID without an actor or a critic,
 * NIG_ERR_UNSUPPORTED for an env shape without the MFMA actor.
 */
int nig_rollout_mlp_safe(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out,
                         int64_t out_stride, float *obs_out, int64_t obs_step_stride, float *act_out,
                         int64_t ld_act, int64_t act_step_stride, float *prob_out, void *stream);

/*
 * nig_rollout_mlp_safe under the installed limits ("nig-limits-v1", nig_set_limits): every argument as the parent's, plus xflags_out
 * uint32 [n_steps][>= B] (row k at xflags_out + k * out_stride; may be NULL; a frozen lane's word is 0), nig_rollout_mlp_limited's
 * layout.  The added constraints are checked on the action the env receives (the halved one where the shield acts); NIG_FLAG_SHIELDED
 * is set as in the parent.  NIG_ERR_INVALID without installed limits, then every refusal of the parent; a refused call launches and writes nothing.  The kernel is the
 * parent's body with the step law of nig_step_limited applied to the action the env receives, so a rollout equals nig_step_limited fed
 * with the rollout's own actions (act_out holds them).
 */
int nig_rollout_mlp_safe_limited(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out,
                                 int64_t out_stride, float *obs_out, int64_t obs_step_stride, float *act_out,
                                 int64_t ld_act, int64_t act_step_stride, float *prob_out, uint32_t *xflags_out, void *stream);

/*
 * Safe-action search of the reference's safety-critical agents (agents/safety_critical.py:173-208,
 * RiskAwareCQLAgent.get_safe_action), fused into the shield's kernel: where the critic finds the actor's
 * action too risky, it scores n_candidates uniform actions and the env receives the least risky one.
 * The law, "nig-search-v1".  For a live lane with global index g, on the step whose launch counter is t
 * (the t its step noise is keyed at), thr the threshold installed with the critic, N = n_candidates:
 *     a  = actor(s)                                  bit for bit nig_rollout_mlp's action
 *     p0 = critic([s, a])                            bit for bit nig_rollout_mlp_safe's p
 *     if (p0 < thr):   the env receives a;  risk = p0;  choice = -1;  no flag
 *     else:
 *         for c = 0 .. N-1:
 *             u_c[j] = fmaf((float)(w >> 8), 2^-23, -1.0f),  j = 0 .. A-1,
 *                      w = word (j & 3) of the generator's block 0xC0000100 + 4*c + (j >> 2) (policy stream,
 *                      block 0x100 + 4*c + (j >> 2)) under the key (g, t, seed): uniform on [-1, 1) in steps
 *                      of 2^-23, whatever the env's action Box (the reference draws uniform(-1, 1))
 *             p_c    = critic([s, u_c])              the arithmetic of p0
 *         best = the first c of least p_c: c = 0, then every c whose p_c < p_best in order; a NaN p_c is
 *                taken only as c = 0 and gives way to the first p_c that is a number
 *         the env receives u_best;  risk = p_best;  choice = best;  NIG_FLAG_SHIELDED ("the critic replaced
 *         the action": no other flag bit is free)
 * As the reference, the law returns the safest candidate even where p_best > p0.  A NaN p0 searches.
 * Candidate passes run per 128-lane block and only in blocks with a live lane that searches; a lane's
 * results do not depend on the other lanes of its block.  Cost: up to N + 1 critic passes per step.
 *
 * As nig_rollout_mlp_safe (arguments, minima, obs_out alignment, frozen lanes, tallies, launch counter; actor
 * and critic from nig_set_mlp_policy / nig_set_mlp_safety, no other state).  prob_out: p0.  risk_out /
 * choice_out (optional) float / int32 [n_steps][>= B], row k at base + k*out_stride like prob_out; frozen
 * lanes leave their words untouched.  act_out: the action the env received.  NIG_ERR_INVALID (nothing
 * launched or written): n_candidates outside 1 .. NIG_MAX_CANDIDATES, no actor or no critic, and every
 * refusal of nig_rollout_mlp_safe; NIG_ERR_UNSUPPORTED where that is unsupported.
 */
#define NIG_MAX_CANDIDATES 128
int nig_rollout_mlp_search(nig_handle *h, int32_t n_steps, int32_t n_candidates, float *reward_out,
                           uint32_t *flags_out, int64_t out_stride, float *obs_out, int64_t obs_step_stride,
                           float *act_out, int64_t ld_act, int64_t act_step_stride, float *prob_out,
                           float *risk_out, int32_t *choice_out, void *stream);

/*
 * nig_rollout_mlp_search under the installed limits: the parent's arguments plus xflags_out (nig_rollout_mlp_safe_limited's).  The
 * added constraints are checked on the chosen candidate where the search acts.  NIG_ERR_INVALID without installed limits, then every refusal of the parent; a refused call launches and writes nothing.  The kernel is the
 * parent's body with the step law of nig_step_limited applied to the action the env receives, so a rollout equals nig_step_limited fed
 * with the rollout's own actions.
 */
int nig_rollout_mlp_search_limited(nig_handle *h, int32_t n_steps, int32_t n_candidates, float *reward_out,
                                   uint32_t *flags_out, int64_t out_stride, float *obs_out, int64_t obs_step_stride,
                                   float *act_out, int64_t ld_act, int64_t act_step_stride, float *prob_out,
                                   float *risk_out, int32_t *choice_out, uint32_t *xflags_out, void *stream);

/*
 * Distributional safety critic of the reference's RiskAwareCQLAgent (agents/safety_critical.py:92-110, 151-171,
 * DistributionalSafetyCritic / compute_safety_violation_probability): an (S + A) -> 256 -> 256 -> N ReLU MLP whose
 * softmax is a distribution over N atoms; the violation probability is its mass on the atoms that count as
 * a violation (the reference: N = 51, linspace(-1, 1, 51) < 0: atoms 0 .. 24).
 * The law, "nig-categorical-v1".  One lane, one (s, a); N = atoms, 2 <= N <= 64; below_mask a uint64 with bit j
 * set where atom j counts as a violation:
 *     z_j  = logit j of the network ([s, a]) -> 256 -> 256 -> N, j = 0 .. N-1.  Layers 1 and 2 are the shield
 *            critic's, bit for bit.  Head column j has the summation order of the shield's one-row head (each
 *            lane half's fma chain over the hidden rows it holds, the bias as one more k-step of B = 1 / 0,
 *            then the one joining add): z_j is bit for bit the logit of the one-output critic (C3[:, j], c3[j]).
 *     m    = max_j z_j                  a NaN z_j takes no part (fmaxf); rows j >= N take no part in anything
 *     e_j  = det_expf(z_j - m)
 *     Row j = 16 P + 4 q + i (P, q, i in 0 .. 3) belongs to group q.  With the terms of rows j >= N (and, for V,
 *     of rows outside below_mask) replaced by +0, float32:
 *         t_q = the left-to-right sum, from +0, of e_j over the group's 16 rows in ascending j
 *               (4q, 4q+1, 4q+2, 4q+3, 16+4q, ..., 48+4q+3)
 *         T   = (t_0 + t_1) + (t_2 + t_3)
 *         v_q, V likewise over the rows of below_mask
 *     p    = V / T                      IEEE division; T >= 1 whenever it is a number: the max term is det_expf(0) = 1
 * (The groups are the lanes that hold the head rows after four 16-row passes of v_mfma_f32_16x16x1: lane
 * 16 q + c holds rows 16 P + 4 q + i of env column c, so each sum runs where its terms lie and two butterfly
 * steps join the four lanes.)
 * Non-finite logits.  A NaN z_j gives e_j = NaN and p = NaN.  z_j = -inf is an atom of no mass: det_expf's
 * stated domain gives exactly +0 below -104 (tests/test_detmath.py "expf.exact"; the code returns +0 for every
 * x < -103, -inf included).  z_j = +inf gives m = +inf, e_j = det_expf(inf - inf) = NaN and p = NaN; so does
 * every z_j = -inf (m = -inf).  A head bias c3[j] = -inf does NOT give z_j = -inf: the bias k-step multiplies
 * it by B = 0 on the second lane half, so z_j = NaN (the one-row head's arithmetic, which the oracle restates).
 * In the closed loops a lane whose p is not below the threshold (!(p < threshold)) counts as risky: a NaN p shields.
 *
 * nig_set_mlp_safety_categorical installs the critic: C1 .. c2 as nig_set_mlp_safety, C3 [hidden][atoms], c3 [atoms],
 * row-major [in][out]; hidden must be 256.  The handle has ONE critic slot with a kind: this call and nig_set_mlp_safety
 * replace each other (threshold included); installing an actor keeps the critic; the gate's and the projection's
 * networks are separate and untouched.  NIG_ERR_INVALID: a NULL argument, atoms outside 2 .. 64, a mask bit >= atoms;
 * NIG_ERR_UNSUPPORTED: another hidden width, an env shape without the MFMA actor.  A refused call changes nothing.
 * A HIP failure while the weights are copied leaves the slot empty (kind none).
 * nig_get_mlp_safety_kind: which critic the slot holds (NIG_SAFETY_*); -1 for a NULL handle.
 * nig_get_mlp_safety_atoms: the installed categorical critic's atoms, 0 without one; -1 for a NULL handle.
 *
 * With the categorical critic installed, nig_rollout_mlp_safe, nig_rollout_mlp_search and their _limited twins run their
 * own laws with p, p0 and p_c from "nig-categorical-v1" in place of the sigmoid; prototypes, arguments, refusals, outputs,
 * NIG_FLAG_SHIELDED, frozen lanes and tallies are unchanged, the raw action stays nig_rollout_mlp's and the candidates
 * "nig-search-v1"'s draws.  With the sigmoid critic installed nothing changes.
 */
#define NIG_SAFETY_NONE        0
#define NIG_SAFETY_SIGMOID     1
#define NIG_SAFETY_CATEGORICAL 2
#define NIG_MAX_ATOMS 64
int nig_set_mlp_safety_categorical(nig_handle *h, int32_t hidden, int32_t atoms, const float *C1, const float *c1,
                                   const float *C2, const float *c2, const float *C3, const float *c3,
                                   uint64_t below_mask, float threshold, void *stream);
int nig_get_mlp_safety_kind(const nig_handle *h);
int nig_get_mlp_safety_atoms(const nig_handle *h);

/*
 * The safety critic with LayerNorm and the fused shield of a LayerNorm agent: agents/networks.py SafetyCritic built with
 * use_layer_norm=True, (S + A) -> 256 -> LayerNorm -> ReLU -> 256 -> LayerNorm -> ReLU -> 1, played by agents/cql.py
 * predict_with_safety beside a LayerNorm actor.  The law "nig-mlp-ln-shield-v1" (stated in csrc/nig_mlp_ln_shield.hpp, restated
 * here).  For one live lane and one step on state s:
 *   a     = actor(s): "nig-mlp-ln-v1" bit for bit, the action nig_rollout_mlp computes with the same LayerNorm actor.
 *   x     = [s_0 .. s_{S-1}, a_0 .. a_{A-1}, 0 ..], zero-padded to the critic's layer-1 width (S + A rounded up to even).
 *   pre   = the head pre-activation of the critic under "nig-mlp-ln-v1" with IN = S + A, OUT = 1 and the critic's own eps: layer 1
 *           the fma chain in natural k order on x, the mean, two-pass variance, det_rsqrtf and fma(d, rs * gamma, beta) of that
 *           law on both layers, the head the one-row case of the four-row head (each lane half's fma chain over the hidden rows
 *           it holds, the bias as one more k-step of B = 1 / 0, then the one joining add).
 *   p     = det_sigmoidf(pre);  shield = !(p < threshold).
 *   The env receives a_j * 0.5f where shield and a_j otherwise, and steps on it exactly as nig_step does.
 * Outputs are nig_rollout_mlp_safe's: prob_out gets p, act_out the action the env received, NIG_FLAG_SHIELDED is set on shielded
 * live lanes; a frozen lane writes the INACTIVE flag word and a zero reward and leaves its obs / act / prob words untouched.
 * Non-finite inputs are outside the law.
 *
 * nig_set_mlp_safety_ln installs the critic: nig_set_mlp_safety's arrays plus g1 / be1 and g2 / be2 [256], the scale and bias of
 * the two LayerNorms, eps (flax's default: 1e-6) and the threshold, all host pointers.  It fills the ONE critic slot with the kind
 * NIG_SAFETY_SIGMOID_LN: nig_set_mlp_safety, nig_set_mlp_safety_categorical and this call replace each other (threshold included);
 * installing any actor keeps the critic.  Refusals, with nothing changed: NIG_ERR_INVALID for a NULL pointer and for an eps that
 * is not finite and positive (the threshold is taken as nig_set_mlp_safety takes it); NIG_ERR_UNSUPPORTED for hidden != 256 and
 * for an env shape without the MFMA actor.  A HIP failure while the weights are copied leaves the slot empty (kind none).
 *
 * nig_rollout_mlp_safe keeps its prototype and dispatches on both slots: a LayerNorm actor AND a LayerNorm critic run this law; a
 * LayerNorm actor beside any other critic is refused as before (NIG_ERR_UNSUPPORTED), and without a critic NIG_ERR_INVALID; a
 * plain, shaped or bf16 actor beside the LayerNorm critic is NIG_ERR_UNSUPPORTED ("... LayerNorm critic ...").  While the
 * LayerNorm critic is installed every other reader of the critic slot refuses the same way, with nothing launched or written:
 * nig_rollout_mlp_search, nig_mlp_violation_prob and every _limited twin, nig_rollout_mlp_safe_limited included.
 * Out of scope: the _limited, search, categorical, gate, projection and disturbed forms on LayerNorm networks, and LayerNorm
 * networks of other shapes -- they stay on the host.
 */
#define NIG_SAFETY_SIGMOID_LN  3
int nig_set_mlp_safety_ln(nig_handle *h, int32_t hidden, const float *C1, const float *c1, const float *g1, const float *be1,
                          const float *C2, const float *c2, const float *g2, const float *be2, const float *C3, const float *c3,
                          float eps, float threshold, void *stream);

/*
 * The safety critic of the other hidden shapes and the fused shield of a shaped agent: the reference builds every agent's
 * SafetyCritic with the actor's own hidden_dims, and agents/cql.py predict_with_safety plays the pair.  The law
 * "nig-mlp-shape-shield-v1" (stated in csrc/nig_mlp_shape_shield.hpp, restated here).  For one live lane and one step on state s:
 *   a     = actor(s): "nig-mlp-shape-v1" bit for bit, the action nig_rollout_mlp computes with the same shaped actor of class K.
 *   x     = [s_0 .. s_{S-1}, a_0 .. a_{A-1}, 0 ..], zero-padded to the critic's layer-1 width (S + A rounded up to even).
 *   pre   = the head pre-activation of the critic under "nig-mlp-shape-v1" with IN = S + A, OUT = 1, its hidden widths zero-padded
 *           to the actor's class K: layer 1 the fma chain in natural k order on x, the hidden layers that law's chains, the head
 *           the one-row case of the 4 x 4 x 1 head on every env (each lane half's fma chain over the hidden rows it holds, the
 *           bias as one more k-step of B = 1 / 0 behind the last tile, then the one joining add).
 *   p     = det_sigmoidf(pre);  shield = !(p < threshold).
 *   The env receives a_j * 0.5f where shield and a_j otherwise, and steps on it exactly as nig_step does.
 * Outputs are nig_rollout_mlp_safe's: prob_out gets p of the unshielded action, act_out the action the env received,
 * NIG_FLAG_SHIELDED is set on shielded live lanes; a frozen lane writes the INACTIVE flag word and a zero reward and leaves its
 * obs / act / prob words untouched; tallies and the launch counter behave as in nig_rollout_mlp_safe.  Non-finite inputs are
 * outside the law.
 *
 * nig_set_mlp_safety_dims installs the critic: n_hidden in 2 .. 3, the unpadded widths hidden[l] in 1 .. 512, and n_hidden + 1
 * layers C[l] [in][out] row-major with biases c[l] -- the first has S + A rows, the last one column -- all host pointers; the
 * threshold is taken as nig_set_mlp_safety takes it.  The class is the cheapest that holds the widths at S + A (rounded up to
 * even) inputs.  A shaped class fills the ONE critic slot with the kind NIG_SAFETY_SIGMOID_SHAPED; the reference class is padded
 * to 256 x 256 on the host and fills it exactly as nig_set_mlp_safety does on the padded arrays (kind NIG_SAFETY_SIGMOID, the
 * same image bit for bit).  The four critic installs replace each other (threshold included); installing any actor keeps the
 * critic.  Refusals, with nothing changed: NIG_ERR_INVALID for a NULL pointer, n_hidden outside 2 .. 3, a width outside 1 .. 512
 * and widths no class holds; NIG_ERR_UNSUPPORTED for an env shape without the MFMA actor.  A HIP failure while the weights are
 * copied leaves the slot empty (kind none).
 * nig_get_mlp_safety_dims mirrors nig_get_mlp_policy_dims: the installed critic's n_hidden, its unpadded widths into hidden[3]
 * (may be NULL); 0 without a critic; 2 and 256, 256 for the plain, categorical and LayerNorm critics; -1 for a NULL handle.
 *
 * nig_rollout_mlp_safe keeps its prototype and dispatches on both slots: a shaped actor of class K AND a shaped critic of the same
 * class K run this law.  A shaped actor beside a plain, categorical, LayerNorm or absent critic is refused as before
 * (NIG_ERR_UNSUPPORTED, "... shaped actor ..."); a shaped critic beside a reference, LayerNorm or absent actor, or a shaped actor
 * of another class, is NIG_ERR_UNSUPPORTED ("... shaped critic ...").  While the shaped critic is installed every other reader of
 * the critic slot refuses the same way, with nothing launched or written: nig_rollout_mlp_search, nig_mlp_violation_prob and every
 * _limited twin, nig_rollout_mlp_safe_limited included.
 * Out of scope: the _limited, search, categorical, gate, projection, ensemble, disturbed and bf16 forms on shaped networks, an
 * actor and a critic of different classes, and a shaped critic beside the reference actor -- they stay on the host.
 */
#define NIG_SAFETY_SIGMOID_SHAPED 4
int nig_set_mlp_safety_dims(nig_handle *h, int32_t n_hidden, const int32_t *hidden, const float *const *C, const float *const *c,
                            float threshold, void *stream);
int nig_get_mlp_safety_dims(const nig_handle *h, int32_t *hidden /*[3]*/);

/*
 * compute_safety_violation_probability over a batch: p of "nig-categorical-v1" (and, optionally, the logits) of n
 * caller-supplied (state, action) columns.  obs float [S][ld_obs], act float [A][ld_act] (device; the action is used as
 * given: the reference does not clip), prob_out float [n], logit_out float [atoms][ld_logit] or NULL (ld_logit is then
 * ignored).  A kernel of its own: it reads nothing of the handle's env state and writes none of it -- no counter, tally,
 * generator position or state matrix changes.  n >= 1 need not be a multiple of anything; words of the outputs past column
 * n - 1 keep their values.  NIG_ERR_INVALID (nothing launched or written): a NULL handle, obs, act or prob_out, no
 * categorical critic installed, n < 1, or a pitch below n or above 2^26.
 */
int nig_mlp_violation_prob(nig_handle *h, int64_t n, const float *obs, int64_t ld_obs, const float *act, int64_t ld_act,
                           float *prob_out, float *logit_out, int64_t ld_logit, void *stream);

/*
 * Ensemble of MLP actors (agents/ensemble.py EnsembleAgent: predict, predict_with_uncertainty,
 * get_high_uncertainty_mask) fused with IndustrialEnv.step: n_members actors of nig_set_mlp_policy's
 * shape and layouts are evaluated per step by the same f32-MFMA scheme, one after the other through
 * the same LDS image, and reduced in registers.  With p_k the float32 action of member k (bit for bit
 * what nig_rollout_mlp computes for that network on the same observation), K = n_members:
 *   NIG_ENSEMBLE_AVERAGE ("mean" / "weighted", np.average: a float64 action)
 *       acc = (double)p_0 * weights[0];  acc = acc + (double)p_k * weights[k], k = 1 .. K-1 in order
 *       (every product rounded);  action = acc / weight_sum.
 *       ChemicalReactor / PowerGrid / RobotAssembly step on that float64 action with nig_step64's
 *       arithmetic; every other env receives it rounded to float32 (nig_step64's rule for them).
 *       weights = the ACTIVE weights (for "mean": w[:K] / np.sum(w[:K]); for "weighted": w[:K]);
 *       weight_sum = np.sum(weights), computed by the caller -- the library never sums weights.
 *   NIG_ENSEMBLE_VOTING (np.mean of a float32 array: a float32 action, nig_step's arithmetic)
 *       acc = p_0;  acc = acc + p_k;  action = acc / (float)K.   weights / weight_sum are ignored.
 *   uncertainty (float32; np.std over the members, mean over the action dimensions) -- the order the
 *   library documents and its tests restate, per action dimension about member 0, d_k = p_k - p_0:
 *       s1 = 0, s2 = 0;  s1 = s1 + d_k, s2 = s2 + d_k * d_k for k = 1 .. K-1 in order;
 *       v = s2 - (s1 * s1) / (float)K;  v = v > 0 ? v : 0;  sd = sqrt(v / (float)K);
 *       uncertainty = (((0 + sd_0) + sd_1) + ... + sd_{A-1}) / (float)A.
 *   It is exactly 0 for identical members and for K = 1, and agrees with the reference's two-pass
 *   np.std to 1e-5 relative (the subtraction loses at most a factor 1 + K of float32's precision,
 *   because member 0's own deviation is part of v).  All divisions and the square root are IEEE
 *   correctly rounded; no product is fused into a sum.
 * A live step whose uncertainty > uncertainty_threshold (strict) carries NIG_FLAG_UNCERTAIN.
 * W1 .. b3: host arrays [n_members] of host pointers.  NIG_ERR_INVALID: n_members outside
 * 1 .. NIG_MAX_ENSEMBLE, a NULL array, an unknown method, (AVERAGE) a non-finite weight or weight_sum,
 * weight_sum == 0.  NIG_ERR_UNSUPPORTED: hidden != 256, an env shape without the MFMA actor.
 * The handle's single actor and critic (nig_set_mlp_policy / _safety) are left alone, and vice versa.
 * NIG_MAX_ENSEMBLE bounds the handle's operand streams (341 KB per member); the kernel's registers
 * do not depend on it.
 */
#define NIG_MAX_ENSEMBLE 8
#define NIG_ENSEMBLE_AVERAGE 0
#define NIG_ENSEMBLE_VOTING 1
int nig_set_mlp_ensemble(nig_handle *h, int32_t n_members, int32_t hidden, const float *const *W1,
                         const float *const *b1, const float *const *W2, const float *const *b2,
                         const float *const *W3, const float *const *b3, int32_t method,
                         const double *weights, double weight_sum, float uncertainty_threshold, void *stream);

/*
 * As nig_rollout_mlp (arguments, minima, obs_out alignment, frozen lanes, tallies, launch counter), with
 * the installed ensemble.  act_out: the action the env received, rounded to float32 for
 * NIG_ENSEMBLE_AVERAGE (the exact float64 action is the law above applied to member_act_out).
 * unc_out (optional) float [n_steps][>= B], row k at unc_out + k*out_stride.  member_act_out (optional)
 * float: member m of step k is one [A][ld_act] block at member_act_out + (k*n_members + m)*act_step_stride
 * (ld_act / act_step_stride are checked as for act_out when either is given).  Frozen lanes leave their
 * unc_out / member_act_out words untouched.  NIG_ERR_INVALID without an installed ensemble.
 */
int nig_rollout_mlp_ensemble(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out,
                             int64_t out_stride, float *obs_out, int64_t obs_step_stride, float *act_out,
                             int64_t ld_act, int64_t act_step_stride, float *unc_out,
                             float *member_act_out, void *stream);

/*
 * nig_rollout_mlp_ensemble under the installed limits: the parent's arguments plus xflags_out (nig_rollout_mlp_safe_limited's).  With
 * NIG_ENSEMBLE_AVERAGE on an env that steps on the float64 action (nig_step64's rule) the added constraints are checked on that
 * float64 action against the float32 bounds widened to double: the law of nig_step64_limited.  NIG_FLAG_UNCERTAIN is set as in the
 * parent.  NIG_ERR_INVALID without installed limits, then every refusal of the parent; a refused call launches and writes nothing.  The kernel is the
 * parent's body with the step law of nig_step_limited applied to the action the env receives, so a rollout equals nig_step_limited fed
 * with the rollout's own actions (nig_step64_limited and the float64 action where the env steps on one).
 */
int nig_rollout_mlp_ensemble_limited(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out,
                                     int64_t out_stride, float *obs_out, int64_t obs_step_stride, float *act_out,
                                     int64_t ld_act, int64_t act_step_stride, float *unc_out,
                                     float *member_act_out, uint32_t *xflags_out, void *stream);

/*
 * Safety-ensemble gate of the reference's SafeEnsembleAgent.get_safe_action (agents/safety_critical.py:391-532),
 * fused into the shield's kernel: K safety predictors with one head row per constraint score the actor's
 * action; the env receives it only if every constraint's violation probability and every spread is small,
 * and the zero action otherwise.  A member is a (S + A) -> 256 -> 256 -> C ReLU MLP in nig_set_mlp_safety's
 * layouts with C3 [hidden][n_outputs], c3 [n_outputs]; hidden must be 256 (policies.pad_safety_member pads the
 * reference's 128-wide members).  With K = 1, T = 1 and an infinite spread limit the gate is
 * ConstrainedIQLAgent's acceptance test all(sigmoid(predictor(s, a)) < thr).
 * The law, "nig-gate-v1".  Installed: K = n_members, C = n_outputs, T = temperature, thr = prob_threshold,
 * umax = uncertainty_threshold.  For a live lane on a step:
 *     a        = actor(s)                          bit for bit nig_rollout_mlp's action
 *     z_m[c]   = head row c of member m on [s, a]  m = 0 .. K-1, c = 0 .. C-1; each row the two lane-half fma
 *                                                  chains joined by one add, exactly the arithmetic of
 *                                                  nig_rollout_mlp_safe's one-row head on C3[:, c], c3[c];
 *                                                  rows do not interact
 *     acc[c]   = z_0[c];  acc[c] = acc[c] + z_m[c]   (m = 1 .. K-1 in order);   mean[c] = acc[c] / (float)K
 *     d_m      = z_m[c] - z_0[c];  s1 = s1 + d_m;  s2 = s2 + d_m * d_m   (m = 1 .. K-1 in order, from 0)
 *     v        = s2 - (s1 * s1) / (float)K;  v = v < 0 ? 0 : v  (a NaN stays a NaN);  sd[c] = sqrt(v / (float)K)
 *     pen      = sd[c] > 1 ? 1 : sd[c]
 *     p[c]     = det_sigmoidf(mean[c] / T) + 0.5f * pen;   p[c] = p[c] < 0 ? 0 : (p[c] > 1 ? 1 : p[c])
 *     safe     = p[c] < thr for every c;   certain = sd[c] < umax for every c      (false on NaN)
 *     the env receives a if safe && certain, else the zero action ("reject_conservative")
 *     flags:   NIG_FLAG_SHIELDED where the action was replaced;  NIG_FLAG_UNCERTAIN where !certain
 * Every division and the square root are IEEE correctly rounded; no product is fused into a sum.  The spread
 * is the ensemble actor's shifted variance (4 C registers whatever K is; exactly 0 for identical members and
 * for K = 1) with one deliberate difference: the clamp keeps a NaN, so that a member whose logit is -inf
 * rejects (the reference's jnp.std is NaN there and NaN < umax is false).  Against the reference's float64
 * two-pass formula p and sd agree to 1e-5 relative.  A disturbance installed on the handle is ignored.
 * C1 .. c3: host arrays [n_members] of host pointers.  NIG_ERR_INVALID: n_members outside
 * 1 .. NIG_MAX_ENSEMBLE, n_outputs outside 1 .. 4, a NULL array or member pointer, a temperature that is not
 * finite or <= 0, a NaN threshold.  NIG_ERR_UNSUPPORTED: hidden != 256, an env shape without the MFMA actor.
 * The handle's actor, single critic and actor ensemble are left alone, and vice versa.
 */
int nig_set_mlp_safety_ensemble(nig_handle *h, int32_t n_members, int32_t hidden, int32_t n_outputs,
                                const float *const *C1, const float *const *c1, const float *const *C2,
                                const float *const *c2, const float *const *C3, const float *const *c3,
                                float temperature, float prob_threshold, float uncertainty_threshold, void *stream);

/*
 * As nig_rollout_mlp (arguments, minima, obs_out alignment, frozen lanes, tallies, launch counter), with the
 * installed gate.  act_out: the action the env received.  prob_out / unc_out (optional) float: row c of
 * step k at base + k*c_step_stride + c*ld_c, c = 0 .. C-1 (p[c] / sd[c]).  logit_out (optional) float: member m
 * of step k is one [C][ld_c] block at logit_out + (k*n_members + m)*c_step_stride (member_act_out's
 * convention).  Frozen lanes leave their words untouched; rows >= C of a block are never written.  With any of
 * the three: ld_c in [batch, 2^26] and c_step_stride >= C*ld_c.  NIG_ERR_INVALID (nothing launched or
 * written): no actor or no members installed, a bad ld_c / c_step_stride, and every refusal of nig_rollout_mlp;
 * NIG_ERR_UNSUPPORTED for an env shape without the MFMA actor.
 */
int nig_rollout_mlp_gated(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out,
                          int64_t out_stride, float *obs_out, int64_t obs_step_stride, float *act_out,
                          int64_t ld_act, int64_t act_step_stride, float *prob_out, float *unc_out,
                          float *logit_out, int64_t ld_c, int64_t c_step_stride, void *stream);

/*
 * nig_rollout_mlp_gated under the installed limits: the parent's arguments plus xflags_out (nig_rollout_mlp_safe_limited's).  The
 * added constraints are checked on the zero action where the gate rejects.  NIG_ERR_INVALID without installed limits, then every refusal of the parent; a refused call launches and writes nothing.  The kernel is the
 * parent's body with the step law of nig_step_limited applied to the action the env receives, so a rollout equals nig_step_limited fed
 * with the rollout's own actions.
 */
int nig_rollout_mlp_gated_limited(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out,
                                  int64_t out_stride, float *obs_out, int64_t obs_step_stride, float *act_out,
                                  int64_t ld_act, int64_t act_step_stride, float *prob_out, float *unc_out,
                                  float *logit_out, int64_t ld_c, int64_t c_step_stride, uint32_t *xflags_out, void *stream);

/*
 * Constraint projection of the reference's ConstrainedIQLAgent.get_safe_action (agents/safety_critical.py:240-370),
 * fused into the shield's kernel: a constraint predictor f(s, a) with one head row per constraint scores the actor's
 * action; where some violation probability is not below the threshold, the action walks down the gradient of the
 * summed positive logits until every logit is below the tolerance or the steps run out.  The predictor is a
 * (S + A) -> 256 -> 256 -> C ReLU MLP in nig_set_mlp_safety_ensemble's member layouts (C3 [hidden][n_outputs],
 * c3 [n_outputs]); hidden must be 256 (policies.pad_safety_member pads the reference's 128-wide predictor).
 * The law, "nig-project-v1".  Installed: C = n_outputs, thr = threshold (the reference's uncertainty_threshold),
 * tol = tolerance (constraint_tolerance); per call max_iters and step (the reference: 10 and 0.1).  All arithmetic is
 * float32, no product is fused into a sum.  For a live lane on a step:
 *     a0 = actor(s)                                    bit for bit nig_rollout_mlp's action
 *     z  = f(s, a0);  p0[c] = det_sigmoidf(z[c])       each row the arithmetic of nig_rollout_mlp_gated's member rows
 *     if p0[c] < thr for every c < C:                  the env receives a0; iters = -1; viol = p0
 *     else (projected; NIG_FLAG_SHIELDED):
 *         a = a0
 *         for k = 0 .. max_iters-1:                    (z is pass 0's for k = 0)
 *             if z[c] < tol for every c < C: break     (the raw logits, as the reference: safety_critical.py:352)
 *             g = dG/da at (s, a),  G(a) = sum_c relu(f_c(s, a))
 *             a = a - step * g;  a = a < -1 ? -1 : (a > 1 ? 1 : a)        (a NaN stays a NaN)
 *             z = f(s, a)
 *         iters = the gradient steps taken (0 .. max_iters);  viol[c] = det_sigmoidf(z[c]) of the action the env receives
 * The gradient is the analytic backward pass with the derivative of relu at 0 taken as 0 (jax.nn.relu's):
 *     g = W1[S:S+A, :] (m1 . (W2 (m2 . (W3 d)))),   d_c = (z_c > 0),  m1 / m2 = the masks (pre-activation > 0) of the
 * two hidden layers of the forward pass that gave z, "." a select (mask ? x : 0, not a product).  It is evaluated as
 * the network C -> 256 -> 256 -> A with the weights W3^T (zero-padded to four input rows), W2^T, W1[S:S+A, :]^T and
 * zero biases in the forward pass's summation order (layer 1 in natural k order, layers 2 and 3 in the accumulator
 * tiles' row order, the head as two lane-half fma chains joined by one add; tests/mlp_project_ref.c restates it).
 * iters = 0 occurs: a lane whose p0 is not below thr but whose logits are all below tol is "projected" without a
 * step (at the reference's defaults 0.1 and 0.01: -2.2 <~ z < 0.01).  Comparisons with NaN are false: such a lane is
 * projected and walks until the steps run out; a NaN passes through the update.  A disturbance installed on the
 * handle is ignored.  NIG_ERR_INVALID: a NULL argument, n_outputs outside 1 .. 4, a non-finite threshold or
 * tolerance.  NIG_ERR_UNSUPPORTED: hidden != 256, an env shape without the MFMA actor.  The handle's actor, critic,
 * gate and actor ensemble are left alone, and vice versa.
 */
#define NIG_MAX_PROJECT_ITERS 16
int nig_set_mlp_constraint(nig_handle *h, int32_t hidden, int32_t n_outputs, const float *C1, const float *c1,
                           const float *C2, const float *c2, const float *C3, const float *c3, float threshold,
                           float tolerance, void *stream);

/*
 * As nig_rollout_mlp (arguments, minima, obs_out alignment, frozen lanes, tallies, launch counter), with the
 * installed constraint projection.  act_out: the action the env received.  prob_out / viol_out (optional) float:
 * row c of step k at base + k*c_step_stride + c*ld_c, c = 0 .. C-1 (p0[c] / viol[c]).  iters_out (optional) int32:
 * row k at iters_out + k*out_stride.  grad_out (optional) float, act_out's layout and pitches: the FIRST gradient
 * of the step, written where iters >= 1 and untouched elsewhere.  Frozen lanes leave their words untouched; rows
 * >= C of a block are never written.  With prob_out or viol_out: ld_c in [batch, 2^26] and c_step_stride >= C*ld_c;
 * with grad_out: ld_act in [batch, 2^26] and act_step_stride >= A*ld_act.  NIG_ERR_INVALID (nothing launched or
 * written): no actor or no predictor installed, max_iters outside 1 .. NIG_MAX_PROJECT_ITERS, a non-finite step, a
 * bad pitch, and every refusal of nig_rollout_mlp; NIG_ERR_UNSUPPORTED for an env shape without the MFMA actor.
 */
int nig_rollout_mlp_projected(nig_handle *h, int32_t n_steps, int32_t max_iters, float step, float *reward_out,
                              uint32_t *flags_out, int64_t out_stride, float *obs_out, int64_t obs_step_stride,
                              float *act_out, int64_t ld_act, int64_t act_step_stride, float *prob_out,
                              float *viol_out, int32_t *iters_out, float *grad_out, int64_t ld_c,
                              int64_t c_step_stride, void *stream);

/*
 * nig_rollout_mlp_projected under the installed limits: the parent's arguments plus xflags_out (nig_rollout_mlp_safe_limited's).  The
 * added constraints are checked on the projected action.  NIG_ERR_INVALID without installed limits, then every refusal of the parent; a refused call launches and writes nothing.  The kernel is the
 * parent's body with the step law of nig_step_limited applied to the action the env receives, so a rollout equals nig_step_limited fed
 * with the rollout's own actions.
 */
int nig_rollout_mlp_projected_limited(nig_handle *h, int32_t n_steps, int32_t max_iters, float step, float *reward_out,
                                      uint32_t *flags_out, int64_t out_stride, float *obs_out, int64_t obs_step_stride,
                                      float *act_out, int64_t ld_act, int64_t act_step_stride, float *prob_out,
                                      float *viol_out, int32_t *iters_out, float *grad_out, int64_t ld_c,
                                      int64_t c_step_stride, uint32_t *xflags_out, void *stream);

/*
 * Sensor / actuator noise inside the closed loop ("nig-disturb-v1"): the policy sees a noisy observation, the plant
 * receives a noisy action.  Stands in for the observation_noise / action_noise runs of the reference's
 * RobustnessBenchmark (benchmarks/industrial_benchmarks.py:455-573) and for predict(obs, deterministic=False) of
 * CQL / IQL / TD3BC, clip(actor + 0.1 N(0,1), -1, 1) (agents/cql.py:345-350).
 * For a live lane with global index g, on the step with launch counter t, step_pre = the lane's step count before the
 * step; float32 throughout, every product rounded before its sum:
 *     td = (hold == NIG_HOLD_EPISODE) ? t - step_pre : t          uint32; the counter the episode's first step had
 *     zo[0..S) = normals of generator stream "policy", blocks +32.. at key (g, td, seed): normal k = word k & 3 of block
 *                +32 + (k >> 2);   za[0..A) = the same of blocks +48..
 *     o_k = s_k + sigma_obs[k] * zo_k                             if any sigma_obs[k] != 0, else o = s (no draw is made)
 *     u   = policy(o)                                             nig_rollout_policy_disturbed: the whole "nig-policy-v1" law
 *                                                                 on o (PID: e = setpoint - o), its own draws keyed at t, its
 *                                                                 own clip; nig_rollout_mlp_disturbed: the actor with its tanh
 *     u_j = u_j + sigma_act[j] * za_j                             if any sigma_act[j] != 0
 *     a_j = u_j < clip_lo ? clip_lo : u_j;  a_j = a_j > clip_hi ? clip_hi : a_j
 *     IndustrialEnv.step(a) unchanged (the env's own clip follows).
 * The policy stream's own blocks (+0 mixture draw, +1.. normals, +8.. uniform noise, +16.. random action) stay where they
 * are, keyed at t.  NIG_HOLD_EPISODE is upstream's law: the reference calls jax.random.normal(episode_key, ...) with the same
 * key on every step of an episode (industrial_benchmarks.py:492-508), i.e. one offset per episode.
 */
#define NIG_HOLD_STEP 0      /* fresh draws every step */
#define NIG_HOLD_EPISODE 1   /* one draw vector per episode, reused on each of its steps: upstream's law */
typedef struct nig_disturbance {
    float sigma_obs[NIG_MAX_STATE_DIM];   /* >= 0, finite */
    float sigma_act[NIG_MAX_ACTION_DIM];  /* >= 0, finite */
    float clip_lo, clip_hi;               /* -inf / +inf = no clip; clip_lo <= clip_hi */
    int32_t hold;
} nig_disturbance;

/* Install (copy) the disturbance the _disturbed rollouts apply; d == NULL removes it.  NIG_ERR_INVALID, the installed one
 * kept: a negative / NaN / infinite sigma, clip_lo > clip_hi or a NaN bound, an unknown hold.  Only the two entry points
 * below read it: nig_rollout_policy, nig_rollout_mlp, nig_rollout_mlp_safe, nig_rollout_mlp_gated, nig_rollout_mlp_projected and nig_rollout_mlp_ensemble ignore an installed
 * disturbance (the shield and the ensemble have no disturbed form). */
int nig_set_disturbance(nig_handle *h, const nig_disturbance *d /* host; NULL clears */, void *stream);

/*
 * nig_rollout_policy / nig_rollout_mlp (arguments, minima, alignment, frozen lanes, tallies, launch counter) under the
 * installed disturbance.  obs_out holds the TRUE state s, act_out the action a the env received, and
 *   seen_out  optional float row-major [n_steps][B][S]: the observation o the policy acted on, step k at
 *             seen_out + k*seen_step_stride; obs_out's rules (16-byte aligned, stride >= S*B and a multiple of 4 floats);
 *             frozen lanes leave their rows untouched.
 * With all sigmas zero and infinite clip bounds a call equals its undisturbed twin bit for bit (seen_out == obs_out).
 * nig_rollout_policy_disturbed always runs the one-wave closed-loop kernel, whatever the batch.
 * NIG_ERR_INVALID (nothing launched or written): no disturbance installed, no policy / actor installed, and every
 * refusal of the twin.  NIG_ERR_UNSUPPORTED: nig_rollout_mlp_disturbed on an env shape without the MFMA actor.
 */
int nig_rollout_policy_disturbed(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out, int64_t out_stride,
                                 float *obs_out, int64_t obs_step_stride, float *act_out, int64_t ld_act,
                                 int64_t act_step_stride, float *seen_out, int64_t seen_step_stride, void *stream);
int nig_rollout_mlp_disturbed(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out, int64_t out_stride,
                              float *obs_out, int64_t obs_step_stride, float *act_out, int64_t ld_act,
                              int64_t act_step_stride, float *seen_out, int64_t seen_step_stride, void *stream);

/*
 * nig_rollout_policy_disturbed / nig_rollout_mlp_disturbed under the installed limits: the parents' arguments plus xflags_out
 * (nig_rollout_mlp_safe_limited's).  The added constraints are checked on the true state and on the disturbed, clipped action the
 * plant receives (act_out's rows).  The policy twin has the one-wave kernel form only.  NIG_ERR_INVALID without installed limits, then every refusal of the parent; a refused call launches and writes nothing.  The kernel is the
 * parent's body with the step law of nig_step_limited applied to the action the env receives, so a rollout equals nig_step_limited fed
 * with the rollout's own actions.
 */
int nig_rollout_policy_disturbed_limited(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out, int64_t out_stride,
                                         float *obs_out, int64_t obs_step_stride, float *act_out, int64_t ld_act,
                                         int64_t act_step_stride, float *seen_out, int64_t seen_step_stride, uint32_t *xflags_out,
                                         void *stream);
int nig_rollout_mlp_disturbed_limited(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out, int64_t out_stride,
                                      float *obs_out, int64_t obs_step_stride, float *act_out, int64_t ld_act,
                                      int64_t act_step_stride, float *seen_out, int64_t seen_step_stride, uint32_t *xflags_out,
                                      void *stream);

/*
 * Host-buffer forms for SMALL batches -- the single-env drop-in classes (env.reset() / env.step()
 * return NumPy arrays, base.py:133-213).  Inputs are host arrays, results are copied back to host
 * arrays; the library stages through pinned memory it owns and synchronises `stream` once before
 * returning.  PCIe-/launch-latency bound by construction (tens of microseconds per call); use the
 * device-pointer entry points above for throughput.
 *   actions     float  [A][B] host            step_noise  double [k_step][B] host or NULL (fast mode)
 *   init_noise  double [k_reset][B] host or NULL
 *   state_out   float  [S][B] host (new state == observation)
 *   reward64_out double [B] host,  flags_out uint32 [B] host
 */
int nig_reset_host(nig_handle *h, const double *init_noise, float *state_out, void *stream);
int nig_step_host(nig_handle *h, const float *actions, const double *step_noise, float *state_out,
                  double *reward64_out, uint32_t *flags_out, void *stream);
/* the same with float64 actions double [A][B] (nig_step64's arithmetic) */
int nig_step_host64(nig_handle *h, const double *actions, const double *step_noise, float *state_out,
                    double *reward64_out, uint32_t *flags_out, void *stream);

/*
 * Mixed batch: several environment types in ONE padded structure-of-arrays batch (BASELINE config
 * "all 7 envs mixed-batch, heterogeneous state dims, padded SoA").  Lanes are grouped in contiguous
 * segments, one env type each, every segment starting on a multiple of 256 lanes (wavefronts and
 * blocks are homogeneous); all segments share ONE observation matrix float [S_max][ld] (rows >= S of
 * a segment stay zero), and actions / per-step outputs use the same column layout ([A_max][ld],
 * [n_steps][ld]).  The reference has no vectorised env at all: this stands in for N_total calls of
 * utils.make with different ids stepped by one loop (performance_benchmark.py:106-133 over a list of envs).
 * Global lane index of column c = env_index0 + c (keys the generator: results do not depend on the
 * other segments).  The fused rollout over the whole mixed batch is ONE kernel launch: a block finds
 * its segment in a table passed with the launch, the most expensive envs' blocks are issued first.
 */
#define NIG_MIXED_MAX_SEGMENTS 12
typedef struct nig_mixed nig_mixed;
typedef struct nig_mixed_info {
    int32_t n_segments, state_dim_max, action_dim_max, reserved;
    int64_t lanes;                                   /* sum of the segment counts                       */
    int64_t ld;                                      /* columns of the padded matrices (256-aligned)    */
    int32_t env[NIG_MIXED_MAX_SEGMENTS];             /* env id of segment k                             */
    int64_t offset[NIG_MIXED_MAX_SEGMENTS];          /* first column of segment k                       */
    int64_t count[NIG_MIXED_MAX_SEGMENTS];           /* lanes of segment k                              */
} nig_mixed_info;

/* flags as for nig_create (apply to every segment); seed / env_index0 as for nig_create */
int nig_create_mixed(int32_t n_segments, const int32_t *env_ids, const int64_t *counts, int device, uint64_t seed,
                     uint64_t env_index0, uint32_t flags, nig_mixed **out);
int nig_mixed_destroy(nig_mixed *m);
int nig_mixed_get_info(const nig_mixed *m, nig_mixed_info *out);
float *nig_mixed_state(const nig_mixed *m);                 /* device float [S_max][ld], library-owned          */
nig_handle *nig_mixed_segment(const nig_mixed *m, int32_t k);   /* borrowed handle of segment k: tallies, counters,
                                                               constraint mask, nig_step ... all per-handle calls */
int nig_mixed_reset(nig_mixed *m, void *stream);            /* IndustrialEnv.reset for every lane, fast mode    */
int nig_mixed_fill_actions(nig_mixed *m, uint32_t t, float *actions /* [A_max][ld] */, void *stream);
/* IndustrialEnv.step for every lane (fast mode): actions float [A_max][ld] (rows >= A of a segment ignored),
 * reward_out float [ld] / flags_out uint32 [ld] optional.  One step-kernel launch per segment on `stream`. */
int nig_mixed_step(nig_mixed *m, const float *actions, float *reward_out, uint32_t *flags_out, void *stream);
/* n_steps of IndustrialEnv.step for every lane of every segment in ONE launch; arguments as nig_rollout with
 * ld_act = ld: action_ring slot s at action_ring + s*slot_stride laid out [A_max][ld]; reward_out / flags_out
 * rows [ld] (both or neither), row of step k at base + k*out_stride (0 = overwrite). */
int nig_mixed_rollout(nig_mixed *m, int32_t n_steps, const float *action_ring, int64_t slot_stride, int32_t ring_len,
                      float *reward_out, uint32_t *flags_out, int64_t out_stride, void *stream);
/* The same single launch for handles the caller created itself (e.g. bound to its own matrix with
 * nig_bind_state): handle k uses columns [lane_offsets[k], lane_offsets[k] + batch_k) of the action ring and of
 * the output rows (pitch ld_act / out_stride as above).  All handles on one device, fast mode. */
int nig_rollout_mixed(nig_handle *const *handles, const int64_t *lane_offsets, int32_t n_handles, int32_t n_steps,
                      const float *action_ring, int64_t ld_act, int64_t slot_stride, int32_t ring_len,
                      float *reward_out, uint32_t *flags_out, int64_t out_stride, void *stream);
/* The same launch also returning the observation of every env.step (the obs of base.py:157-213's return tuple; what
 * get_dataset stores per transition, chemical_reactor.py:395-412, power_grid.py:234-249): obs_out float
 * [n_steps][S_max][ld_obs], the padded SoA layout of the state matrix per step -- handle k writes rows < S_k of its
 * columns [lane_offsets[k], +batch_k) of step s at obs_out + s*obs_step_stride (>= S_max*ld_obs, or 0 = overwrite),
 * rows >= S_k are not touched.  Needs reward_out and flags_out.  nig_mixed_rollout_obs: ld_obs = the batch's ld. */
int nig_rollout_mixed_obs(nig_handle *const *handles, const int64_t *lane_offsets, int32_t n_handles, int32_t n_steps,
                          const float *action_ring, int64_t ld_act, int64_t slot_stride, int32_t ring_len,
                          float *reward_out, uint32_t *flags_out, int64_t out_stride,
                          float *obs_out, int64_t ld_obs, int64_t obs_step_stride, void *stream);
int nig_mixed_rollout_obs(nig_mixed *m, int32_t n_steps, const float *action_ring, int64_t slot_stride, int32_t ring_len,
                          float *reward_out, uint32_t *flags_out, int64_t out_stride, float *obs_out, int64_t obs_step_stride,
                          void *stream);

/* Fill float [A][ld_act] with the synthetic uniform [-1,1) actions of stream
 * "action" for launch counter `t` (bench / parity workload generator). */
int nig_fill_actions(nig_handle *h, uint32_t t, float *actions, int64_t ld_act, void *stream);

/* Teacher forcing / checkpointing: copy state, counter words in or out (device pointers,
 * float [S][ld], uint32 [B]); either pointer may be NULL. */
int nig_set_state(nig_handle *h, const float *state, int64_t ld, const uint32_t *ctr, void *stream);
int nig_get_state(nig_handle *h, float *state, int64_t ld, uint32_t *ctr, void *stream);

/*
 * env.get_safety_metrics() for every lane (named by the reference README; defined as
 * the SafetyMetrics of the last step, base.py:94-124): int32 [5][ld_out] rows =
 * constraints_satisfied, total_constraints, violation_count, critical_violations,
 * and safety_score*total (== satisfied), decoded from a flag array of the last step.
 * total_constraints = the handle's ENABLED built-in constraints (nig_env_spec.n_constraints minus
 * those removed with nig_set_constraint_mask; 4 for AdvancedChemicalReactor); violation_count
 * includes NIG_FLAG_NVIOL_HI.
 */
int nig_get_safety_metrics(nig_handle *h, const uint32_t *flags, int32_t *out, int64_t ld_out,
                           void *stream);

/*
 * Reduce the per-lane tallies (NIG_F_TALLY) to one partial vector double[NIG_T_ROWS]
 * on the device (sum rows, min/max rows).  `partial_out` is a DEVICE pointer.  The
 * cross-GPU combine is an all-gather of these vectors (see parallel.py).
 */
int nig_reduce_tally(nig_handle *h, double *partial_out, void *stream);

/*
 * Per-episode records ("episode log") from the per-step rows every rollout entry point writes.  The tally above can say
 * thirteen sums about the episodes it saw; what the reference's evaluation layer does with single episodes -- median_return,
 * violation_rate, metadata["individual_returns"] / ["episode_violations"] of SafetyBenchmark / PerformanceBenchmark
 * (benchmarks/industrial_benchmarks.py:95-341), the per-episode lists benchmarks/statistical_analysis.py tests -- needs one
 * number per episode.  The log is built from reward_out / flags_out rows alone, so it serves nig_rollout, _sampled, _policy,
 * _mlp, _mlp_safe, _mlp_ensemble, the _disturbed twins, nig_step and nig_plan_* alike, in every kernel form.
 *
 * The law, per lane, per step row in order (csrc/nig_episodes.hpp episode_row: the one statement; episodes.episodes_from_rows
 * restates it in NumPy):
 *   - a flag word with NIG_FLAG_INACTIVE is skipped (frozen lane);
 *   - otherwise return += reward -- in float32 for an env with nig_env_spec.reward_is_f32, (double)((float)ret + reward), which
 *     is the kernels' own sum bit for bit; in float64 over the float rows for every other env (the kernels add the float64
 *     reward there: a lane's return agrees within 2^-23 x the sum of |reward_k|) --, violations += bits 5-6 (+ 4 with
 *     NIG_FLAG_NVIOL_HI), the four per-constraint bits, NIG_FLAG_SHIELDED and NIG_FLAG_UNCERTAIN are counted;
 *   - on NIG_FLAG_TERMINATED | NIG_FLAG_TRUNCATED the episode becomes record number count[lane] if count[lane] < capacity,
 *     count[lane] += 1 regardless (count > capacity tells an overflow), and the running values start over.
 * The running values persist in the log between calls: rows cut into several calls give the records of one call.
 *
 * Layout: ONE caller-owned device allocation of nig_episode_log_layout.bytes (8-byte aligned), structure-of-arrays with row
 * pitch ld (>= batch; any value, multiples of 64 not required), record k of lane i at element k*ld + i of
 *   ret    double [capacity][ld]   episode return
 *   w[0]   uint32 [capacity][ld]   NIG_CTR_* format: length (the done step's step field) | NIG_CTR_DONE | violations << 16
 *   w[1]   uint32 [capacity][ld]   the done step's flag word & (TERMINATED | TRUNCATED | the NCRIT field | SHUTDOWN)
 *   w[2]   uint32 [capacity][ld]   steps with constraint 0 violated (low 16 bits), constraint 1 (high 16 bits)
 *   w[3]   uint32 [capacity][ld]   the same for constraint 2 and NIG_FLAG_VIOL3
 *   w[4]   uint32 [capacity][ld]   NIG_FLAG_SHIELDED steps (low 16 bits), NIG_FLAG_UNCERTAIN steps (high 16 bits)
 *   count  uint32 [ld]             finished episodes of the lane
 *   carry  double [ld] + uint32 [4][ld]   the running return; running violations, w[2], w[3], w[4]
 *   tally  double [NIG_T_ROWS + 1][ld], scratch double [256][NIG_T_ROWS]   work space of nig_reduce_episodes
 * Written set (columns [0, batch) only -- the pad columns [batch, ld) of every row are never written):
 *   nig_episode_log_init     count and carry;
 *   nig_collect_episodes     count and carry, and of lane i the record rows [count_before, min(count_after, capacity)): never a
 *                            record row at or beyond the lane's count, never one at or beyond capacity; reward / flags are inputs;
 *   nig_reduce_episodes      tally and scratch; partial_out; the records are inputs.
 */
typedef struct nig_episode_log_layout {
    int64_t batch, capacity, ld, bytes;
    int64_t off_ret;         /* double [capacity][ld]                    */
    int64_t off_w[5];        /* uint32 [capacity][ld] each               */
    int64_t off_count;       /* uint32 [ld]                              */
    int64_t off_carry_ret;   /* double [ld]                              */
    int64_t off_carry_w;     /* uint32 [4][ld]                           */
    int64_t off_tally;       /* double [NIG_T_ROWS + 1][ld]              */
    int64_t off_scratch;     /* double [256][NIG_T_ROWS]                 */
} nig_episode_log_layout;
#define NIG_MAX_EPISODE_CAPACITY (1 << 20)   /* records per lane */

/* Size / layout of a log of `capacity` records per lane for `batch` lanes at row pitch ld (0 = batch rounded up to 64).
 * NIG_ERR_INVALID: batch outside [1, 2^24], capacity outside [1, 2^20], ld != 0 outside [batch, 2^26], NULL out. */
int nig_episode_log_query(int64_t batch, int64_t capacity, int64_t ld, nig_episode_log_layout *out);
/* Every entry point below takes the log with the (capacity, ld) its memory was sized for (ld 0 = the default pitch again), checks
 * every argument before anything is enqueued (a refused call launches and writes nothing), and enqueues on `stream`.
 * nig_episode_log_init: no episode finished, nothing running. */
int nig_episode_log_init(nig_handle *h, void *log, int64_t capacity, int64_t ld, void *stream);
/* n_steps (>= 1) step rows: reward float / flags uint32, both required, row of step k at base + k*out_stride, out_stride >= batch
 * (<= 2^26; with n_steps == 1 it is not used and may be 0: the [B] arrays nig_step writes). */
int nig_collect_episodes(nig_handle *h, int32_t n_steps, const float *reward, const uint32_t *flags, int64_t out_stride,
                         void *log, int64_t capacity, int64_t ld, void *stream);
/* The tally of the records that count: record (k, i) counts iff k < min(count[i], capacity) and k*batch + i < n_episodes (a
 * fixed episode count per lane: the first n_episodes / batch episodes of every lane, one more of the first n_episodes % batch
 * lanes -- the episodes the rounds of evaluate_with_safety play).  Each lane's counted records go, in order, through the
 * arithmetic of the kernels' own tally (total_constraints = the handle's enabled constraints), the lanes are reduced as
 * nig_reduce_tally reduces them: partial_out (DEVICE double [NIG_T_ROWS + 1]) holds the NIG_T_* rows, then the number of
 * counted episodes with a non-zero violation count.  partial_out[NIG_T_EPISODES] < n_episodes: lanes had not finished their
 * share, or capacity was too small.  NIG_ERR_INVALID: n_episodes outside [1, capacity*batch]. */
int nig_reduce_episodes(nig_handle *h, void *log, int64_t capacity, int64_t ld, int64_t n_episodes, double *partial_out,
                        void *stream);

/*
 * The path's one exchange (BASELINE north_star: "an RCCL all-reduce over xGMI only for the final return /
 * safety-violation reduction"), for hosts that do not go through torch.distributed: reduce the tallies of this
 * rank's handles (one, or the segments of a mixed batch) to one partial vector, ncclAllGather the partial vectors
 * of all ranks of `comm` (an ncclComm_t the caller created, one rank per GPU; NULL = single process, no collective)
 * and combine them in RANK ORDER on every rank: sums as fixed-order fp64 additions, exact integer counts, min / max
 * rows -- bit-identical on all ranks.  The 13 aggregates of evaluate_with_safety (utils.py:128-152) follow from
 * `out` (DEVICE double [NIG_T_ROWS]).  `scratch`: DEVICE doubles, at least (n_handles + 1 + ranks) * NIG_T_ROWS.
 * RCCL is taken from the copy already loaded in the process (dlsym), else librccl.so is dlopen'ed.
 */
int nig_reduce_metrics(nig_handle *const *handles, int32_t n_handles, void *nccl_comm, double *scratch,
                       int64_t scratch_doubles, double *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NIG_H */
