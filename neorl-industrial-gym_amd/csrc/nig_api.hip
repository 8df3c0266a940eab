// nig_api.hip -- C ABI of libnig.so (include/nig.h) and the environment-independent kernels.
// The per-environment kernels are instantiated in env_*.hip and the family units beside them, and reached through nig::EnvLaunch.
#include <dlfcn.h>

#include <atomic>
#include <vector>

#include "nig_launch.hpp"
#include "nig_episodes.hpp"

namespace nig {

__global__ void __launch_bounds__(BLOCK) init_ws_kernel(uint32_t *ctr, long long *life, double *ep_ret, double *tally,
                                                        int64_t ld, int64_t B)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= ld) return;
    ctr[i] = NIG_CTR_DONE;   // nothing steps before the first reset
    life[i] = 0;
    if (ep_ret) ep_ret[i] = 0.0;
    if (tally) {
#pragma unroll
        for (int r = 0; r < NIG_T_ROWS; ++r) tally[(int64_t)r * ld + i] = 0.0;
        tally[(int64_t)NIG_T_RET_MIN * ld + i] = __builtin_inf();
        tally[(int64_t)NIG_T_RET_MAX * ld + i] = -__builtin_inf();
    }
}

__global__ void set_u32_kernel(uint32_t *p, uint32_t v) { *p = v; }

// row-major action ring [R][B][A] (slot stride `aos_stride` floats) -> rows [R][A][ld]: one thread per lane, slots blockIdx.y,
// blockIdx.y + gridDim.y, ... (the grid's y extent is capped at 65 535)
__global__ void __launch_bounds__(BLOCK) action_rows_kernel(const float *aos, int64_t aos_stride, float *soa, int64_t ld, int64_t B, int A, int slots)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= B) return;
    for (int r = (int)blockIdx.y; r < slots; r += (int)gridDim.y) {
        const float *src = aos + (int64_t)r * aos_stride + i * A;
        float *dst = soa + (int64_t)r * A * ld + i;
        for (int k = 0; k < A; ++k) dst[(int64_t)k * ld] = src[k];
    }
}

// nig_clock_stamp: one wave per block, many more blocks than compute units; a block stamps the slot of the compute unit it
// runs on -- slot = XCD (HW_REG_XCC_ID) x 256 + HW_REG_HW_ID's {se_id, sh_id, cu_id} -- because s_memtime is NOT one counter per
// chip (round 5, first attempt: per-XCD slots written by whichever block came last gave 2 030 .. 5 570 "MHz" across the XCDs of
// one run).  Waves of one compute unit write the same pair of words with values a few cycles apart (any of them will do).
__global__ void __launch_bounds__(64) clock_stamp_kernel(unsigned long long *o)
{
    const unsigned long long t = __builtin_amdgcn_s_memtime(), r = __builtin_amdgcn_s_memrealtime();
    const unsigned xcc = __builtin_amdgcn_s_getreg((4 - 1) << 11 | 0 << 6 | 20) & 7u;        // HW_REG_XCC_ID (id 20), bits 3:0
    const unsigned cu = __builtin_amdgcn_s_getreg((8 - 1) << 11 | 8 << 6 | 4) & 0xFFu;       // HW_REG_HW_ID (id 4), bits 15:8: cu_id, sh_id, se_id
    const unsigned slot = xcc * 256u + cu;
    if (threadIdx.x == 0) { o[2 * slot] = t; o[2 * slot + 1] = r; }
}

// n_total = the handle's enabled built-in constraints (3, 4 for AdvancedChemicalReactor, fewer after
// nig_set_constraint_mask): SafetyMetrics.total_constraints, base.py:115
__global__ void __launch_bounds__(BLOCK) safety_metrics_kernel(const uint32_t *flags, int32_t *out, int64_t ld_out,
                                                               int64_t B, int n_total)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= B) return;
    const uint32_t f = flags[i];
    const int nv = (int)((f >> NIG_FLAG_NVIOL_SHIFT) & 3u) + ((f & NIG_FLAG_NVIOL_HI) ? 4 : 0);
    const int nc = (int)((f >> NIG_FLAG_NCRIT_SHIFT) & 3u);
    out[0 * ld_out + i] = n_total - nv;   // constraints_satisfied   base.py:96-106
    out[1 * ld_out + i] = n_total;        // total_constraints       base.py:115
    out[2 * ld_out + i] = nv;             // violation_count
    out[3 * ld_out + i] = nc;             // critical_violations
    out[4 * ld_out + i] = n_total - nv;   // safety_score * total    base.py:116
}

// deterministic two-stage reduction of the tally rows: fixed grid, fixed tree order
__global__ void __launch_bounds__(BLOCK) reduce_tally_stage1(const double *tally, int64_t ld, int64_t B, double *scratch)
{
    __shared__ double sh[BLOCK];
    for (int r = 0; r < NIG_T_ROWS; ++r) {
        const bool is_min = (r == NIG_T_RET_MIN), is_max = (r == NIG_T_RET_MAX);
        double acc = is_min ? __builtin_inf() : (is_max ? -__builtin_inf() : 0.0);
        for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < B; i += (int64_t)gridDim.x * BLOCK) {
            const double v = tally[(int64_t)r * ld + i];
            acc = is_min ? fmin(acc, v) : (is_max ? fmax(acc, v) : acc + v);
        }
        sh[threadIdx.x] = acc;
        __syncthreads();
        for (int w = BLOCK / 2; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) {
                const double o = sh[threadIdx.x + w];
                sh[threadIdx.x] = is_min ? fmin(sh[threadIdx.x], o) : (is_max ? fmax(sh[threadIdx.x], o) : sh[threadIdx.x] + o);
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) scratch[(int64_t)blockIdx.x * NIG_T_ROWS + r] = sh[0];
        __syncthreads();
    }
}

// Second stage: the block partials of stage 1 in block order, one thread per tally row.  The sums keep their fixed
// sequential order (bit-reproducible, and the same bits as rounds 1-2), but the partials are brought into LDS by the
// whole block first: read one by one from global memory by 13 threads, the 256 dependent load -> add steps took 65 us
// on the critical path of the path's one cross-GPU exchange; from LDS they take ~1 us.
__global__ void __launch_bounds__(REDUCE_BLOCKS) reduce_tally_stage2(const double *scratch, int nblk, double *out)
{
    __shared__ double sh[REDUCE_BLOCKS * NIG_T_ROWS];
    for (int i = (int)threadIdx.x; i < nblk * NIG_T_ROWS; i += REDUCE_BLOCKS) sh[i] = scratch[i];
    __syncthreads();
    const int r = threadIdx.x;
    if (r >= NIG_T_ROWS) return;
    const bool is_min = (r == NIG_T_RET_MIN), is_max = (r == NIG_T_RET_MAX);
    double acc = is_min ? __builtin_inf() : (is_max ? -__builtin_inf() : 0.0);
    for (int b = 0; b < nblk; ++b) {
        const double v = sh[b * NIG_T_ROWS + r];
        acc = is_min ? fmin(acc, v) : (is_max ? fmax(acc, v) : acc + v);
    }
    out[r] = acc;
}

// float64 action rows -> float32 (envs whose own arithmetic converts the action on entry)
__global__ void __launch_bounds__(BLOCK) narrow_rows_kernel(const double *src, int64_t ld_src, float *dst, int64_t ld_dst,
                                                            int rows, int64_t B)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= B) return;
    for (int k = 0; k < rows; ++k) dst[(int64_t)k * ld_dst + i] = (float)src[(int64_t)k * ld_src + i];
}

// combine `n` partial tally vectors [n][NIG_T_ROWS] in index order: sums, min / max rows (one thread per row)
__global__ void combine_partials_kernel(const double *parts, int n, double *out)
{
    const int r = threadIdx.x;
    if (r >= NIG_T_ROWS) return;
    const bool is_min = (r == NIG_T_RET_MIN), is_max = (r == NIG_T_RET_MAX);
    double acc = is_min ? __builtin_inf() : (is_max ? -__builtin_inf() : 0.0);
    for (int b = 0; b < n; ++b) {
        const double v = parts[(int64_t)b * NIG_T_ROWS + r];
        acc = is_min ? fmin(acc, v) : (is_max ? fmax(acc, v) : acc + v);
    }
    out[r] = acc;
}

__global__ void __launch_bounds__(BLOCK) copy_rows_kernel(const float *src, int64_t ld_src, float *dst, int64_t ld_dst,
                                                          int rows, int64_t B)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= B) return;
    for (int k = 0; k < rows; ++k) dst[(int64_t)k * ld_dst + i] = src[(int64_t)k * ld_src + i];
}

}  // namespace nig

// =====================================================================================
// host side: C ABI
// =====================================================================================
using namespace nig;

struct nig_handle {
    int env = 0;
    int device = 0;
    unsigned cus = 0;          // compute units of `device`: default of the kernel-form thresholds (nig_tune)
    int64_t B = 0;
    uint64_t seed = 0, env0 = 0;
    int max_steps = 0;
    double dt = 0.0;
    uint32_t flags = 0;
    uint32_t t = 0;            // RNG launch counter
    uint32_t cmask = 0;        // enabled built-in constraints (bit k)
    nig_layout lay = {};
    char *ws = nullptr;
    bool owns_ws = false;
    double *scratch = nullptr; // reduce scratch [REDUCE_BLOCKS][NIG_T_ROWS] (inside workspace tail)
    uint32_t *t_dev = nullptr; // device copy of t read by graph-replayed step kernels
    float *state = nullptr;    // state rows: inside the workspace, or an array bound by the caller
    int64_t ld_state = 0;
    nig_policy *pol_dev = nullptr;   // device copy of the installed policy
    nig_policy pol_host = {};  // staging copy (must outlive the async H2D copy)
    bool has_policy = false;
    float *mlp_stream = nullptr;     // device copy of the MFMA operand stream of the MLP actor (owned)
    float *mlp_cstream = nullptr;    // device copy of the MFMA operand stream of the safety critic (owned)
    float *mlp_bf16_stream = nullptr;   // device copy of the bf16 operand image of the MLP actor (owned; nig_set_mlp_policy_bf16), BF16_STREAM_BYTES bytes
    // the ONE actor slot's kind (SHAPE_KIND_*, nig_mlp_shape_stream.hpp): mlp_stream holds the reference image (nig_set_mlp_policy, or a
    // nig_set_mlp_policy_dims call of the reference class), mlp_shape_stream the shaped image of any other class (owned, allocated once
    // for the env's largest class); actor_dims: the installed actor's unpadded hidden widths
    int actor_kind = SHAPE_KIND_NONE, actor_nh = 0; int32_t actor_dims[3] = {0, 0, 0}; float *mlp_shape_stream = nullptr;
    // ACTOR_KIND_LN ("nig-mlp-ln-v1", nig_set_mlp_policy_ln): the LayerNorm actor's image (owned) and its eps
    float *mlp_ln_stream = nullptr; float ln_eps = 0.0f;
    float mlp_threshold = 0.0f;      // shield threshold of nig_rollout_mlp_safe
    // the ONE critic slot's kind (NIG_SAFETY_*): mlp_cstream holds the sigmoid critic's image (nig_set_mlp_safety) or the categorical
    // critic's (nig_set_mlp_safety_categorical), whose head rows 16 .. 63 lie in mlp_ctail (owned, MLP_TAIL_FLOATS floats)
    int mlp_ckind = NIG_SAFETY_NONE; float *mlp_ctail = nullptr; int cat_atoms = 0; uint64_t cat_mask = 0;
    // NIG_SAFETY_SIGMOID_LN ("nig-mlp-ln-shield-v1", nig_set_mlp_safety_ln): the LayerNorm critic's image (owned) and its eps
    float *mlp_cln_stream = nullptr; float cln_eps = 0.0f;
    // NIG_SAFETY_SIGMOID_SHAPED ("nig-mlp-shape-shield-v1", nig_set_mlp_safety_dims): the shaped critic's image (owned, allocated once
    // for the env's largest class) and its class (SHAPE_KIND_128 .. SHAPE_KIND_3); critic_dims: the installed critic's unpadded hidden widths
    float *mlp_cshape_stream = nullptr; int critic_class = SHAPE_KIND_NONE, critic_nh = 0; int32_t critic_dims[3] = {0, 0, 0};
    // nig_set_mlp_ensemble (owned): the members' operand streams back to back, MLP_STREAM_FLOATS floats each; their active weights
    // nig_set_mlp_safety_ensemble: the gate's member streams (owned), MLP_CSTREAM_FLOATS apart, and its law's parameters
    float *gate_stream = nullptr; int gate_members = 0, gate_cap = 0, gate_outputs = 0; float gate_T = 1.0f, gate_thr = 0.0f, gate_umax = 0.0f;
    // nig_set_mlp_constraint: the constraint predictor's forward and backward operand streams (owned) and its law's parameters
    float *proj_cstream = nullptr, *proj_bstream = nullptr; int proj_outputs = 0; float proj_thr = 0.0f, proj_tol = 0.0f;
    float *ens_stream = nullptr; double *ens_w = nullptr; int ens_members = 0, ens_cap = 0, ens_method = 0; double ens_wsum = 0.0; float ens_threshold = 0.0f;
    nig_disturbance dist = {}; bool has_dist = false;      // nig_set_disturbance: what the _disturbed rollouts apply
    float *act32 = nullptr;    // nig_step64 on an env that takes float32 actions: the narrowed rows [A][ld] (owned, lazy)
    float *pid_mem = nullptr;  // PID policies: per-lane integral / previous error, float [2*A][ld] (owned, lazy)
    bool may_hold_done = true; // some lane may carry NIG_CTR_DONE although the handle auto-resets (see HF_MAY_HOLD_DONE)
    char *hst_pinned = nullptr;      // host-buffer entry points: pinned staging + its device mirror (owned, lazy)
    char *hst_dev = nullptr;
    size_t hst_bytes = 0;
    float *mirror = nullptr; uint32_t ld_mirror = 0;    // StepArgs::mirror of the next step launch (nig_step_host*), else NULL
    float *act_soa = nullptr; size_t act_soa_floats = 0;   // nig_rollout with a row-major action ring on a kernel form that reads rows: the [A][ld] copy (owned, lazy)
    LimitTable *lim_dev = nullptr; int n_limits = 0;       // nig_set_limits: the device copy of the added constraints (owned, lazy) and their number
};

// the handle's views of its workspace (nig_layout): per-lane counter words, lifetime violation counts, episode returns, tally rows
static uint32_t *ws_ctr(const nig_handle *h) { return (uint32_t *)(h->ws + h->lay.off_ctr); }
static long long *ws_life_viol(const nig_handle *h) { return (long long *)(h->ws + h->lay.off_life_viol); }
static double *ws_ep_return(const nig_handle *h) { return h->lay.off_ep_return >= 0 ? (double *)(h->ws + h->lay.off_ep_return) : nullptr; }
static double *ws_tally(const nig_handle *h) { return h->lay.off_tally >= 0 ? (double *)(h->ws + h->lay.off_tally) : nullptr; }

struct nig_plan {
    nig_handle *h;
    int n_steps;
    hipGraph_t graph;
    hipGraphExec_t exec;
};

static unsigned grid_for(int64_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

static thread_local char g_err[512] = "";

static int fail(int code, const char *msg) { snprintf(g_err, sizeof g_err, "%s", msg); return code; }      // (msg is text, not a format)
static int fail(int code, const char *fmt, const char *detail) { snprintf(g_err, sizeof g_err, fmt, detail); return code; }
// "<fn>: <what>": the refusal of a check that several entry points share (formatted on refusal only)
static int refuse(const char *fn, const char *what, int code = NIG_ERR_INVALID) { snprintf(g_err, sizeof g_err, "%s: %s", fn, what); return code; }

// While limits are installed (nig_set_limits) every entry point that steps the env but the _limited ones refuses, on the host,
// before anything is launched or written: their kernels do not know the added constraints.
static int refuse_limited(const nig_handle *h, const char *fn);

#define HIP_TRY(expr)                                                        \
    do {                                                                     \
        hipError_t e_ = (expr);                                              \
        if (e_ != hipSuccess) return fail(NIG_ERR_HIP, #expr ": %s", hipGetErrorString(e_)); \
    } while (0)
#define NIG_TRY(expr)                                                        \
    do {                                                                     \
        const int rc_ = (expr);                                              \
        if (rc_ != NIG_OK) return rc_;                                       \
    } while (0)

// The static row of one environment, read off its struct in nig_envs.hpp (dt: the base default, base.py:28).
template <class Env>
constexpr nig_env_spec spec_row()
{
    return {Env::S, Env::A, Env::N_CONSTRAINTS, Env::MAX_STEPS, Env::KS, Env::KR, 0.1,
            {Env::penalty(0), Env::penalty(1), Env::penalty(2)},
            {(int32_t)(Env::CRIT_MASK & 1u), (int32_t)((Env::CRIT_MASK >> 1) & 1u), (int32_t)((Env::CRIT_MASK >> 2) & 1u)}, Env::RET_F32};
}
// the tables indexed by env id, from NIG_ENV_LIST (which checks that position is id)
#define NIG_ENV_SPEC(EnvType, key, id) spec_row<EnvType>(),
#define NIG_ENV_NAME(EnvType, key, id) #EnvType "-v0",
#define NIG_ENV_TABLE(EnvType, key, id) nig_launch_##key(),
static constexpr nig_env_spec SPECS[NIG_NUM_ENVS] = {NIG_ENV_LIST(NIG_ENV_SPEC)};      // (constexpr: every row is evaluated at compile time)
static const char *NAMES[NIG_NUM_ENVS] = {NIG_ENV_LIST(NIG_ENV_NAME)};

// per-environment kernel launchers (env_*.hip)
static const EnvLaunch *launch_of(int env)
{
    static const EnvLaunch *const T[NIG_NUM_ENVS] = {NIG_ENV_LIST(NIG_ENV_TABLE)};
    return T[env];
}
#undef NIG_ENV_SPEC
#undef NIG_ENV_NAME
#undef NIG_ENV_TABLE

// SafetyMetrics.total_constraints of this handle: built-in constraints still enabled (base.py:115,224-228)
static int enabled_constraints(const nig_handle *h);
namespace nig { unsigned split_blocks_for(unsigned cus); unsigned wide_min_blocks_for(unsigned cus); }

namespace nig { static std::atomic<unsigned> g_diag_ring_fault{0u}; }   // NIG_RING_SPIN_LIMIT builds: nig_tune(NIG_TUNE_DIAG_RING_FAULT)

static StepArgs base_step_args(const nig_handle *h)
{
    StepArgs a;
    memset(&a, 0, sizeof a);
    a.state = h->state; a.ld_state = (uint32_t)h->ld_state;
    a.ctr = ws_ctr(h); a.life_viol = ws_life_viol(h); a.ep_ret = ws_ep_return(h); a.tally = ws_tally(h);
    a.ld = (uint32_t)h->lay.ld; a.B = (uint32_t)h->B;
    a.env0 = h->env0; a.seed_lo = (uint32_t)h->seed; a.seed_hi = (uint32_t)(h->seed >> 32);
    a.split_blocks = nig::split_blocks_for(h->cus); a.wide_min_blocks = nig::wide_min_blocks_for(h->cus);
    a.max_steps = h->max_steps; a.dt32 = (float)h->dt; a.dt = h->dt; a.cmask = h->cmask;
    a.hflags = h->flags | (h->may_hold_done ? HF_MAY_HOLD_DONE : 0u);
    a.n_en = enabled_constraints(h);
    a.mirror = h->mirror; a.ld_mirror = h->ld_mirror;      // (set by the host-buffer entry points around their step launch)
#ifdef NIG_RING_SPIN_LIMIT
    a.ring_err = h->t_dev + 16;                    // a spare word of the 256-byte launch-counter slot (zeroed at nig_create)
    if (nig::g_diag_ring_fault.load(std::memory_order_relaxed)) a.hflags |= HF_DIAG_RING_FAULT;
#endif
    return a;
}

// NIG_RING_SPIN_LIMIT builds (test-only, nig_ring.hpp): after a launch of a cooperating-wave kernel, wait for it and turn a
// recorded ring time-out into NIG_ERR_HIP.  The production build returns at once: no hidden synchronisation there.
static int ring_check(nig_handle *h, hipStream_t st, const char *who)
{
#ifdef NIG_RING_SPIN_LIMIT
    uint32_t code = 0;
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(&code, h->t_dev + 16, 4, hipMemcpyDeviceToHost));
    if (code != 0u) {
        HIP_TRY(hipMemset(h->t_dev + 16, 0, 4));
        // the counter index means different rings per kernel family: three-wave kernels (nig_split*.hpp) have
        // {produced inputs, stepped results, released slots}; PowerGrid's paired kernels (nig_pg_lds.hpp) {produced draws, consumed}
        static const char *const ring3[3] = {"inputs (producer -> stepper)", "results (stepper -> recorder)", "slots released (consumer -> producer)"};
        static const char *const ring2[3] = {"draws (producer -> stepper)", "slots released (stepper -> producer)", "(no such counter in the paired form)"};
        const char *const *ring = (h->env == NIG_ENV_POWER_GRID) ? ring2 : ring3;
        char detail[320];
        snprintf(detail, sizeof detail, "%s: a wave waited more than %d polls for count %u of ring counter %u, '%s'; every role left its loop, "
                 "results of this launch are invalid", who, (int)(NIG_RING_SPIN_LIMIT), (code >> 16) & 0x7FFFu, code & 3u, ring[(code & 3u) % 3]);
        return fail(NIG_ERR_HIP, "ring protocol time-out -- %s", detail);
    }
#else
    (void)h; (void)st; (void)who;
#endif
    return NIG_OK;
}

static int enabled_constraints(const nig_handle *h)
{
    return __builtin_popcount(h->cmask & ((1u << SPECS[h->env].n_constraints) - 1u));
}

static int refuse_limited(const nig_handle *h, const char *fn)
{
    if (h && h->n_limits > 0)
        return refuse(fn, "limits are installed (nig_set_limits): this entry point does not know them -- use nig_step_limited / nig_step64_limited / "
                          "nig_rollout_policy_limited / nig_rollout_mlp_limited, or remove them with nig_set_limits(h, 0, ...)", NIG_ERR_UNSUPPORTED);
    return NIG_OK;
}
// the _limited entry points' own prerequisite (a handle of an env that takes no limits never has any installed) ...
static int check_limits(const nig_handle *h, const char *fn)
{
    return h->n_limits <= 0 ? refuse(fn, "no limits installed (nig_set_limits)") : NIG_OK;
}
// ... and the kernel's view of the limits.  n_en counts the added constraints as well: SafetyMetrics.total_constraints of every
// step (base.py:115)
static void limit_args(const nig_handle *h, uint32_t *xflags_out, StepArgs &s, LimitArgs &l)
{
    s.n_en += h->n_limits;
    s.mirror = nullptr;
    l.table = h->lim_dev; l.xflags = xflags_out;
}

static void dispatch_step(const nig_handle *h, const StepArgs &a, bool parity, hipStream_t st)
{
    launch_of(h->env)->step(a, parity, grid_for(h->B), st);
}

namespace nig {
// Kernel-form thresholds (nig_tune).  An explicit setting (environment variable at load, nig_tune later) is
// process-wide and atomic; without one the threshold is a property of the HANDLE's device -- its compute-unit count,
// read at nig_create (256 on an MI355X in SPX mode) -- and travels with the launch arguments, so handles on devices
// with different CU counts (partition modes) or created from several threads never see each other's value
// (it used to be one plain global set from whichever device came first).
constexpr unsigned TUNE_UNSET = 0xffffffffu;
static unsigned tune_from_env(const char *name)
{
    const char *e = getenv(name);
    return e ? (unsigned)strtoul(e, nullptr, 10) : TUNE_UNSET;
}
static std::atomic<unsigned> g_split_override{tune_from_env("NIG_SPLIT_BLOCKS")};      // 256-lane blocks per round of the three-wave form
static std::atomic<unsigned> g_wide_override{tune_from_env("NIG_WIDE_MIN_BLOCKS")};    // smallest batch, in 512-lane blocks, of the wide form
static std::atomic<unsigned> g_last_cus{256u};                                         // CU count of the device of the latest handle (reporting only)
unsigned split_blocks_for(unsigned cus)
{
    const unsigned o = g_split_override.load(std::memory_order_relaxed);
    return o != TUNE_UNSET ? o : cus;
}
unsigned wide_min_blocks_for(unsigned cus)
{
    // default: the wide form (two 512-lane blocks per CU, four waves per SIMD) from the first batch that no longer fits ONE round of
    // the 256-lane form (three blocks per CU): a round of either takes a time proportional to its waves per SIMD (4 : 3), so up to
    // 1.5 wide blocks per CU the 256-lane form's single round wins -- 196 608 lanes x 250 steps, reward + flags: 1.23 ms against
    // 1.54 ms wide; 262 144 lanes (config 3): wide 1.57 ms against 1.67 ms (profiles/r04/pg_forms.txt).  Up to round 3: `cus`.
    const unsigned o = g_wide_override.load(std::memory_order_relaxed);
    return o != TUNE_UNSET ? o : cus + cus / 2 + 1;
}
}

// ---- argument contracts that several entry points share; `fn` names the entry point in the refusal -----------------------------
// Per-step outputs: reward / flags rows of step k lie k * out_stride elements on (0: every step overwrites one row).  Checked in two
// places of an entry point's order of checks: the stride first, the launch counter after the trajectory pitches.
static int check_out_span(const char *fn, int32_t n_steps, int64_t out_stride)
{
    return (int64_t)n_steps * out_stride > 0xffffffffLL ? refuse(fn, "n_steps*out_stride >= 2^32") : NIG_OK;
}
static int check_out_stride(const nig_handle *h, const char *fn, int32_t n_steps, int64_t out_stride)
{
    if (out_stride != 0 && (out_stride < h->B || out_stride > NIG_MAX_PITCH)) return refuse(fn, "out_stride outside {0} U [batch, 2^26]");
    return check_out_span(fn, n_steps, out_stride);
}
static int check_counter(const nig_handle *h, const char *fn, int32_t n_steps)
{
    return (int64_t)h->t + n_steps > 0xffffffffLL ? refuse(fn, "launch counter would wrap") : NIG_OK;
}
static int check_reward_flags(const char *fn, const float *reward_out, const uint32_t *flags_out)
{
    return (reward_out == nullptr) != (flags_out == nullptr) ? refuse(fn, "reward_out and flags_out go together (both or neither)") : NIG_OK;
}

// Closed-loop outputs (nig_rollout_policy / _mlp / _mlp_safe / _mlp_ensemble): the row-major observation trajectory and the action rows
struct ClosedLoopOut {
    float *reward; uint32_t *flags; int64_t out_stride;
    float *obs; int64_t obs_step_stride;
    float *act; int64_t ld_act, act_step_stride;
    uint32_t *xflags;           // a _limited twin's xflags_out (a parent leaves it out: NULL)
};
// what every closed-loop entry point passes on, in the struct's order (a twin: {CLOSED_LOOP_OUT, xflags_out})
#define CLOSED_LOOP_OUT reward_out, flags_out, out_stride, obs_out, obs_step_stride, act_out, ld_act, act_step_stride
// A row-major [n_steps][B][S] trajectory (obs_out, seen_out): 16-byte aligned, rows of step k at k * step_stride >= S * batch floats,
// a multiple of 4 (there is no "overwrite" form)
static int check_state_rows(const nig_handle *h, const char *fn, const float *rows, int64_t step_stride, const char *refusal)
{
    if (rows && (step_stride < (int64_t)SPECS[h->env].state_dim * h->B || (step_stride & 3) || ((uintptr_t)rows & 15))) return refuse(fn, refusal);
    return NIG_OK;
}
static int check_closed_loop(const nig_handle *h, const char *fn, const ClosedLoopOut &o)
{
    NIG_TRY(check_state_rows(h, fn, o.obs, o.obs_step_stride, "obs_out needs 16-byte alignment and obs_step_stride >= S*batch (multiple of 4)"));
    if (o.act && (o.ld_act < h->B || o.ld_act > NIG_MAX_PITCH || o.act_step_stride < (int64_t)SPECS[h->env].action_dim * o.ld_act))
        return refuse(fn, "bad action trajectory pitch");
    return NIG_OK;
}

// The checks of both contracts, then the fields PolicyArgs and MlpArgs share (everything else of q stays as it is: zero).
template <class Args>
static int closed_loop_args(const nig_handle *h, const char *fn, int32_t n_steps, const ClosedLoopOut &o, Args &q)
{
    NIG_TRY(check_out_stride(h, fn, n_steps, o.out_stride));
    NIG_TRY(check_closed_loop(h, fn, o));
    NIG_TRY(check_counter(h, fn, n_steps));
    q.s = base_step_args(h);
    q.s.reward = o.reward; q.s.flags = o.flags; q.s.t_off = h->t;
    q.n_steps = n_steps; q.out_stride = (uint32_t)o.out_stride;
    q.obs_out = o.obs; q.obs_step_stride = (uint64_t)o.obs_step_stride;
    q.act_out = o.act; q.ld_act_out = (uint32_t)o.ld_act; q.act_step_stride = (uint64_t)o.act_step_stride;
    return NIG_OK;
}

// nig_set_disturbance ("nig-disturb-v1"): finite sigmas >= 0 on the env's dimensions, ordered clip bounds (NaN refused), a known hold
static int check_disturbance(const nig_handle *h, const char *fn, const nig_disturbance &d)
{
    for (int k = 0; k < SPECS[h->env].state_dim; ++k)
        if (!(d.sigma_obs[k] >= 0.0f) || !std::isfinite(d.sigma_obs[k])) return refuse(fn, "sigma_obs must be finite and >= 0");
    for (int j = 0; j < SPECS[h->env].action_dim; ++j)
        if (!(d.sigma_act[j] >= 0.0f) || !std::isfinite(d.sigma_act[j])) return refuse(fn, "sigma_act must be finite and >= 0");
    if (!(d.clip_lo <= d.clip_hi)) return refuse(fn, "clip_lo > clip_hi (or a NaN bound)");
    if (d.hold != NIG_HOLD_STEP && d.hold != NIG_HOLD_EPISODE) return refuse(fn, "unknown hold (NIG_HOLD_STEP / NIG_HOLD_EPISODE)");
    return NIG_OK;
}

// The _disturbed rollouts: an installed disturbance and seen_out's pitches (before the twin's own checks); then the kernel's copy.
static int disturb_args(const nig_handle *h, const char *fn, float *seen_out, int64_t seen_step_stride, DisturbArgs &d)
{
    if (!h->has_dist) return refuse(fn, "no disturbance installed (nig_set_disturbance)");
    NIG_TRY(check_state_rows(h, fn, seen_out, seen_step_stride, "seen_out needs 16-byte alignment and seen_step_stride >= S*batch (multiple of 4)"));
    memset(&d, 0, sizeof d);
    static_assert(sizeof d.sigma_obs == sizeof h->dist.sigma_obs && sizeof d.sigma_act == sizeof h->dist.sigma_act);
    memcpy(d.sigma_obs, h->dist.sigma_obs, sizeof d.sigma_obs);
    memcpy(d.sigma_act, h->dist.sigma_act, sizeof d.sigma_act);
    d.clip_lo = h->dist.clip_lo; d.clip_hi = h->dist.clip_hi; d.hold = h->dist.hold;
    d.seen_out = seen_out; d.seen_step_stride = (uint64_t)seen_step_stride;
    return NIG_OK;
}

// ---- the closed loop: what nig_rollout_policy / _mlp / _mlp_bf16 / _mlp_safe / _mlp_search / _mlp_gated / _mlp_projected / _mlp_ensemble /
// _policy_disturbed / _mlp_disturbed and their _limited twins do after their own prerequisites.  A variant's argument block holds the
// shared fields as PolicyArgs or MlpArgs, which also says what grid its kernels take: a thread per env for the policy kernels, 32 envs
// per wave (128 per block) for the MFMA kernels.
static PolicyArgs &shared_args(PolicyArgs &q) { return q; }
static PolicyArgs &shared_args(PolicyDistArgs &q) { return q.p; }
static MlpArgs &shared_args(MlpArgs &q) { return q; }
static PolicyArgs &shared_args(PolicyLimArgs &q) { return q.p; }
static MlpArgs &shared_args(MlpSearchArgs &q) { return q.sh.m; }
static MlpArgs &shared_args(MlpCatShieldArgs &q) { return q.sh.m; }
static MlpArgs &shared_args(MlpCatSearchArgs &q) { return q.sr.sh.m; }
static MlpArgs &shared_args(MlpLnShieldArgs &q) { return q.a.m; }
template <class Shape> static MlpArgs &shared_args(MlpShapeShieldArgs<Shape> &q) { return q.a.m; }
template <class Args> static MlpArgs &shared_args(Args &q) { return q.m; }      // MlpShieldArgs, MlpEnsArgs, MlpDistArgs, MlpGateArgs, MlpProjectArgs, MlpBf16Args, MlpLimArgs
static PolicyArgs &shared_args(PolicyDistLimArgs &q) { return q.p; }
template <class Parent> static MlpArgs &shared_args(MlpLimited<Parent> &q) { return shared_args(q.a); }      // a _limited twin: its parent's
static unsigned closed_loop_grid(const nig_handle *h, const PolicyArgs &) { return grid_for(h->B); }
static unsigned closed_loop_grid(const nig_handle *h, const MlpArgs &) { return (unsigned)((h->B + BLOCK / 2 - 1) / (BLOCK / 2)); }

// A family is stated once, as a function template on LIM: false is the parent entry point, true its _limited twin.  The twin's
// argument block is the parent's beside a LimitArgs `l`; these say which type that is, where the parent's own fields lie in it, and
// which of the family's two EnvLaunch slots a call takes.
template <class Parent> struct limited_twin { using type = MlpLimited<Parent>; };
template <> struct limited_twin<PolicyArgs> { using type = PolicyLimArgs; };
template <> struct limited_twin<PolicyDistArgs> { using type = PolicyDistLimArgs; };
template <> struct limited_twin<MlpArgs> { using type = MlpLimArgs; };
template <class Args> static Args &parent_args(Args &q) { return q; }           // a parent; PolicyDistLimArgs, which restates its parent's members
static PolicyArgs &parent_args(PolicyLimArgs &q) { return q.p; }
static MlpArgs &parent_args(MlpLimArgs &q) { return q.m; }
template <class Parent> static Parent &parent_args(MlpLimited<Parent> &q) { return q.a; }
template <bool LIM, class P, class T>
static auto slot_of(P parent, T twin)
{
    if constexpr (LIM) return twin;
    else return parent;
}

// The zeroed block (the parent's, or with LIM its twin's), the argument checks and the shared fields; `fill` writes the family's
// own fields into the parent's part of the block, a twin gets the limits beside them (o.xflags: its xflags_out); then the launch
// through `launch` (an EnvLaunch entry, or a callable of its shape), its error and the launch counter.  No synchronisation.
template <bool LIM, class Parent, class Launch, class Fill>
static int closed_loop(nig_handle *h, const char *fn, int32_t n_steps, const ClosedLoopOut &o, void *stream, Launch launch, Fill &&fill)
{
    std::conditional_t<LIM, typename limited_twin<Parent>::type, Parent> q;
    memset(&q, 0, sizeof q);
    auto &shared = shared_args(q);
    NIG_TRY(closed_loop_args(h, fn, n_steps, o, shared));
    fill(parent_args(q));
    if constexpr (LIM) limit_args(h, o.xflags, shared.s, q.l);
    launch(q, closed_loop_grid(h, shared), (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    h->t += (uint32_t)n_steps;
    return NIG_OK;
}

// The refusals several families share.  A parent refuses installed limits and a twin needs them: the later families ask at one
// place, right after the bad-argument check (the early pairs -- the step pair, nig_rollout_policy, nig_rollout_mlp -- ask the parent's
// question before their prerequisites and the twin's after them).
template <bool LIM>
static int limits_gate(const nig_handle *h, const char *fn) { return LIM ? check_limits(h, fn) : refuse_limited(h, fn); }
static int need_mfma_actor(const nig_handle *h, const char *fn)
{
    return launch_of(h->env)->mlp ? NIG_OK : refuse(fn, "env shape has no MFMA actor", NIG_ERR_UNSUPPORTED);
}
// a kind of the actor slot beside the shape classes: the LayerNorm actor.  It follows the shaped actor's rule everywhere.
constexpr int ACTOR_KIND_LN = SHAPE_KIND_3 + 1;
static bool shaped_actor(const nig_handle *h) { return h->actor_kind > SHAPE_KIND_REFERENCE; }
// the families that run the 256 x 256 actor only ask this right after their bad-argument check ("nig-mlp-shape-v1")
static int refuse_shaped(const nig_handle *h, const char *fn)
{
    if (h->actor_kind == ACTOR_KIND_LN)
        return refuse(fn, "a LayerNorm actor is installed (nig_set_mlp_policy_ln): this entry point runs the plain 256 x 256 actor only", NIG_ERR_UNSUPPORTED);
    return shaped_actor(h) ? refuse(fn, "a shaped actor is installed (nig_set_mlp_policy_dims): this entry point runs the 256 x 256 actor only", NIG_ERR_UNSUPPORTED) : NIG_OK;
}
static int need_actor(const nig_handle *h, const char *fn)       // (an env without the MFMA actor never has one: nig_set_mlp_policy refuses)
{
    NIG_TRY(refuse_shaped(h, fn));
    return h->actor_kind == SHAPE_KIND_REFERENCE ? NIG_OK : refuse(fn, "no actor installed (nig_set_mlp_policy)");
}
static int need_policy(const nig_handle *h, const char *fn) { return h->has_policy ? NIG_OK : refuse(fn, "no policy installed (nig_set_policy)"); }
static bool ln_critic(const nig_handle *h) { return h->mlp_ckind == NIG_SAFETY_SIGMOID_LN; }
static bool shaped_critic(const nig_handle *h) { return h->mlp_ckind == NIG_SAFETY_SIGMOID_SHAPED; }
static int need_critic(const nig_handle *h, const char *fn)
{
    const float *image = ln_critic(h) ? h->mlp_cln_stream : shaped_critic(h) ? h->mlp_cshape_stream : h->mlp_cstream;
    return image && h->mlp_ckind != NIG_SAFETY_NONE ? NIG_OK : refuse(fn, "no safety critic installed (nig_set_mlp_safety)");
}
// the readers of the critic slot that run the plain critics only ask this right after refuse_shaped ("nig-mlp-ln-shield-v1")
static int refuse_ln_critic(const nig_handle *h, const char *fn)
{
    return ln_critic(h) ? refuse(fn, "a LayerNorm critic is installed (nig_set_mlp_safety_ln): this entry point runs it beside a LayerNorm actor in nig_rollout_mlp_safe only", NIG_ERR_UNSUPPORTED) : NIG_OK;
}
// and this right after refuse_ln_critic ("nig-mlp-shape-shield-v1"): the same rule for the shaped critic
static int refuse_shaped_critic(const nig_handle *h, const char *fn)
{
    return shaped_critic(h) ? refuse(fn, "a shaped critic is installed (nig_set_mlp_safety_dims): this entry point runs it beside a shaped actor of the same class in nig_rollout_mlp_safe only", NIG_ERR_UNSUPPORTED) : NIG_OK;
}
// the per-constraint rows of the gate and the projection: [n_outputs][ld_c] blocks, c_step_stride apart
static int check_constraint_rows(const nig_handle *h, const char *fn, int n_outputs, int64_t ld_c, int64_t c_step_stride)
{
    if (ld_c < h->B || ld_c > NIG_MAX_PITCH) return refuse(fn, "ld_c outside [batch, 2^26]");
    if (c_step_stride < (int64_t)n_outputs * ld_c) return refuse(fn, "c_step_stride smaller than one [n_outputs][ld_c] block");
    return NIG_OK;
}

static void policy_fields(const nig_handle *h, PolicyArgs &q)
{
    q.pol = h->pol_dev;
    q.pid = (h->pol_host.kind == NIG_POLICY_PID) ? h->pid_mem : nullptr;
    q.pol_kind = h->pol_host.kind;
}
static void shield_fields(const nig_handle *h, float *prob_out, MlpShieldArgs &q)
{
    q.m.wstream = h->mlp_stream;
    q.cstream = h->mlp_cstream; q.prob_out = prob_out; q.threshold = h->mlp_threshold;
}
// the categorical critic's part of an argument block ("nig-categorical-v1"); the launchers below choose the kernel by the slot's kind
static bool categorical(const nig_handle *h) { return h->mlp_ckind == NIG_SAFETY_CATEGORICAL; }
static void categorical_fields(const nig_handle *h, MlpCatArgs &c)
{
    c.tail = h->mlp_ctail; c.below_mask = h->cat_mask; c.atoms = h->cat_atoms;
}

// ---- the families with a twin, in the order of their entry points below ---------------------------------------------------
// Order of refusals: bad argument; the question about limits (code 4 from a parent, "no limits installed", NIG_ERR_INVALID, from a
// twin); the family's own refusals; closed_loop's argument contracts.  The Advanced pair never has limits installed, so its twins
// refuse at the second step.  The entry points pass their own name, and a twin its xflags_out in the ClosedLoopOut.
template <bool LIM>
static int rollout_policy(nig_handle *h, const char *fn, int32_t n_steps, const ClosedLoopOut &o, void *stream)
{
    if (!h || n_steps <= 0) return refuse(fn, "bad argument");
    if (!LIM) NIG_TRY(refuse_limited(h, fn));
    NIG_TRY(need_policy(h, fn));
    if (LIM) NIG_TRY(check_limits(h, fn));
    const EnvLaunch *L = launch_of(h->env);
    NIG_TRY((closed_loop<LIM, PolicyArgs>(h, fn, n_steps, o, stream, slot_of<LIM>(L->policy, L->policy_limited),
                                          [&](PolicyArgs &q) { policy_fields(h, q); })));
    return LIM ? NIG_OK : ring_check(h, (hipStream_t)stream, fn);      // (the one closed loop with cooperating-wave forms)
}

// nig_rollout_mlp with a shaped actor in the slot: the class's kernel on the shaped image ("nig-mlp-shape-v1"), or the LayerNorm
// actor's on its own ("nig-mlp-ln-v1")
static int rollout_mlp_shaped(nig_handle *h, const char *fn, int32_t n_steps, const ClosedLoopOut &o, void *stream)
{
    const EnvLaunch *L = launch_of(h->env);
    auto run = [&](auto launch, auto shape) {
        using Args = MlpShapeArgs<decltype(shape)>;
        return closed_loop<false, Args>(h, fn, n_steps, o, stream, launch, [&](Args &q) { q.m.wstream = h->mlp_shape_stream; });
    };
    switch (h->actor_kind) {
    case ACTOR_KIND_LN:
        return closed_loop<false, MlpLnArgs>(h, fn, n_steps, o, stream, L->mlp_ln, [&](MlpLnArgs &q) { q.m.wstream = h->mlp_ln_stream; q.eps = h->ln_eps; });
    case SHAPE_KIND_128: return run(L->mlp_shape128, Shape128{});
    case SHAPE_KIND_512x256: return run(L->mlp_shape512x256, Shape512x256{});
    case SHAPE_KIND_512: return run(L->mlp_shape512, Shape512{});
    case SHAPE_KIND_3: return run(L->mlp_shape3, Shape3{});
    default: return refuse(fn, "no actor installed (nig_set_mlp_policy)");
    }
}

template <bool LIM>
static int rollout_mlp(nig_handle *h, const char *fn, int32_t n_steps, const ClosedLoopOut &o, void *stream)
{
    if (!h || n_steps <= 0) return refuse(fn, "bad argument");
    if (!LIM) NIG_TRY(refuse_limited(h, fn));
    if (!LIM && shaped_actor(h)) return rollout_mlp_shaped(h, fn, n_steps, o, stream);
    NIG_TRY(need_actor(h, fn));
    if (LIM) NIG_TRY(check_limits(h, fn));
    const EnvLaunch *L = launch_of(h->env);
    return closed_loop<LIM, MlpArgs>(h, fn, n_steps, o, stream, slot_of<LIM>(L->mlp, L->mlp_limited),
                                     [&](MlpArgs &q) { q.wstream = h->mlp_stream; });
}

// nig_rollout_mlp_safe with a LayerNorm actor and a LayerNorm critic (or none) in the slots: "nig-mlp-ln-shield-v1"
static int rollout_mlp_safe_ln(nig_handle *h, const char *fn, int32_t n_steps, const ClosedLoopOut &o, float *prob_out, void *stream)
{
    NIG_TRY(refuse_limited(h, fn));
    NIG_TRY(need_mfma_actor(h, fn));
    NIG_TRY(need_critic(h, fn));
    return closed_loop<false, MlpLnShieldArgs>(h, fn, n_steps, o, stream, launch_of(h->env)->mlp_ln_shield, [&](MlpLnShieldArgs &q) {
        q.a.m.wstream = h->mlp_ln_stream; q.a.eps = h->ln_eps;
        q.cstream = h->mlp_cln_stream; q.ceps = h->cln_eps; q.prob_out = prob_out; q.threshold = h->mlp_threshold;
    });
}

// nig_rollout_mlp_safe with a shaped actor and a shaped critic of the same class in the slots: "nig-mlp-shape-shield-v1"
static int rollout_mlp_safe_shaped(nig_handle *h, const char *fn, int32_t n_steps, const ClosedLoopOut &o, float *prob_out, void *stream)
{
    NIG_TRY(refuse_limited(h, fn));
    NIG_TRY(need_mfma_actor(h, fn));
    NIG_TRY(need_critic(h, fn));
    const EnvLaunch *L = launch_of(h->env);
    auto run = [&](auto launch, auto shape) {
        using Args = MlpShapeShieldArgs<decltype(shape)>;
        return closed_loop<false, Args>(h, fn, n_steps, o, stream, launch, [&](Args &q) {
            q.a.m.wstream = h->mlp_shape_stream;
            q.cstream = h->mlp_cshape_stream; q.prob_out = prob_out; q.threshold = h->mlp_threshold;
        });
    };
    switch (h->actor_kind) {
    case SHAPE_KIND_128: return run(L->mlp_shape128_shield, Shape128{});
    case SHAPE_KIND_512x256: return run(L->mlp_shape512x256_shield, Shape512x256{});
    case SHAPE_KIND_512: return run(L->mlp_shape512_shield, Shape512{});
    case SHAPE_KIND_3: return run(L->mlp_shape3_shield, Shape3{});
    default: return refuse(fn, "no actor installed (nig_set_mlp_policy)");
    }
}

template <bool LIM>
static int rollout_mlp_safe(nig_handle *h, const char *fn, int32_t n_steps, const ClosedLoopOut &o, float *prob_out, void *stream)
{
    if (!h || n_steps <= 0) return refuse(fn, "bad argument");
    // (a LayerNorm actor beside any other critic keeps the shaped actor's refusal, below)
    if (!LIM && h->actor_kind == ACTOR_KIND_LN && (ln_critic(h) || h->mlp_ckind == NIG_SAFETY_NONE))
        return rollout_mlp_safe_ln(h, fn, n_steps, o, prob_out, stream);
    // (a shaped critic beside any actor but a shaped one of its own class is refused by name; a shaped actor beside any other critic
    // keeps its refusal, below)
    if (!LIM && shaped_critic(h) && h->actor_kind == h->critic_class)
        return rollout_mlp_safe_shaped(h, fn, n_steps, o, prob_out, stream);
    NIG_TRY(refuse_shaped_critic(h, fn));
    NIG_TRY(refuse_shaped(h, fn));
    NIG_TRY(refuse_ln_critic(h, fn));
    NIG_TRY(limits_gate<LIM>(h, fn));
    NIG_TRY(need_mfma_actor(h, fn));
    NIG_TRY(need_actor(h, fn));
    NIG_TRY(need_critic(h, fn));
    const EnvLaunch *L = launch_of(h->env);
    if (categorical(h))
        return closed_loop<LIM, MlpCatShieldArgs>(h, fn, n_steps, o, stream, slot_of<LIM>(L->mlp_cat_shield, L->mlp_cat_shield_limited),
                                                  [&](MlpCatShieldArgs &q) { shield_fields(h, prob_out, q.sh); categorical_fields(h, q.c); });
    return closed_loop<LIM, MlpShieldArgs>(h, fn, n_steps, o, stream, slot_of<LIM>(L->mlp_shield, L->mlp_shield_limited),
                                           [&](MlpShieldArgs &q) { shield_fields(h, prob_out, q); });
}

template <bool LIM>
static int rollout_mlp_search(nig_handle *h, const char *fn, int32_t n_steps, int32_t n_candidates, const ClosedLoopOut &o, float *prob_out,
                              float *risk_out, int32_t *choice_out, void *stream)
{
    if (!h || n_steps <= 0) return refuse(fn, "bad argument");
    NIG_TRY(refuse_shaped(h, fn));
    NIG_TRY(refuse_ln_critic(h, fn));
    NIG_TRY(refuse_shaped_critic(h, fn));
    NIG_TRY(limits_gate<LIM>(h, fn));
    NIG_TRY(need_mfma_actor(h, fn));
    if (n_candidates < 1 || n_candidates > NIG_MAX_CANDIDATES) return refuse(fn, "n_candidates outside 1 .. NIG_MAX_CANDIDATES");
    NIG_TRY(need_actor(h, fn));
    NIG_TRY(need_critic(h, fn));
    const EnvLaunch *L = launch_of(h->env);
    if (categorical(h))
        return closed_loop<LIM, MlpCatSearchArgs>(h, fn, n_steps, o, stream, slot_of<LIM>(L->mlp_cat_search, L->mlp_cat_search_limited), [&](MlpCatSearchArgs &q) {
            shield_fields(h, prob_out, q.sr.sh); categorical_fields(h, q.c);
            q.sr.n_candidates = n_candidates; q.sr.risk_out = risk_out; q.sr.choice_out = choice_out;
        });
    return closed_loop<LIM, MlpSearchArgs>(h, fn, n_steps, o, stream, slot_of<LIM>(L->mlp_search, L->mlp_search_limited), [&](MlpSearchArgs &q) {
        shield_fields(h, prob_out, q.sh);
        q.n_candidates = n_candidates; q.risk_out = risk_out; q.choice_out = choice_out;
    });
}

template <bool LIM>
static int rollout_mlp_ensemble(nig_handle *h, const char *fn, int32_t n_steps, ClosedLoopOut o, float *unc_out, float *member_act_out, void *stream)
{
    if (!h || n_steps <= 0) return refuse(fn, "bad argument (handle, n_steps)");
    NIG_TRY(limits_gate<LIM>(h, fn));
    NIG_TRY(need_mfma_actor(h, fn));
    if (h->ens_members < 1 || !h->ens_stream) return refuse(fn, "no ensemble installed (nig_set_mlp_ensemble)");
    float *const act_out = o.act;
    if (!o.act) o.act = member_act_out;           // member_act_out shares act_out's pitches: the same checks apply to it when act_out is absent
    const int ens = h->ens_method == NIG_ENSEMBLE_AVERAGE ? ENS_AVERAGE : ENS_VOTING;      // one kernel per combination rule
    const auto launch = [&](const auto &e, unsigned grid, hipStream_t st) {
        const EnvLaunch *L = launch_of(h->env);
        slot_of<LIM>(L->mlp_ensemble, L->mlp_ensemble_limited)(ens, e, grid, st);
    };
    return closed_loop<LIM, MlpEnsArgs>(h, fn, n_steps, o, stream, launch, [&](MlpEnsArgs &q) {
        q.m.act_out = act_out;
        q.m.wstream = h->ens_stream;
        q.n_members = h->ens_members; q.w = h->ens_w; q.wsum = h->ens_wsum; q.kf = (float)h->ens_members; q.threshold = h->ens_threshold;
        q.unc_out = unc_out; q.member_out = member_act_out;
    });
}

template <bool LIM>
static int rollout_mlp_gated(nig_handle *h, const char *fn, int32_t n_steps, const ClosedLoopOut &o, float *prob_out, float *unc_out,
                             float *logit_out, int64_t ld_c, int64_t c_step_stride, void *stream)
{
    if (!h || n_steps <= 0) return refuse(fn, "bad argument");
    NIG_TRY(refuse_shaped(h, fn));
    NIG_TRY(limits_gate<LIM>(h, fn));
    NIG_TRY(need_mfma_actor(h, fn));
    NIG_TRY(need_actor(h, fn));
    if (h->gate_members < 1 || !h->gate_stream) return refuse(fn, "no safety ensemble installed (nig_set_mlp_safety_ensemble)");
    if (prob_out || unc_out || logit_out) NIG_TRY(check_constraint_rows(h, fn, h->gate_outputs, ld_c, c_step_stride));
    const EnvLaunch *L = launch_of(h->env);
    return closed_loop<LIM, MlpGateArgs>(h, fn, n_steps, o, stream, slot_of<LIM>(L->mlp_gated, L->mlp_gated_limited), [&](MlpGateArgs &q) {
        q.m.wstream = h->mlp_stream;
        q.cstreams = h->gate_stream; q.n_members = h->gate_members; q.n_outputs = h->gate_outputs; q.kf = (float)h->gate_members;
        q.temperature = h->gate_T; q.threshold = h->gate_thr; q.umax = h->gate_umax;
        q.prob_out = prob_out; q.unc_out = unc_out; q.logit_out = logit_out;
        q.ld_c = (uint32_t)ld_c; q.c_step_stride = (uint64_t)c_step_stride;
    });
}

template <bool LIM>
static int rollout_mlp_projected(nig_handle *h, const char *fn, int32_t n_steps, int32_t max_iters, float step, const ClosedLoopOut &o,
                                 float *prob_out, float *viol_out, int32_t *iters_out, float *grad_out, int64_t ld_c, int64_t c_step_stride,
                                 void *stream)
{
    if (!h || n_steps <= 0) return refuse(fn, "bad argument");
    NIG_TRY(refuse_shaped(h, fn));
    NIG_TRY(limits_gate<LIM>(h, fn));
    NIG_TRY(need_mfma_actor(h, fn));
    NIG_TRY(need_actor(h, fn));
    if (h->proj_outputs < 1 || !h->proj_cstream || !h->proj_bstream) return refuse(fn, "no constraint predictor installed (nig_set_mlp_constraint)");
    if (max_iters < 1 || max_iters > NIG_MAX_PROJECT_ITERS) return refuse(fn, "max_iters outside 1 .. NIG_MAX_PROJECT_ITERS");
    if (!std::isfinite(step)) return refuse(fn, "step must be finite");
    if (prob_out || viol_out) NIG_TRY(check_constraint_rows(h, fn, h->proj_outputs, ld_c, c_step_stride));
    if (grad_out && (o.ld_act < h->B || o.ld_act > NIG_MAX_PITCH || o.act_step_stride < (int64_t)SPECS[h->env].action_dim * o.ld_act))
        return refuse(fn, "bad action trajectory pitch (grad_out takes act_out's)");
    const EnvLaunch *L = launch_of(h->env);
    return closed_loop<LIM, MlpProjectArgs>(h, fn, n_steps, o, stream, slot_of<LIM>(L->mlp_projected, L->mlp_projected_limited), [&](MlpProjectArgs &q) {
        q.m.wstream = h->mlp_stream;
        q.cstream = h->proj_cstream; q.bstream = h->proj_bstream; q.n_outputs = h->proj_outputs; q.max_iters = max_iters;
        q.threshold = h->proj_thr; q.tolerance = h->proj_tol; q.step = step;
        q.prob_out = prob_out; q.viol_out = viol_out; q.iters_out = iters_out; q.grad_out = grad_out;
        q.ld_c = (uint32_t)ld_c; q.c_step_stride = (uint64_t)c_step_stride;
    });
}

template <bool LIM>
static int rollout_policy_disturbed(nig_handle *h, const char *fn, int32_t n_steps, const ClosedLoopOut &o, float *seen_out,
                                    int64_t seen_step_stride, void *stream)
{
    if (!h || n_steps <= 0) return refuse(fn, "bad argument");
    NIG_TRY(limits_gate<LIM>(h, fn));
    NIG_TRY(need_policy(h, fn));
    DisturbArgs d;
    NIG_TRY(disturb_args(h, fn, seen_out, seen_step_stride, d));
    const EnvLaunch *L = launch_of(h->env);
    return closed_loop<LIM, PolicyDistArgs>(h, fn, n_steps, o, stream, slot_of<LIM>(L->policy_disturbed, L->policy_disturbed_limited), [&](auto &q) {
        q.d = d;
        policy_fields(h, q.p);
    });
}

template <bool LIM>
static int rollout_mlp_disturbed(nig_handle *h, const char *fn, int32_t n_steps, const ClosedLoopOut &o, float *seen_out,
                                 int64_t seen_step_stride, void *stream)
{
    if (!h || n_steps <= 0) return refuse(fn, "bad argument");
    NIG_TRY(refuse_shaped(h, fn));
    NIG_TRY(limits_gate<LIM>(h, fn));
    NIG_TRY(need_mfma_actor(h, fn));
    NIG_TRY(need_actor(h, fn));
    DisturbArgs d;
    NIG_TRY(disturb_args(h, fn, seen_out, seen_step_stride, d));
    const EnvLaunch *L = launch_of(h->env);
    return closed_loop<LIM, MlpDistArgs>(h, fn, n_steps, o, stream, slot_of<LIM>(L->mlp_disturbed, L->mlp_disturbed_limited), [&](MlpDistArgs &q) {
        q.d = d;
        q.m.wstream = h->mlp_stream;
    });
}

extern "C" {

// 0.2.0: the fast-mode generator became "nig-philox-v2" (Philox4x32-7, float32 reset draws for ChemicalReactor / PowerGrid, round 3):
// every (seed, lane, t) trajectory differs from 0.1.0's "nig-philox-v1" -- stored seeds / datasets are tied to the generator id.
// 0.3.0, "nig-philox-v3" (round 4): as v2, except that PowerGrid's eight RESET load factors are 16-bit uniforms taken from the
// low bytes of the reset normals' words (six Philox blocks per reset instead of eight): PowerGrid trajectories differ from v2's
// from the first auto-reset on; ChemicalReactor, RobotAssembly and every other env are bit-identical to v2.
// 0.4.0 (round 4): generator unchanged for the reference's envs; the four build-specified plants moved to their model "v2"
// (spec_plants.py: fused multiply-adds, steps 2k-1 / 2k sharing one generator block) -- their trajectories differ from 0.3.0's.
// 0.5.0 (round 5): generator unchanged -- every fast-mode trajectory of 0.4.0 replays bit for bit (the generator's piece index and
// PowerGrid's clips / economic sum are computed with fewer instructions, same values).  Changed results: nig_rollout_mlp for envs
// with at most four actions (ChemicalReactor, WaterTreatment) sums the head in the order of its v_mfma_f32_4x4x1 form (last-bit
// differences in the action against 0.4.0; the oracle restates the new order).  New entry point: nig_clock_stamp.  A caller
// workspace is refused only when positively identified as host / managed / foreign-device memory.
// 0.6.0: nig_set_mlp_safety / nig_rollout_mlp_safe (the MFMA actor with the safety-critic shield) and NIG_FLAG_SHIELDED.  No
// existing entry point's results changed.
// 0.7.0: det_tanhf takes Cephes' odd polynomial below |x| = 0.625 (the quotient form lost all relative accuracy towards 0):
// the actions of nig_rollout_mlp / nig_rollout_mlp_safe and AdvancedChemicalReactor's step (the mixing term, rpm < 625)
// change wherever a tanh argument lies below the cut-off.  fdiv_c by a divisor below one returns IEEE's inf where the
// quotient overflows (most likely NaN before, not measured on the device; AdvancedChemicalReactor / AdvancedPowerGrid only),
// det_sinf's quadrant is defined for every float (results change only from |x| ~ 6.59e6 on, where |fk| >= 2^22, outside its
// stated domain |x| <= 1e4).  Generator and every other env unchanged.
// 0.8.0: nig_rollout_sampled (the fused rollout draws its uniform actions in the kernel).  Additive: generator and every existing
// entry point's results unchanged.
// Still 0.8.0: nig_set_mlp_ensemble / nig_rollout_mlp_ensemble (K MFMA actors per step, EnsembleAgent's action and uncertainty) and
// NIG_FLAG_UNCERTAIN.  Additive: generator and every existing entry point's results unchanged.  The number did not move because
// tests/test_rollout_sampled_host.py pins the string; a caller tells the two apart by the exported symbol.
// Still 0.8.0, for the same reason (a minor bump is due with the next change that may touch that test): nig_set_disturbance /
// nig_rollout_policy_disturbed / nig_rollout_mlp_disturbed ("nig-disturb-v1": sensor / actuator noise inside the closed loop; blocks
// +32.. and +48.. of the generator's policy stream).  Additive: generator and every existing entry point's results unchanged.
// Still 0.8.0, for the same reason: nig_episode_log_query / _init, nig_collect_episodes, nig_reduce_episodes (per-episode records from the
// reward / flag rows; csrc/nig_episodes.hpp).  Additive: no existing kernel or entry point changed.
// Still 0.8.0, for the same reason: nig_rollout_mlp_search ("nig-search-v1": the safety-critical agents' get_safe_action -- the critic
// scores n_candidates uniform actions where the actor's is too risky; blocks +0x100.. of the generator's policy stream).  Additive:
// no new state on the handle, no existing kernel or entry point changed.
// Still 0.8.0, for the same reason: nig_set_mlp_safety_ensemble / nig_rollout_mlp_gated ("nig-gate-v1": SafeEnsembleAgent's
// get_safe_action -- K safety predictors of up to four head rows vote on the actor's action).  Additive: no existing kernel or entry
// point changed.
// Still 0.8.0, for the same reason: nig_set_mlp_constraint / nig_rollout_mlp_projected ("nig-project-v1": ConstrainedIQLAgent's
// get_safe_action -- a gradient projection of the actor's action towards the constraint predictor's feasible set).  Additive: no
// existing kernel or entry point changed, no draw added.
// Still 0.8.0, for the same reason: nig_set_mlp_safety_categorical / nig_get_mlp_safety_kind / nig_mlp_violation_prob
// ("nig-categorical-v1": RiskAwareCQLAgent's distributional critic -- a softmax head of up to 64 atoms in the shield's and the search's
// critic slot, and its violation probability over a caller's batch).  Additive: no existing kernel changed, no draw added.
// Still 0.8.0, for the same reason: nig_set_limits / nig_get_limit_count / nig_step_limited / nig_step64_limited /
// nig_rollout_policy_limited / nig_rollout_mlp_limited ("nig-limits-v1": box constraints added by the user, on the device).  Additive:
// no existing kernel changed, no draw added; while limits are installed the other stepping entry points return NIG_ERR_UNSUPPORTED.
const char *nig_version(void) { return "nig 0.8.0 (gfx950; generator nig-philox-v3)"; }
const char *nig_last_error(void) { return g_err; }

int nig_tune(int32_t key, int64_t value)
{
    if (key == NIG_TUNE_DIAG_RING_FAULT) {
#ifdef NIG_RING_SPIN_LIMIT
        nig::g_diag_ring_fault.store(value != 0 ? 1u : 0u, std::memory_order_relaxed);
        return NIG_OK;
#else
        return fail(NIG_ERR_UNSUPPORTED, "nig_tune: NIG_TUNE_DIAG_RING_FAULT exists in NIG_RING_SPIN_LIMIT test builds only");
#endif
    }
    if ((key != NIG_TUNE_SPLIT_BLOCKS && key != NIG_TUNE_WIDE_MIN_BLOCKS) || value < -1 || value >= (int64_t)nig::TUNE_UNSET)
        return fail(NIG_ERR_INVALID, "nig_tune: unknown key or value out of range");
    // -1 = back to "no explicit setting": every handle uses its own device's default again
    (key == NIG_TUNE_WIDE_MIN_BLOCKS ? nig::g_wide_override : nig::g_split_override).store(value < 0 ? nig::TUNE_UNSET : (unsigned)value, std::memory_order_relaxed);
    return NIG_OK;
}
int64_t nig_tune_get(int32_t key)
{
    const unsigned cus = nig::g_last_cus.load(std::memory_order_relaxed);
    return key == NIG_TUNE_SPLIT_BLOCKS ? (int64_t)nig::split_blocks_for(cus) : key == NIG_TUNE_WIDE_MIN_BLOCKS ? (int64_t)nig::wide_min_blocks_for(cus) : -1;
}

int64_t nig_handle_tune_get(const nig_handle *h, int32_t key)
{
    if (!h) return -1;
    return key == NIG_TUNE_SPLIT_BLOCKS ? (int64_t)nig::split_blocks_for(h->cus) : key == NIG_TUNE_WIDE_MIN_BLOCKS ? (int64_t)nig::wide_min_blocks_for(h->cus) : -1;
}

int nig_clock_stamp(void *stream, uint64_t *out)
{
    if (!out) return fail(NIG_ERR_INVALID, "nig_clock_stamp: NULL buffer");
    hipLaunchKernelGGL(nig::clock_stamp_kernel, dim3(4096), dim3(64), 0, (hipStream_t)stream, (unsigned long long *)out);
    HIP_TRY(hipGetLastError());
    return NIG_OK;
}

int nig_env_id(const char *name)
{
    if (!name) return -1;
    for (int i = 0; i < NIG_NUM_ENVS; ++i)
        if (strcmp(name, NAMES[i]) == 0) return i;
    return -1;
}

const char *nig_env_name(int env) { return (env >= 0 && env < NIG_NUM_ENVS) ? NAMES[env] : nullptr; }

int nig_env_spec_get(int env, nig_env_spec *out)
{
    if (env < 0 || env >= NIG_NUM_ENVS || !out) return fail(NIG_ERR_INVALID, "nig_env_spec_get: bad env id");
    *out = SPECS[env];
    return NIG_OK;
}

static int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

int nig_layout_query(int env, int64_t batch, uint32_t flags, nig_layout *out)
{
    if (env < 0 || env >= NIG_NUM_ENVS || !out) return fail(NIG_ERR_INVALID, "nig_layout_query: bad env id");
    if (batch <= 0) return fail(NIG_ERR_INVALID, "nig_layout_query: batch must be positive");
    nig_layout L;
    L.batch = batch;
    L.ld = align_up(batch, 64);
    int64_t off = 0;
    L.off_state = off;      off = align_up(off + (int64_t)SPECS[env].state_dim * L.ld * 4, 256);
    L.off_ctr = off;        off = align_up(off + L.ld * 4, 256);
    L.off_life_viol = off;  off = align_up(off + L.ld * 8, 256);
    if (flags & NIG_F_TALLY) {
        L.off_ep_return = off;  off = align_up(off + L.ld * 8, 256);
        L.off_tally = off;      off = align_up(off + (int64_t)NIG_T_ROWS * L.ld * 8, 256);
    } else {
        L.off_ep_return = -1;
        L.off_tally = -1;
    }
    // tail: reduce scratch + the device-resident launch counter used by plans
    off = align_up(off + (int64_t)REDUCE_BLOCKS * NIG_T_ROWS * 8, 256) + 256 + POLICY_BYTES;
    L.bytes = off;
    *out = L;
    return NIG_OK;
}


int nig_create(int env, int64_t batch, int device, uint64_t seed, uint64_t env_index0, int32_t max_episode_steps,
               double dt, uint32_t flags, void *workspace, nig_handle **out)
{
    if (!out) return fail(NIG_ERR_INVALID, "nig_create: out is NULL");
    *out = nullptr;
    if (env < 0 || env >= NIG_NUM_ENVS) return fail(NIG_ERR_INVALID, "nig_create: unknown env id");
    if (batch <= 0 || batch > NIG_MAX_BATCH) return fail(NIG_ERR_INVALID, "nig_create: batch outside [1, 2^24]");
    if (max_episode_steps < 0 || max_episode_steps > NIG_MAX_EPISODE_STEPS)
        return fail(NIG_ERR_INVALID, "nig_create: max_episode_steps outside [1, 21845]");
    if (dt < 0.0 || dt != dt) return fail(NIG_ERR_INVALID, "nig_create: bad dt");
    if (SPECS[env].n_constraints > 3 && max_episode_steps > 16383)
        return fail(NIG_ERR_INVALID, "nig_create: max_episode_steps > 16383 for an env with 4 safety conditions");
    if (env == NIG_ENV_CHEMICAL_REACTOR && dt != 0.0 && dt != 0.1)
        return fail(NIG_ERR_UNSUPPORTED, "nig_create: ChemicalReactor hard-codes dt=0.1 upstream (chemical_reactor.py:68)");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(NIG_ERR_NODEVICE, "nig_create: no HIP device (%s); there is no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    if (device < 0 || device >= ndev) return fail(NIG_ERR_INVALID, "nig_create: device index out of range");
    HIP_TRY(hipSetDevice(device));
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
    nig::g_last_cus.store((unsigned)cus, std::memory_order_relaxed);

    nig_handle *h = new (std::nothrow) nig_handle();
    if (!h) return fail(NIG_ERR_INVALID, "nig_create: out of host memory");
    h->env = env; h->device = device; h->B = batch; h->seed = seed; h->env0 = env_index0; h->cus = (unsigned)cus;
    h->max_steps = max_episode_steps ? max_episode_steps : SPECS[env].max_episode_steps;
    h->dt = (dt != 0.0) ? dt : SPECS[env].dt;
    h->flags = flags; h->cmask = 0xFu;
    nig_layout_query(env, batch, flags, &h->lay);
    if (workspace) {
        if (((uintptr_t)workspace & 255u) != 0) { delete h; return fail(NIG_ERR_INVALID, "nig_create: workspace not 256-byte aligned"); }
        // the step kernel updates the episode tally and the lifetime violation count with hardware atomics executed at the
        // memory side: on host-pinned / fine-grained memory they would silently miscount
        hipPointerAttribute_t at;
        memset(&at, 0, sizeof at);
        const hipError_t pe = hipPointerGetAttributes(&at, workspace);
        // Rejected: memory POSITIVELY identified as host, managed or another device's.  A query that fails (device-local
        // memory mapped through the virtual-memory API -- hipMemCreate / hipMemMap, e.g. torch's expandable_segments allocator --
        // is not known to hipPointerGetAttributes on every ROCm release) or that reports a type this code does not know is
        // accepted: the caller has stated in the contract that it is device-local memory of `device`.
        if (pe != hipSuccess) (void)hipGetLastError();
        else if (at.type == hipMemoryTypeHost || at.type == hipMemoryTypeManaged || at.isManaged ||
                 (at.type == hipMemoryTypeDevice && at.device != device)) {
            delete h;
            return fail(NIG_ERR_INVALID, "nig_create: workspace must be ordinary device-local memory of `device` (hipMalloc / a torch CUDA tensor), "
                                         "not host-pinned, managed or another device's memory");
        }
        h->ws = (char *)workspace; h->owns_ws = false;
    } else {
        void *p = nullptr;
        hipError_t me = hipMalloc(&p, (size_t)h->lay.bytes);
        if (me != hipSuccess) { delete h; return fail(NIG_ERR_HIP, "hipMalloc workspace: %s", hipGetErrorString(me)); }
        h->ws = (char *)p; h->owns_ws = true;
    }
    h->pol_dev = (nig_policy *)(h->ws + h->lay.bytes - POLICY_BYTES);
    h->t_dev = (uint32_t *)(h->ws + h->lay.bytes - POLICY_BYTES - 256);
    h->scratch = (double *)(h->ws + h->lay.bytes - POLICY_BYTES - 256 - align_up((int64_t)REDUCE_BLOCKS * NIG_T_ROWS * 8, 256));
    h->state = (float *)(h->ws + h->lay.off_state); h->ld_state = h->lay.ld;
    const nig_layout &L = h->lay;
    hipLaunchKernelGGL(init_ws_kernel, dim3(grid_for(L.ld)), dim3(BLOCK), 0, (hipStream_t)0,
                       ws_ctr(h), ws_life_viol(h), ws_ep_return(h), ws_tally(h), L.ld, L.batch);
    hipError_t le = hipGetLastError();
    if (le == hipSuccess) le = hipMemsetAsync(h->ws + L.off_state, 0, (size_t)SPECS[env].state_dim * L.ld * 4, (hipStream_t)0);
    if (le == hipSuccess) le = hipMemsetAsync(h->t_dev, 0, 256, (hipStream_t)0);      // launch counter of plans + the ring error word of test builds
    if (le == hipSuccess) le = hipStreamSynchronize((hipStream_t)0);
    if (le != hipSuccess) {
        if (h->owns_ws) (void)hipFree(h->ws);
        delete h;
        return fail(NIG_ERR_HIP, "nig_create: workspace init failed: %s", hipGetErrorString(le));
    }
    *out = h;
    return NIG_OK;
}

int nig_destroy(nig_handle *h)
{
    if (!h) return NIG_OK;
    if (h->mlp_stream) (void)hipFree(h->mlp_stream);
    if (h->mlp_shape_stream) (void)hipFree(h->mlp_shape_stream);
    if (h->mlp_cshape_stream) (void)hipFree(h->mlp_cshape_stream);
    if (h->mlp_ln_stream) (void)hipFree(h->mlp_ln_stream);
    if (h->mlp_cln_stream) (void)hipFree(h->mlp_cln_stream);
    if (h->mlp_bf16_stream) (void)hipFree(h->mlp_bf16_stream);
    if (h->mlp_cstream) (void)hipFree(h->mlp_cstream);
    if (h->mlp_ctail) (void)hipFree(h->mlp_ctail);
    if (h->ens_stream) (void)hipFree(h->ens_stream);
    if (h->ens_w) (void)hipFree(h->ens_w);
    if (h->gate_stream) (void)hipFree(h->gate_stream);
    if (h->proj_cstream) (void)hipFree(h->proj_cstream);
    if (h->proj_bstream) (void)hipFree(h->proj_bstream);
    if (h->pid_mem) (void)hipFree(h->pid_mem);
    if (h->act32) (void)hipFree(h->act32);
    if (h->act_soa) (void)hipFree(h->act_soa);
    if (h->lim_dev) (void)hipFree(h->lim_dev);
    if (h->hst_dev) (void)hipFree(h->hst_dev);
    if (h->hst_pinned) (void)hipHostFree(h->hst_pinned);
    if (h->owns_ws && h->ws) (void)hipFree(h->ws);
    delete h;
    return NIG_OK;
}

int nig_get_layout(const nig_handle *h, nig_layout *out)
{
    if (!h || !out) return fail(NIG_ERR_INVALID, "nig_get_layout: NULL argument");
    *out = h->lay;
    return NIG_OK;
}

void *nig_workspace(const nig_handle *h) { return h ? (void *)h->ws : nullptr; }

int nig_get_counter(const nig_handle *h, uint32_t *t)
{
    if (!h || !t) return fail(NIG_ERR_INVALID, "nig_get_counter: NULL argument");
    *t = h->t;
    return NIG_OK;
}

int nig_bind_state(nig_handle *h, float *state, int64_t ld)
{
    if (!h) return fail(NIG_ERR_INVALID, "nig_bind_state: NULL handle");
    if (!state) { h->state = (float *)(h->ws + h->lay.off_state); h->ld_state = h->lay.ld; return NIG_OK; }
    if (ld < h->B || ld > NIG_MAX_PITCH) return fail(NIG_ERR_INVALID, "nig_bind_state: ld outside [batch, 2^26]");
    if (((uintptr_t)state & 3u) != 0) return fail(NIG_ERR_INVALID, "nig_bind_state: unaligned pointer");
    h->state = state; h->ld_state = ld;
    return NIG_OK;
}

int nig_set_constraint_mask(nig_handle *h, uint32_t mask)
{
    if (!h) return fail(NIG_ERR_INVALID, "nig_set_constraint_mask: NULL handle");
    h->cmask = mask & 0xFu;
    return NIG_OK;
}

int nig_set_counter(nig_handle *h, uint32_t t)
{
    if (!h) return fail(NIG_ERR_INVALID, "nig_set_counter: NULL handle");
    h->t = t;
    return NIG_OK;
}

int nig_reset(nig_handle *h, const uint8_t *mask, const double *init_noise, int64_t ld_noise, void *stream)
{
    if (!h) return fail(NIG_ERR_INVALID, "nig_reset: NULL handle");
    if (init_noise && ld_noise < h->B) return fail(NIG_ERR_INVALID, "nig_reset: ld_noise < batch");
    ResetArgs a;
    a.state = h->state; a.ld_state = h->ld_state; a.ctr = ws_ctr(h); a.life_viol = ws_life_viol(h); a.ep_ret = ws_ep_return(h);
    a.ld = h->lay.ld; a.B = h->B; a.mask = mask; a.noise = init_noise; a.ld_noise = ld_noise;
    a.env0 = h->env0; a.seed_lo = (uint32_t)h->seed; a.seed_hi = (uint32_t)(h->seed >> 32); a.t = h->t;
    hipStream_t st = (hipStream_t)stream;
    launch_of(h->env)->reset(a, init_noise != nullptr, grid_for(a.B), st);
    HIP_TRY(hipGetLastError());
    if (!mask) h->may_hold_done = false;          // every lane starts an episode: none is left waiting for a reset
    return NIG_OK;
}

// Every argument check of nig_step / nig_step64 (`fn`: the entry point's name).  Parity mode = the caller supplies every value the
// reference's RNG would have drawn.
static int check_step(const nig_handle *h, const char *fn, const void *actions, int64_t ld_act, const double *step_noise,
                      const double *reset_noise, int64_t ld_noise, const float *final_obs, int64_t ld_obs)
{
    if (!h) return refuse(fn, "NULL handle");
    if (!actions || ld_act < h->B || ld_act > NIG_MAX_PITCH) return refuse(fn, "actions NULL or ld_act outside [batch, 2^26]");
    if (step_noise || reset_noise) {
        if (SPECS[h->env].k_step > 0 && !step_noise) return refuse(fn, "parity mode needs step_noise");
        if ((h->flags & NIG_F_AUTORESET) != 0 && !reset_noise) return refuse(fn, "parity mode with auto-reset needs reset_noise");
        if (ld_noise < h->B || ld_noise > NIG_MAX_PITCH) return refuse(fn, "ld_noise outside [batch, 2^26]");
    }
    if (final_obs && (ld_obs < h->B || ld_obs > NIG_MAX_PITCH)) return refuse(fn, "ld_obs outside [batch, 2^26]");
    return NIG_OK;
}

// Counts the step and returns its kernel arguments, all but the action pointer (float32 or float64: the caller's).
static StepArgs next_step_args(nig_handle *h, int64_t ld_act, const double *step_noise, const double *reset_noise, int64_t ld_noise,
                               float *reward_out, double *reward64_out, uint32_t *flags_out, float *final_obs, int64_t ld_obs)
{
    h->t += 1;
    StepArgs a = base_step_args(h);
    a.ld_act = (uint32_t)ld_act;
    a.step_noise = step_noise; a.reset_noise = reset_noise; a.ld_noise = (uint32_t)ld_noise;
    a.reward = reward_out; a.reward64 = reward64_out; a.flags = flags_out; a.final_obs = final_obs; a.ld_obs = (uint32_t)ld_obs;
    a.t_off = h->t;
    return a;
}

// nig_step / nig_step64 (act64: float64 action rows) and, with lim, their _limited twins (xflags_out: the twins').  The parent asks
// whether limits are installed before anything else (a NULL handle has none), the twin after its argument checks.  Every argument
// is checked before anything is launched: a refused call enqueues nothing, the narrowing copy included.
static int step_impl(nig_handle *h, const char *fn, bool lim, bool act64, const void *actions, int64_t ld_act, const double *step_noise,
                     const double *reset_noise, int64_t ld_noise, float *reward_out, double *reward64_out, uint32_t *flags_out,
                     uint32_t *xflags_out, float *final_obs, int64_t ld_obs, void *stream)
{
    if (!lim) NIG_TRY(refuse_limited(h, fn));
    NIG_TRY(check_step(h, fn, actions, ld_act, step_noise, reset_noise, ld_noise, final_obs, ld_obs));
    if (lim) NIG_TRY(check_limits(h, fn));
    const EnvLaunch *L = launch_of(h->env);
    const unsigned grid = grid_for(h->B);
    if (act64 && !L->step64) {                    // this env's own arithmetic takes the action as float32: narrow the rows, step on them
        const int A = SPECS[h->env].action_dim;
        if (!h->act32) HIP_TRY(hipMalloc((void **)&h->act32, (size_t)A * h->lay.ld * sizeof(float)));
        hipLaunchKernelGGL(narrow_rows_kernel, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, (const double *)actions, ld_act,
                           h->act32, h->lay.ld, A, h->B);
        HIP_TRY(hipGetLastError());
        actions = h->act32; ld_act = h->lay.ld; act64 = false;
    }
    StepLimArgs q;
    memset(&q, 0, sizeof q);
    q.p = next_step_args(h, ld_act, step_noise, reset_noise, ld_noise, reward_out, reward64_out, flags_out, final_obs, ld_obs);
    if (act64) q.p.actions64 = (const double *)actions;
    else q.p.actions = (const float *)actions;
    const bool parity = step_noise || reset_noise;
    if (lim) {
        limit_args(h, xflags_out, q.p, q.l);
        (act64 ? L->step64_limited : L->step_limited)(q, parity, grid, (hipStream_t)stream);
    } else {
        (act64 ? L->step64 : L->step)(q.p, parity, grid, (hipStream_t)stream);
    }
    HIP_TRY(hipGetLastError());
    return NIG_OK;
}

int nig_step(nig_handle *h, const float *actions, int64_t ld_act, const double *step_noise, const double *reset_noise,
             int64_t ld_noise, float *reward_out, double *reward64_out, uint32_t *flags_out, float *final_obs,
             int64_t ld_obs, void *stream)
{
    return step_impl(h, "nig_step", false, false, actions, ld_act, step_noise, reset_noise, ld_noise, reward_out, reward64_out, flags_out,
                     nullptr, final_obs, ld_obs, stream);
}

int nig_step64(nig_handle *h, const double *actions, int64_t ld_act, const double *step_noise, const double *reset_noise,
               int64_t ld_noise, float *reward_out, double *reward64_out, uint32_t *flags_out, float *final_obs,
               int64_t ld_obs, void *stream)
{
    return step_impl(h, "nig_step64", false, true, actions, ld_act, step_noise, reset_noise, ld_noise, reward_out, reward64_out, flags_out,
                     nullptr, final_obs, ld_obs, stream);
}

int nig_step_limited(nig_handle *h, const float *actions, int64_t ld_act, const double *step_noise, const double *reset_noise,
                     int64_t ld_noise, float *reward_out, double *reward64_out, uint32_t *flags_out, uint32_t *xflags_out,
                     float *final_obs, int64_t ld_obs, void *stream)
{
    return step_impl(h, "nig_step_limited", true, false, actions, ld_act, step_noise, reset_noise, ld_noise, reward_out, reward64_out,
                     flags_out, xflags_out, final_obs, ld_obs, stream);
}

int nig_step64_limited(nig_handle *h, const double *actions, int64_t ld_act, const double *step_noise, const double *reset_noise,
                       int64_t ld_noise, float *reward_out, double *reward64_out, uint32_t *flags_out, uint32_t *xflags_out,
                       float *final_obs, int64_t ld_obs, void *stream)
{
    return step_impl(h, "nig_step64_limited", true, true, actions, ld_act, step_noise, reset_noise, ld_noise, reward_out, reward64_out,
                     flags_out, xflags_out, final_obs, ld_obs, stream);
}


// ---- box constraints added by the user ("nig-limits-v1", csrc/nig_limits.hpp) -------------------------------------------------
int nig_set_limits(nig_handle *h, int32_t n, const nig_limit *limits, void *stream)
{
    const char *const fn = "nig_set_limits";
    if (!h) return refuse(fn, "NULL handle");
    const nig_env_spec &sp = SPECS[h->env];
    if (!launch_of(h->env)->step_limited)
        return refuse(fn, "the Advanced envs override step() wholesale: no added constraints", NIG_ERR_UNSUPPORTED);
    if (n < 0 || n > NIG_MAX_LIMITS) return refuse(fn, "n outside 0 .. NIG_MAX_LIMITS");
    if (n == 0) { h->n_limits = 0; return NIG_OK; }
    if (!limits) return refuse(fn, "limits is NULL");
    const int rows = sp.state_dim + sp.action_dim;
    static_assert(NIG_MAX_STATE_DIM + NIG_MAX_ACTION_DIM <= NIG_LIMIT_ROWS, "a bound for every state and action row");
    for (int c = 0; c < n; ++c) {
        const nig_limit &l = limits[c];
        if (l.mask == 0) return refuse(fn, "a constraint lists no row (empty mask)");
        if ((l.mask >> rows) != 0) return refuse(fn, "a mask bit >= S + A");
        for (int r = 0; r < rows; ++r)
            if (((l.mask >> r) & 1u) && !(l.lo[r] <= l.hi[r])) return refuse(fn, "lo > hi (or a NaN bound) on a listed row");
        if (l.penalty != l.penalty) return refuse(fn, "a NaN penalty");
    }
    if ((int64_t)(sp.n_constraints + n) * h->max_steps > 65535)
        return refuse(fn, "(built-in constraints + n) * max_episode_steps > 65535: the counter word keeps an episode's violations in 16 bits");
    LimitTable T;
    memset(&T, 0, sizeof T);
    for (int c = 0; c < n; ++c) {
        T.c[c] = limits[c];
        T.c[c].critical = limits[c].critical != 0; T.c[c].reserved = 0;
        for (int r = 0; r < NIG_LIMIT_ROWS; ++r)      // rows that are not listed are never read: a defined value all the same
            if (r >= rows || !((limits[c].mask >> r) & 1u)) { T.c[c].lo[r] = 0.0f; T.c[c].hi[r] = 0.0f; }
    }
    T.n = n;
    if (!h->lim_dev) HIP_TRY(hipMalloc((void **)&h->lim_dev, sizeof(LimitTable)));
    HIP_TRY(hipMemcpyAsync(h->lim_dev, &T, sizeof T, hipMemcpyHostToDevice, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));        // (the source is this frame's)
    h->n_limits = n;
    return NIG_OK;
}

int nig_get_limit_count(const nig_handle *h) { return h ? h->n_limits : -1; }

// ---- fused rollout ---------------------------------------------------------------------------------------------------------
// What nig_rollout / nig_rollout_sampled / nig_rollout_noise (and nig_rollout_mixed_obs, per segment) ask for
struct RolloutSpec {
    int32_t n_steps;
    const float *action_ring; int64_t ld_act, slot_stride; int32_t ring_len;      // (sampled: not looked at)
    const double *step_noise; int64_t step_noise_stride; const double *reset_noise; int64_t reset_noise_stride, ld_noise;
    float *reward_out; uint32_t *flags_out; int64_t out_stride;
    float *obs_out; int64_t ld_obs, obs_step_stride;
    bool sampled;
};

// The kernel arguments of handle h's lanes, which start `lane0` columns into every array of the request (recorded draws apart)
static RolloutArgs rollout_args(const nig_handle *h, const RolloutSpec &c, int64_t lane0)
{
    RolloutArgs q;
    memset(&q, 0, sizeof q);
    q.s = base_step_args(h);
    q.s.actions = c.action_ring ? c.action_ring + lane0 : nullptr; q.s.ld_act = (uint32_t)c.ld_act;
    q.s.reward = c.reward_out ? c.reward_out + lane0 : nullptr;
    q.s.flags = c.flags_out ? c.flags_out + lane0 : nullptr;
    q.s.t_off = h->t;
    q.n_steps = c.n_steps; q.ring_len = c.ring_len; q.slot_stride = (uint32_t)c.slot_stride; q.out_stride = (uint32_t)c.out_stride;
    q.obs_out = c.obs_out ? c.obs_out + lane0 : nullptr; q.ld_obs_out = (uint32_t)c.ld_obs; q.obs_step_stride = (uint64_t)c.obs_step_stride;
    q.obs_aos = (c.obs_out && c.ld_obs == 0) ? 1 : 0;
    return q;
}

static int rollout_impl(nig_handle *h, RolloutSpec c, void *stream)
{
    const char *const fn = "nig_rollout";
    NIG_TRY(refuse_limited(h, fn));
    // 1. validate
    if (!h || c.n_steps <= 0 || (!c.sampled && (!c.action_ring || c.ring_len <= 0))) return refuse(fn, "bad argument");
    const nig_env_spec &sp = SPECS[h->env];
    // ld_act == 0: the ring is ROW-MAJOR, slot s = [B][A] at action_ring + s * slot_stride (what an agent's batched output looks like)
    const bool act_aos = !c.sampled && c.ld_act == 0;
    const bool noise = c.step_noise || c.reset_noise;      // nig_rollout_noise: the reference's recorded draws
    if (c.sampled) {                                       // no ring: the kernel's ring fields take fixed values
        c.action_ring = nullptr; c.ld_act = h->lay.ld; c.slot_stride = 0; c.ring_len = 1;
    } else if (act_aos) {
        if (noise) return fail(NIG_ERR_UNSUPPORTED, "nig_rollout_noise: the recorded-draw launches take [A][ld_act] action rows");
        if (c.slot_stride < (int64_t)sp.action_dim * h->B || c.slot_stride > 0xffffffffLL)
            return refuse(fn, "row-major action ring: slot_stride smaller than one [batch][A] slot (or >= 2^32)");
    } else {
        if (c.ld_act < h->B || c.ld_act > NIG_MAX_PITCH) return refuse(fn, "ld_act outside {0} U [batch, 2^26]");
        if (c.slot_stride < (int64_t)sp.action_dim * c.ld_act || c.slot_stride > 0xffffffffLL)
            return refuse(fn, "slot_stride smaller than one [A][ld_act] slot (or >= 2^32)");
    }
    NIG_TRY(check_out_stride(h, fn, c.n_steps, c.out_stride));
    const bool obs_aos = c.obs_out && c.ld_obs == 0;
    if (c.obs_out && !obs_aos && (c.ld_obs < h->B || c.ld_obs > NIG_MAX_PITCH ||
                                  (c.obs_step_stride != 0 && c.obs_step_stride < (int64_t)sp.state_dim * c.ld_obs)))
        return refuse(fn, "bad observation trajectory pitch");
    if (obs_aos && ((c.obs_step_stride != 0 && c.obs_step_stride < (int64_t)sp.state_dim * h->B) || (c.obs_step_stride & 3) || ((uintptr_t)c.obs_out & 15)))
        return refuse(fn, "row-major trajectory needs 16-byte alignment and obs_step_stride 0 or >= S*batch (multiple of 4)");
    NIG_TRY(check_counter(h, fn, c.n_steps));
    NIG_TRY(check_reward_flags(fn, c.reward_out, c.flags_out));
    if (c.obs_out && !c.reward_out) return refuse(fn, "an observation trajectory needs reward_out and flags_out too");
    const int out_mode = !c.reward_out ? 0 : (!c.obs_out ? 1 : (obs_aos ? 3 : 2));
    if (noise) {
        const char *const nf = "nig_rollout_noise";
        if (h->env > NIG_ENV_ROBOT_ASSEMBLY)
            return refuse(nf, "only the envs the reference can record draws for (ChemicalReactor, PowerGrid, RobotAssembly)", NIG_ERR_UNSUPPORTED);
        if (out_mode != 3)
            return refuse(nf, "the injected-draw kernels exist for the row-major trajectory (obs_out with ld_obs == 0) only", NIG_ERR_UNSUPPORTED);
        if (c.ring_len < c.n_steps) return refuse(nf, "recorded draws belong to recorded actions: ring_len >= n_steps");
        if (c.ld_noise < h->B || c.ld_noise > NIG_MAX_PITCH) return refuse(nf, "ld_noise outside [batch, 2^26]");
        if (sp.k_step > 0 && (!c.step_noise || c.step_noise_stride < (int64_t)sp.k_step * c.ld_noise))
            return refuse(nf, "step_noise NULL or its step stride smaller than one [k_step][ld_noise] row set");
        if ((h->flags & NIG_F_AUTORESET) != 0 && sp.k_reset > 0 && (!c.reset_noise || c.reset_noise_stride < (int64_t)sp.k_reset * c.ld_noise))
            return refuse(nf, "an auto-reset handle needs reset_noise, step stride >= one [k_reset][ld_noise] row set");
    }
    // 2. kernel arguments
    RolloutArgs q = rollout_args(h, c, 0);
    hipStream_t st = (hipStream_t)stream;
    // 3. row-major action ring
    if (act_aos) {
        // NATIVE where every kernel of the launch reads a lane's actions as contiguous bytes: PowerGrid's LDS-resident body
        // (csrc/nig_pg_lds.hpp: two 16-byte loads per lane, 2 KiB contiguous per wave instead of eight 256-byte row segments) in its
        // wide 512 / 256 and paired forms -- the launcher's own predicate (rollout_rows_native, next to launch_rollout_form) -- and
        // 16-byte aligned slots.  Every other launch reads [A][ld] rows: the ring is transposed into a buffer the handle owns, on
        // the caller's stream, per call.
        const int A = sp.action_dim;
        const bool native = launch_of(h->env)->rows_native(out_mode, q) && ((uintptr_t)c.action_ring & 15) == 0 && (c.slot_stride & 3) == 0;
        if (!native) {
            if ((int64_t)A * h->lay.ld > 0xffffffffLL) return refuse(fn, "row-major action ring: batch too large for the row copy");
            const int used = c.ring_len < c.n_steps ? c.ring_len : c.n_steps;     // the slots this call reads: step k takes slot k % ring_len, from 0
            const size_t need = (size_t)used * A * (size_t)h->lay.ld;
            if (h->act_soa_floats < need) {
                if (h->act_soa) { HIP_TRY(hipStreamSynchronize(st)); (void)hipFree(h->act_soa); h->act_soa = nullptr; h->act_soa_floats = 0; }
                HIP_TRY(hipMalloc((void **)&h->act_soa, need * sizeof(float)));
                h->act_soa_floats = need;
            }
            hipLaunchKernelGGL(nig::action_rows_kernel, dim3(grid_for(h->B), (unsigned)(used < 65535 ? used : 65535)), dim3(BLOCK), 0, st,
                               c.action_ring, c.slot_stride, h->act_soa, h->lay.ld, h->B, A, used);
            HIP_TRY(hipGetLastError());
            q.s.actions = h->act_soa; q.s.ld_act = (uint32_t)h->lay.ld; q.slot_stride = (uint32_t)((int64_t)A * h->lay.ld);
        }
    }
    // 4. recorded draws
    if (noise) {
        q.s.step_noise = sp.k_step > 0 ? c.step_noise : nullptr;
        q.s.reset_noise = c.reset_noise;
        if (!q.s.step_noise && !q.s.reset_noise) q.s.reset_noise = c.step_noise;   // (keeps the launcher on the injected-draw path)
        q.s.ld_noise = (uint32_t)c.ld_noise;
        q.nz_step_stride = (uint64_t)c.step_noise_stride; q.nz_reset_stride = (uint64_t)c.reset_noise_stride;
    }
    // 5. launch
    if (c.sampled) launch_of(h->env)->rollout_sampled(out_mode, q, h->t + 1u, grid_for(h->B), st);
    else launch_of(h->env)->rollout(out_mode, q, h->t + 1u, grid_for(h->B), st);
    HIP_TRY(hipGetLastError());
    h->t += (uint32_t)c.n_steps;
    return ring_check(h, st, fn);
}

int nig_rollout(nig_handle *h, int32_t n_steps, const float *action_ring, int64_t ld_act, int64_t slot_stride,
                int32_t ring_len, float *reward_out, uint32_t *flags_out, int64_t out_stride,
                float *obs_out, int64_t ld_obs, int64_t obs_step_stride, void *stream)
{
    return rollout_impl(h, {n_steps, action_ring, ld_act, slot_stride, ring_len, nullptr, 0, nullptr, 0, 0, reward_out, flags_out,
                            out_stride, obs_out, ld_obs, obs_step_stride, false}, stream);
}

int nig_rollout_sampled(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out, int64_t out_stride,
                        float *obs_out, int64_t ld_obs, int64_t obs_step_stride, void *stream)
{
    return rollout_impl(h, {n_steps, nullptr, 0, 0, 0, nullptr, 0, nullptr, 0, 0, reward_out, flags_out,
                            out_stride, obs_out, ld_obs, obs_step_stride, true}, stream);
}

int nig_rollout_noise(nig_handle *h, int32_t n_steps, const float *action_ring, int64_t ld_act, int64_t slot_stride,
                      int32_t ring_len, const double *step_noise, int64_t step_noise_stride, const double *reset_noise,
                      int64_t reset_noise_stride, int64_t ld_noise, float *reward_out, uint32_t *flags_out, int64_t out_stride,
                      float *obs_out, int64_t obs_step_stride, void *stream)
{
    if (!step_noise && !reset_noise) return fail(NIG_ERR_INVALID, "nig_rollout_noise: no recorded draws given (use nig_rollout)");
    return rollout_impl(h, {n_steps, action_ring, ld_act, slot_stride, ring_len, step_noise, step_noise_stride, reset_noise,
                            reset_noise_stride, ld_noise, reward_out, flags_out, out_stride, obs_out, 0, obs_step_stride, false}, stream);
}

int nig_set_policy(nig_handle *h, const nig_policy *policy, void *stream)
{
    if (!h || !policy) return fail(NIG_ERR_INVALID, "nig_set_policy: NULL argument");
    static_assert(sizeof(nig_policy) <= POLICY_BYTES, "policy struct outgrew its device slot");
    if (policy->kind != NIG_POLICY_AFFINE && policy->kind != NIG_POLICY_PID)
        return fail(NIG_ERR_INVALID, "nig_set_policy: unknown policy kind");
    if (!(policy->clip_lo <= policy->clip_hi)) return fail(NIG_ERR_INVALID, "nig_set_policy: clip_lo > clip_hi");
    h->pol_host = *policy;
    // recompute the non-zero column mask here so a caller cannot get it wrong
    uint32_t cm = 0;
    for (int k = 0; k < SPECS[h->env].state_dim; ++k)
        for (int j = 0; j < SPECS[h->env].action_dim; ++j)
            if (policy->Wt[k][j] != 0.0f) cm |= (1u << k);
    h->pol_host.colmask = cm;
    if (policy->kind == NIG_POLICY_PID) {         // the agent's constructor: integral = previous_error = 0 (baseline_agents.py:55-57)
        const size_t bytes = (size_t)2 * SPECS[h->env].action_dim * h->lay.ld * sizeof(float);
        if (!h->pid_mem) HIP_TRY(hipMalloc((void **)&h->pid_mem, bytes));
        HIP_TRY(hipMemsetAsync(h->pid_mem, 0, bytes, (hipStream_t)stream));
    }
    HIP_TRY(hipMemcpyAsync(h->pol_dev, &h->pol_host, sizeof(nig_policy), hipMemcpyHostToDevice, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));   // pageable source: make the staging copy reusable
    h->has_policy = true;
    return NIG_OK;
}

int nig_rollout_policy(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out, int64_t out_stride,
                       float *obs_out, int64_t obs_step_stride, float *act_out, int64_t ld_act,
                       int64_t act_step_stride, void *stream)
{
    return rollout_policy<false>(h, "nig_rollout_policy", n_steps, {CLOSED_LOOP_OUT}, stream);
}

int nig_rollout_policy_limited(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out, int64_t out_stride,
                               float *obs_out, int64_t obs_step_stride, float *act_out, int64_t ld_act,
                               int64_t act_step_stride, uint32_t *xflags_out, void *stream)
{
    return rollout_policy<true>(h, "nig_rollout_policy_limited", n_steps, {CLOSED_LOOP_OUT, xflags_out}, stream);
}

// nig_set_mlp_policy / _safety / _ensemble: `count` operand-stream images of `floats` floats, back to back, network k (in_dim -> 256 ->
// 256 -> rows) from the k-th entry of the six arrays; refuses another hidden width and an env without the MFMA actor.  *host: calloc'd.
static int build_network_images(const nig_handle *h, const char *fn, int32_t hidden, int in_dim, int rows, size_t floats, int count,
                                const float *const *W1, const float *const *b1, const float *const *W2, const float *const *b2,
                                const float *const *W3, const float *const *b3, float **host)
{
    if (hidden != MLP_H) return refuse(fn, "hidden must be 256 (agents/networks.py default)", NIG_ERR_UNSUPPORTED);
    if (!launch_of(h->env)->mlp) return refuse(fn, "env shape not supported (even state dim, at most 16 actions)", NIG_ERR_UNSUPPORTED);
    *host = (float *)calloc((size_t)count * floats, sizeof(float));
    if (!*host) return refuse(fn, "out of host memory");
    for (int k = 0; k < count; ++k)
        if (!put_network(in_dim, rows, W1[k], b1[k], W2[k], b2[k], W3[k], b3[k], *host + (size_t)k * floats, floats)) {
            free(*host);
            return refuse(fn, "the operand stream does not fit its image, or an internal record count mismatch");
        }
    return NIG_OK;
}

// A built host image (malloc'd; freed here) -> the device stream *dev, allocated on first use; copied on `stream` and waited for.
static int upload_stream(const char *fn, float **dev, float *host, size_t floats, void *stream)
{
    hipError_t e = hipSuccess;
    if (!*dev) e = hipMalloc((void **)dev, floats * sizeof(float));
    if (e == hipSuccess) e = hipMemcpyAsync(*dev, host, floats * sizeof(float), hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    free(host);
    return e == hipSuccess ? NIG_OK : refuse(fn, hipGetErrorString(e), NIG_ERR_HIP);
}

int nig_set_mlp_policy(nig_handle *h, int32_t hidden, const float *W1, const float *b1, const float *W2, const float *b2,
                       const float *W3, const float *b3, void *stream)
{
    if (!h || !W1 || !b1 || !W2 || !b2 || !W3 || !b3) return fail(NIG_ERR_INVALID, "nig_set_mlp_policy: NULL argument");
    const int S = SPECS[h->env].state_dim, A = SPECS[h->env].action_dim;
    float *host = nullptr;
    NIG_TRY(build_network_images(h, "nig_set_mlp_policy", hidden, S, A, MLP_STREAM_FLOATS, 1, &W1, &b1, &W2, &b2, &W3, &b3, &host));
    NIG_TRY(upload_stream("nig_set_mlp_policy", &h->mlp_stream, host, MLP_STREAM_FLOATS, stream));
    h->actor_kind = SHAPE_KIND_REFERENCE; h->actor_nh = 2; h->actor_dims[0] = h->actor_dims[1] = MLP_H; h->actor_dims[2] = 0;
    return NIG_OK;
}

// ---- the actor of the other hidden shapes ("nig-mlp-shape-v1", include/nig.h) ----
int nig_set_mlp_policy_dims(nig_handle *h, int32_t n_hidden, const int32_t *hidden, const float *const *W, const float *const *b, void *stream)
{
    const char *fn = "nig_set_mlp_policy_dims";
    if (!h || !hidden || !W || !b) return refuse(fn, "NULL argument");
    if (n_hidden < 2 || n_hidden > 3) return refuse(fn, "n_hidden outside 2 .. 3");
    int dims[3] = {0, 0, 0};
    for (int l = 0; l < n_hidden; ++l) {
        if (hidden[l] < 1 || hidden[l] > SHAPE_MAX_WIDTH) return refuse(fn, "a hidden width outside 1 .. 512");
        dims[l] = hidden[l];
    }
    for (int l = 0; l <= n_hidden; ++l)
        if (!W[l] || !b[l]) return refuse(fn, "NULL layer");
    if (!launch_of(h->env)->mlp) return refuse(fn, "env shape not supported (even state dim, at most 16 actions)", NIG_ERR_UNSUPPORTED);
    const int S = SPECS[h->env].state_dim, A = SPECS[h->env].action_dim;
    const int kind = shape_class_of(n_hidden, dims, S);
    if (kind == SHAPE_KIND_NONE) return refuse(fn, "no shape class holds these hidden widths");
    auto installed = [&]() {
        h->actor_kind = kind; h->actor_nh = n_hidden;
        for (int l = 0; l < 3; ++l) h->actor_dims[l] = dims[l];
        return NIG_OK;
    };
    if (kind == SHAPE_KIND_REFERENCE) {                     // padded to 256 x 256 on the host: the existing image and kernel
        float *pad = (float *)calloc(reference_pad_floats(S, A), sizeof(float));
        float *host = (float *)calloc(MLP_STREAM_FLOATS, sizeof(float));
        const bool ok = pad && host && put_reference_padded(S, A, dims, W, b, pad, host, MLP_STREAM_FLOATS);
        free(pad);
        if (!ok) { free(host); return refuse(fn, "out of host memory, or the operand stream does not fit its image"); }
        NIG_TRY(upload_stream(fn, &h->mlp_stream, host, MLP_STREAM_FLOATS, stream));
        return installed();
    }
    size_t cap = 0;                                         // the env's largest shaped image: the slot is allocated once
    for (int k = SHAPE_KIND_128; k <= SHAPE_KIND_3; ++k) {
        const size_t f = shape_plan(SHAPE_CLASSES[k], S).floats();
        cap = f > cap ? f : cap;
    }
    const size_t floats = shape_plan(SHAPE_CLASSES[kind], S).floats();
    float *host = (float *)calloc(floats, sizeof(float));
    if (!host) return refuse(fn, "out of host memory");
    if (!put_shape_network(SHAPE_CLASSES[kind], S, A, n_hidden, dims, W, b, host, floats)) {
        free(host);
        return refuse(fn, "the operand image does not fit its chunk plan");
    }
    if (!h->mlp_shape_stream) {
        const hipError_t e = hipMalloc((void **)&h->mlp_shape_stream, cap * sizeof(float));
        if (e != hipSuccess) { h->mlp_shape_stream = nullptr; free(host); return refuse(fn, hipGetErrorString(e), NIG_ERR_HIP); }
    }
    NIG_TRY(upload_stream(fn, &h->mlp_shape_stream, host, floats, stream));
    return installed();
}

int nig_get_mlp_policy_dims(const nig_handle *h, int32_t *hidden)
{
    if (!h) return -1;
    if (hidden)
        for (int l = 0; l < 3; ++l) hidden[l] = l < h->actor_nh ? h->actor_dims[l] : 0;
    return h->actor_kind == SHAPE_KIND_NONE ? 0 : h->actor_nh;
}

// ---- the LayerNorm actor ("nig-mlp-ln-v1", csrc/nig_mlp_ln.hpp) ----
int nig_set_mlp_policy_ln(nig_handle *h, int32_t hidden, const float *W1, const float *b1, const float *g1, const float *be1,
                          const float *W2, const float *b2, const float *g2, const float *be2, const float *W3, const float *b3,
                          float eps, void *stream)
{
    const char *fn = "nig_set_mlp_policy_ln";
    if (!h || !W1 || !b1 || !g1 || !be1 || !W2 || !b2 || !g2 || !be2 || !W3 || !b3) return refuse(fn, "NULL argument");
    if (!(eps > 0.0f) || !(eps < __builtin_inff())) return refuse(fn, "eps must be finite and positive");
    if (hidden != MLP_H) return refuse(fn, "hidden must be 256: the LayerNorm actor has hidden widths (256, 256)", NIG_ERR_UNSUPPORTED);
    if (!launch_of(h->env)->mlp_ln) return refuse(fn, "env shape not supported (even state dim, at most 16 actions)", NIG_ERR_UNSUPPORTED);
    const int S = SPECS[h->env].state_dim, A = SPECS[h->env].action_dim;
    const size_t floats = ln_plan(S).floats();
    float *host = (float *)calloc(floats, sizeof(float));
    if (!host) return refuse(fn, "out of host memory");
    if (!put_ln_network(S, A, W1, b1, g1, be1, W2, b2, g2, be2, W3, b3, host, floats)) {
        free(host);
        return refuse(fn, "the operand image does not fit its chunk plan");
    }
    NIG_TRY(upload_stream(fn, &h->mlp_ln_stream, host, floats, stream));
    h->actor_kind = ACTOR_KIND_LN; h->actor_nh = 2; h->actor_dims[0] = h->actor_dims[1] = MLP_H; h->actor_dims[2] = 0;
    h->ln_eps = eps;
    return NIG_OK;
}

int nig_get_mlp_policy_norm(const nig_handle *h) { return !h ? -1 : h->actor_kind == ACTOR_KIND_LN ? 1 : 0; }

int nig_rollout_mlp(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out, int64_t out_stride,
                    float *obs_out, int64_t obs_step_stride, float *act_out, int64_t ld_act, int64_t act_step_stride,
                    void *stream)
{
    return rollout_mlp<false>(h, "nig_rollout_mlp", n_steps, {CLOSED_LOOP_OUT}, stream);
}

int nig_rollout_mlp_limited(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out, int64_t out_stride,
                            float *obs_out, int64_t obs_step_stride, float *act_out, int64_t ld_act, int64_t act_step_stride,
                            uint32_t *xflags_out, void *stream)
{
    return rollout_mlp<true>(h, "nig_rollout_mlp_limited", n_steps, {CLOSED_LOOP_OUT, xflags_out}, stream);
}

// ---- the actor on the bf16 matrix unit ("nig-mlp-bf16-v1", include/nig.h) ----
int nig_bf16_from_f32(const float *x, uint16_t *out, int64_t n)
{
    if (n < 0 || (n > 0 && (!x || !out))) return fail(NIG_ERR_INVALID, "nig_bf16_from_f32: bad argument");
    for (int64_t i = 0; i < n; ++i) out[i] = bf16_from_f32(x[i]);
    return NIG_OK;
}

int nig_set_mlp_policy_bf16(nig_handle *h, int32_t hidden, const float *W1, const float *b1, const float *W2, const float *b2,
                            const float *W3, const float *b3, void *stream)
{
    const char *fn = "nig_set_mlp_policy_bf16";
    if (!h || !W1 || !b1 || !W2 || !b2 || !W3 || !b3) return refuse(fn, "NULL argument");
    if (hidden != MLP_H) return refuse(fn, "hidden must be 256 (agents/networks.py default)", NIG_ERR_UNSUPPORTED);
    if (!launch_of(h->env)->mlp_bf16) return refuse(fn, "env shape not supported (even state dim, at most 16 actions)", NIG_ERR_UNSUPPORTED);
    static_assert(BF16_STREAM_BYTES % sizeof(float) == 0);
    float *host = (float *)calloc(BF16_STREAM_BYTES / sizeof(float), sizeof(float));
    if (!host) return refuse(fn, "out of host memory");
    if (!put_network_bf16(SPECS[h->env].state_dim, SPECS[h->env].action_dim, W1, b1, W2, b2, W3, b3, (unsigned char *)host, BF16_STREAM_BYTES)) {
        free(host);
        return refuse(fn, "the operand image does not fit its chunk plan");
    }
    return upload_stream(fn, &h->mlp_bf16_stream, host, BF16_STREAM_BYTES / sizeof(float), stream);
}

int nig_rollout_mlp_bf16(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out, int64_t out_stride,
                         float *obs_out, int64_t obs_step_stride, float *act_out, int64_t ld_act, int64_t act_step_stride,
                         uint16_t *hid_out, int64_t ld_hid, int64_t hid_step_stride, void *stream)
{
    const char *fn = "nig_rollout_mlp_bf16";
    if (!h || n_steps <= 0) return refuse(fn, "bad argument");
    NIG_TRY(refuse_limited(h, fn));
    if (!launch_of(h->env)->mlp_bf16) return refuse(fn, "env shape not supported (even state dim, at most 16 actions)", NIG_ERR_UNSUPPORTED);
    if (!h->mlp_bf16_stream) return refuse(fn, "no bf16 actor installed (nig_set_mlp_policy_bf16)");
    if (hid_out && (ld_hid < h->B || ld_hid > NIG_MAX_PITCH || hid_step_stride < 2 * (int64_t)MLP_H * ld_hid)) return refuse(fn, "bad hidden-activation pitch");
    return closed_loop<false, MlpBf16Args>(h, fn, n_steps, {CLOSED_LOOP_OUT}, stream, launch_of(h->env)->mlp_bf16, [&](MlpBf16Args &q) {
        q.m.wstream = h->mlp_bf16_stream;
        q.hid_out = hid_out; q.ld_hid = (uint32_t)ld_hid; q.hid_step_stride = (uint64_t)hid_step_stride;
    });
}

// what nig_get_mlp_safety_dims reports for the critics of hidden widths (256, 256): the plain, the categorical and the LayerNorm one
static void critic_dims_256(nig_handle *h)
{
    h->critic_class = SHAPE_KIND_REFERENCE; h->critic_nh = 2; h->critic_dims[0] = h->critic_dims[1] = MLP_H; h->critic_dims[2] = 0;
}

int nig_set_mlp_safety(nig_handle *h, int32_t hidden, const float *C1, const float *c1, const float *C2, const float *c2,
                       const float *C3, const float *c3, float threshold, void *stream)
{
    if (!h || !C1 || !c1 || !C2 || !c2 || !C3 || !c3) return fail(NIG_ERR_INVALID, "nig_set_mlp_safety: NULL argument");
    const int S = SPECS[h->env].state_dim, A = SPECS[h->env].action_dim;
    float *host = nullptr;
    NIG_TRY(build_network_images(h, "nig_set_mlp_safety", hidden, S + A, 1, MLP_CSTREAM_FLOATS, 1, &C1, &c1, &C2, &c2, &C3, &c3, &host));
    NIG_TRY(upload_stream("nig_set_mlp_safety", &h->mlp_cstream, host, MLP_CSTREAM_FLOATS, stream));
    h->mlp_threshold = threshold;
    h->mlp_ckind = NIG_SAFETY_SIGMOID;
    critic_dims_256(h);
    return NIG_OK;
}

// ---- the distributional safety critic ("nig-categorical-v1") ------------------------------------
int nig_set_mlp_safety_categorical(nig_handle *h, int32_t hidden, int32_t atoms, const float *C1, const float *c1, const float *C2,
                                   const float *c2, const float *C3, const float *c3, uint64_t below_mask, float threshold, void *stream)
{
    const char *const fn = "nig_set_mlp_safety_categorical";
    // (the law's own bounds first: they need no handle)
    if (atoms < 2 || atoms > NIG_MAX_ATOMS) return refuse(fn, "atoms outside 2 .. NIG_MAX_ATOMS");
    if (atoms < 64 && (below_mask >> atoms) != 0) return refuse(fn, "below_mask has a bit at or above atoms");
    if (!h || !C1 || !c1 || !C2 || !c2 || !C3 || !c3) return refuse(fn, "NULL argument");
    if (hidden != MLP_H) return refuse(fn, "hidden must be 256 (agents/networks.py default)", NIG_ERR_UNSUPPORTED);
    if (!launch_of(h->env)->mlp_cat_eval) return refuse(fn, "env shape not supported (even state dim, at most 16 actions)", NIG_ERR_UNSUPPORTED);
    const int S = SPECS[h->env].state_dim, A = SPECS[h->env].action_dim;
    float *host = (float *)calloc(MLP_CSTREAM_FLOATS, sizeof(float)), *tail = (float *)calloc(MLP_TAIL_FLOATS, sizeof(float));
    if (!host || !tail || !put_network_wide(S + A, atoms, C1, c1, C2, c2, C3, c3, host, MLP_CSTREAM_FLOATS, tail)) {
        free(host); free(tail);
        return refuse(fn, "out of host memory, or the operand stream does not fit its image");
    }
    // Both uploads overwrite device arrays the installed critic may be using, so a HIP failure in either leaves no critic at all: a
    // slot of kind none refuses every rollout and evaluation, where a half-replaced critic would compute with mixed weights.
    const int rc_tail = upload_stream(fn, &h->mlp_ctail, tail, MLP_TAIL_FLOATS, stream);
    const int rc = rc_tail ? (free(host), rc_tail) : upload_stream(fn, &h->mlp_cstream, host, MLP_CSTREAM_FLOATS, stream);
    if (rc) { h->mlp_ckind = NIG_SAFETY_NONE; return rc; }
    h->mlp_threshold = threshold;
    h->cat_atoms = atoms; h->cat_mask = below_mask;
    h->mlp_ckind = NIG_SAFETY_CATEGORICAL;
    critic_dims_256(h);
    return NIG_OK;
}

// ---- the LayerNorm safety critic ("nig-mlp-ln-shield-v1", csrc/nig_mlp_ln_shield.hpp) ----
int nig_set_mlp_safety_ln(nig_handle *h, int32_t hidden, const float *C1, const float *c1, const float *g1, const float *be1,
                          const float *C2, const float *c2, const float *g2, const float *be2, const float *C3, const float *c3,
                          float eps, float threshold, void *stream)
{
    const char *fn = "nig_set_mlp_safety_ln";
    if (!h || !C1 || !c1 || !g1 || !be1 || !C2 || !c2 || !g2 || !be2 || !C3 || !c3) return refuse(fn, "NULL argument");
    if (!(eps > 0.0f) || !(eps < __builtin_inff())) return refuse(fn, "eps must be finite and positive");
    if (hidden != MLP_H) return refuse(fn, "hidden must be 256: the LayerNorm critic has hidden widths (256, 256)", NIG_ERR_UNSUPPORTED);
    if (!launch_of(h->env)->mlp_ln_shield) return refuse(fn, "env shape not supported (even state dim, at most 16 actions)", NIG_ERR_UNSUPPORTED);
    const int S = SPECS[h->env].state_dim, A = SPECS[h->env].action_dim;
    // (the slot's device image has room for either layer-1 form: it is allocated once and reused)
    const size_t floats = LN_STREAM_MAX_FLOATS;
    float *host = (float *)calloc(floats, sizeof(float));
    if (!host) return refuse(fn, "out of host memory");
    if (!put_ln_network(S + A, 1, C1, c1, g1, be1, C2, c2, g2, be2, C3, c3, host, floats)) {
        free(host);
        return refuse(fn, "the operand image does not fit its chunk plan");
    }
    // (the upload overwrites the image an installed LayerNorm critic may be using: after a HIP failure the slot holds no critic)
    const int rc = upload_stream(fn, &h->mlp_cln_stream, host, floats, stream);
    if (rc) { if (ln_critic(h)) h->mlp_ckind = NIG_SAFETY_NONE; return rc; }
    h->mlp_threshold = threshold;
    h->cln_eps = eps;
    h->mlp_ckind = NIG_SAFETY_SIGMOID_LN;
    critic_dims_256(h);
    return NIG_OK;
}

// ---- the safety critic of the other hidden shapes ("nig-mlp-shape-shield-v1", csrc/nig_mlp_shape_shield.hpp) ----
int nig_set_mlp_safety_dims(nig_handle *h, int32_t n_hidden, const int32_t *hidden, const float *const *C, const float *const *c,
                            float threshold, void *stream)
{
    const char *fn = "nig_set_mlp_safety_dims";
    if (!h || !hidden || !C || !c) return refuse(fn, "NULL argument");
    if (n_hidden < 2 || n_hidden > 3) return refuse(fn, "n_hidden outside 2 .. 3");
    int dims[3] = {0, 0, 0};
    for (int l = 0; l < n_hidden; ++l) {
        if (hidden[l] < 1 || hidden[l] > SHAPE_MAX_WIDTH) return refuse(fn, "a hidden width outside 1 .. 512");
        dims[l] = hidden[l];
    }
    for (int l = 0; l <= n_hidden; ++l)
        if (!C[l] || !c[l]) return refuse(fn, "NULL layer");
    if (!launch_of(h->env)->mlp) return refuse(fn, "env shape not supported (even state dim, at most 16 actions)", NIG_ERR_UNSUPPORTED);
    const int IN = SPECS[h->env].state_dim + SPECS[h->env].action_dim;
    const int kind = shape_class_of(n_hidden, dims, (IN + 1) & ~1);
    if (kind == SHAPE_KIND_NONE) return refuse(fn, "no shape class holds these hidden widths");
    auto installed = [&](int ckind) {
        h->mlp_threshold = threshold;
        h->mlp_ckind = ckind;
        h->critic_class = kind; h->critic_nh = n_hidden;
        for (int l = 0; l < 3; ++l) h->critic_dims[l] = dims[l];
        return NIG_OK;
    };
    if (kind == SHAPE_KIND_REFERENCE) {                     // padded to 256 x 256 on the host: nig_set_mlp_safety's image and kernels
        float *pad = (float *)calloc(reference_pad_floats(IN, 1), sizeof(float));
        float *host = (float *)calloc(MLP_CSTREAM_FLOATS, sizeof(float));
        const bool ok = pad && host && put_reference_padded(IN, 1, dims, C, c, pad, host, MLP_CSTREAM_FLOATS);
        free(pad);
        if (!ok) { free(host); return refuse(fn, "out of host memory, or the operand stream does not fit its image"); }
        NIG_TRY(upload_stream(fn, &h->mlp_cstream, host, MLP_CSTREAM_FLOATS, stream));
        return installed(NIG_SAFETY_SIGMOID);
    }
    size_t cap = 0;                                         // the env's largest shaped image: the slot is allocated once
    for (int k = SHAPE_KIND_128; k <= SHAPE_KIND_3; ++k) {
        const size_t f = shape_plan(SHAPE_CLASSES[k], IN).floats();
        cap = f > cap ? f : cap;
    }
    const size_t floats = shape_plan(SHAPE_CLASSES[kind], IN).floats();
    float *host = (float *)calloc(floats, sizeof(float));
    if (!host) return refuse(fn, "out of host memory");
    if (!put_shape_network(SHAPE_CLASSES[kind], IN, 1, n_hidden, dims, C, c, host, floats)) {
        free(host);
        return refuse(fn, "the operand image does not fit its chunk plan");
    }
    if (!h->mlp_cshape_stream) {
        const hipError_t e = hipMalloc((void **)&h->mlp_cshape_stream, cap * sizeof(float));
        if (e != hipSuccess) { h->mlp_cshape_stream = nullptr; free(host); return refuse(fn, hipGetErrorString(e), NIG_ERR_HIP); }
    }
    // (the upload overwrites the image an installed shaped critic may be using: after a HIP failure the slot holds no critic)
    const int rc = upload_stream(fn, &h->mlp_cshape_stream, host, floats, stream);
    if (rc) { if (shaped_critic(h)) h->mlp_ckind = NIG_SAFETY_NONE; return rc; }
    return installed(NIG_SAFETY_SIGMOID_SHAPED);
}

int nig_get_mlp_safety_dims(const nig_handle *h, int32_t *hidden)
{
    if (!h) return -1;
    const int nh = h->mlp_ckind == NIG_SAFETY_NONE ? 0 : h->critic_nh;
    if (hidden)
        for (int l = 0; l < 3; ++l) hidden[l] = l < nh ? h->critic_dims[l] : 0;
    return nh;
}

int nig_get_mlp_safety_kind(const nig_handle *h) { return h ? h->mlp_ckind : -1; }
int nig_get_mlp_safety_atoms(const nig_handle *h) { return h ? (h->mlp_ckind == NIG_SAFETY_CATEGORICAL ? h->cat_atoms : 0) : -1; }

int nig_mlp_violation_prob(nig_handle *h, int64_t n, const float *obs, int64_t ld_obs, const float *act, int64_t ld_act,
                           float *prob_out, float *logit_out, int64_t ld_logit, void *stream)
{
    const char *const fn = "nig_mlp_violation_prob";
    if (!h || !obs || !act || !prob_out) return refuse(fn, "NULL argument");
    NIG_TRY(refuse_ln_critic(h, fn));
    NIG_TRY(refuse_shaped_critic(h, fn));
    if (!categorical(h) || !h->mlp_cstream || !h->mlp_ctail) return refuse(fn, "no categorical critic installed (nig_set_mlp_safety_categorical)");
    if (n < 1) return refuse(fn, "n < 1");
    if (ld_obs < n || ld_obs > NIG_MAX_PITCH || ld_act < n || ld_act > NIG_MAX_PITCH) return refuse(fn, "ld_obs / ld_act outside [n, 2^26]");
    if (logit_out && (ld_logit < n || ld_logit > NIG_MAX_PITCH)) return refuse(fn, "ld_logit outside [n, 2^26]");
    MlpCatEvalArgs q;
    memset(&q, 0, sizeof q);
    // the body's view of a batch: its "state rows" are the caller's observations, read and never written (CAT_EVAL)
    q.sh.m.s.state = const_cast<float *>(obs); q.sh.m.s.ld_state = (uint32_t)ld_obs; q.sh.m.s.B = (uint32_t)n;
    q.sh.cstream = h->mlp_cstream; q.sh.prob_out = prob_out;
    categorical_fields(h, q.c);
    q.c.act = act; q.c.ld_act = (uint32_t)ld_act; q.c.logit_out = logit_out; q.c.ld_logit = (uint32_t)ld_logit;
    launch_of(h->env)->mlp_cat_eval(q, (unsigned)((n + BLOCK / 2 - 1) / (BLOCK / 2)), (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return NIG_OK;
}

int nig_rollout_mlp_safe(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out, int64_t out_stride,
                         float *obs_out, int64_t obs_step_stride, float *act_out, int64_t ld_act, int64_t act_step_stride,
                         float *prob_out, void *stream)
{
    return rollout_mlp_safe<false>(h, "nig_rollout_mlp_safe", n_steps, {CLOSED_LOOP_OUT}, prob_out, stream);
}

int nig_rollout_mlp_safe_limited(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out, int64_t out_stride,
                                 float *obs_out, int64_t obs_step_stride, float *act_out, int64_t ld_act, int64_t act_step_stride,
                                 float *prob_out, uint32_t *xflags_out, void *stream)
{
    return rollout_mlp_safe<true>(h, "nig_rollout_mlp_safe_limited", n_steps, {CLOSED_LOOP_OUT, xflags_out}, prob_out, stream);
}

int nig_rollout_mlp_search(nig_handle *h, int32_t n_steps, int32_t n_candidates, float *reward_out, uint32_t *flags_out, int64_t out_stride,
                           float *obs_out, int64_t obs_step_stride, float *act_out, int64_t ld_act, int64_t act_step_stride,
                           float *prob_out, float *risk_out, int32_t *choice_out, void *stream)
{
    return rollout_mlp_search<false>(h, "nig_rollout_mlp_search", n_steps, n_candidates, {CLOSED_LOOP_OUT}, prob_out, risk_out, choice_out, stream);
}

int nig_rollout_mlp_search_limited(nig_handle *h, int32_t n_steps, int32_t n_candidates, float *reward_out, uint32_t *flags_out, int64_t out_stride,
                                   float *obs_out, int64_t obs_step_stride, float *act_out, int64_t ld_act, int64_t act_step_stride,
                                   float *prob_out, float *risk_out, int32_t *choice_out, uint32_t *xflags_out, void *stream)
{
    return rollout_mlp_search<true>(h, "nig_rollout_mlp_search_limited", n_steps, n_candidates, {CLOSED_LOOP_OUT, xflags_out}, prob_out, risk_out, choice_out, stream);
}

int nig_set_mlp_ensemble(nig_handle *h, int32_t n_members, int32_t hidden, const float *const *W1, const float *const *b1,
                         const float *const *W2, const float *const *b2, const float *const *W3, const float *const *b3,
                         int32_t method, const double *weights, double weight_sum, float uncertainty_threshold, void *stream)
{
    if (!h) return fail(NIG_ERR_INVALID, "nig_set_mlp_ensemble: NULL handle");
    if (n_members < 1 || n_members > NIG_MAX_ENSEMBLE) return fail(NIG_ERR_INVALID, "nig_set_mlp_ensemble: n_members outside 1 .. NIG_MAX_ENSEMBLE");
    if (!W1 || !b1 || !W2 || !b2 || !W3 || !b3) return fail(NIG_ERR_INVALID, "nig_set_mlp_ensemble: NULL member array (W1 / b1 / W2 / b2 / W3 / b3)");
    for (int k = 0; k < n_members; ++k)
        if (!W1[k] || !b1[k] || !W2[k] || !b2[k] || !W3[k] || !b3[k]) return fail(NIG_ERR_INVALID, "nig_set_mlp_ensemble: NULL member array (W1 / b1 / W2 / b2 / W3 / b3 of a member)");
    if (method != NIG_ENSEMBLE_AVERAGE && method != NIG_ENSEMBLE_VOTING) return fail(NIG_ERR_INVALID, "nig_set_mlp_ensemble: unknown method");
    double w[NIG_MAX_ENSEMBLE] = {0};
    if (method == NIG_ENSEMBLE_AVERAGE) {
        if (!weights) return fail(NIG_ERR_INVALID, "nig_set_mlp_ensemble: NULL weights with NIG_ENSEMBLE_AVERAGE");
        for (int k = 0; k < n_members; ++k) {
            if (!std::isfinite(weights[k])) return fail(NIG_ERR_INVALID, "nig_set_mlp_ensemble: non-finite entry of weights");
            w[k] = weights[k];
        }
        if (!std::isfinite(weight_sum)) return fail(NIG_ERR_INVALID, "nig_set_mlp_ensemble: non-finite weight_sum");
        if (weight_sum == 0.0) return fail(NIG_ERR_INVALID, "nig_set_mlp_ensemble: weight_sum is zero (np.average raises)");
    }
    const int S = SPECS[h->env].state_dim, A = SPECS[h->env].action_dim;
    float *host = nullptr;
    NIG_TRY(build_network_images(h, "nig_set_mlp_ensemble", hidden, S, A, MLP_STREAM_FLOATS, n_members, W1, b1, W2, b2, W3, b3, &host));
    h->ens_members = 0;                                     // no ensemble while the streams are being replaced
    if (h->ens_cap < n_members) {                           // too small: upload_stream allocates the new one
        if (h->ens_stream) (void)hipFree(h->ens_stream);
        h->ens_stream = nullptr; h->ens_cap = 0;
    }
    hipError_t e = hipSuccess;                              // the weights first, on the same stream: upload_stream waits for both copies
    if (!h->ens_w) e = hipMalloc((void **)&h->ens_w, sizeof w);
    if (e == hipSuccess) e = hipMemcpyAsync(h->ens_w, w, sizeof w, hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e != hipSuccess) { free(host); return fail(NIG_ERR_HIP, "nig_set_mlp_ensemble: %s", hipGetErrorString(e)); }
    NIG_TRY(upload_stream("nig_set_mlp_ensemble", &h->ens_stream, host, (size_t)n_members * MLP_STREAM_FLOATS, stream));
    if (h->ens_cap == 0) h->ens_cap = n_members;
    h->ens_members = n_members; h->ens_method = method; h->ens_wsum = weight_sum; h->ens_threshold = uncertainty_threshold;
    return NIG_OK;
}

int nig_rollout_mlp_ensemble(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out, int64_t out_stride,
                             float *obs_out, int64_t obs_step_stride, float *act_out, int64_t ld_act, int64_t act_step_stride,
                             float *unc_out, float *member_act_out, void *stream)
{
    return rollout_mlp_ensemble<false>(h, "nig_rollout_mlp_ensemble", n_steps, {CLOSED_LOOP_OUT}, unc_out, member_act_out, stream);
}

int nig_rollout_mlp_ensemble_limited(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out, int64_t out_stride,
                                     float *obs_out, int64_t obs_step_stride, float *act_out, int64_t ld_act, int64_t act_step_stride,
                                     float *unc_out, float *member_act_out, uint32_t *xflags_out, void *stream)
{
    return rollout_mlp_ensemble<true>(h, "nig_rollout_mlp_ensemble_limited", n_steps, {CLOSED_LOOP_OUT, xflags_out}, unc_out, member_act_out, stream);
}

// ---- the safety-ensemble gate ("nig-gate-v1") ------------------------------------------------
int nig_set_mlp_safety_ensemble(nig_handle *h, int32_t n_members, int32_t hidden, int32_t n_outputs,
                                const float *const *C1, const float *const *c1, const float *const *C2, const float *const *c2,
                                const float *const *C3, const float *const *c3, float temperature, float prob_threshold,
                                float uncertainty_threshold, void *stream)
{
    const char *const fn = "nig_set_mlp_safety_ensemble";
    if (!h) return fail(NIG_ERR_INVALID, "nig_set_mlp_safety_ensemble: NULL handle");
    if (n_members < 1 || n_members > NIG_MAX_ENSEMBLE) return refuse(fn, "n_members outside 1 .. NIG_MAX_ENSEMBLE");
    if (n_outputs < 1 || n_outputs > 4) return refuse(fn, "n_outputs outside 1 .. 4");
    if (!C1 || !c1 || !C2 || !c2 || !C3 || !c3) return refuse(fn, "NULL member array (C1 / c1 / C2 / c2 / C3 / c3)");
    for (int k = 0; k < n_members; ++k)
        if (!C1[k] || !c1[k] || !C2[k] || !c2[k] || !C3[k] || !c3[k]) return refuse(fn, "NULL member array (C1 / c1 / C2 / c2 / C3 / c3 of a member)");
    if (!std::isfinite(temperature) || !(temperature > 0.0f)) return refuse(fn, "temperature must be finite and > 0");
    if (prob_threshold != prob_threshold || uncertainty_threshold != uncertainty_threshold) return refuse(fn, "a NaN threshold");
    const int S = SPECS[h->env].state_dim, A = SPECS[h->env].action_dim;
    float *host = nullptr;
    NIG_TRY(build_network_images(h, fn, hidden, S + A, n_outputs, MLP_CSTREAM_FLOATS, n_members, C1, c1, C2, c2, C3, c3, &host));
    h->gate_members = 0;                                    // no gate while the streams are being replaced
    if (h->gate_cap < n_members) {                          // too small: upload_stream allocates the new one
        if (h->gate_stream) (void)hipFree(h->gate_stream);
        h->gate_stream = nullptr; h->gate_cap = 0;
    }
    NIG_TRY(upload_stream(fn, &h->gate_stream, host, (size_t)n_members * MLP_CSTREAM_FLOATS, stream));
    if (h->gate_cap == 0) h->gate_cap = n_members;
    h->gate_members = n_members; h->gate_outputs = n_outputs;
    h->gate_T = temperature; h->gate_thr = prob_threshold; h->gate_umax = uncertainty_threshold;
    return NIG_OK;
}

int nig_rollout_mlp_gated(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out, int64_t out_stride,
                          float *obs_out, int64_t obs_step_stride, float *act_out, int64_t ld_act, int64_t act_step_stride,
                          float *prob_out, float *unc_out, float *logit_out, int64_t ld_c, int64_t c_step_stride, void *stream)
{
    return rollout_mlp_gated<false>(h, "nig_rollout_mlp_gated", n_steps, {CLOSED_LOOP_OUT}, prob_out, unc_out, logit_out, ld_c, c_step_stride, stream);
}

int nig_rollout_mlp_gated_limited(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out, int64_t out_stride,
                                  float *obs_out, int64_t obs_step_stride, float *act_out, int64_t ld_act, int64_t act_step_stride,
                                  float *prob_out, float *unc_out, float *logit_out, int64_t ld_c, int64_t c_step_stride,
                                  uint32_t *xflags_out, void *stream)
{
    return rollout_mlp_gated<true>(h, "nig_rollout_mlp_gated_limited", n_steps, {CLOSED_LOOP_OUT, xflags_out}, prob_out, unc_out, logit_out, ld_c, c_step_stride, stream);
}

// ---- the constraint projection ("nig-project-v1") ------------------------------------------
int nig_set_mlp_constraint(nig_handle *h, int32_t hidden, int32_t n_outputs, const float *C1, const float *c1, const float *C2,
                           const float *c2, const float *C3, const float *c3, float threshold, float tolerance, void *stream)
{
    const char *const fn = "nig_set_mlp_constraint";
    if (!h) return fail(NIG_ERR_INVALID, "nig_set_mlp_constraint: NULL handle");
    if (!C1 || !c1 || !C2 || !c2 || !C3 || !c3) return refuse(fn, "NULL argument (C1 / c1 / C2 / c2 / C3 / c3)");
    if (n_outputs < 1 || n_outputs > 4) return refuse(fn, "n_outputs outside 1 .. 4");
    if (!std::isfinite(threshold) || !std::isfinite(tolerance)) return refuse(fn, "threshold and tolerance must be finite");
    const int S = SPECS[h->env].state_dim, A = SPECS[h->env].action_dim;
    float *fwd = nullptr, *bwd = nullptr;
    NIG_TRY(build_network_images(h, fn, hidden, S + A, n_outputs, MLP_CSTREAM_FLOATS, 1, &C1, &c1, &C2, &c2, &C3, &c3, &fwd));
    // The backward network 4 -> 256 -> 256 -> A: W3^T zero-padded to four input rows, W2^T, W1[S:S+A, :]^T, zero biases -- an image
    // of the same builder, so a backward pass is a forward pass of this stream (nig_mlp.hpp, MlpProjectArgs)
    std::vector<float> T1((size_t)4 * MLP_H, 0.0f), T2((size_t)MLP_H * MLP_H), T3((size_t)MLP_H * A), zero(MLP_H, 0.0f);
    for (int c = 0; c < n_outputs; ++c)
        for (int u = 0; u < MLP_H; ++u) T1[(size_t)c * MLP_H + u] = C3[(size_t)u * n_outputs + c];
    for (int k = 0; k < MLP_H; ++k)
        for (int j = 0; j < MLP_H; ++j) T2[(size_t)j * MLP_H + k] = C2[(size_t)k * MLP_H + j];
    for (int j = 0; j < A; ++j)
        for (int u = 0; u < MLP_H; ++u) T3[(size_t)u * A + j] = C1[(size_t)(S + j) * MLP_H + u];
    const float *t1 = T1.data(), *t2 = T2.data(), *t3 = T3.data(), *z = zero.data();
    if (const int rc = build_network_images(h, fn, hidden, 4, A, MLP_STREAM_FLOATS, 1, &t1, &z, &t2, &z, &t3, &z, &bwd)) {
        free(fwd);
        return rc;
    }
    h->proj_outputs = 0;                                    // no projection while the streams are being replaced
    if (const int rc = upload_stream(fn, &h->proj_cstream, fwd, MLP_CSTREAM_FLOATS, stream)) {
        free(bwd);
        return rc;
    }
    NIG_TRY(upload_stream(fn, &h->proj_bstream, bwd, MLP_STREAM_FLOATS, stream));
    h->proj_outputs = n_outputs; h->proj_thr = threshold; h->proj_tol = tolerance;
    return NIG_OK;
}

int nig_rollout_mlp_projected(nig_handle *h, int32_t n_steps, int32_t max_iters, float step, float *reward_out, uint32_t *flags_out,
                              int64_t out_stride, float *obs_out, int64_t obs_step_stride, float *act_out, int64_t ld_act,
                              int64_t act_step_stride, float *prob_out, float *viol_out, int32_t *iters_out, float *grad_out,
                              int64_t ld_c, int64_t c_step_stride, void *stream)
{
    return rollout_mlp_projected<false>(h, "nig_rollout_mlp_projected", n_steps, max_iters, step, {CLOSED_LOOP_OUT}, prob_out, viol_out, iters_out, grad_out, ld_c, c_step_stride, stream);
}

int nig_rollout_mlp_projected_limited(nig_handle *h, int32_t n_steps, int32_t max_iters, float step, float *reward_out, uint32_t *flags_out,
                                      int64_t out_stride, float *obs_out, int64_t obs_step_stride, float *act_out, int64_t ld_act,
                                      int64_t act_step_stride, float *prob_out, float *viol_out, int32_t *iters_out, float *grad_out,
                                      int64_t ld_c, int64_t c_step_stride, uint32_t *xflags_out, void *stream)
{
    return rollout_mlp_projected<true>(h, "nig_rollout_mlp_projected_limited", n_steps, max_iters, step, {CLOSED_LOOP_OUT, xflags_out}, prob_out, viol_out, iters_out, grad_out, ld_c, c_step_stride, stream);
}

// ---- sensor / actuator noise in the closed loop ("nig-disturb-v1") --------------------------
int nig_set_disturbance(nig_handle *h, const nig_disturbance *d, void * /*stream*/)
{
    if (!h) return fail(NIG_ERR_INVALID, "nig_set_disturbance: NULL handle");
    if (!d) { h->has_dist = false; return NIG_OK; }
    NIG_TRY(check_disturbance(h, "nig_set_disturbance", *d));
    h->dist = *d;                                  // (travels in the kernel arguments: no device copy, nothing to wait for)
    h->has_dist = true;
    return NIG_OK;
}

int nig_rollout_policy_disturbed(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out, int64_t out_stride,
                                 float *obs_out, int64_t obs_step_stride, float *act_out, int64_t ld_act,
                                 int64_t act_step_stride, float *seen_out, int64_t seen_step_stride, void *stream)
{
    return rollout_policy_disturbed<false>(h, "nig_rollout_policy_disturbed", n_steps, {CLOSED_LOOP_OUT}, seen_out, seen_step_stride, stream);
}

int nig_rollout_policy_disturbed_limited(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out, int64_t out_stride,
                                         float *obs_out, int64_t obs_step_stride, float *act_out, int64_t ld_act,
                                         int64_t act_step_stride, float *seen_out, int64_t seen_step_stride, uint32_t *xflags_out, void *stream)
{
    return rollout_policy_disturbed<true>(h, "nig_rollout_policy_disturbed_limited", n_steps, {CLOSED_LOOP_OUT, xflags_out}, seen_out, seen_step_stride, stream);
}

int nig_rollout_mlp_disturbed(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out, int64_t out_stride,
                              float *obs_out, int64_t obs_step_stride, float *act_out, int64_t ld_act,
                              int64_t act_step_stride, float *seen_out, int64_t seen_step_stride, void *stream)
{
    return rollout_mlp_disturbed<false>(h, "nig_rollout_mlp_disturbed", n_steps, {CLOSED_LOOP_OUT}, seen_out, seen_step_stride, stream);
}

int nig_rollout_mlp_disturbed_limited(nig_handle *h, int32_t n_steps, float *reward_out, uint32_t *flags_out, int64_t out_stride,
                                      float *obs_out, int64_t obs_step_stride, float *act_out, int64_t ld_act,
                                      int64_t act_step_stride, float *seen_out, int64_t seen_step_stride, uint32_t *xflags_out, void *stream)
{
    return rollout_mlp_disturbed<true>(h, "nig_rollout_mlp_disturbed_limited", n_steps, {CLOSED_LOOP_OUT, xflags_out}, seen_out, seen_step_stride, stream);
}

// ---- host-buffer entry points (small batches) -------------------------------------------------
// staging layout (same on host and device): [actions f32 A*B][noise f64 K*B] | [state f32 S*B][reward64 f64 B][flags u32 B]
// (uploads = the first part, downloads = the second part: one memcpy each way)
struct HostStage { size_t off_act, off_noise, off_state, off_rew, off_flags, bytes; };

static HostStage host_stage_layout(const nig_handle *h)
{
    const nig_env_spec &sp = SPECS[h->env];
    const size_t B = (size_t)h->B;
    const size_t K = (size_t)(sp.k_step > sp.k_reset ? sp.k_step : sp.k_reset);
    HostStage L;
    L.off_act = 0;
    L.off_noise = (size_t)align_up((int64_t)(sp.action_dim * B * 8), 256);     // float32 or float64 action rows
    L.off_state = L.off_noise + (size_t)align_up((int64_t)(K * B * 8), 256);
    L.off_rew = L.off_state + (size_t)align_up((int64_t)(sp.state_dim * B * 4), 256);
    L.off_flags = L.off_rew + (size_t)align_up((int64_t)(B * 8), 256);
    L.bytes = L.off_flags + (size_t)align_up((int64_t)(B * 4), 256);
    return L;
}

constexpr int64_t HOST_ZERO_COPY_MAX = 1024;   // lanes up to which the host-buffer entry points skip the staging copies

static int host_stage_ensure(nig_handle *h, const HostStage &L)
{
    if (h->hst_pinned && h->hst_bytes >= L.bytes) return NIG_OK;
    if (h->B > 65536) return fail(NIG_ERR_UNSUPPORTED, "host-buffer entry points are for small batches (<= 65536 lanes)");
    if (h->hst_dev) { (void)hipFree(h->hst_dev); h->hst_dev = nullptr; }
    if (h->hst_pinned) { (void)hipHostFree(h->hst_pinned); h->hst_pinned = nullptr; }
    HIP_TRY(hipHostMalloc((void **)&h->hst_pinned, L.bytes, hipHostMallocDefault));
    HIP_TRY(hipMalloc((void **)&h->hst_dev, L.bytes));
    h->hst_bytes = L.bytes;
    return NIG_OK;
}

int nig_reset_host(nig_handle *h, const double *init_noise, float *state_out, void *stream)
{
    if (!h || !state_out) return fail(NIG_ERR_INVALID, "nig_reset_host: NULL argument");
    const nig_env_spec &sp = SPECS[h->env];
    const HostStage L = host_stage_layout(h);
    NIG_TRY(host_stage_ensure(h, L));
    hipStream_t st = (hipStream_t)stream;
    const size_t B = (size_t)h->B;
    const double *dn = nullptr;
    if (init_noise && sp.k_reset > 0) {
        memcpy(h->hst_pinned + L.off_noise, init_noise, (size_t)sp.k_reset * B * 8);
        HIP_TRY(hipMemcpyAsync(h->hst_dev + L.off_noise, h->hst_pinned + L.off_noise, (size_t)sp.k_reset * B * 8, hipMemcpyHostToDevice, st));
        dn = (const double *)(h->hst_dev + L.off_noise);
    }
    NIG_TRY(nig_reset(h, nullptr, dn, (int64_t)B, stream));
    // gather the rows (ld apart on the device) into the contiguous staging image, then ONE download
    hipLaunchKernelGGL(copy_rows_kernel, dim3(grid_for(h->B)), dim3(BLOCK), 0, st, (const float *)h->state, h->ld_state,
                       (float *)(h->hst_dev + L.off_state), (int64_t)B, sp.state_dim, h->B);
    HIP_TRY(hipMemcpyAsync(h->hst_pinned + L.off_state, h->hst_dev + L.off_state, (size_t)sp.state_dim * B * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(state_out, h->hst_pinned + L.off_state, (size_t)sp.state_dim * B * 4);
    return NIG_OK;
}

static int step_host_impl(nig_handle *h, const void *actions, bool act64, const double *step_noise, float *state_out,
                          double *reward64_out, uint32_t *flags_out, void *stream);

int nig_step_host(nig_handle *h, const float *actions, const double *step_noise, float *state_out, double *reward64_out,
                  uint32_t *flags_out, void *stream)
{
    return step_host_impl(h, actions, false, step_noise, state_out, reward64_out, flags_out, stream);
}

int nig_step_host64(nig_handle *h, const double *actions, const double *step_noise, float *state_out, double *reward64_out,
                    uint32_t *flags_out, void *stream)
{
    return step_host_impl(h, actions, true, step_noise, state_out, reward64_out, flags_out, stream);
}

static int step_host_impl(nig_handle *h, const void *actions, bool act64, const double *step_noise, float *state_out,
                          double *reward64_out, uint32_t *flags_out, void *stream)
{
    if (!h || !actions || !state_out || !reward64_out || !flags_out) return fail(NIG_ERR_INVALID, "nig_step_host: NULL argument");
    NIG_TRY(refuse_limited(h, "nig_step_host"));
    const nig_env_spec &sp = SPECS[h->env];
    const HostStage L = host_stage_layout(h);
    NIG_TRY(host_stage_ensure(h, L));
    hipStream_t st = (hipStream_t)stream;
    const size_t B = (size_t)h->B;
    const size_t act_bytes = (size_t)sp.action_dim * B * (act64 ? 8 : 4);
    memcpy(h->hst_pinned + L.off_act, actions, act_bytes);
    size_t up = act_bytes;
    const double *dn = nullptr;
    if (step_noise && sp.k_step > 0) {
        memcpy(h->hst_pinned + L.off_noise, step_noise, (size_t)sp.k_step * B * 8);
        up = L.off_noise + (size_t)sp.k_step * B * 8;          // one contiguous upload covers both
        dn = (const double *)(h->hst_dev + L.off_noise);
    }
    // Small batches (the single-env drop-in class is B = 1): the kernels read the actions / noise from, and
    // write state / reward / flags to, the pinned staging buffer itself -- hipHostMalloc memory is mapped
    // and coherent, a few hundred bytes over PCIe cost less than two copy commands -- so a step is two
    // kernel launches and one stream sync.  Larger batches keep one upload + one download.
    const bool zero_copy = h->B <= HOST_ZERO_COPY_MAX;
    char *io = zero_copy ? h->hst_pinned : h->hst_dev;
    if (!zero_copy) HIP_TRY(hipMemcpyAsync(h->hst_dev, h->hst_pinned, up, hipMemcpyHostToDevice, st));
    if (dn) dn = (const double *)(io + L.off_noise);
    h->mirror = (float *)(io + L.off_state); h->ld_mirror = (uint32_t)B;
    const int rc = act64 ? nig_step64(h, (const double *)(io + L.off_act), (int64_t)B, dn, nullptr, (int64_t)B, nullptr,
                                      (double *)(io + L.off_rew), (uint32_t *)(io + L.off_flags), nullptr, 0, stream)
                         : nig_step(h, (const float *)(io + L.off_act), (int64_t)B, dn, nullptr, (int64_t)B, nullptr,
                                    (double *)(io + L.off_rew), (uint32_t *)(io + L.off_flags), nullptr, 0, stream);
    h->mirror = nullptr;
    if (rc != NIG_OK) return rc;
    // (the state rows land next to reward64 and flags -- one download for everything the call returns -- written by the step
    // kernel itself: StepArgs::mirror.  Until round 4 a row-gather kernel was launched behind every step for them.)
    if (!zero_copy) HIP_TRY(hipMemcpyAsync(h->hst_pinned + L.off_state, h->hst_dev + L.off_state, L.bytes - L.off_state, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(state_out, h->hst_pinned + L.off_state, (size_t)sp.state_dim * B * 4);
    memcpy(reward64_out, h->hst_pinned + L.off_rew, B * 8);
    memcpy(flags_out, h->hst_pinned + L.off_flags, B * 4);
    return NIG_OK;
}

int nig_plan_create(nig_handle *h, int32_t n_steps, const float *action_ring, int64_t ld_act, int64_t slot_stride,
                    int32_t ring_len, float *reward_out, uint32_t *flags_out, int64_t out_stride, nig_plan **out)
{
    if (!out) return fail(NIG_ERR_INVALID, "nig_plan_create: out is NULL");
    *out = nullptr;
    if (!h || !action_ring || n_steps <= 0 || ring_len <= 0 || ld_act < h->B || ld_act > NIG_MAX_PITCH)
        return fail(NIG_ERR_INVALID, "nig_plan_create: bad argument");
    NIG_TRY(refuse_limited(h, "nig_plan_create"));
    if (slot_stride < (int64_t)SPECS[h->env].action_dim * ld_act)
        return fail(NIG_ERR_INVALID, "nig_plan_create: slot_stride smaller than one [A][ld_act] slot");
    if (out_stride != 0 && out_stride < h->B) return fail(NIG_ERR_INVALID, "nig_plan_create: out_stride < batch");
    nig_plan *p = new (std::nothrow) nig_plan();
    if (!p) return fail(NIG_ERR_INVALID, "nig_plan_create: out of host memory");
    p->h = h; p->n_steps = n_steps; p->graph = nullptr; p->exec = nullptr;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t cs = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);
    if (e != hipSuccess) { delete p; return fail(NIG_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
    e = hipStreamBeginCapture(cs, hipStreamCaptureModeRelaxed);
    if (e == hipSuccess) {
        for (int k = 0; k < n_steps; ++k) {
            StepArgs a = base_step_args(h);
            const int slot = k % ring_len;
            a.actions = action_ring + (int64_t)slot * slot_stride; a.ld_act = (uint32_t)ld_act;
            a.reward = reward_out ? reward_out + (int64_t)slot * out_stride : nullptr;
            a.flags = flags_out ? flags_out + (int64_t)slot * out_stride : nullptr;
            a.t_ptr = h->t_dev; a.t_off = (uint32_t)(k + 1);
            dispatch_step(h, a, false, cs);
        }
        e = hipStreamEndCapture(cs, &p->graph);
    }
    if (e == hipSuccess) e = hipGraphInstantiate(&p->exec, p->graph, nullptr, nullptr, 0);
    (void)hipStreamDestroy(cs);
    if (e != hipSuccess) {
        if (p->graph) (void)hipGraphDestroy(p->graph);
        delete p;
        return fail(NIG_ERR_HIP, "nig_plan_create: graph capture failed: %s", hipGetErrorString(e));
    }
    *out = p;
    return NIG_OK;
}

int nig_plan_launch(nig_plan *p, void *stream)
{
    if (!p) return fail(NIG_ERR_INVALID, "nig_plan_launch: NULL plan");
    NIG_TRY(refuse_limited(p->h, "nig_plan_launch"));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(set_u32_kernel, dim3(1), dim3(1), 0, st, p->h->t_dev, p->h->t);
    HIP_TRY(hipGraphLaunch(p->exec, st));
    p->h->t += (uint32_t)p->n_steps;
    return NIG_OK;
}

int nig_plan_destroy(nig_plan *p)
{
    if (!p) return NIG_OK;
    if (p->exec) (void)hipGraphExecDestroy(p->exec);
    if (p->graph) (void)hipGraphDestroy(p->graph);
    delete p;
    return NIG_OK;
}

// ---- mixed batch -------------------------------------------------------------------------------
struct nig_mixed {
    int n = 0;
    int device = 0;
    nig_handle *seg[NIG_MIXED_MAX_SEGMENTS] = {};
    int64_t off[NIG_MIXED_MAX_SEGMENTS] = {};
    int64_t ld = 0, lanes = 0;
    int s_max = 0, a_max = 0;
    float *state = nullptr;    // [s_max][ld], owned
};

// relative cost of one env-step (fused rollout, measured per-env rates): launch order = most expensive first.  (Round 4,
// profiles/r04/mixed_order.txt: PowerGrid before RobotAssembly or after makes no difference, 2.69 vs 2.70 ms; the cheap
// envs first costs +10 %, RobotAssembly last +13 %.)
static int env_cost(int env)
{
    static const int C[NIG_NUM_ENVS] = {10, 44, 50, 15, 20, 14, 9, 17, 29};
    return C[env];
}

int nig_rollout_mixed(nig_handle *const *handles, const int64_t *lane_offsets, int32_t n_handles, int32_t n_steps,
                      const float *action_ring, int64_t ld_act, int64_t slot_stride, int32_t ring_len,
                      float *reward_out, uint32_t *flags_out, int64_t out_stride, void *stream)
{
    return nig_rollout_mixed_obs(handles, lane_offsets, n_handles, n_steps, action_ring, ld_act, slot_stride, ring_len, reward_out,
                                 flags_out, out_stride, nullptr, 0, 0, stream);
}

int nig_rollout_mixed_obs(nig_handle *const *handles, const int64_t *lane_offsets, int32_t n_handles, int32_t n_steps,
                          const float *action_ring, int64_t ld_act, int64_t slot_stride, int32_t ring_len,
                          float *reward_out, uint32_t *flags_out, int64_t out_stride,
                          float *obs_out, int64_t ld_obs, int64_t obs_step_stride, void *stream)
{
    if (!handles || !lane_offsets || n_handles <= 0 || n_handles > NIG_MIXED_MAX_SEGMENTS)
        return fail(NIG_ERR_INVALID, "nig_rollout_mixed: 1..12 handles");
    const char *const fn = "nig_rollout_mixed";
    if (!action_ring || n_steps <= 0 || ring_len <= 0) return refuse(fn, "bad argument");
    NIG_TRY(check_reward_flags(fn, reward_out, flags_out));
    if (ld_act <= 0 || ld_act > NIG_MAX_PITCH || slot_stride > 0xffffffffLL)
        return fail(NIG_ERR_INVALID, "nig_rollout_mixed: ld_act outside [1, 2^26] or slot_stride >= 2^32");
    if (out_stride != 0 && out_stride > NIG_MAX_PITCH) return fail(NIG_ERR_INVALID, "nig_rollout_mixed: out_stride > 2^26");
    NIG_TRY(check_out_span(fn, n_steps, out_stride));      // (no lower bound on out_stride here: the segments' fit, below)
    if (obs_out && !reward_out) return fail(NIG_ERR_INVALID, "nig_rollout_mixed: an observation trajectory needs reward_out and flags_out too");
    if (obs_out && (ld_obs <= 0 || ld_obs > NIG_MAX_PITCH)) return fail(NIG_ERR_INVALID, "nig_rollout_mixed: ld_obs outside [1, 2^26]");
    int order[NIG_MIXED_MAX_SEGMENTS];
    int a_max = 0, s_max = 0;
    for (int k = 0; k < n_handles; ++k) {
        const nig_handle *h = handles[k];
        if (!h) return fail(NIG_ERR_INVALID, "nig_rollout_mixed: NULL handle");
        NIG_TRY(refuse_limited(h, fn));
        if (h->device != handles[0]->device) return fail(NIG_ERR_INVALID, "nig_rollout_mixed: handles on different devices");
        if (lane_offsets[k] < 0 || lane_offsets[k] + h->B > ld_act || (out_stride != 0 && lane_offsets[k] + h->B > out_stride))
            return fail(NIG_ERR_INVALID, "nig_rollout_mixed: a segment does not fit the row pitch");
        NIG_TRY(check_counter(h, fn, n_steps));
        if (SPECS[h->env].action_dim > a_max) a_max = SPECS[h->env].action_dim;
        if (SPECS[h->env].state_dim > s_max) s_max = SPECS[h->env].state_dim;
        if (obs_out && lane_offsets[k] + h->B > ld_obs) return fail(NIG_ERR_INVALID, "nig_rollout_mixed: a segment does not fit ld_obs");
        order[k] = k;
    }
    if (obs_out && obs_step_stride != 0 && obs_step_stride < (int64_t)s_max * ld_obs)
        return fail(NIG_ERR_INVALID, "nig_rollout_mixed: obs_step_stride smaller than one [S_max][ld_obs] step");
    if (slot_stride < (int64_t)a_max * ld_act) return fail(NIG_ERR_INVALID, "nig_rollout_mixed: slot_stride smaller than one [A_max][ld_act] slot");
    for (int i = 1; i < n_handles; ++i)           // insertion sort: most expensive env first, ties in segment order
        for (int j = i; j > 0 && env_cost(handles[order[j]]->env) > env_cost(handles[order[j - 1]]->env); --j) {
            const int tmp = order[j]; order[j] = order[j - 1]; order[j - 1] = tmp;
        }
    MixedArgs m;
    memset(&m, 0, sizeof m);
    m.n_seg = n_handles;
    const RolloutSpec c = {n_steps, action_ring, ld_act, slot_stride, ring_len, nullptr, 0, nullptr, 0, 0, reward_out, flags_out, out_stride,
                           obs_out, obs_out ? ld_obs : 0, obs_out ? obs_step_stride : 0, false};
    uint32_t blocks = 0;
    for (int i = 0; i < n_handles; ++i) {
        const nig_handle *h = handles[order[i]];
        m.seg[i] = rollout_args(h, c, lane_offsets[order[i]]);
        blocks += grid_for(h->B);
        m.blk_end[i] = blocks;
        m.env[i] = h->env;
    }
    HIP_TRY(hipSetDevice(handles[0]->device));
    nig_launch_mixed_rollout(!reward_out ? 0 : (obs_out ? 2 : 1), m, blocks, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    for (int k = 0; k < n_handles; ++k) handles[k]->t += (uint32_t)n_steps;
    return NIG_OK;
}

int nig_create_mixed(int32_t n_segments, const int32_t *env_ids, const int64_t *counts, int device, uint64_t seed,
                     uint64_t env_index0, uint32_t flags, nig_mixed **out)
{
    if (!out) return fail(NIG_ERR_INVALID, "nig_create_mixed: out is NULL");
    *out = nullptr;
    if (!env_ids || !counts || n_segments <= 0 || n_segments > NIG_MIXED_MAX_SEGMENTS)
        return fail(NIG_ERR_INVALID, "nig_create_mixed: 1..12 segments");
    nig_mixed *m = new (std::nothrow) nig_mixed();
    if (!m) return fail(NIG_ERR_INVALID, "nig_create_mixed: out of host memory");
    m->n = n_segments; m->device = device;
    int64_t off = 0;
    for (int k = 0; k < n_segments; ++k) {
        if (env_ids[k] < 0 || env_ids[k] >= NIG_NUM_ENVS || counts[k] <= 0 || counts[k] > NIG_MAX_BATCH) {
            delete m;
            return fail(NIG_ERR_INVALID, "nig_create_mixed: bad env id or lane count");
        }
        m->off[k] = off;
        off += align_up(counts[k], BLOCK);            // every segment starts on a block boundary
        m->lanes += counts[k];
        if (SPECS[env_ids[k]].state_dim > m->s_max) m->s_max = SPECS[env_ids[k]].state_dim;
        if (SPECS[env_ids[k]].action_dim > m->a_max) m->a_max = SPECS[env_ids[k]].action_dim;
    }
    m->ld = off;
    if (m->ld > NIG_MAX_PITCH) { delete m; return fail(NIG_ERR_INVALID, "nig_create_mixed: more than 2^26 columns"); }
    int rc = NIG_OK;
    for (int k = 0; k < n_segments && rc == NIG_OK; ++k)
        rc = nig_create(env_ids[k], counts[k], device, seed, env_index0 + (uint64_t)m->off[k], 0, 0.0, flags, nullptr, &m->seg[k]);
    if (rc == NIG_OK) {
        const size_t bytes = (size_t)m->s_max * m->ld * sizeof(float);
        hipError_t e = hipMalloc((void **)&m->state, bytes);
        if (e == hipSuccess) e = hipMemset(m->state, 0, bytes);      // rows >= S of a segment stay zero
        if (e != hipSuccess) rc = fail(NIG_ERR_HIP, "nig_create_mixed: state matrix: %s", hipGetErrorString(e));
    }
    for (int k = 0; k < n_segments && rc == NIG_OK; ++k) rc = nig_bind_state(m->seg[k], m->state + m->off[k], m->ld);
    if (rc != NIG_OK) { nig_mixed_destroy(m); return rc; }
    *out = m;
    return NIG_OK;
}

int nig_mixed_destroy(nig_mixed *m)
{
    if (!m) return NIG_OK;
    for (int k = 0; k < m->n; ++k) nig_destroy(m->seg[k]);
    if (m->state) (void)hipFree(m->state);
    delete m;
    return NIG_OK;
}

int nig_mixed_get_info(const nig_mixed *m, nig_mixed_info *out)
{
    if (!m || !out) return fail(NIG_ERR_INVALID, "nig_mixed_get_info: NULL argument");
    memset(out, 0, sizeof *out);
    out->n_segments = m->n; out->state_dim_max = m->s_max; out->action_dim_max = m->a_max;
    out->lanes = m->lanes; out->ld = m->ld;
    for (int k = 0; k < m->n; ++k) { out->env[k] = m->seg[k]->env; out->offset[k] = m->off[k]; out->count[k] = m->seg[k]->B; }
    return NIG_OK;
}

float *nig_mixed_state(const nig_mixed *m) { return m ? m->state : nullptr; }

nig_handle *nig_mixed_segment(const nig_mixed *m, int32_t k) { return (m && k >= 0 && k < m->n) ? m->seg[k] : nullptr; }

int nig_mixed_reset(nig_mixed *m, void *stream)
{
    if (!m) return fail(NIG_ERR_INVALID, "nig_mixed_reset: NULL handle");
    for (int k = 0; k < m->n; ++k) {
        NIG_TRY(nig_reset(m->seg[k], nullptr, nullptr, 0, stream));
    }
    return NIG_OK;
}

int nig_mixed_fill_actions(nig_mixed *m, uint32_t t, float *actions, void *stream)
{
    if (!m || !actions) return fail(NIG_ERR_INVALID, "nig_mixed_fill_actions: NULL argument");
    for (int k = 0; k < m->n; ++k) {
        NIG_TRY(nig_fill_actions(m->seg[k], t, actions + m->off[k], m->ld, stream));
    }
    return NIG_OK;
}

int nig_mixed_step(nig_mixed *m, const float *actions, float *reward_out, uint32_t *flags_out, void *stream)
{
    if (!m || !actions) return fail(NIG_ERR_INVALID, "nig_mixed_step: NULL argument");
    for (int k = 0; k < m->n; ++k) NIG_TRY(refuse_limited(m->seg[k], "nig_mixed_step"));      // (before any segment steps)
    for (int k = 0; k < m->n; ++k) {              // one step kernel per segment (each its own env type), same stream
        const int64_t o = m->off[k];
        NIG_TRY(nig_step(m->seg[k], actions + o, m->ld, nullptr, nullptr, 0, reward_out ? reward_out + o : nullptr, nullptr,
                                flags_out ? flags_out + o : nullptr, nullptr, 0, stream));
    }
    return NIG_OK;
}

int nig_mixed_rollout(nig_mixed *m, int32_t n_steps, const float *action_ring, int64_t slot_stride, int32_t ring_len,
                      float *reward_out, uint32_t *flags_out, int64_t out_stride, void *stream)
{
    if (!m) return fail(NIG_ERR_INVALID, "nig_mixed_rollout: NULL handle");
    return nig_rollout_mixed(m->seg, m->off, m->n, n_steps, action_ring, m->ld, slot_stride, ring_len, reward_out, flags_out,
                             out_stride, stream);
}

int nig_mixed_rollout_obs(nig_mixed *m, int32_t n_steps, const float *action_ring, int64_t slot_stride, int32_t ring_len,
                          float *reward_out, uint32_t *flags_out, int64_t out_stride, float *obs_out, int64_t obs_step_stride,
                          void *stream)
{
    if (!m) return fail(NIG_ERR_INVALID, "nig_mixed_rollout_obs: NULL handle");
    return nig_rollout_mixed_obs(m->seg, m->off, m->n, n_steps, action_ring, m->ld, slot_stride, ring_len, reward_out, flags_out,
                                 out_stride, obs_out, m->ld, obs_step_stride, stream);
}

// ---- the path's one collective: all-gather of the partial tallies over RCCL ----------------------
// RCCL is resolved at run time from whatever copy the process already holds (a PyTorch process has its own
// librccl.so; a plain C host links or loads /opt/rocm/lib/librccl.so): a communicator is only meaningful to the
// library instance that created it, so libnig.so must not bring a second one.
typedef int (*nccl_allgather_fn)(const void *, void *, size_t, int, void *, hipStream_t);
typedef int (*nccl_count_fn)(void *, int *);
static bool rccl_resolve(nccl_allgather_fn *ag, nccl_count_fn *cnt)
{
    static nccl_allgather_fn s_ag = nullptr;
    static nccl_count_fn s_cnt = nullptr;
    if (!s_ag) {
        void *f = dlsym(RTLD_DEFAULT, "ncclAllGather"), *c = dlsym(RTLD_DEFAULT, "ncclCommCount");
        if (!f || !c) {
            void *lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
            if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
            if (lib) { f = dlsym(lib, "ncclAllGather"); c = dlsym(lib, "ncclCommCount"); }
        }
        s_ag = (nccl_allgather_fn)f; s_cnt = (nccl_count_fn)c;
    }
    *ag = s_ag; *cnt = s_cnt;
    return s_ag && s_cnt;
}

int nig_reduce_metrics(nig_handle *const *handles, int32_t n_handles, void *comm, double *scratch, int64_t scratch_doubles,
                       double *out, void *stream)
{
    if (!handles || n_handles <= 0 || !scratch || !out) return fail(NIG_ERR_INVALID, "nig_reduce_metrics: NULL argument");
    int world = 1;
    nccl_allgather_fn allgather = nullptr;
    nccl_count_fn count = nullptr;
    if (comm) {
        if (!rccl_resolve(&allgather, &count)) return fail(NIG_ERR_UNSUPPORTED, "nig_reduce_metrics: RCCL (librccl.so) not found in this process");
        if (count(comm, &world) != 0 || world <= 0) return fail(NIG_ERR_INVALID, "nig_reduce_metrics: ncclCommCount failed");
    }
    // scratch: [n_handles][ROWS] local partials | [ROWS] this rank's partial | [world][ROWS] gathered
    const int64_t need = ((int64_t)n_handles + 1 + world) * NIG_T_ROWS;
    if (scratch_doubles < need) return fail(NIG_ERR_INVALID, "nig_reduce_metrics: scratch smaller than (n_handles + 1 + ranks) * NIG_T_ROWS doubles");
    hipStream_t st = (hipStream_t)stream;
    double *local = scratch, *mine = scratch + (int64_t)n_handles * NIG_T_ROWS, *all = mine + NIG_T_ROWS;
    for (int k = 0; k < n_handles; ++k) {
        NIG_TRY(nig_reduce_tally(handles[k], local + (int64_t)k * NIG_T_ROWS, stream));
    }
    hipLaunchKernelGGL(combine_partials_kernel, dim3(1), dim3(64), 0, st, (const double *)local, n_handles, mine);
    if (comm) {
        // ncclAllGather (RCCL; over xGMI between the GPUs of a node): NIG_T_ROWS doubles per rank, rank order
        if (allgather(mine, all, (size_t)NIG_T_ROWS, /*ncclDouble*/ 8, comm, st) != 0)
            return fail(NIG_ERR_HIP, "nig_reduce_metrics: ncclAllGather failed");
        hipLaunchKernelGGL(combine_partials_kernel, dim3(1), dim3(64), 0, st, (const double *)all, world, out);
    } else {
        hipLaunchKernelGGL(combine_partials_kernel, dim3(1), dim3(64), 0, st, (const double *)mine, 1, out);
    }
    HIP_TRY(hipGetLastError());
    return NIG_OK;
}

int nig_fill_actions(nig_handle *h, uint32_t t, float *actions, int64_t ld_act, void *stream)
{
    if (!h || !actions || ld_act < h->B) return fail(NIG_ERR_INVALID, "nig_fill_actions: bad argument");
    hipStream_t st = (hipStream_t)stream;
    const uint32_t lo = (uint32_t)h->seed, hi = (uint32_t)(h->seed >> 32);
    launch_of(h->env)->fill(actions, ld_act, h->B, h->env0, lo, hi, t, grid_for(h->B), st);
    HIP_TRY(hipGetLastError());
    return NIG_OK;
}

int nig_set_state(nig_handle *h, const float *state, int64_t ld, const uint32_t *ctr, void *stream)
{
    if (!h) return fail(NIG_ERR_INVALID, "nig_set_state: NULL handle");
    hipStream_t st = (hipStream_t)stream;
    if (state) {
        if (ld < h->B) return fail(NIG_ERR_INVALID, "nig_set_state: ld < batch");
        hipLaunchKernelGGL(copy_rows_kernel, dim3(grid_for(h->B)), dim3(BLOCK), 0, st, state, ld,
                           h->state, h->ld_state, SPECS[h->env].state_dim, h->B);
        HIP_TRY(hipGetLastError());
    }
    if (ctr) {
        HIP_TRY(hipMemcpyAsync(ws_ctr(h), ctr, (size_t)h->B * 4, hipMemcpyDeviceToDevice, st));
        h->may_hold_done = true;                  // the caller's counter words may mark lanes done
    }
    return NIG_OK;
}

int nig_get_state(nig_handle *h, float *state, int64_t ld, uint32_t *ctr, void *stream)
{
    if (!h) return fail(NIG_ERR_INVALID, "nig_get_state: NULL handle");
    hipStream_t st = (hipStream_t)stream;
    if (state) {
        if (ld < h->B) return fail(NIG_ERR_INVALID, "nig_get_state: ld < batch");
        hipLaunchKernelGGL(copy_rows_kernel, dim3(grid_for(h->B)), dim3(BLOCK), 0, st,
                           (const float *)h->state, h->ld_state, state, ld, SPECS[h->env].state_dim, h->B);
        HIP_TRY(hipGetLastError());
    }
    if (ctr) HIP_TRY(hipMemcpyAsync(ctr, ws_ctr(h), (size_t)h->B * 4, hipMemcpyDeviceToDevice, st));
    return NIG_OK;
}

int nig_get_safety_metrics(nig_handle *h, const uint32_t *flags, int32_t *out, int64_t ld_out, void *stream)
{
    if (!h || !flags || !out || ld_out < h->B) return fail(NIG_ERR_INVALID, "nig_get_safety_metrics: bad argument");
    hipLaunchKernelGGL(safety_metrics_kernel, dim3(grid_for(h->B)), dim3(BLOCK), 0, (hipStream_t)stream, flags, out, ld_out, h->B,
                       enabled_constraints(h));
    HIP_TRY(hipGetLastError());
    return NIG_OK;
}

int nig_reduce_tally(nig_handle *h, double *partial_out, void *stream)
{
    if (!h || !partial_out) return fail(NIG_ERR_INVALID, "nig_reduce_tally: NULL argument");
    if (h->lay.off_tally < 0) return fail(NIG_ERR_INVALID, "nig_reduce_tally: handle created without NIG_F_TALLY");
    hipStream_t st = (hipStream_t)stream;
    int nblk = (int)((h->B + BLOCK - 1) / BLOCK);
    if (nblk > REDUCE_BLOCKS) nblk = REDUCE_BLOCKS;
    hipLaunchKernelGGL(reduce_tally_stage1, dim3(nblk), dim3(BLOCK), 0, st, (const double *)ws_tally(h), h->lay.ld, h->B, h->scratch);
    hipLaunchKernelGGL(reduce_tally_stage2, dim3(1), dim3(REDUCE_BLOCKS), 0, st, (const double *)h->scratch, nblk, partial_out);
    HIP_TRY(hipGetLastError());
    return NIG_OK;
}

// ---- per-episode records from reward / flag rows (csrc/nig_episodes.hpp) ------------------------------------------------------
// The shape of a log: what nig_episode_log_query refuses, every entry point refuses
static int check_episode_log_shape(const char *fn, int64_t batch, int64_t capacity, int64_t ld)
{
    if (batch <= 0 || batch > NIG_MAX_BATCH) return refuse(fn, "batch outside [1, 2^24]");
    if (capacity < 1 || capacity > NIG_MAX_EPISODE_CAPACITY) return refuse(fn, "capacity outside [1, 2^20]");
    if (ld != 0 && (ld < batch || ld > NIG_MAX_PITCH)) return refuse(fn, "ld outside {0} U [batch, 2^26]");
    return NIG_OK;
}

int nig_episode_log_query(int64_t batch, int64_t capacity, int64_t ld, nig_episode_log_layout *out)
{
    if (!out) return refuse("nig_episode_log_query", "out is NULL");
    NIG_TRY(check_episode_log_shape("nig_episode_log_query", batch, capacity, ld));
    *out = episode_log_layout(batch, capacity, ld);
    return NIG_OK;
}

// A handle, a log (8-byte aligned: it holds doubles) and its shape; then the kernels' view of the log
static int episode_log_args(const nig_handle *h, const char *fn, void *log, int64_t capacity, int64_t ld, EpisodeLogArgs &a)
{
    if (!h) return refuse(fn, "NULL handle");
    if (!log || ((uintptr_t)log & 7u) != 0) return refuse(fn, "log NULL or not 8-byte aligned");
    NIG_TRY(check_episode_log_shape(fn, h->B, capacity, ld));
    const nig_episode_log_layout L = episode_log_layout(h->B, capacity, ld);
    char *p = (char *)log;
    a.ret = (double *)(p + L.off_ret);
    for (int w = 0; w < 5; ++w) a.w[w] = (uint32_t *)(p + L.off_w[w]);
    a.count = (uint32_t *)(p + L.off_count); a.carry_ret = (double *)(p + L.off_carry_ret); a.carry_w = (uint32_t *)(p + L.off_carry_w);
    a.tally = (double *)(p + L.off_tally);
    a.ld = L.ld; a.B = h->B; a.capacity = (uint32_t)capacity;
    return NIG_OK;
}

int nig_episode_log_init(nig_handle *h, void *log, int64_t capacity, int64_t ld, void *stream)
{
    EpisodeLogArgs a;
    NIG_TRY(episode_log_args(h, "nig_episode_log_init", log, capacity, ld, a));
    hipLaunchKernelGGL(episode_log_init_kernel<>, dim3(grid_for(h->B)), dim3(BLOCK), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return NIG_OK;
}

int nig_collect_episodes(nig_handle *h, int32_t n_steps, const float *reward, const uint32_t *flags, int64_t out_stride,
                         void *log, int64_t capacity, int64_t ld, void *stream)
{
    const char *fn = "nig_collect_episodes";
    EpisodeLogArgs a;
    NIG_TRY(episode_log_args(h, fn, log, capacity, ld, a));
    NIG_TRY(refuse_limited(h, fn));               // (the records are decoded from the main flag word alone)
    if (n_steps < 1) return refuse(fn, "n_steps < 1");
    if (!reward || !flags) return refuse(fn, "reward and flags rows are both required");
    if (n_steps > 1 ? (out_stride < h->B || out_stride > NIG_MAX_PITCH) : (out_stride != 0 && (out_stride < h->B || out_stride > NIG_MAX_PITCH)))
        return refuse(fn, "out_stride outside [batch, 2^26] (0 allowed with n_steps == 1)");
    auto kernel = SPECS[h->env].reward_is_f32 ? collect_episodes_kernel<true> : collect_episodes_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(grid_for(h->B)), dim3(BLOCK), 0, (hipStream_t)stream, a, reward, flags, out_stride, (int)n_steps);
    HIP_TRY(hipGetLastError());
    return NIG_OK;
}

int nig_reduce_episodes(nig_handle *h, void *log, int64_t capacity, int64_t ld, int64_t n_episodes, double *partial_out,
                        void *stream)
{
    const char *fn = "nig_reduce_episodes";
    EpisodeLogArgs a;
    NIG_TRY(episode_log_args(h, fn, log, capacity, ld, a));
    if (!partial_out) return refuse(fn, "partial_out is NULL");
    if (n_episodes < 1 || n_episodes > capacity * h->B) return refuse(fn, "n_episodes outside [1, capacity*batch]");
    hipStream_t st = (hipStream_t)stream;
    double *scratch = (double *)((char *)log + episode_log_layout(h->B, capacity, ld).off_scratch);
    int nblk = (int)((h->B + BLOCK - 1) / BLOCK);
    if (nblk > REDUCE_BLOCKS) nblk = REDUCE_BLOCKS;
    hipLaunchKernelGGL(episode_tally_kernel<>, dim3(grid_for(h->B)), dim3(BLOCK), 0, st, a, n_episodes, enabled_constraints(h));
    hipLaunchKernelGGL(reduce_tally_stage1, dim3(nblk), dim3(BLOCK), 0, st, (const double *)a.tally, a.ld, h->B, scratch);
    hipLaunchKernelGGL(reduce_tally_stage2, dim3(1), dim3(REDUCE_BLOCKS), 0, st, (const double *)scratch, nblk, partial_out);
    hipLaunchKernelGGL(episode_row_sum_kernel<>, dim3(1), dim3(BLOCK), 0, st, (const double *)(a.tally + (int64_t)NIG_T_ROWS * a.ld), h->B,
                       partial_out + NIG_T_ROWS);
    HIP_TRY(hipGetLastError());
    return NIG_OK;
}

}  // extern "C"
