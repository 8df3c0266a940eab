// nig_device.hpp -- what every kernel family of libnig.so shares (device code only): the block size, the 16-byte and
// streaming stores, the argument block of one step (StepArgs) and the internal handle-flag bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <type_traits>

#include "../../include/nig.h"
#include "nig_envs.hpp"

namespace nig {

constexpr int BLOCK = 256;

// One 16-byte store per call.  A HIP float4 assignment is scalarised and re-merged by hipcc, which can
// pick 12+16+16+4-byte pieces for a 48-byte row (misaligned dwordx4: -20 % on the row-major
// trajectory); a native vector store stays one aligned global_store_dwordx4.
typedef float v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store16(float *dst16, float a, float b, float c, float d)
{
    v4f v = {a, b, c, d};
    *reinterpret_cast<v4f *>(dst16) = v;
}
// Per-step rollout outputs are written once and read by nobody on the device: streaming (nt) stores
// keep them from evicting the action ring and the generator table from L2 (+5..16 % on the fused
// rollout).  Only for stores that cover whole lines per instruction -- nt on the lane-strided 16-byte
// pieces of an untransposed row-major row HALVED the 1M-lane rate (no write-combining in L2).
template <class T>
__device__ __forceinline__ void stream_store(T *dst, T v)
{
#ifdef NIG_DIAG_STORE_POLICY           // (diagnostic builds only, profiles/r05: another cache policy for the 16-byte trajectory stores --
    // 1 = sc1 (write-through, dropped from L2), 2 = sc0 sc1, 3 = nt sc1; the production nt keeps the line in L2)
    if constexpr (sizeof(T) == 16) {
#if NIG_DIAG_STORE_POLICY == 1
        asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(dst), "v"(v) : "memory");
#elif NIG_DIAG_STORE_POLICY == 2
        asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" :: "v"(dst), "v"(v) : "memory");
#else
        asm volatile("global_store_dwordx4 %0, %1, off nt sc1" :: "v"(dst), "v"(v) : "memory");
#endif
        return;
    }
#endif
    __builtin_nontemporal_store(v, dst);
}
constexpr int REDUCE_BLOCKS = 256;
constexpr int64_t POLICY_BYTES = 2048;     // device copy of nig_policy at the workspace tail

struct StepArgs {
    // library-owned
    float *state; uint32_t *ctr; long long *life_viol; double *ep_ret; double *tally;
    uint32_t ld; uint32_t B;          // 32-bit on purpose: row offsets k*ld stay in scalar registers
    uint32_t ld_state;                // pitch of the state rows (== ld unless the caller bound its own array)
    // caller-owned
    const float *actions; uint32_t ld_act;
    const double *actions64;          // nig_step64: the same rows as float64 (actions is then unused)
    const double *step_noise; const double *reset_noise; uint32_t ld_noise;
    float *reward; double *reward64; uint32_t *flags; float *final_obs; uint32_t ld_obs;
    // scalars
    uint64_t env0; uint32_t seed_lo, seed_hi;
    const uint32_t *t_ptr; uint32_t t_off;   // launch counter t = (t_ptr ? *t_ptr : 0) + t_off (graph replay keeps t on the device)
    int max_steps; float dt32; double dt; uint32_t hflags; uint32_t cmask;
    int n_en;                         // enabled built-in constraints = SafetyMetrics.total_constraints of every step (base.py:115)
    // host side only (which kernel form a launch takes, nig_tune): thresholds in effect for this handle's device
    uint32_t split_blocks, wide_min_blocks;
    uint32_t *ring_err;               // device word a timed-out ring wait is reported in (NIG_RING_SPIN_LIMIT builds only; nig_ring.hpp)
    // nig_step_host: a second copy of every lane's post-step state rows, [S][ld_mirror], written by the step kernel itself
    // (the host-buffer entry points used to launch a row-gather kernel behind every step: one launch less per env.step)
    float *mirror; uint32_t ld_mirror;
};
// internal bit of StepArgs::hflags (above the public NIG_F_* bits): some lane of the handle may hold
// NIG_CTR_DONE although the handle auto-resets (never reset, left out by reset(mask), set by
// nig_set_state); cleared by a full nig_reset.  Lets the rollout kernel keep its no-freeze fast path.
constexpr uint32_t HF_MAY_HOLD_DONE = 0x10000u;
// test-only (NIG_RING_SPIN_LIMIT builds, nig_ring.hpp): producing roles stop posting after 7 steps
constexpr uint32_t HF_DIAG_RING_FAULT = 0x20000u;
}  // namespace nig
