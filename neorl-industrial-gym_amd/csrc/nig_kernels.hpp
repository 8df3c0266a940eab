// nig_kernels.hpp -- HIP kernel templates (gfx950) of libnig.so, one instantiation set per environment.
//
// One wavefront lane per environment instance.  State, actions, noise and outputs are
// structure-of-arrays ([row][lane], row pitch ld) so every global access of a wave is one
// fully coalesced 256-byte row segment.  The step kernel fuses the whole of
// IndustrialEnv.step (environments/base.py:157-213): clip -> constraint checks on the
// pre-state -> dynamics -> reward -> penalties -> counters -> done/truncation -> critical
// shutdown -> (optional) episode tally flush and in-kernel auto-reset.  No MFMA: these are
// elementwise ODE updates (HBM-bound, DESIGN.md "Roofline").
//
// Device code only: the host side that launches these kernels is nig_launch.hpp (what the .hip units include).
// Translation units: every environment's kernels are instantiated in a file of their own
// (env_*.hip: `NIG_DEFINE_ENV_LAUNCH(Env, name)`), the C ABI and the env-independent kernels
// live in nig_api.hip; _build.py compiles them in parallel and links libnig.so.
// Build flags: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-slp-vectorize.
//
// One header per kernel family; each includes what it uses and compiles on its own (tests/test_headers_standalone.py).
#pragma once
#include "nig_device.hpp"            // BLOCK, store16 / stream_store, StepArgs, HF_*
#include "nig_ring.hpp"              // LDS ring counters of the cooperating-wave kernels
#include "nig_episode.hpp"           // the episode bookkeeping every body shares
#include "nig_step.hpp"              // IndustrialEnv.step for one lane, generator glue, cooperative reset
#include "nig_step_kernel.hpp"       // step_kernel, reset_kernel, fill_actions_kernel
#include "nig_rollout.hpp"           // RolloutArgs, rollout_body, rollout_kernel, rollout_sampled_kernel
#include "nig_policy.hpp"            // PolicyArgs and the feedback-policy law
#include "nig_pg_lds.hpp"            // PowerGrid's LDS-staged bodies and kernels
#include "nig_rollout_wide.hpp"      // rollout_wide_kernel, rollout_sampled_wide_kernel
#include "nig_split.hpp"             // the three-wave open-loop form
#include "nig_rollout_policy.hpp"    // rollout_policy_kernel
#include "nig_split_policy.hpp"      // the three-wave closed-loop form
#include "nig_mlp.hpp"               // the MFMA actor, its shield and its ensemble
#include "nig_mlp_bf16.hpp"          // the MFMA actor on the bf16 matrix unit ("nig-mlp-bf16-v1")
#include "nig_mlp_shape.hpp"         // the MFMA actor of the other hidden shapes ("nig-mlp-shape-v1")
#include "nig_mlp_shape_shield.hpp"  // the shaped actor with its shaped safety-critic shield ("nig-mlp-shape-shield-v1")
#include "nig_mlp_ln.hpp"            // the MFMA actor with LayerNorm ("nig-mlp-ln-v1")
#include "nig_mlp_ln_shield.hpp"     // the LayerNorm actor with its LayerNorm safety-critic shield ("nig-mlp-ln-shield-v1")
#include "nig_episodes.hpp"          // per-episode records from reward / flag rows (env-independent)
