// HVACControl's kernels of nig_step_limited / nig_step64_limited / nig_rollout_policy_limited / nig_rollout_mlp_limited (the user's added box constraints on the device) -- a translation unit of their own (launcher: nig_launch_families.hpp)
#include "nig_launch_families.hpp"
NIG_DEFINE_ENV_LIMITED(HVACControl)
