// HVACControl's kernels of the distributional safety critic under the user's added box constraints (nig_rollout_mlp_safe_limited / _search_limited with the categorical critic) -- a translation unit of their own (launcher: nig_launch_families.hpp)
#include "nig_launch_families.hpp"
NIG_DEFINE_ENV_CATEGORICAL_LIMITED(HVACControl)
