// ChemicalReactor's kernels of nig_rollout_mlp_projected_limited (the family under the user's added box constraints) -- a translation unit of their own (launcher: nig_launch_families.hpp)
#include "nig_launch_families.hpp"
NIG_DEFINE_ENV_PROJECTED_LIMITED(ChemicalReactor)
