// AdvancedPowerGrid's kernels of the distributional safety critic ("nig-categorical-v1": the shield and the search with the categorical critic, nig_mlp_violation_prob) -- a translation unit of their own (launcher: nig_launch_families.hpp)
#include "nig_launch_families.hpp"
NIG_DEFINE_ENV_CATEGORICAL(AdvancedPowerGrid)
