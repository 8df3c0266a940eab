// AdvancedPowerGrid's kernel of nig_rollout_mlp_search (the fused safe-action search) -- a translation unit of its own
#define NIG_SEARCH_TU
#include "nig_launch.hpp"
NIG_DEFINE_ENV_SEARCH(AdvancedPowerGrid)
