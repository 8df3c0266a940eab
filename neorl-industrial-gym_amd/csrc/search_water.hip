// WaterTreatment's kernel of nig_rollout_mlp_search (the fused safe-action search) -- a translation unit of its own (launcher: nig_launch_families.hpp)
#include "nig_launch_families.hpp"
NIG_DEFINE_ENV_SEARCH(WaterTreatment)
