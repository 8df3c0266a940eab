// PowerGrid's kernels of nig_rollout_mlp_ensemble (the fused ensemble actor) -- a translation unit of their own (launcher: nig_launch_families.hpp)
#include "nig_launch_families.hpp"
NIG_DEFINE_ENV_ENSEMBLE(PowerGrid)
