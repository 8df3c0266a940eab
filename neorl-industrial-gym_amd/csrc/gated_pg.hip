// PowerGrid's kernel of nig_rollout_mlp_gated (the fused safety-ensemble gate) -- a translation unit of its own (launcher: nig_launch_families.hpp)
#include "nig_launch_families.hpp"
NIG_DEFINE_ENV_GATED(PowerGrid)
