// PowerGrid's kernel of nig_rollout_mlp_safe for a LayerNorm actor and critic ("nig-mlp-ln-shield-v1") -- a translation unit of its own (launcher: nig_launch_families.hpp)
#include "nig_launch_families.hpp"
NIG_DEFINE_ENV_LN_SHIELD(PowerGrid)
