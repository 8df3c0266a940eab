// HVACControl's kernel of nig_rollout_mlp for a LayerNorm actor ("nig-mlp-ln-v1") -- a translation unit of its own (launcher: nig_launch_families.hpp)
#include "nig_launch_families.hpp"
NIG_DEFINE_ENV_LN(HVACControl)
