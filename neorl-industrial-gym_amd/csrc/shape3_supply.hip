// SupplyChain's kernel of nig_rollout_mlp for a shaped actor of class 256x256x256 ("nig-mlp-shape-v1") -- a translation unit of its own (launcher: nig_launch_families.hpp)
#include "nig_launch_families.hpp"
NIG_DEFINE_ENV_SHAPE(SupplyChain, Shape3)
