// AdvancedPowerGrid's kernel of nig_rollout_mlp for a shaped actor of class 128x128 ("nig-mlp-shape-v1") -- a translation unit of its own (launcher: nig_launch_families.hpp)
#include "nig_launch_families.hpp"
NIG_DEFINE_ENV_SHAPE(AdvancedPowerGrid, Shape128)
