// RobotAssembly's kernel of nig_rollout_mlp_projected (the fused constraint projection) -- a translation unit of its own (launcher: nig_launch_families.hpp)
#include "nig_launch_families.hpp"
NIG_DEFINE_ENV_PROJECTED(RobotAssembly)
