// RobotAssembly's kernels of nig_rollout_sampled (the fused rollout that draws its actions) -- a translation unit of their own (launcher: nig_launch_families.hpp)
#include "nig_launch_families.hpp"
NIG_DEFINE_ENV_SAMPLED(RobotAssembly)
