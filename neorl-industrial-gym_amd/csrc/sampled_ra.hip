// RobotAssembly's kernels of nig_rollout_sampled (the fused rollout that draws its actions) -- a translation unit of their own
#define NIG_SAMPLED_TU
#include "nig_launch.hpp"
NIG_DEFINE_ENV_SAMPLED(RobotAssembly)
