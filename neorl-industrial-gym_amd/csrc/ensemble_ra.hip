// RobotAssembly's kernels of nig_rollout_mlp_ensemble (the fused ensemble actor) -- a translation unit of their own
#define NIG_ENSEMBLE_TU
#include "nig_launch.hpp"
NIG_DEFINE_ENV_ENSEMBLE(RobotAssembly)
