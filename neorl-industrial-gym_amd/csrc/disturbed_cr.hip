// ChemicalReactor's kernels of nig_rollout_policy_disturbed / nig_rollout_mlp_disturbed (sensor / actuator noise in the closed loop) -- a translation unit of their own (launcher: nig_launch_families.hpp)
#include "nig_launch_families.hpp"
NIG_DEFINE_ENV_DISTURBED(ChemicalReactor)
