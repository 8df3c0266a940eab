// AdvancedChemicalReactor's kernel of nig_rollout_mlp_bf16 (the actor on the bf16 matrix unit) -- a translation unit of its own (launcher: nig_launch_families.hpp)
#include "nig_launch_families.hpp"
NIG_DEFINE_ENV_BF16(AdvancedChemicalReactor)
