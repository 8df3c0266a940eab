// kernels of AdvancedChemicalReactor (nig_envs.hpp) -- one translation unit per environment
#include "nig_launch.hpp"
NIG_DEFINE_ENV_LAUNCH(AdvancedChemicalReactor, nig_launch_acr)
