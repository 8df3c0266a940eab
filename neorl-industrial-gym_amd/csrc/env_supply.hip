// kernels of SupplyChain (nig_envs.hpp) -- one translation unit per environment
#include "nig_launch.hpp"
NIG_DEFINE_ENV_LAUNCH(SupplyChain, nig_launch_supply)
