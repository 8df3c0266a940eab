// SteelAnnealing's kernel of nig_rollout_mlp_safe for a shaped actor and a shaped critic of class 512x512 ("nig-mlp-shape-shield-v1") -- a translation unit of its own (launcher: nig_launch_families.hpp)
#include "nig_launch_families.hpp"
NIG_DEFINE_ENV_SHAPE_SHIELD(SteelAnnealing, Shape512)
