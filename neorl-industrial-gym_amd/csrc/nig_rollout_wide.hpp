// nig_rollout_wide.hpp -- the wide form of the open-loop rollout (device code only): whole BLK-lane blocks of a handle without
// frozen lanes run rollout_body's NOFREEZE form, or, for PowerGrid, the LDS-staged body of nig_pg_lds.hpp.
#pragma once
#include "nig_pg_lds.hpp"
#include "nig_rollout.hpp"

namespace nig {

template <class Env, int OUT, int BLK, bool NOISE = false, bool SAMPLED = false>
struct wide_body {                                // default: the register-resident body without freeze handling
    static constexpr int LDS_BYTES = RolloutLds<Env, OUT, BLK>::BYTES;
    __device__ static __forceinline__ void run(const RolloutArgs &q, uint32_t base, unsigned char *smem)
    {
        rollout_body<Env, OUT, false, true, true, BLK, NOISE, false, SAMPLED>(q, base, smem);
    }
};
template <int OUT, int BLK, bool NOISE, bool SAMPLED>
struct wide_body<PowerGrid, OUT, BLK, NOISE, SAMPLED> {    // PowerGrid: state staged in LDS (nig_pg_lds.hpp)
    static constexpr int LDS_BYTES = PgLds<BLK>::BYTES;
    __device__ static __forceinline__ void run(const RolloutArgs &q, uint32_t base, unsigned char *smem)
    {
        pg_lds_rollout_body<OUT, BLK, false, NOISE, false, RolloutArgs, SAMPLED>(q, base, smem);
    }
};

template <class Env, int OUT, int BLK, bool NOISE = false>
__global__ void __launch_bounds__(BLK, (BLK / 256) * Env::WIDE_ROLLOUT_WAVES) rollout_wide_kernel(const RolloutArgs q)
{
    __shared__ __attribute__((aligned(16))) unsigned char smem[wide_body<Env, OUT, BLK, NOISE>::LDS_BYTES];
    wide_body<Env, OUT, BLK, NOISE>::run(q, q.block0 * 256u + blockIdx.x * BLK, smem);
}
template <class Env, int OUT, int BLK>            // nig_rollout_sampled's twin
__global__ void __launch_bounds__(BLK, (BLK / 256) * Env::WIDE_ROLLOUT_WAVES) rollout_sampled_wide_kernel(const RolloutArgs q)
{
    __shared__ __attribute__((aligned(16))) unsigned char smem[wide_body<Env, OUT, BLK, false, true>::LDS_BYTES];
    wide_body<Env, OUT, BLK, false, true>::run(q, q.block0 * 256u + blockIdx.x * BLK, smem);
}

}  // namespace nig
