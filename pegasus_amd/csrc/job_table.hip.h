// job_table.hip.h -- the lookup that the per-launch job tables share across kernel families (pose errors, ADI, sweeps).
// Device helpers only: no __global__ kernel and no __constant__ table lives here, so any number of translation units may
// include it (DESIGN.md "Source layout").
#pragma once
#include "pgr_common.h"

namespace pgr {

// which job of the launch's table a workgroup belongs to: the last one whose first workgroup (block0) is not behind it
template <typename Table>
__device__ __forceinline__ int pose_job_of_block(const Table& T, uint32_t block) {
    int k = 0;
    for (int q = 1; q < T.count; ++q)
        if (block >= T.job[q].block0) k = q;
    return k;
}

}  // namespace pgr
