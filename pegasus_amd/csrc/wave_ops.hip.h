// wave_ops.hip.h -- wave-wide float reductions shared across kernel families.  Device helpers only: no __global__ kernel
// and no __constant__ table lives here, so any number of translation units may include it (DESIGN.md "Source layout").
#pragma once
#include "pgr_common.h"

namespace pgr {

// wave-wide min / max, result in lane 63 (DPP row shifts + the two row broadcasts, like pgr_common.h's prefix sums;
// out-of-row reads return the identity through bound_ctrl = 0 -> the old value)
__device__ __forceinline__ float dpp_f32(float old, float v, int ctrl) {
    switch (ctrl) {
        case 0x111: return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), 0x111, 0xF, 0xF, false));
        case 0x112: return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), 0x112, 0xF, 0xF, false));
        case 0x114: return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), 0x114, 0xF, 0xF, false));
        case 0x118: return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), 0x118, 0xF, 0xF, false));
        case 0x142: return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), 0x142, 0xA, 0xF, false));
        default:    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), 0x143, 0xC, 0xF, false));
    }
}
template <bool MAX>
__device__ __forceinline__ float wave_reduce_to_last(float v) {
    const int ctrls[6] = {0x111, 0x112, 0x114, 0x118, 0x142, 0x143};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float o = dpp_f32(v, v, ctrls[k]);      // lanes without a source keep their own value
        v = MAX ? fmaxf(v, o) : fminf(v, o);
    }
    return v;
}
__device__ __forceinline__ float wave_min_f(float v) { return wave_reduce_to_last<false>(v); }
__device__ __forceinline__ float wave_max_f(float v) { return wave_reduce_to_last<true>(v); }

}  // namespace pgr
