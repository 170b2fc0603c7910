// mmw_wave.hpp -- cross-lane helpers of the wave-per-scene export kernels (k_zone.hip, k_trail.hip): registers only, no LDS.
#pragma once

#include <hip/hip_runtime.h>

namespace mmw {

// exclusive prefix sum over the wave and the wave's total (all 64 lanes call)
__device__ __forceinline__ int wave_excl_sum(int v, int lane, int &total)
{
    int inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o);
        inc += lane >= o ? up : 0;
    }
    total = __shfl(inc, 63);
    return inc - v;
}

}  // namespace mmw
