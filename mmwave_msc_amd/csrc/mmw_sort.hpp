// mmw_sort.hpp -- the 64-row sort of the CNN's feature maps (np.argsort(padded[:, 0]), Utils.py:513): a bitonic network over one
// wave on (key, row), and the gather + store it drives.  Shared by k_features / k_format_frames (k_misc.hip) and the training
// samples' MMW_SAMPLE_INPUT form (k_sample.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace mmw {

// lane ^ J of a 32-bit value without the LDS crossbar where the hardware allows it: DPP inside quads (J = 1, 2) and inside rows of 16
// (J = 4, 8: the two row shifts, picked by the lane's bit J); ds_bpermute for 16 and 32 (mmw_cloud.hpp's xor_lane_d, for ints)
template <int J>
__device__ __forceinline__ int xor_lane_i(int v)
{
    if constexpr (J == 1) return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);        // quad_perm [1,0,3,2]
    else if constexpr (J == 2) return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
    else if constexpr (J == 4 || J == 8) {
        const int up = __builtin_amdgcn_update_dpp(0, v, 0x100 + J, 0xF, 0xF, true), dn = __builtin_amdgcn_update_dpp(0, v, 0x110 + J, 0xF, 0xF, true);   // row_shl: lane i <- i + J; row_shr: i - J
        return (__lane_id() & J) ? dn : up;
    } else return __shfl_xor(v, J);
}
// one compare-exchange step of the bitonic network on (key, row): block size SZ, partner lane ^ STRIDE
template <int SZ, int STRIDE>
__device__ __forceinline__ void bitonic_step(int lane, double &key, int &src)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(key);
    const int olo = xor_lane_i<STRIDE>((int)(unsigned)u), ohi = xor_lane_i<STRIDE>((int)(unsigned)(u >> 32)), os = xor_lane_i<STRIDE>(src);
    const double ok = __longlong_as_double((long long)(((unsigned long long)(unsigned)ohi << 32) | (unsigned)olo));
    const bool up = (lane & SZ) == 0;          // ascending block
    const bool lower = (lane & STRIDE) == 0;   // this lane keeps the smaller of the pair
    const bool other_less = ok < key || (ok == key && os < src);
    const bool take = (up == lower) ? other_less : !other_less;
    if (take) { key = ok; src = os; }
}
template <int SZ, int STRIDE>
__device__ __forceinline__ void bitonic_merge(int lane, double &key, int &src)
{
    bitonic_step<SZ, STRIDE>(lane, key, src);
    if constexpr (STRIDE > 1) bitonic_merge<SZ, STRIDE / 2>(lane, key, src);
}

// the whole network for a caller with a tie rule of its own (k_sample.hip): the wave's 64 (key, src) pairs ascending by key, ties
// by src.  (sort_rows_store below spells the six merges out as it always did: k_features compiles instruction for instruction as before.)
__device__ __forceinline__ void bitonic_sort64(int lane, double &key, int &src)
{
    bitonic_merge<2, 1>(lane, key, src);
    bitonic_merge<4, 2>(lane, key, src);
    bitonic_merge<8, 4>(lane, key, src);
    bitonic_merge<16, 8>(lane, key, src);
    bitonic_merge<32, 16>(lane, key, src);
    bitonic_merge<64, 32>(lane, key, src);
}

// np.argsort(padded[:, 0]) (Utils.py:513) + the gather it drives: a bitonic network over
// the wave on (x, row) -- ties ordered by row position -- then 5 fp32 stores per lane.  18 of its 21 steps exchange by DPP (partners inside a row of
// 16 lanes); with every step three trips through the LDS crossbar the kernel was a chain of ds_bpermute latencies (118 us at 98 k sorts).
// The keys must not be NaN: bitonic_step's `<` and `==` are both false on a NaN, so both lanes of a pair keep the same element and
// the result is no permutation.  The callers that feed it from a track's ring (k_features<SITE>) cannot meet one: the
// gate refuses a row whose x is not finite, DBSCAN raises on one, so no ring frame holds such a row, and the centroid subtracted
// from it is a mean of ring rows.  Caller data (k_format_frames) goes through sort_rows_store_nan_last.
__device__ inline void sort_rows_store(int lane, double v0, double v1, double v2, double v3, double v4, float *dst)
{
    double key = v0;
    int src = lane;
    bitonic_merge<2, 1>(lane, key, src);
    bitonic_merge<4, 2>(lane, key, src);
    bitonic_merge<8, 4>(lane, key, src);
    bitonic_merge<16, 8>(lane, key, src);
    bitonic_merge<32, 16>(lane, key, src);
    bitonic_merge<64, 32>(lane, key, src);
    const double s0 = __shfl(v0, src), s1 = __shfl(v1, src), s2 = __shfl(v2, src), s3 = __shfl(v3, src), s4 = __shfl(v4, src);
    // a lane's five values are 20 consecutive bytes: one 16-byte and one 4-byte store (4-byte aligned: global memory takes that)
    struct __attribute__((packed, aligned(4))) F4 { float a, b, c, d; };
    *reinterpret_cast<F4 *>(dst + lane * 5) = F4{(float)s0, (float)s1, (float)s2, (float)s3};
    dst[lane * 5 + 4] = (float)s4;
}

// The same for keys that may be NaN, as np.argsort orders them: rows with a NaN x behind every other row, +inf included, in row
// order.  A NaN key sorts as +inf with bit 6 of its row set (the tie rule then puts it behind a true +inf, and NaN rows among
// themselves by row); the bit is masked off before the gather, which moves the row's own values, the NaN with them.  (A function
// of its own, gather and stores repeated: sort_rows_store, which k_features runs every frame, compiles instruction for instruction
// as it did -- sharing the gather cost it an instruction and a register.)
__device__ inline void sort_rows_store_nan_last(int lane, double v0, double v1, double v2, double v3, double v4, float *dst)
{
    const bool nan = v0 != v0;
    double key = nan ? __builtin_huge_val() : v0;
    int src = (nan ? 64 : 0) | lane;
    bitonic_sort64(lane, key, src);
    src &= 63;
    const double s0 = __shfl(v0, src), s1 = __shfl(v1, src), s2 = __shfl(v2, src), s3 = __shfl(v3, src), s4 = __shfl(v4, src);
    struct __attribute__((packed, aligned(4))) F4 { float a, b, c, d; };
    *reinterpret_cast<F4 *>(dst + lane * 5) = F4{(float)s0, (float)s1, (float)s2, (float)s3};
    dst[lane * 5 + 4] = (float)s4;
}

}  // namespace mmw
