// mmw_scan.hpp -- the one workgroup scan of the library: an inclusive Hillis-Steele scan over 1024 LDS slots, one per thread of a
// 1024-thread workgroup, advancing up to TWO independent values in the same rounds (10 rounds, one barrier pair each -- two
// scans one after the other would pay the barriers twice).  Used by k_feat_scan (k_misc.hip), k_snap_scan (k_snapshot.hip) and
// k_pair_scan (k_scan.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace mmw {

struct ScanAdd { template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
struct ScanMax { template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a > b ? a : b; } };

// One value of a scan: its 1024 LDS slots (the caller's), how two values combine and what a thread without a predecessor takes.
template <class T, class Op>
struct ScanLane {
    T *part;
    T identity;
    __device__ __forceinline__ T prev(int tid, int o) const { return tid >= o ? part[tid - o] : identity; }
    __device__ __forceinline__ void fold(int tid, T v) const { part[tid] = Op()(part[tid], v); }
};
// (the second value of a scan that has only one: nothing is read, nothing is written)
struct ScanNoLane {
    __device__ __forceinline__ int prev(int, int) const { return 0; }
    __device__ __forceinline__ void fold(int, int) const {}
};
template <class Op, class T>
__device__ __forceinline__ ScanLane<T, Op> scan_lane(T *part, T identity = T(0)) { return ScanLane<T, Op>{part, identity}; }

// All 1024 threads call, each having stored its own value in part[tid] of every lane (no barrier needed in between: the first one
// is here).  On return part[tid] holds the combination of slots 0 .. tid, visible to every thread.
template <class A, class B = ScanNoLane>
__device__ __forceinline__ void workgroup_scan_1024(int tid, A a, B b = B())
{
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const auto va = a.prev(tid, o);
        const auto vb = b.prev(tid, o);
        __syncthreads();
        a.fold(tid, va);
        b.fold(tid, vb);
        __syncthreads();
    }
}

}  // namespace mmw
