// k_scan.hip -- the two kernels the live-track exports share.  k_pair_scan: each export's count kernel leaves two counts per scene
// in off[2][S + 1], the scan turns both into offsets in place and takes the capacity decision that the export's write kernel and
// the host read.  k_uid_rebase: the generation words of the exports that remember uids (mmw_uidlist.hpp), bumped in one launch.
#include "mmw_scan.hpp"
#include "mmw_kernels.hpp"

namespace mmw {

// single workgroup: in-place exclusive scans of both count arrays, then the capacity decision -- both totals, formed in 64 bits,
// against the caller's two capacities.  A total above INT32_MAX fits no buffer (the capacities are int32) and is reported
// saturated; the per-scene offsets are then meaningless and nobody reads them.
//   off[s], off[S + 1 + s]    the scene's offsets;  off[S], off[2S + 1] the totals
//   totals[0..3]              total 0, total 1, 1 = both fit, 0
__global__ __launch_bounds__(1024) void k_pair_scan(int S, int32_t *off /*[2][S+1]*/, int32_t *totals /*[4]*/, int cap0, int cap1)
{
    __shared__ long long part[2][1024];
    const int tid = threadIdx.x;
    const int per = (S + 1023) / 1024;
    const int s0 = min(S, tid * per), s1 = min(S, s0 + per);
    int32_t *off0 = off, *off1 = off + S + 1;
    long long sum0 = 0, sum1 = 0;
    for (int s = s0; s < s1; s++) { sum0 += off0[s]; sum1 += off1[s]; }
    part[0][tid] = sum0;
    part[1][tid] = sum1;
    workgroup_scan_1024(tid, scan_lane<ScanAdd>(part[0]), scan_lane<ScanAdd>(part[1]));
    long long run0 = part[0][tid] - sum0, run1 = part[1][tid] - sum1;
    for (int s = s0; s < s1; s++) {
        const int c0 = off0[s], c1 = off1[s];
        off0[s] = (int32_t)run0; run0 += c0;
        off1[s] = (int32_t)run1; run1 += c1;
    }
    if (tid == 1023) {
        const long long tot0 = part[0][1023], tot1 = part[1][1023], lim = 0x7fffffffLL;
        const int32_t t0 = (int32_t)(tot0 < lim ? tot0 : lim), t1 = (int32_t)(tot1 < lim ? tot1 : lim);
        off0[S] = t0;
        off1[S] = t1;
        totals[0] = t0;
        totals[1] = t1;
        totals[2] = (tot0 <= (long long)cap0 && tot1 <= (long long)cap1) ? 1 : 0;
        totals[3] = 0;
    }
}

// mmw_reset / mmw_reset_scenes / mmw_restore / mmw_set_zones: the uids of the touched scenes restart (or, for the zones alone, their
// table changed), so every consumer's memory of them is void.  flags == nullptr: every scene; else the scenes whose flag is non-zero.
__global__ __launch_bounds__(256) void k_uid_rebase(int n_scenes, const int32_t *__restrict__ flags, UidGens gens)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n_scenes || (flags && !flags[s])) return;
#pragma unroll
    for (int i = 0; i < UidGens::kMax; i++)
        if (gens.gen[i]) gens.gen[i][s] += 1;
}

void launch_uid_rebase(int n_scenes, const int32_t *flags, const UidGens &gens, hipStream_t st)
{
    hipLaunchKernelGGL(k_uid_rebase, dim3((n_scenes + 255) / 256), dim3(256), 0, st, n_scenes, flags, gens);
}

void launch_pair_scan(int S, int32_t *off, int32_t *totals, int cap0, int cap1, hipStream_t st)
{
    hipLaunchKernelGGL(k_pair_scan, dim3(1), dim3(1024), 0, st, S, off, totals, cap0, cap1);
}

}  // namespace mmw
