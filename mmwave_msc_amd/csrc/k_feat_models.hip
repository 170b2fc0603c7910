// k_feat_models.hip -- the scan in front of k_features for a context whose scenes are served by several posture models
// (mmw_posture_attach_models): rows are handed out MODEL BY MODEL, so that each model's rows form one contiguous band of the
// chain's buffers and the CNN kernels run once per band, unchanged.
#include "mmw_scan.hpp"
#include "mmw_kernels.hpp"

namespace mmw {

__device__ __forceinline__ unsigned pad256(unsigned v) { return (v + 255u) & ~255u; }
__device__ __forceinline__ unsigned lo32(unsigned long long v) { return (unsigned)v; }
__device__ __forceinline__ unsigned hi32(unsigned long long v) { return (unsigned)(v >> 32); }

// single workgroup, as k_feat_scan: row_off[s] holds k_feat_count's count of scene s on entry and on return
//   row_off[s] = base[m] + rows of earlier scenes of model m = map[s];  base[0] = 0, base[m + 1] = base[m] + pad256(total[m])
//   row_off[s] = none_off for a scene no model estimates (map[s] outside [0, n_models)): k_features drops its rows
//   row_off[S] = the sum of the totals;  groups[0 .. 8) = total[m], groups[8 .. 16) = base[m]
// workgroup_scan_1024 advances two values per pass; each is a 64-bit word of two 32-bit totals, so a pass scans four models and
// eight models take two.  A pass needs the bases its predecessor ended on, which is why the passes cannot be one.  Integers only,
// no atomics.  (Totals stay far below 2^32: S * track_cap rows are what the int32 offsets can name at all.)
__global__ __launch_bounds__(1024) void k_feat_scan_models(int S, int n_models, int none_off, const int32_t *__restrict__ map /*[S]*/,
                                                            int32_t *__restrict__ row_off /*[S+1]*/, int32_t *__restrict__ groups /*[16]*/)
{
    __shared__ unsigned long long part[2][1024];
    const int tid = threadIdx.x;
    const int per = (S + 1023) / 1024;
    const int s0 = min(S, tid * per), s1 = min(S, s0 + per);
    unsigned base = 0, grand = 0;
    for (int m0 = 0; m0 < n_models; m0 += 4) {
        unsigned long long a = 0, b = 0;
        for (int s = s0; s < s1; s++) {
            const int m = map[s];
            const unsigned l = (unsigned)(m - m0);
            if (l < 4u && m < n_models) {
                const unsigned long long v = (unsigned long long)(unsigned)row_off[s] << ((l & 1u) * 32u);
                if (l & 2u) b += v; else a += v;
            }
        }
        part[0][tid] = a;
        part[1][tid] = b;
        workgroup_scan_1024(tid, scan_lane<ScanAdd>(part[0]), scan_lane<ScanAdd>(part[1]));
        const unsigned long long ia = part[0][tid] - a, ib = part[1][tid] - b;   // rows of this pass's models in front of this thread's scenes
        const unsigned long long ta = part[0][1023], tb = part[1][1023];
        const unsigned t0 = lo32(ta), t1 = hi32(ta), t2 = lo32(tb), t3 = hi32(tb);
        const unsigned b0 = base, b1 = b0 + pad256(t0), b2 = b1 + pad256(t1), b3 = b2 + pad256(t2);
#ifdef MMW_DIAG_SCAN_ALL_MODELS   // (mutant, DESIGN 8h: the prefix inside a band counts the earlier scenes of every model of the pass)
        const unsigned all = lo32(ia) + hi32(ia) + lo32(ib) + hi32(ib);
        unsigned r0 = b0 + all, r1 = b1 + all, r2 = b2 + all, r3 = b3 + all;
#else
        unsigned r0 = b0 + lo32(ia), r1 = b1 + hi32(ia), r2 = b2 + lo32(ib), r3 = b3 + hi32(ib);
#endif
        for (int s = s0; s < s1; s++) {
            const int m = map[s];
            const unsigned l = (unsigned)(m - m0);
            if (l < 4u && m < n_models) {
                const unsigned c = (unsigned)row_off[s];
                row_off[s] = (int32_t)(l == 0u ? r0 : l == 1u ? r1 : l == 2u ? r2 : r3);
                r0 += l == 0u ? c : 0u;
                r1 += l == 1u ? c : 0u;
                r2 += l == 2u ? c : 0u;
                r3 += l == 3u ? c : 0u;
            } else if (m0 == 0 && (m < 0 || m >= n_models)) {
                row_off[s] = none_off;
            }
        }
        if (tid == 1023) {
            groups[m0] = (int32_t)t0; groups[m0 + 1] = (int32_t)t1; groups[m0 + 2] = (int32_t)t2; groups[m0 + 3] = (int32_t)t3;
            groups[8 + m0] = (int32_t)b0; groups[8 + m0 + 1] = (int32_t)b1; groups[8 + m0 + 2] = (int32_t)b2; groups[8 + m0 + 3] = (int32_t)b3;
        }
        base = b3 + pad256(t3);
        grand += t0 + t1 + t2 + t3;
        __syncthreads();   // (the totals have been read: the next pass may overwrite the slots)
    }
    if (tid == 1023) row_off[S] = (int32_t)grand;
}

void launch_feat_scan_models(int S, int n_models, int none_off, const int32_t *map, int32_t *row_off, int32_t *groups, hipStream_t st)
{
    hipLaunchKernelGGL(k_feat_scan_models, dim3(1), dim3(1024), 0, st, S, n_models, none_off, map, row_off, groups);
}

}  // namespace mmw
