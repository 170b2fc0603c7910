// mmw_assoc.hpp -- association rules of TrackBuffer.track (Tracking.py:664-703), defined ONCE for the two kernels that run them:
// k_track (bulk: a workgroup per scene between k_predict and k_post) and k_scene (one scene start to finish).  The kernels
// differ in schedule -- who loads what when, which wave takes which job, where the barriers are -- and that stays with them: the
// functions here take values and plain pointers, and know no LDS layout, record staging, wave role or barrier.  All arithmetic
// fp64 with a fixed operation order (mmw_math.hpp): the order the parity oracle restates.
// Every function is forced inline; how the kernels' instruction streams compare with the rules written out in place is in
// profiles/assoc_shared_isa.txt (scripts/isa_diff.py).  Still written out in both kernels, because as functions they moved
// registers, scratch or the loops' code (profiles/assoc_shared_attempts.txt): the counter reset, the scalar-cache warm-up, the
// ring push, the live-slot OR, the column-sum and min / max loops, the leaf-list registration, the dispersion blend, the keep rule.
#pragma once

#include "mmw_device.hpp"
#include "mmw_math.hpp"

namespace mmw {

// Diagnostic build only (make STAMPS=1 -> libmmw_hip_stamps.so): never compiled into the product library.
#ifdef MMW_STAMPS
// PROBE(id): raw clock of lane 0 of every wave of ONE workgroup (block MMW_PROBE_BLOCK), for timelines (scripts/probe_timeline.py)
#ifndef MMW_PROBE_BLOCK
#define MMW_PROBE_BLOCK 460   // (k_track: st.perm puts the scenes with the most tracks first; k_scene.hip defines its own AHEAD of this header)
#endif
#define PROBE(id)                                                                             \
    do {                                                                                      \
        if (blockIdx.x == MMW_PROBE_BLOCK && (threadIdx.x & 63) == 0)                         \
            st.stats[kStatSlots * kStatWords + (threadIdx.x >> 6) * 64 + (id)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
// WGTIME(k): s_memrealtime (100 MHz, chip-wide) and s_memtime of every workgroup's start (k = 0) and end (k = 1), scripts/wg_times.py
// (-DMMW_STAMPS_POST: k_post's workgroups write these words instead, k_dbscan.hip)
#ifdef MMW_STAMPS_POST
#define WGTIME(k)
#else
// (2048 slots: a launch of more workgroups stamps every second / fourth ... one)
#define WGTIME(k)                                                                             \
    do {                                                                                      \
        int wg_sh = 0;                                                                        \
        while (((int)gridDim.x >> wg_sh) > 2048) wg_sh++;                                     \
        if (threadIdx.x == 0 && (blockIdx.x & ((1u << wg_sh) - 1)) == 0) {                    \
            const unsigned wg_slot = blockIdx.x >> wg_sh;                                     \
            st.stats[kStatSlots * kStatWords + 256 + wg_slot * 4 + (k) * 2] = __builtin_amdgcn_s_memrealtime(); \
            st.stats[kStatSlots * kStatWords + 256 + wg_slot * 4 + (k) * 2 + 1] = __builtin_amdgcn_s_memtime(); \
        }                                                                                     \
    } while (0)
#endif
#else
#define PROBE(id)
#define WGTIME(k)
#endif

// Columns of the point tile are NP + 2 doubles apart: with a power-of-two stride the same row of all six
// columns -- what the lanes of one track read together -- would sit in one LDS bank (6-way conflicts).
constexpr int kTilePad = 2;
// per track: gate record in (352) + spread, N_est, group dispersion, ring state in (392) + centroid, min, max,
// spread, group dispersion, N_est, lifetime, counters, ring state out (540)  (bench.py prices the Kalman stages itself)
constexpr int kTrackBytesPerTrack = 352 + 392 + 540;

__host__ __device__ inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// ---- frame head ----
// A frame that does not reach track() (offline_main.py:56: empty frames never do; one thread): no DBSCAN, and the scene is not in
// this frame's update lists -- the next k_predict finds its tracks by this flag (the ring's size and non-finite flags in
// `skipped`, the header's word as the caller read it, stay).  A count the context was not sized for is an error.
__device__ __forceinline__ void frame_skipped(SceneHdr *hdr, int skipped, int n_raw)
{
    hdr->need_db = 0;
    hdr->skipped = (skipped & ~255) | 1;
    if (n_raw != 0) atomicOr(&hdr->err, ERR_BADCOUNT);
}

// ---- the gate (Tracking.py:553-572) ----
// The gate record of a track (C^-1, log|det C|, predicted position: 43 doubles, k_predict -> gate_buf) is the same for every
// point, i.e. wave-uniform: it is read through the SCALAR cache (a pointer into the constant address space, uniform address ->
// s_load) and enters the fp64 VALU ops as their SGPR operand (no LDS staging, no barriers in the gate phase).
#ifdef MMW_DIAG_VGATE   // (diagnostic build, scripts/dual_run.py: the records by VECTOR loads -- volatile global -- instead of through the scalar cache)
typedef const volatile double *gate_ptr;
#else
typedef const double __attribute__((address_space(4))) *gate_ptr;
#endif

// Records written by THIS launch: the constant address space promises the compiler memory that does not change, so the pointer
// itself is made opaque behind the caller's scalar-cache invalidate: no load through it can be moved above this statement.
__device__ __forceinline__ gate_ptr gate_records_opaque(gate_ptr gb)
{
    asm volatile("; mmw: gate pointer opaque from here" : "+s"(gb) : : "memory");
    return gb;
}

// _calc_dist_fun of one (point row, gate record) pair: log|det C| + y' C^-1 y, y = x - the predicted position.
// y' C^-1 y as k-ordered FUSED chains, v_k = fma(y_a, Ci[a][k], v_k) row by row over C^-1, then q = fma(v_k, y_k, q): the
// arithmetic definition the oracle shares (oracle/c/mmw_oracle.c, _calc_dist_fun); with the operands in SGPRs the phase is
// bound by fp64 issue, and the fused form is 49 instead of 84 instructions per (point, track).
__device__ __forceinline__ double gate_distance(gate_ptr G, double x0, double x1, double x2, double x3, double x4, double x5)
{
    const double y0 = x0 - G[37], y1 = x1 - G[38], y2 = x2 - G[39], y3 = x3 - G[40], y4 = x4 - G[41], y5 = x5 - G[42];
    double v[6];
#pragma unroll
    for (int k = 0; k < 6; k++) v[k] = y0 * G[k];
#pragma unroll
    for (int k = 0; k < 6; k++) v[k] = __builtin_fma(y1, G[6 + k], v[k]);
#pragma unroll
    for (int k = 0; k < 6; k++) v[k] = __builtin_fma(y2, G[12 + k], v[k]);
#pragma unroll
    for (int k = 0; k < 6; k++) v[k] = __builtin_fma(y3, G[18 + k], v[k]);
#pragma unroll
    for (int k = 0; k < 6; k++) v[k] = __builtin_fma(y4, G[24 + k], v[k]);
#pragma unroll
    for (int k = 0; k < 6; k++) v[k] = __builtin_fma(y5, G[30 + k], v[k]);
    double quad = v[0] * y0;
    quad = __builtin_fma(v[1], y1, quad);
    quad = __builtin_fma(v[2], y2, quad);
    quad = __builtin_fma(v[3], y3, quad);
    quad = __builtin_fma(v[4], y4, quad);
    quad = __builtin_fma(v[5], y5, quad);
    return G[36] + quad;
}

// the first best: track j takes a row of the frame (`in_frame`) inside its gate only from no track or at a strictly smaller d
__device__ __forceinline__ void gate_first_best(const DevCfg &cfg, bool in_frame, double d, int j, int &bestj, double &bestd)
{
    if (in_frame && d < cfg.tr_gate) {
        if (bestj < 0 || d < bestd) { bestj = j; bestd = d; }
    }
}

// ---- non-finite rows in the global ring ----
// two flag bits per physical slot, in SceneHdr.skipped: the word after this frame's bits have replaced those of the slot it was
// written to
__device__ __forceinline__ int nf_ring_flags(int skipped, int phys, int frame_bits)
{
    return nf_flags_with((skipped >> kSkipNfShift) & kSkipNfMask, phys, frame_bits);
}

// ---- PointCluster statistics (associate_pointcloud, Tracking.py:314-341) ----

// _estimate_measurement_spread (Tracking.py:246-268) of column m of a cloud of nj rows; old = the track's estimate so far
__device__ __forceinline__ double spread_estimate(const DevCfg &cfg, int m, int nj, double mn, double mx, double old)
{
    double spread = mx - mn;
    const double lim = cfg.kf_spread_lim[m], lim2 = 2 * lim;
    if (nj != 1) spread = spread * (double)(nj + 1) / (double)(nj - 1);
    spread = spread < lim2 ? spread : lim2;
    spread = spread > lim ? spread : lim;
    return spread > old ? spread : (1.0 - cfg.kf_a_spr) * old + cfg.kf_a_spr * spread;
}

// _estimate_point_num (Tracking.py:232-244)
__device__ __forceinline__ double point_num_estimate(const DevCfg &cfg, int nj, double ne)
{
    if (cfg.kf_enable_est) return ((double)nj > ne) ? (double)nj : (1 - cfg.kf_a_n) * ne + cfg.kf_a_n * (double)nj;
    return cfg.kf_est_pointnum > (double)nj ? cfg.kf_est_pointnum : (double)nj;
}

// cluster.status: sqrt(sum(centroid[3:6]^2)) < TR_VEL_THRES (Tracking.py:132-136)
__device__ __forceinline__ int centroid_is_static(const DevCfg &cfg, double v3, double v4, double v5)
{
    return sqrt((v3 * v3 + v4 * v4) + v5 * v5) < cfg.tr_vel_thres ? 1 : 0;
}

// ---- _estimate_group_disp_matrix + _get_D (Tracking.py:270-297) ----
// numpy pairwise_sum_DOUBLE (the summation order of the 1-D np.mean in ClusterTrack._get_D, Tracking.py:286):
//   n < 8      : one by one
//   n <= 128   : eight interleaved accumulators r[k] += x[i+k], ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the
//                n%8 leftovers one by one                                   -- a LEAF
//   otherwise  : n2 = n/2 - (n/2)%8 ;  pairwise(x, n2) + pairwise(x+n2, n-n2)
// The leaves of one sum are independent, so they are spread over lanes (pw_leaf) and only the few adds of
// the recursion (pw_combine) stay serial.  D = recursion depth budget: 4 levels cover n <= 2048.

// numpy's split point and the bound on leaves per frame: a leaf that comes from a split holds at least 57 rows, so a frame has at
// most max_pts/57 of them.
__host__ __device__ inline int pw_split(int n) { const int h = n / 2; return h - h % 8; }
__host__ __device__ inline int pw_max_leaves(int np) { return np > 128 ? np / 57 + 1 : 0; }

template <int D, typename F>
__device__ __forceinline__ void pw_for_each_leaf(int off, int n, F f)
{
    if constexpr (D == 0) f(off, n);
    else {
        if (n <= 128) f(off, n);
        else { const int n2 = pw_split(n); pw_for_each_leaf<D - 1>(off, n2, f); pw_for_each_leaf<D - 1>(off + n2, n - n2, f); }
    }
}

// sums of the leaves, in leaf order, back into the value numpy returns
template <int D>
__device__ __forceinline__ double pw_combine(int n, const double *leafsum, int stride, int &idx)
{
    if constexpr (D == 0) { const double v = leafsum[idx * stride]; idx++; return v; }
    else {
        if (n <= 128) { const double v = leafsum[idx * stride]; idx++; return v; }
        const int n2 = pw_split(n);
        const double l = pw_combine<D - 1>(n2, leafsum, stride, idx);
        const double r = pw_combine<D - 1>(n - n2, leafsum, stride, idx);
        return l + r;
    }
}
constexpr int kPwDepth = 4;

// one leaf (n <= 128) of sum_r (pa[r]-ca)*(pb[r]-cb)
__device__ __forceinline__ double pw_leaf(const double *pa, const double *pb, double ca, double cb, int n)
{
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; i++) res += (pa[i] - ca) * (pb[i] - cb);
        return res;
    }
    const int lim = n - (n & 7);
    double r[8], xa[8], xb[8];
#pragma unroll
    for (int u = 0; u < 8; u++) { xa[u] = pa[u]; xb[u] = pb[u]; }
#pragma unroll
    for (int u = 0; u < 8; u++) r[u] = (xa[u] - ca) * (xb[u] - cb);
    for (int i = 8; i < lim; i += 8) {
#pragma unroll
        for (int u = 0; u < 8; u++) { xa[u] = pa[i + u]; xb[u] = pb[i + u]; }
#pragma unroll
        for (int u = 0; u < 8; u++) r[u] += (xa[u] - ca) * (xb[u] - cb);
    }
    const int left = n - lim;  // the n%8 leftovers, loaded together, added one by one
#pragma unroll
    for (int u = 0; u < 7; u++) { xa[u] = (u < left) ? pa[lim + u] : 0.0; xb[u] = (u < left) ? pb[lim + u] : 0.0; }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
    for (int u = 0; u < 7; u++) if (u < left) res += (xa[u] - ca) * (xb[u] - cb);
    return res;
}

// words of a frame's leaf list: [0] leaves, [1] clouds of more than 128 rows, then per leaf (track, off, len) and, behind
// pw_max_leaves(np) of those, per cloud (track, first leaf)
__host__ __device__ inline int ml_words(int np) { return 2 + 5 * (pw_max_leaves(np) + 1); }
// entry e = 0..20 of the symmetric 6 x 6 dispersion matrix, row by row over the upper triangle: (a, b), a <= b
__device__ __forceinline__ void disp_entry(int e, int &a, int &b) { a = 0; while (e >= 6 - a) { e -= 6 - a; a++; } b = a + e; }
// ---- step statistics: algorithmic bytes of this scene-frame -- points in, assoc out, per track the gate record
// and the record fields the step reads and writes, nun unassigned rows appended to the global ring, ring_rows rows appended to
// track rings --, frames, tracks, (point, track) pairs
__device__ __forceinline__ void step_account(unsigned long long *sl, bool f32, int n, int Tin, int nun, int ring_rows)
{
    atomicAdd(&sl[0], (unsigned long long)((f32 ? 32 : 64) * n + 4 * n + Tin * kTrackBytesPerTrack + 64 * nun + 64 * ring_rows));
    atomicAdd(&sl[2], 1ULL);
    atomicAdd(&sl[5], (unsigned long long)Tin);
    atomicAdd(&sl[6], (unsigned long long)n * (unsigned long long)Tin);
}

}  // namespace mmw
