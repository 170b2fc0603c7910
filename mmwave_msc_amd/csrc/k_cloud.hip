// k_cloud.hip -- the live tracks' point clouds (mmw_clouds_*): every track's effective_data (Tracking.py:43-58: the ring's frames
// concatenated, oldest first) and, when asked for, every scene's global ring, compacted into one output in the report's (scene, slot)
// order with a directory entry per cloud.  Reads SceneHdr, order, TrackRec and the two rings after the step, the way k_snap_pack
// does; nothing of the step is touched and nothing is kept between two calls.
//   k_cloud_count   entries and points per scene: a wave per scene, a lane per track (t_cap <= 64)
//   k_pair_scan     (k_scan.hip) one workgroup: the two offset scans, the capacity decision, the totals (formed in 64 bits)
//   k_cloud_write   a workgroup per scene: the directory and the rows (MMW_CLOUD_ROWS) or points (MMW_CLOUD_POINTS) -- only if everything fits
//
// The rings are slot-permuted: logical frame k (k-th oldest) lives in physical slot ring_slot[k] of the track's ring, g_slot[k] of
// the global ring.  A track frame stores min(ring_n[k], ring_rows) rows; what the reference holds beyond that is the entry's `dropped`.
#include <cstddef>
#include "mmw_device.hpp"
#include "mmw_math.hpp"
#include "mmw_ring.hpp"
#include "mmw_kernels.hpp"

namespace mmw {

static_assert(sizeof(mmw_cloud_track) == 32 && alignof(mmw_cloud_track) == 4, "mmw_cloud_track");
static_assert(sizeof(mmw_cloud_point) == 16, "mmw_cloud_point");
static_assert(offsetof(mmw_cloud_track, dropped) + 4 == sizeof(mmw_cloud_track) && offsetof(mmw_cloud_point, track) == 12, "no padding");
static_assert(MMW_TRACK_CAP_LIMIT <= 64, "one lane per track");
static_assert(MMW_RING_MAX == 4, "the frames of a ring are walked unrolled");

constexpr int kRowUnits = 4;   // a row = 8 fp64 = four 16-byte units

__device__ __forceinline__ Ring global_ring(const DevCfg &cfg, const SceneHdr *hdr)
{
    Ring r;
    r.len = clampi(hdr->g_len, 0, cfg.ring);
    r.stored = r.dropped = 0;
#pragma unroll
    for (int k = 0; k < MMW_RING_MAX; k++) {
        r.n[k] = k < r.len ? clampi(hdr->g_n[k], 0, cfg.max_pts) : 0;
        r.stored += r.n[k];
        r.phys[k] = phys_slot(k, hdr->g_slot[k], cfg.ring);
    }
    return r;
}
__device__ __forceinline__ int newest_rows(const Ring &r)
{
    int v = 0;
#pragma unroll
    for (int k = 0; k < MMW_RING_MAX; k++) v = (k == r.len - 1) ? r.n[k] : v;
    return v;
}

__global__ __launch_bounds__(256) void k_cloud_count(DevCfg cfg, DevState st, ExportScratch sc, int unassigned)
{
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= cfg.n_scenes) return;   // (wave-uniform)
    const SceneHdr *hdr = st.hdr + s;
    const int T = live_tracks(cfg, st, s);
    int rows = 0;
    if (lane < T) rows = track_ring(cfg, st.trk + (size_t)s * cfg.t_cap + live_slot(cfg, st, s, lane)).stored;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rows += __shfl_xor(rows, o);
    if (lane == 0) {
        sc.off[s] = T + (unassigned ? 1 : 0);
        sc.off[cfg.n_scenes + 1 + s] = rows + (unassigned ? global_ring(cfg, hdr).stored : 0);
    }
}

// `n` rows of one frame, stored contiguously at `src`, to position `first` of the output: thread t of `stride`.
//   ROWS    a row is 64 bytes, 16-byte aligned on both sides: four lanes move one row, a 16-byte load and a 16-byte store each, so a
//           wave instruction touches 1 KiB contiguous in source and destination.  Four loads are in flight per lane before the first store.
//   POINTS  a lane per row: the leading 24 bytes (x, y | z), one rounding each to fp32, one 16-byte mmw_cloud_point store
template <int MODE>
__device__ __forceinline__ void move_rows(const double *__restrict__ src, int n, void *__restrict__ out, int first, int entry, int t, int stride)
{
    if constexpr (MODE == MMW_CLOUD_ROWS) {
        const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
        uint4 *d4 = reinterpret_cast<uint4 *>(out) + (size_t)first * kRowUnits;
        const int units = n * kRowUnits;
        int u = t;
        for (; u + 3 * stride < units; u += 4 * stride) {
            const uint4 a = s4[u], b = s4[u + stride], c = s4[u + 2 * stride], d = s4[u + 3 * stride];
            d4[u] = a;
            d4[u + stride] = b;
            d4[u + 2 * stride] = c;
            d4[u + 3 * stride] = d;
        }
        for (; u < units; u += stride) d4[u] = s4[u];
    } else {
        uint4 *d = reinterpret_cast<uint4 *>(out) + (size_t)first;
        for (int r = t; r < n; r += stride) {
            const double2 xy = reinterpret_cast<const double2 *>(src)[(size_t)r * kRowUnits];
            const double z = src[(size_t)r * 8 + 2];
            d[r] = uint4{__float_as_uint((float)xy.x), __float_as_uint((float)xy.y), __float_as_uint((float)z), (unsigned)entry};
        }
    }
}

// Every wave of the scene's workgroup reads the scene's track list (a lane per track) and forms the wave-prefix of the stored rows:
// each entry's `first` without a barrier or LDS.  Wave 0 writes the directory, a lane per entry.  The waves then take the track
// entries in turn -- the entry's ring comes out of its lane by readlane, so frame counts, slots and addresses are scalars -- and
// walk its frames oldest first through the slot permutation.  The global ring (up to ring x max_pts rows, many times a track's)
// is moved by all four waves together.
template <int MODE>
__global__ __launch_bounds__(256) void k_cloud_write(DevCfg cfg, DevState st, ExportScratch sc, mmw_cloud_track *__restrict__ dir, void *__restrict__ out,
                                                     int unassigned, int scene_base)
{
    if (!sc.totals[2]) return;   // (uniform over the launch) something does not fit: neither buffer is written
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int s = blockIdx.x, S = cfg.n_scenes;
    const SceneHdr *hdr = st.hdr + s;
    const int T = live_tracks(cfg, st, s);
    const int e0 = sc.off[s], p0 = sc.off[S + 1 + s];

    Ring r;
    r.len = r.stored = r.dropped = 0;
#pragma unroll
    for (int k = 0; k < MMW_RING_MAX; k++) r.n[k] = r.phys[k] = 0;
    int rslot = 0, uid = -1;
    if (lane < T) {
        rslot = live_slot(cfg, st, s, lane);
        const TrackRec *rec = st.trk + (size_t)s * cfg.t_cap + rslot;
        r = track_ring(cfg, rec);
        uid = rec->uid;
    }
    int incl = r.stored;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int w = __shfl_up(incl, o);
        if (lane >= o) incl += w;
    }
    const int first = p0 + incl - r.stored;
    const int trk_rows = __shfl(incl, 63);

    if (wave == 0 && lane < T) dir[e0 + lane] = mmw_cloud_track{scene_base + s, lane, uid, first, r.stored, r.len, newest_rows(r), r.dropped};

    const size_t frame_doubles = (size_t)cfg.ring_rows * 8;
    for (int e = wave; e < T; e += 4) {   // (uniform)
        const int es = __builtin_amdgcn_readfirstlane(__shfl(rslot, e));
        int run = __builtin_amdgcn_readfirstlane(__shfl(first, e));
        const double *base = st.trk_ring + ((size_t)s * cfg.t_cap + es) * (size_t)cfg.ring * frame_doubles;
#pragma unroll
        for (int k = 0; k < MMW_RING_MAX; k++) {
            const int nk = __builtin_amdgcn_readfirstlane(__shfl(r.n[k], e)), ph = __builtin_amdgcn_readfirstlane(__shfl(r.phys[k], e));
            if (nk > 0) move_rows<MODE>(base + (size_t)ph * frame_doubles, nk, out, run, e0 + e, lane, 64);
            run += nk;
        }
    }

    if (!unassigned) return;
    const Ring g = global_ring(cfg, hdr);   // (hdr is uniform: scalar loads)
    if (wave == 0 && lane == 0) dir[e0 + T] = mmw_cloud_track{scene_base + s, -1, -1, p0 + trk_rows, g.stored, g.len, newest_rows(g), 0};
    int run = p0 + trk_rows;
#pragma unroll
    for (int k = 0; k < MMW_RING_MAX; k++) {
        if (g.n[k] > 0) move_rows<MODE>(st.g_ring + ((size_t)s * cfg.ring + g.phys[k]) * (size_t)cfg.max_pts * 8, g.n[k], out, run, e0 + T, (int)threadIdx.x, 256);
        run += g.n[k];
    }
}

void launch_clouds(const DevCfg &cfg, const DevState &s, const ExportScratch &sc, mmw_cloud_track *dir, int cap_tracks, void *out, int cap_points, int mode,
                   int scene_base, hipStream_t st)
{
    const int unassigned = (mode & MMW_CLOUD_UNASSIGNED) ? 1 : 0;
    hipLaunchKernelGGL(k_cloud_count, dim3((cfg.n_scenes + 3) / 4), dim3(256), 0, st, cfg, s, sc, unassigned);
    launch_pair_scan(cfg.n_scenes, sc.off, sc.totals, cap_tracks, cap_points, st);
    if (mode & MMW_CLOUD_ROWS) hipLaunchKernelGGL(k_cloud_write<MMW_CLOUD_ROWS>, dim3(cfg.n_scenes), dim3(256), 0, st, cfg, s, sc, dir, out, unassigned, scene_base);
    else hipLaunchKernelGGL(k_cloud_write<MMW_CLOUD_POINTS>, dim3(cfg.n_scenes), dim3(256), 0, st, cfg, s, sc, dir, out, unassigned, scene_base);
}

}  // namespace mmw
