// k_snapshot.hip -- snapshot / restore of scene state (include/mmw.h: format version 1, DESIGN.md "Snapshots").
//
//   k_snap_size    a wave per selected scene: the section's byte count and its directory entry (as k_feat_count)
//   k_snap_scan    one workgroup: the sections' offsets (exclusive scan, as k_feat_scan) and the blob's total
//   k_snap_pack    gather: a workgroup per (scene, part) -- part 0 the canonical header + the track records, parts 1..kGParts
//                  a share of the global ring, the others one track's ring each -- so that one scene with many long track
//                  rings does not serialise a workgroup; frames move as 16-byte vectors
//   k_snap_check   restore, before anything is written: every section agrees with its directory entry (a blob whose inside
//                  disagrees is refused, with no scene changed)
//   k_snap_scrub   restore: the last step's update / spawn lists no longer name tracks of the destination scenes
//   k_snap_unpack  scatter, the inverse of k_snap_pack: identity slots (g_slot, ring_slot), order[] the identity, `skipped` bit 0 set
//
// Canonical: the bytes depend only on the reference-visible state.  Records in effective_tracks order, ring_slot / g_slot
// the identity, the ring's non-finite flags re-mapped from physical to logical slots, the per-step scheduling words
// (need_db, db_u, n_upd, skipped bit 0) and all padding zero -- k_export's rule for what is not state.
//
// The restored scenes' `skipped` bit 0 sends them to the header path of the next _predict_all (k_kalman.hip: the skipped
// scan; mmw_reset_scenes relies on the same path).  The track-wise k_predict ALSO walks the previous step's update lists and
// spawn list, whose entries of the scenes that occupied the destination slots are guarded only by j < n_tracks -- enough for
// a reset scene (no track), not for a restored one: its tracks would be predicted twice.  k_snap_scrub moves such an entry's
// position to 63 (>= every n_tracks: the track-wise layout runs with t_cap <= 63, upd_pack) and a spawn entry's first new
// track to t_cap.  Every other consumer of last-step state reads the scene header (per-scene k_predict, the PRED head of
// k_track, k_scene) or lists built in its own step (k_post's update, the DBSCAN queues and work lists); the next step's
// perm[] is a schedule, any permutation gives the same results.
#include "mmw_device.hpp"
#include "mmw_kalman.hpp"
#include "mmw_scan.hpp"
#include "mmw_kernels.hpp"

namespace mmw {

constexpr int kSnapHdr = MMW_SNAP_SCENE_HDR_BYTES;
constexpr int kSnapRec = MMW_SNAP_TRACK_BYTES;
constexpr int kSnapRecWords = kSnapRec / 8;          // 188: the record's 187 words + one of zeros
constexpr int kRecWords = sizeof(TrackRec) / 8;      // 187
constexpr int kRowBytes = 64, kRowUnits = 4;         // a row = 8 fp64 = four 16-byte units
constexpr int kGParts = 4;                           // workgroups per scene on its global ring
// word positions inside TrackRec (8-byte words)
constexpr int kWX = 0, kWP = 9, kWRingLen = 153, kWRingN = 154, kWRingSlot = 156;
static_assert(offsetof(TrackRec, P) == kWP * 8 && offsetof(TrackRec, ring_len) == kWRingLen * 8 && offsetof(TrackRec, ring_n) == kWRingN * 8 &&
                  offsetof(TrackRec, ring_slot) == kWRingSlot * 8 && sizeof(TrackRec) == kRecWords * 8,
              "TrackRec word map");
static_assert(kSnapRec == (kRecWords + 1) * 8 && kSnapRec % 16 == 0 && kSnapHdr == sizeof(SceneHdr), "snapshot record / header sizes");
static_assert(sizeof(mmw_snapshot_entry) == 48, "mmw_snapshot_entry");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wave_max(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ unsigned long long pack2(int lo, int hi) { return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo; }

// rows a track's ring frame k stores, and the frames' total / largest count
struct RingRows { int stored, maxn; };
__device__ __forceinline__ RingRows track_rows(int ring_len, const int32_t *ring_n, int ring_rows)
{
    RingRows r{0, 0};
#pragma unroll
    for (int k = 0; k < MMW_RING_MAX; k++) {
        if (k < ring_len) {
            const int nk = ring_n[k] < 0 ? 0 : ring_n[k];
            r.stored += min(nk, ring_rows);
            r.maxn = max(r.maxn, nk);
        }
    }
    return r;
}

// word w of the canonical form of `rec` (w < kSnapRecWords)
__device__ __forceinline__ unsigned long long canon_word(const TrackRec *rec, int w, int dx, int ring)
{
    if (w >= kRecWords) return 0ULL;
    const unsigned long long *src = reinterpret_cast<const unsigned long long *>(rec);
    if (w >= kWRingSlot && w < kWRingSlot + 2) return pack2(2 * (w - kWRingSlot), 2 * (w - kWRingSlot) + 1);
    const unsigned long long v = src[w];
    if (w < kWP) return w - kWX < dx ? v : 0ULL;
    if (w < kWP + 81) { const int e = w - kWP; return (e / 9 < dx && e % 9 < dx) ? v : 0ULL; }
    if (w >= kWRingN && w < kWRingN + 2) {
        const int len = clampi(rec->ring_len, 0, ring), k0 = 2 * (w - kWRingN);
        return pack2(k0 < len ? (int)(unsigned)v : 0, k0 + 1 < len ? (int)(unsigned)(v >> 32) : 0);
    }
    return v;
}

// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_snap_size(DevCfg cfg, DevState st, const int32_t *__restrict__ sel, int n, mmw_snapshot_entry *__restrict__ dir,
                                                   unsigned long long *__restrict__ bytes)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;   // (wave-uniform)
    const int s = sel[i];
    const SceneHdr *hdr = st.hdr + s;
    const int T = clampi(hdr->n_tracks, 0, cfg.t_cap), gl = clampi(hdr->g_len, 0, cfg.ring);
    RingRows tr{0, 0};
    if (lane < T) {
        const TrackRec *rec = st.trk + (size_t)s * cfg.t_cap + st.order[(size_t)s * cfg.t_cap + lane];
        tr = track_rows(clampi(rec->ring_len, 0, cfg.ring), rec->ring_n, cfg.ring_rows);
    }
    const int trk_rows = wave_sum(tr.stored), trk_max = wave_max(tr.maxn);
    if (lane == 0) {
        int g_rows = 0, g_max = 0;
        for (int k = 0; k < gl; k++) {
            const int nk = clampi(hdr->g_n[k], 0, cfg.max_pts);
            g_rows += nk;
            g_max = max(g_max, nk);
        }
        const unsigned long long b = (unsigned long long)kSnapHdr + (unsigned long long)T * kSnapRec + (unsigned long long)(trk_rows + g_rows) * kRowBytes;
        mmw_snapshot_entry e;
        e.offset = 0;   // (k_snap_scan)
        e.bytes = b;
        e.n_tracks = T;
        e.g_len = gl;
        e.max_g_rows = g_max;
        e.max_trk_rows = trk_max;
        e.err = hdr->err;
        e.ring_size = hdr_ring_size(hdr->skipped);
        e.reserved_[0] = e.reserved_[1] = 0;
        dir[i] = e;
        bytes[i] = b;
    }
}

// one workgroup: offsets from `base` in blob order; bytes[n] = the blob's total, bytes[n + 1] = the largest track count
__global__ __launch_bounds__(1024) void k_snap_scan(int n, unsigned long long base, mmw_snapshot_entry *__restrict__ dir, unsigned long long *__restrict__ bytes)
{
    __shared__ unsigned long long part[1024];
    __shared__ int tmax[1024];
    const int tid = threadIdx.x;
    const int per = (n + 1023) / 1024;
    const int i0 = tid * per, i1 = min(n, i0 + per);
    unsigned long long sum = 0;
    int mt = 0;
    for (int i = i0; i < i1; i++) { sum += bytes[i]; mt = max(mt, dir[i].n_tracks); }
    part[tid] = sum;
    tmax[tid] = mt;
    workgroup_scan_1024(tid, scan_lane<ScanAdd>(part), scan_lane<ScanMax>(tmax));
    unsigned long long run = base + part[tid] - sum;
    for (int i = i0; i < i1; i++) { dir[i].offset = run; run += bytes[i]; }
    if (tid == 1023) { bytes[n] = base + part[1023]; bytes[n + 1] = (unsigned long long)tmax[1023]; }
}

// Moves `units` 16-byte units of up to MMW_RING_MAX frames between a contiguous run (the blob) and per-frame places (the
// rings).  pre[f] = units in front of frame f; unit u of frame f is at frame[f] + (u - pre[f]).
struct FrameRun { const char *src[MMW_RING_MAX] = {}; char *dst[MMW_RING_MAX] = {}; int pre[MMW_RING_MAX + 1]; int nf; };
__device__ __forceinline__ void move_units(const FrameRun &R, bool gather, const uint4 *__restrict__ flat_src, uint4 *__restrict__ flat_dst, int first,
                                           int stride)
{
    const int tot = R.pre[MMW_RING_MAX];   // (frames past nf add nothing)
    for (int u = first; u < tot; u += stride) {
        // (the frame by selects, not by an index into R: R stays in registers)
        const char *fs = R.src[0];
        char *fd = R.dst[0];
        int fb = 0;
#pragma unroll
        for (int k = 1; k < MMW_RING_MAX; k++) {
            if (k < R.nf && u >= R.pre[k]) { fs = R.src[k]; fd = R.dst[k]; fb = R.pre[k]; }
        }
        if (gather) flat_dst[u] = reinterpret_cast<const uint4 *>(fs)[u - fb];
        else reinterpret_cast<uint4 *>(fd)[u - fb] = flat_src[u];
    }
}

// rows of each listed track (effective_tracks position j < T) and their prefix, in LDS: part y of the launch needs the place
// of its tracks' frames inside the section
__device__ __forceinline__ void track_row_prefix(int T, const int *rows_of /* per thread j < T */, int *pre /* LDS [65] */)
{
    // (T <= 64: one wave's inclusive scan)
    const int tid = threadIdx.x;
    if (tid < 64) {
        int v = tid < T ? rows_of[0] : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int w = __shfl_up(v, o);
            if (tid >= o) v += w;
        }
        pre[tid + 1] = v;
        if (tid == 0) pre[0] = 0;
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_snap_pack(DevCfg cfg, DevState st, const int32_t *__restrict__ sel, const mmw_snapshot_entry *__restrict__ dir,
                                                   char *__restrict__ blob)
{
    __shared__ int pre[65];
    const int i = blockIdx.x, y = blockIdx.y, tid = threadIdx.x;
    const int s = sel[i];
    const SceneHdr *hdr = st.hdr + s;
    const int T = clampi(hdr->n_tracks, 0, cfg.t_cap), gl = clampi(hdr->g_len, 0, cfg.ring);
    const int32_t *order = st.order + (size_t)s * cfg.t_cap;
    const TrackRec *trk = st.trk + (size_t)s * cfg.t_cap;
    char *sec = blob + dir[i].offset;
    if (y == 0) {
        if (tid == 0) {
            SceneHdr h;
            h.n_tracks = T;
            h.g_len = gl;
            const int nf = (hdr->skipped >> kSkipNfShift) & kSkipNfMask;
            int lflags = 0;
            for (int k = 0; k < MMW_RING_MAX; k++) {
                const bool live = k < gl;
                const int phys = hdr->g_slot[k] & (MMW_RING_MAX - 1);
                h.g_n[k] = live ? clampi(hdr->g_n[k], 0, cfg.max_pts) : 0;
                h.g_slot[k] = k;
                if (live) lflags |= ((nf >> (2 * phys)) & 3) << (2 * k);
            }
            h.need_db = 0;
            h.err = hdr->err;
            h.db_u = 0;
            h.next_uid = hdr->next_uid;
            h.n_upd = 0;
            h.skipped = (hdr_ring_size(hdr->skipped) << kSkipRingShift) | (lflags << kSkipNfShift);
            *reinterpret_cast<SceneHdr *>(sec) = h;
        }
        unsigned long long *rw = reinterpret_cast<unsigned long long *>(sec + kSnapHdr);
        for (int w = tid; w < T * kSnapRecWords; w += blockDim.x) {
            const int r = w / kSnapRecWords, k = w - r * kSnapRecWords;
            rw[w] = canon_word(trk + order[r], k, cfg.dx, cfg.ring);
        }
        return;
    }
    // per-thread row counts of the tracks (thread j < T: track j), their prefix
    int my_rows = 0;
    if (tid < T) {
        const TrackRec *rec = trk + order[tid];
        my_rows = track_rows(clampi(rec->ring_len, 0, cfg.ring), rec->ring_n, cfg.ring_rows).stored;
    }
    track_row_prefix(T, &my_rows, pre);
    uint4 *rings = reinterpret_cast<uint4 *>(sec + kSnapHdr + (size_t)T * kSnapRec);   // the track rings, then the global ring
    if (y <= kGParts) {
        FrameRun R;
        R.nf = gl;
        R.pre[0] = 0;
        for (int k = 0; k < MMW_RING_MAX; k++) {
            const int nk = k < gl ? clampi(hdr->g_n[k], 0, cfg.max_pts) : 0;
            R.src[k] = reinterpret_cast<const char *>(st.g_ring + ((size_t)s * cfg.ring + (hdr->g_slot[k] & (MMW_RING_MAX - 1)) % cfg.ring) * (size_t)cfg.max_pts * 8);
            R.pre[k + 1] = R.pre[k] + nk * kRowUnits;
        }
        move_units(R, true, nullptr, rings + (size_t)pre[T] * kRowUnits, (y - 1) * blockDim.x + tid, kGParts * blockDim.x);
        return;
    }
    for (int j = y - 1 - kGParts; j < T; j += gridDim.y - 1 - kGParts) {
        const TrackRec *rec = trk + order[j];
        const int rl = clampi(rec->ring_len, 0, cfg.ring);
        const double *base = st.trk_ring + ((size_t)s * cfg.t_cap + order[j]) * (size_t)cfg.ring * cfg.ring_rows * 8;
        FrameRun R;
        R.nf = rl;
        R.pre[0] = 0;
        for (int k = 0; k < MMW_RING_MAX; k++) {
            const int nk = k < rl ? min(max(rec->ring_n[k], 0), cfg.ring_rows) : 0;
            R.src[k] = reinterpret_cast<const char *>(base + (size_t)((rec->ring_slot[k] & (MMW_RING_MAX - 1)) % cfg.ring) * cfg.ring_rows * 8);
            R.pre[k + 1] = R.pre[k] + nk * kRowUnits;
        }
        move_units(R, true, nullptr, rings + (size_t)pre[j] * kRowUnits, tid, blockDim.x);
    }
}

// ---------------------------------------------------------------------------
// restore, first: does every section say what its directory entry says (and the header checked on the host)?  bad[0] =
// 1 + the first blob scene found wrong (0 = none).  `src_ring_rows`: the source's, which decided the rows a frame stores.
__global__ __launch_bounds__(256) void k_snap_check(DevCfg cfg, const char *__restrict__ blob, const mmw_snapshot_entry *__restrict__ dir, int n,
                                                    int src_ring_rows, int32_t *__restrict__ bad)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const mmw_snapshot_entry e = dir[i];
    const char *sec = blob + e.offset;
    const SceneHdr *h = reinterpret_cast<const SceneHdr *>(sec);
    const int T = h->n_tracks;
    bool ok = T == e.n_tracks && T >= 0 && T <= cfg.t_cap;
    int stored = 0, maxn = 0;
    if (ok && lane < T) {
        const TrackRec *rec = reinterpret_cast<const TrackRec *>(sec + kSnapHdr + (size_t)lane * kSnapRec);
        const int rl = rec->ring_len;
        if (rl < 0 || rl > cfg.ring) ok = false;
        for (int k = 0; k < MMW_RING_MAX; k++) if (k < rl && rec->ring_n[k] < 0) ok = false;
        const RingRows r = track_rows(clampi(rl, 0, cfg.ring), rec->ring_n, src_ring_rows);
        stored = r.stored;
        maxn = r.maxn;
        if ((rec->inner & 255) > cfg.ring) ok = false;
    }
    ok = __all(ok);
    const int trk_rows = wave_sum(stored), trk_max = wave_max(maxn);
    if (lane == 0) {
        int g_rows = 0, g_max = 0;
        bool hok = ok && h->g_len == e.g_len && h->g_len >= 0 && h->g_len <= cfg.ring && trk_max == e.max_trk_rows && h->err == e.err &&
                   hdr_ring_size(h->skipped) == e.ring_size && e.ring_size <= cfg.ring;
        for (int k = 0; k < MMW_RING_MAX; k++) {
            if (hok && k < h->g_len) {
                const int nk = h->g_n[k];
                if (nk < 0 || nk > cfg.max_pts) hok = false;
                g_rows += nk;
                g_max = max(g_max, nk);
            }
        }
        hok = hok && g_max == e.max_g_rows &&
              e.bytes == (unsigned long long)kSnapHdr + (unsigned long long)T * kSnapRec + (unsigned long long)(trk_rows + g_rows) * kRowBytes;
        if (!hok) bad[0] = i + 1;
    }
}

// restore, second: the last step's update lists (both parities, up to their lengths) and spawn lists no longer name tracks of
// the flagged scenes.  Grid: 2 * kUpdShards workgroups for the update lists, 2 for the spawn lists.
__global__ __launch_bounds__(256) void k_snap_scrub(DevCfg cfg, DevState st, const int32_t *__restrict__ flags)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b < 2 * kUpdShards) {
        const int p = b / kUpdShards, sh = b - p * kUpdShards;
        const size_t region = upd_region(cfg.n_scenes, cfg.t_cap);
        const int cnt = min(st.upd_count[p * kUpdWords + sh], (int)region);
        int32_t *list = st.upd_list + ((size_t)p * kUpdShards + sh) * region;
        for (int k = tid; k < cnt; k += blockDim.x) {
            const int e = list[k], s = e >> 12;
            if (s >= 0 && s < cfg.n_scenes && flags[s]) list[k] = e | (63 << 6);   // position 63 >= every n_tracks (t_cap <= 63 here)
        }
        return;
    }
    const int p = b - 2 * kUpdShards;
    const int cnt = min(st.spc_count[p], cfg.n_scenes);
    int32_t *list = st.spc_list + (size_t)p * cfg.n_scenes * 2;
    for (int k = tid; k < cnt; k += blockDim.x) {
        const int s = list[2 * k];
        if (s >= 0 && s < cfg.n_scenes && flags[s]) list[2 * k + 1] = cfg.t_cap;   // first new track past every track
    }
}

// restore, third: blob scene i -> scene dst[i] (grid as k_snap_pack's)
__global__ __launch_bounds__(256) void k_snap_unpack(DevCfg cfg, DevState st, const char *__restrict__ blob, const mmw_snapshot_entry *__restrict__ dir,
                                                     const int32_t *__restrict__ dst, int src_ring_rows, int32_t *__restrict__ kp_gen)
{
    __shared__ int pre[65];
    const int i = blockIdx.x, y = blockIdx.y, tid = threadIdx.x;
    const int s = dst[i];
    const char *sec = blob + dir[i].offset;
    const SceneHdr *bh = reinterpret_cast<const SceneHdr *>(sec);
    const int T = clampi(bh->n_tracks, 0, cfg.t_cap), gl = clampi(bh->g_len, 0, cfg.ring);
    const TrackRec *brec = reinterpret_cast<const TrackRec *>(sec + kSnapHdr);   // (stride kSnapRec: see rec_at)
    auto rec_at = [&](int j) { return reinterpret_cast<const TrackRec *>(reinterpret_cast<const char *>(brec) + (size_t)j * kSnapRec); };
    TrackRec *trk = st.trk + (size_t)s * cfg.t_cap;
    if (y == 0) {
        if (tid == 0) {
            SceneHdr h = *bh;
            h.n_tracks = T;
            h.g_len = gl;
            for (int k = 0; k < MMW_RING_MAX; k++) { h.g_slot[k] = k; h.g_n[k] = k < gl ? clampi(h.g_n[k], 0, cfg.max_pts) : 0; }
            h.need_db = 0;
            h.db_u = 0;
            h.n_upd = 0;
            h.skipped = (h.skipped & ~255) | 1;   // in no update list: the next _predict_all takes its tracks from this header
            st.hdr[s] = h;
            kp_gen[s] += 1;   // (the deferred keypoint scatter's generation, as k_reset bumps it: rows taken of the scene before this are dropped)
        }
        for (int k = tid; k < cfg.t_cap; k += blockDim.x) st.order[(size_t)s * cfg.t_cap + k] = k;
        unsigned long long *out = reinterpret_cast<unsigned long long *>(trk);
        const unsigned long long *in = reinterpret_cast<const unsigned long long *>(brec);
        for (int w = tid; w < T * kRecWords; w += blockDim.x) {
            const int r = w / kRecWords, k = w - r * kRecWords;
            // (ring_slot: version 1 stores the identity, and the identity is what is written -- a slot index from the blob would
            //  address the track ring unchecked in every later step)
            out[w] = (k >= kWRingSlot && k < kWRingSlot + 2) ? pack2(2 * (k - kWRingSlot), 2 * (k - kWRingSlot) + 1) : in[(size_t)r * kSnapRecWords + k];
        }
        return;
    }
    int my_rows = 0;
    if (tid < T) {
        const TrackRec *rec = rec_at(tid);
        my_rows = track_rows(clampi(rec->ring_len, 0, cfg.ring), rec->ring_n, src_ring_rows).stored;
    }
    track_row_prefix(T, &my_rows, pre);
    const uint4 *rings = reinterpret_cast<const uint4 *>(sec + kSnapHdr + (size_t)T * kSnapRec);
    if (y <= kGParts) {
        FrameRun R;
        R.nf = gl;
        R.pre[0] = 0;
        for (int k = 0; k < MMW_RING_MAX; k++) {
            const int nk = k < gl ? clampi(bh->g_n[k], 0, cfg.max_pts) : 0;
            R.dst[k] = reinterpret_cast<char *>(st.g_ring + ((size_t)s * cfg.ring + (k < cfg.ring ? k : 0)) * (size_t)cfg.max_pts * 8);
            R.pre[k + 1] = R.pre[k] + nk * kRowUnits;
        }
        move_units(R, false, rings + (size_t)pre[T] * kRowUnits, nullptr, (y - 1) * blockDim.x + tid, kGParts * blockDim.x);
        return;
    }
    for (int j = y - 1 - kGParts; j < T; j += gridDim.y - 1 - kGParts) {
        const TrackRec *rec = rec_at(j);
        const int rl = clampi(rec->ring_len, 0, cfg.ring);
        double *base = st.trk_ring + ((size_t)s * cfg.t_cap + j) * (size_t)cfg.ring * cfg.ring_rows * 8;
        FrameRun R;
        R.nf = rl;
        R.pre[0] = 0;
        for (int k = 0; k < MMW_RING_MAX; k++) {
            // (k_snap_check and the host have made sure that what the source stored fits this context's ring_rows)
            const int nk = k < rl ? min(min(max(rec->ring_n[k], 0), src_ring_rows), cfg.ring_rows) : 0;
            R.dst[k] = reinterpret_cast<char *>(base + (size_t)(k < cfg.ring ? k : 0) * cfg.ring_rows * 8);
            R.pre[k + 1] = R.pre[k] + nk * kRowUnits;
        }
        move_units(R, false, rings + (size_t)pre[j] * kRowUnits, nullptr, tid, blockDim.x);
    }
}

// ---------------------------------------------------------------------------
static int snap_parts_y(int max_tracks) { return 1 + kGParts + (max_tracks > 0 ? max_tracks : 0); }

void launch_snap_size(const DevCfg &cfg, const DevState &st, const int32_t *sel, int n, mmw_snapshot_entry *dir, unsigned long long *bytes,
                      unsigned long long base, hipStream_t stream)
{
    if (n > 0) hipLaunchKernelGGL(k_snap_size, dim3((n + 3) / 4), dim3(256), 0, stream, cfg, st, sel, n, dir, bytes);
    hipLaunchKernelGGL(k_snap_scan, dim3(1), dim3(1024), 0, stream, n, base, dir, bytes);
}
void launch_snap_pack(const DevCfg &cfg, const DevState &st, const int32_t *sel, int n, const mmw_snapshot_entry *dir, char *blob, int max_tracks,
                      hipStream_t stream)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_snap_pack, dim3(n, snap_parts_y(max_tracks)), dim3(256), 0, stream, cfg, st, sel, dir, blob);
}
void launch_snap_check(const DevCfg &cfg, const char *blob, const mmw_snapshot_entry *dir, int n, int src_ring_rows, int32_t *bad, hipStream_t stream)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_snap_check, dim3((n + 3) / 4), dim3(256), 0, stream, cfg, blob, dir, n, src_ring_rows, bad);
}
void launch_snap_restore(const DevCfg &cfg, const DevState &st, const char *blob, const mmw_snapshot_entry *dir, const int32_t *dst, const int32_t *flags,
                         int n, int max_tracks, int src_ring_rows, int32_t *kp_gen, hipStream_t stream)
{
    if (n <= 0) return;
#ifndef MMW_MUTANT_NO_SCRUB   // (diagnostic build `make DIAG=noscrub DIAGFLAGS=-DMMW_MUTANT_NO_SCRUB`, never the product: what
                              //  tests/test_gpu_snapshot.py's live-slot test must catch)
    hipLaunchKernelGGL(k_snap_scrub, dim3(2 * kUpdShards + 2), dim3(256), 0, stream, cfg, st, flags);
#endif
    hipLaunchKernelGGL(k_snap_unpack, dim3(n, snap_parts_y(max_tracks)), dim3(256), 0, stream, cfg, st, blob, dir, dst, src_ring_rows, kp_gen);
}

}  // namespace mmw
