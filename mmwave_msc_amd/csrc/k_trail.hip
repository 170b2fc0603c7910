// k_trail.hip -- track trails (mmw_trails_*): per live uid a ring of its last `depth` sampled positions with the time of the first
// sample and the distance walked.  The one state of the exports that outlives a call: mmw_trails_sample appends to it, the export
// reads it.  Reads SceneHdr, order and two lines of each live TrackRec after the step; nothing of the step is touched.  No LDS, no
// atomics: a wave per scene, four scenes per workgroup, a lane per track AND per trail slot (t_cap <= 64) -- lane i holds track i's
// uid, lane j slot j's words, and uid -> slot is the one slot table's uid_slots_pick(), which is uid_find() both ways (mmw_uidlist.hpp).
//   k_uid_rebase    (k_scan.hip) mmw_reset / mmw_reset_scenes / mmw_restore: the touched scenes' generation word
//   k_trail_sample  free the slots of uids that are gone, hand free slots to the newcomers, append one sample per live track
//   k_trail_count   entries (= live tracks) and points per scene
//   k_pair_scan     (k_scan.hip) one workgroup: the two offset scans, the capacity decision, the totals
//   k_trail_write   the directory and the points, rings unwrapped oldest first -- only if everything fits
#include <cstddef>
#include "mmw_device.hpp"
#include "mmw_uidlist.hpp"
#include "mmw_wave.hpp"
#include "mmw_kernels.hpp"

namespace mmw {

static_assert(sizeof(mmw_trail_point) == 24 && alignof(mmw_trail_point) == 8, "mmw_trail_point");
static_assert(sizeof(mmw_trail_track) == 40 && alignof(mmw_trail_track) == 8, "mmw_trail_track");
static_assert(offsetof(mmw_trail_track, t_first) == 24 && offsetof(mmw_trail_point, flags) == 20, "no padding");
static_assert(MMW_TRACK_CAP_LIMIT <= 64, "one lane per track, one lane per trail slot");
static_assert(MMW_TRAIL_DEPTH_MAX == 256, "a scene's points stay below 2^14");

__global__ __launch_bounds__(256) void k_trail_sample(DevCfg cfg, DevState st, TrailState ts, const int32_t *__restrict__ flags, const double *__restrict__ t)
{
    const auto [s, lane] = wave_scene();
    if (s >= cfg.n_scenes) return;     // (wave-uniform)
    if (flags && !flags[s]) return;    // (wave-uniform) not asked: not touched
    const int cap = cfg.t_cap, T = live_tracks(cfg, st, s);
    const size_t base = (size_t)s * cap;
    const int ord = ts.ug.ordinal[s];
    const bool rebased = ts.ug.rebased(s);
    const double tt = t ? t[s] : (double)ord;

    // this lane's track ...
    int cuid = -1, pflags = 0;
    double x = 0.0, y = 0.0, z = 0.0;
    if (lane < T) {
        const TrackRec *rec = st.trk + base + live_slot(cfg, st, s, lane);
        cuid = rec->uid;
        x = rec->x[0]; y = rec->x[1]; z = rec->x[2];
        pflags = (rec->is_static != 0 ? MMW_TRAIL_STATIC : 0) | (rec->lifetime == 0.0 ? MMW_TRAIL_UPDATED : 0);
    }
    // ... and this lane's slot: every old word is in a register before anything is stored
    int raw_owner = -1, s_total = 0;
    double s_first = 0.0, s_trav = 0.0, s_lx = 0.0, s_ly = 0.0;
    if (lane < cap) {
        raw_owner = ts.ug.owner[base + lane];
        s_total = ts.total[base + lane];
        s_first = ts.t_first[base + lane];
        s_trav = ts.travelled[base + lane];
        s_lx = ts.last_x[base + lane];
        s_ly = ts.last_y[base + lane];
    }
    const auto [slot, fresh, release] = uid_slots_pick(cuid, raw_owner, rebased, T, cap, lane);   // (all 64 lanes)

    // the words of this lane's TRACK's slot come out of that slot's lane
    const int src = slot < 0 ? lane : slot;
    int total = __shfl(s_total, src);
    double t_first = __shfl(s_first, src), trav = __shfl(s_trav, src);
    const double lx = __shfl(s_lx, src), ly = __shfl(s_ly, src);
    if (fresh) { total = 0; trav = 0.0; }
    if (total == 0) {
        t_first = tt;
    } else {
        const double dx = x - lx, dy = y - ly;
        trav = trav + sqrt(dx * dx + dy * dy);
    }
    total += 1;

    if (lane < T && slot >= 0) {   // (a track writes its own slot, all of it: no word has two writers)
        const size_t at = base + slot;
        ts.ug.owner[at] = cuid;
        ts.total[at] = total;
        ts.t_first[at] = t_first;
        ts.travelled[at] = trav;
        ts.last_x[at] = x;
        ts.last_y[at] = y;
        ts.ring[at * (size_t)ts.depth + (unsigned)(total - 1) % (unsigned)ts.depth] = mmw_trail_point{tt, (float)x, (float)y, (float)z, pflags};
    }
    uid_slots_done(ts.ug, s, lane, base + lane, release, ord);
}

// What the export says of this lane's track.  All 64 lanes call.
struct TrailView {
    int T, uid, slot;        // live tracks; this lane's track's uid and trail slot (-1: none)
    int count, total;        // points exported of it; samples ever taken
    double t_first, travelled;
};

__device__ __forceinline__ TrailView trail_view(const DevCfg &cfg, const DevState &st, const TrailState &ts, int s, int lane, int max_per_track)
{
    TrailView v;
    const int cap = cfg.t_cap;
    const size_t base = (size_t)s * cap;
    v.T = live_tracks(cfg, st, s);
    v.uid = live_uid(cfg, st, s, lane, v.T);
    const int owner = (lane < cap && !ts.ug.rebased(s)) ? ts.ug.owner[base + lane] : -1;
    v.slot = uid_find(v.uid, owner, cap);
    v.count = v.total = 0;
    v.t_first = v.travelled = 0.0;
    if (v.slot >= 0) {
        v.total = ts.total[base + v.slot];
        v.t_first = ts.t_first[base + v.slot];
        v.travelled = ts.travelled[base + v.slot];
        v.count = min(max(v.total, 0), ts.depth);
        if (max_per_track > 0) v.count = min(v.count, max_per_track);
    }
    return v;
}

__global__ __launch_bounds__(256) void k_trail_count(DevCfg cfg, DevState st, TrailState ts, int max_per_track)
{
    const auto [s, lane] = wave_scene();
    if (s >= cfg.n_scenes) return;   // (wave-uniform)
    const TrailView v = trail_view(cfg, st, ts, s, lane, max_per_track);
    int n_points;
    wave_excl_sum(v.count, lane, n_points);
    if (lane == 0) {
        ts.sc.off[s] = v.T;
        ts.sc.off[cfg.n_scenes + 1 + s] = n_points;
    }
}

__global__ __launch_bounds__(256) void k_trail_write(DevCfg cfg, DevState st, TrailState ts, mmw_trail_track *__restrict__ dir,
                                                     mmw_trail_point *__restrict__ points, int max_per_track, int scene_base)
{
    if (!ts.sc.totals[2]) return;   // (uniform over the launch) something does not fit: neither buffer is written
    const auto [s, lane] = wave_scene();
    const int S = cfg.n_scenes;
    if (s >= S) return;             // (wave-uniform)
    const TrailView v = trail_view(cfg, st, ts, s, lane, max_per_track);
    const int e0 = ts.sc.off[s], p0 = ts.sc.off[S + 1 + s];
    int n_points;
    const int first = p0 + wave_excl_sum(v.count, lane, n_points);
    if (lane < v.T) dir[e0 + lane] = mmw_trail_track{scene_base + s, lane, v.uid, first, v.count, v.total, v.t_first, v.travelled};

    // track after track, the lanes stride over its points: sample n of a uid lies at n % depth, the exported ones are
    // total - count .. total - 1
    const unsigned depth = (unsigned)ts.depth;
    for (int e = 0; e < v.T; e++) {   // (uniform)
        const int cnt = __builtin_amdgcn_readfirstlane(__shfl(v.count, e));
        if (cnt <= 0) continue;
        const int slot = __builtin_amdgcn_readfirstlane(__shfl(v.slot, e)), tot = __builtin_amdgcn_readfirstlane(__shfl(v.total, e));
        const int at = __builtin_amdgcn_readfirstlane(__shfl(first, e));
        const mmw_trail_point *ring = ts.ring + ((size_t)s * cfg.t_cap + slot) * depth;
        for (int k = lane; k < cnt; k += 64) points[at + k] = ring[(unsigned)(tot - cnt + k) % depth];
    }
}

void launch_trail_sample(const DevCfg &cfg, const DevState &s, const TrailState &ts, const int32_t *flags, const double *t, hipStream_t st)
{
    hipLaunchKernelGGL(k_trail_sample, dim3((cfg.n_scenes + 3) / 4), dim3(256), 0, st, cfg, s, ts, flags, t);
}
void launch_trails(const DevCfg &cfg, const DevState &s, const TrailState &ts, mmw_trail_track *dir, int cap_tracks, mmw_trail_point *points, int cap_points,
                   int max_per_track, int scene_base, hipStream_t st)
{
    const dim3 grid((cfg.n_scenes + 3) / 4);
    hipLaunchKernelGGL(k_trail_count, grid, dim3(256), 0, st, cfg, s, ts, max_per_track);
    // (points <= S * t_cap * depth can pass 2^31: the scan forms the totals in 64 bits and reports them saturated)
    launch_pair_scan(cfg.n_scenes, ts.sc.off, ts.sc.totals, cap_tracks, cap_points, st);
    hipLaunchKernelGGL(k_trail_write, grid, dim3(256), 0, st, cfg, s, ts, dir, points, max_per_track, scene_base);
}

}  // namespace mmw
