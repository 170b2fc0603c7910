// k_zone.hip -- zone occupancy (mmw_zones_*): per defined zone a row of counts, and every change of a track's zone membership
// since the previous export as an event with the track's uid.  Reads SceneHdr, order and three lines of each live TrackRec after
// the step, the way k_report does; nothing of the step is touched.  No LDS, no atomics: a wave per scene, a lane per track
// (t_cap <= 64), the scene's zones walked with the wave -- s is wave-uniform, so the table comes through scalar loads.
//   k_uid_rebase    (k_scan.hip) mmw_reset / mmw_reset_scenes / mmw_restore / mmw_set_zones: the touched scenes' generation word
//   k_zone_count    rows (= defined zones) and events per scene
//   k_pair_scan     (k_scan.hip) one workgroup: the two offset scans, the capacity decision, the totals
//   k_zone_write    events, rows, the new baseline -- only if everything fits
#include <cstddef>
#include "mmw_device.hpp"
#include "mmw_uidlist.hpp"
#include "mmw_math.hpp"
#include "mmw_wave.hpp"
#include "mmw_kernels.hpp"

namespace mmw {

static_assert(sizeof(mmw_zone) == 48 && alignof(mmw_zone) == 8, "mmw_zone");
static_assert(sizeof(mmw_zone_row) == 32, "mmw_zone_row");
static_assert(sizeof(mmw_zone_event) == 24, "mmw_zone_event");
static_assert(MMW_ZONES_MAX == 16, "a membership mask is 16 bits; lane z writes the row of zone z");
static_assert(MMW_TRACK_CAP_LIMIT <= 64, "one lane per track");
constexpr int kZoneChunk = 2;   // zones whose table entries are requested together (20 SGPRs of bounds and margins; at 4 the compares' lane masks spill SGPRs in k_zone_write)
static_assert(MMW_ZONES_MAX % kZoneChunk == 0, "a chunk stays inside the scene's table entries");

// A scene's memberships, now and at the baseline, one track per lane in either list.  All 64 lanes of the wave call.
struct ZoneDiff {
    int T, Tb, nz;            // live tracks now / at the previous export; zones defined
    int cuid, buid;           // this lane's entry of either list (lanes past the list: -1)
    bool rebased;             // the generation moved since the baseline was taken: no LEAVE, membership by core alone
    bool is_static;           // (current list)
    unsigned now;             // current list: zones this lane's track is a member of now
    unsigned enter;           // current list: ... and was not at the baseline
    unsigned leave;           // baseline list: zones this lane's uid was a member of and is not now (or is not live any more)
};

__device__ __forceinline__ ZoneDiff zone_diff(const DevCfg &cfg, const DevState &st, const ZoneState &zs, int s, int lane)
{
    ZoneDiff d;
    d.T = live_tracks(cfg, st, s);
    d.Tb = zs.base.len(s, cfg.t_cap);
    d.nz = min(max(zs.n_zones[s], 0), MMW_ZONES_MAX);
    d.rebased = zs.base.ug.rebased(s);
    double px = 0.0, py = 0.0;
    d.cuid = -1;
    d.is_static = false;
    if (lane < d.T) {   // (uid, position and is_static off one record pointer: live_uid would load the order word twice)
        const TrackRec *rec = st.trk + (size_t)s * cfg.t_cap + live_slot(cfg, st, s, lane);
        d.cuid = rec->uid;
        px = rec->x[0];
        py = rec->x[1];
        d.is_static = rec->is_static != 0;
    }
    d.buid = zs.base.uid(s, cfg.t_cap, lane, d.Tb);
    const unsigned all = (1u << d.nz) - 1u;
    const unsigned bmask = (lane < d.Tb && !d.rebased) ? ((unsigned)zs.base_mask[(size_t)s * cfg.t_cap + lane] & all) : 0u;

    // what the baseline holds for this lane's track.  uid_find's loop with the mask dragged along: on uid_find and one fetch of the
    // mask behind it, k_zone_count and k_zone_write both take a 30th VGPR (profiles/uid_state_isa.txt)
    unsigned prev = 0u;
    for (int k = 0; k < d.Tb; k++) {   // (uniform)
        const int b = __shfl(d.buid, k);
        const unsigned m = (unsigned)__shfl((int)bmask, k);
        prev |= (lane < d.T && d.cuid == b) ? m : 0u;
    }

    // the zones: a member stays inside the widened rectangle, a newcomer has to reach the rectangle itself
    const mmw_zone *zt = zs.zones + (size_t)s * MMW_ZONES_MAX;
    unsigned now = 0u;
    for (int z0 = 0; z0 < d.nz; z0 += kZoneChunk) {   // (uniform; zt[z] is the same address in every lane)
        // a chunk's scalar loads are all in flight before the first compare: one round trip per chunk, not per zone.  The table
        // always holds MMW_ZONES_MAX entries per scene (zero past nz), so a chunk never reads outside it.
        double x0[kZoneChunk], x1[kZoneChunk], y0[kZoneChunk], y1[kZoneChunk], mg[kZoneChunk];
#pragma unroll
        for (int u = 0; u < kZoneChunk; u++) {
            const mmw_zone *q = zt + z0 + u;
            x0[u] = q->x0; x1[u] = q->x1; y0[u] = q->y0; y1[u] = q->y1; mg[u] = q->margin;
        }
#pragma unroll
        for (int u = 0; u < kZoneChunk; u++) {
            const int z = z0 + u;
            const bool core = x0[u] <= px && px < x1[u] && y0[u] <= py && py < y1[u];
            const bool wide = (x0[u] - mg[u]) <= px && px < (x1[u] + mg[u]) && (y0[u] - mg[u]) <= py && py < (y1[u] + mg[u]);
            const bool in = ((prev >> z) & 1u) ? wide : core;
            now |= (in && z < d.nz) ? (1u << z) : 0u;
        }
    }
    d.now = lane < d.T ? now : 0u;
    d.enter = d.now & ~prev;

    // what is left of every baseline entry's memberships
    const int at = uid_find(d.buid, d.cuid, d.T);
    const unsigned still = (unsigned)__shfl((int)d.now, at);   // (at = -1 reads lane 63: discarded)
    d.leave = bmask & ~(at >= 0 ? still : 0u);
    return d;
}

__global__ __launch_bounds__(256) void k_zone_count(DevCfg cfg, DevState st, ZoneState zs)
{
    const auto [s, lane] = wave_scene();
    if (s >= cfg.n_scenes) return;   // (wave-uniform)
    const ZoneDiff d = zone_diff(cfg, st, zs, s, lane);
    int n_leave, n_enter;
    wave_excl_sum(__popc(d.leave), lane, n_leave);
    wave_excl_sum(__popc(d.enter), lane, n_enter);
    if (lane == 0) {
        zs.sc.off[s] = d.nz;
        zs.sc.off[cfg.n_scenes + 1 + s] = (d.rebased ? 1 : 0) + n_leave + n_enter;
    }
}

// the events of one lane's mask, zones ascending, from `at` on
__device__ __forceinline__ void zone_events(mmw_zone_event *__restrict__ events, int at, unsigned mask, const mmw_zone *zt, int scene, int uid, int kind, int slot)
{
    while (mask) {   // (divergent: a lane per track, as many stores as it has events)
        const int z = __ffs((int)mask) - 1;
        mask &= mask - 1u;
        events[at++] = mmw_zone_event{scene, uid, kind, z, zt[z].id, slot};
    }
}

__global__ __launch_bounds__(256) void k_zone_write(DevCfg cfg, DevState st, ZoneState zs, mmw_zone_row *__restrict__ rows,
                                                    mmw_zone_event *__restrict__ events, int scene_base)
{
    if (!zs.sc.totals[2]) return;   // (uniform over the launch) something does not fit: neither buffer, the baseline nor a generation is written
    const auto [s, lane] = wave_scene();
    const int S = cfg.n_scenes;
    if (s >= S) return;             // (wave-uniform)
    const ZoneDiff d = zone_diff(cfg, st, zs, s, lane);
    const int row0 = zs.sc.off[s], ev0 = zs.sc.off[S + 1 + s];
    const mmw_zone *zt = zs.zones + (size_t)s * MMW_ZONES_MAX;

    // events: REBASED, then LEAVE in baseline order, then ENTER in current order -- each lane's at the wave-exclusive prefix of the popcounts
    int n_leave, n_enter;
    const int l_at = wave_excl_sum(__popc(d.leave), lane, n_leave);
    const int e_at = wave_excl_sum(__popc(d.enter), lane, n_enter);
    const int head = d.rebased ? 1 : 0;
    if (d.rebased && lane == 0) events[ev0] = mmw_zone_event{scene_base + s, -1, MMW_ZEV_REBASED, -1, -1, d.T};
    zone_events(events, ev0 + head + l_at, d.leave, zt, scene_base + s, d.buid, MMW_ZEV_LEAVE, lane);
    zone_events(events, ev0 + head + n_leave + e_at, d.enter, zt, scene_base + s, d.cuid, MMW_ZEV_ENTER, lane);

    // rows: lane z writes zone z from ballots over the tracks
    const int id = lane < d.nz ? zt[lane].id : 0;   // (a load per lane, in flight under the ballots)
    int count = 0, count_static = 0, entered = 0, left = 0;
    for (int z = 0; z < d.nz; z++) {   // (uniform)
        const int c = __popcll(__ballot((d.now >> z) & 1u)), cs = __popcll(__ballot(((d.now >> z) & 1u) && d.is_static));
        const int e = __popcll(__ballot((d.enter >> z) & 1u)), l = __popcll(__ballot((d.leave >> z) & 1u));
        if (lane == z) { count = c; count_static = cs; entered = e; left = l; }
    }
    if (lane < d.nz) rows[row0 + lane] = mmw_zone_row{scene_base + s, lane, id, count, count_static, entered, left, 0};

    // the current list is the next export's baseline (behind everything that read the old one: every lane's old entry is in its registers)
    zs.base.store(s, cfg.t_cap, lane, d.T, d.cuid);
    if (lane < d.T) zs.base_mask[(size_t)s * cfg.t_cap + lane] = (int32_t)d.now;
    zs.base.ug.settle(s, lane);
}

void launch_zones(const DevCfg &cfg, const DevState &s, const ZoneState &zs, mmw_zone_row *rows, int cap_rows, mmw_zone_event *events, int cap_events,
                  int scene_base, hipStream_t st)
{
    const dim3 grid((cfg.n_scenes + 3) / 4);
    hipLaunchKernelGGL(k_zone_count, grid, dim3(256), 0, st, cfg, s, zs);
    // (rows <= 16 S, events <= 1 S + 2 * 16 * S * t_cap: below 2^31, so the scan's saturation at INT32_MAX never fires here)
    static_assert((2LL * MMW_ZONES_MAX * MMW_TRACK_CAP_LIMIT + 1) * kUpdMaxScenes < (1LL << 31), "a zone export's totals fit an int32");
    launch_pair_scan(cfg.n_scenes, zs.sc.off, zs.sc.totals, cap_rows, cap_events, st);
    hipLaunchKernelGGL(k_zone_write, grid, dim3(256), 0, st, cfg, s, zs, rows, events, scene_base);
}

}  // namespace mmw
