// k_tripwire.hip -- tripwires (mmw_tripwires_*): per scene up to 16 directed segments, per wire the count of tracks that went
// across it either way, and every crossing as an event with the track's uid in a per-scene ring.  A LOG: mmw_tripwires_sample
// appends behind every step, the export drains.  Reads SceneHdr, order and two lines of each live TrackRec after the step; nothing
// of the step is touched.  No LDS, no atomics: a wave per scene, four scenes per workgroup, a lane per track AND per uid slot
// (t_cap <= 64) AND per wire -- lane i holds track i's uid, lane j slot j's words, lane z wire z's counters; uid -> slot is the one
// slot table's uid_slots_pick(), which is uid_find() both ways (mmw_uidlist.hpp); the scene's wires are walked with the wave -- s is
// wave-uniform, so the table comes through scalar loads.
//   k_uid_rebase       (k_scan.hip) mmw_reset / mmw_reset_scenes / mmw_restore / mmw_set_tripwires: the touched scenes' generation word
//   k_tripwire_zero    mmw_set_tripwires: the listed scenes' counters and marks
//   k_tripwire_sample  free the slots of uids that are gone, hand free slots to the newcomers, every track's side of every wire
//   k_tripwire_count   rows (= defined wires) and undelivered events per scene
//   k_pair_scan        (k_scan.hip) one workgroup: the two offset scans, the capacity decision, the totals
//   k_tripwire_write   rows, events, taken and the marks -- only if everything fits
#include <cstddef>
#include "mmw_device.hpp"
#include "mmw_uidlist.hpp"
#include "mmw_evlog.hpp"
#include "mmw_wave.hpp"
#include "mmw_kernels.hpp"

namespace mmw {

static_assert(sizeof(mmw_tripwire) == 48 && alignof(mmw_tripwire) == 8, "mmw_tripwire");
static_assert(sizeof(mmw_tripwire_row) == 32, "mmw_tripwire_row");
static_assert(sizeof(mmw_tripwire_event) == 32 && alignof(mmw_tripwire_event) == 8 && offsetof(mmw_tripwire_event, t) == 24, "mmw_tripwire_event");
static_assert(sizeof(TripWire) == 56 && sizeof(TripCount) == 16, "the device's table entry and counters");
static_assert(MMW_TRIPWIRES_MAX == 16, "a side word is 2 x 16 bits; lane z owns wire z's counters");
static_assert(MMW_TRACK_CAP_LIMIT <= 64, "one lane per track, one lane per uid slot");
constexpr int kWireChunk = 4;   // wires whose table entries are requested together (48 SGPRs of doubles: 104 SGPRs in all, nothing spilled; at 2 the sample is 0.65 us slower)
static_assert(MMW_TRIPWIRES_MAX % kWireChunk == 0, "a chunk stays inside the scene's table entries");
constexpr unsigned kSideNeg = 1u, kSidePos = 2u;   // (0: unknown)

__device__ __forceinline__ int scene_wires(const TripState &ts, int s) { return min(max(ts.n_wires[s], 0), MMW_TRIPWIRES_MAX); }

__global__ __launch_bounds__(256) void k_tripwire_zero(int n_scenes, const int32_t *__restrict__ flags, TripCount *__restrict__ count)
{
    const int i = blockIdx.x * 256 + threadIdx.x, s = i / MMW_TRIPWIRES_MAX;
    if (s >= n_scenes || !flags[s]) return;
    count[i] = TripCount{0, 0, 0, 0};
}

__global__ __launch_bounds__(256) void k_tripwire_sample(DevCfg cfg, DevState st, TripState ts, const int32_t *__restrict__ flags, const double *__restrict__ t)
{
    const auto [s, lane] = wave_scene();
    if (s >= cfg.n_scenes) return;     // (wave-uniform)
    if (flags && !flags[s]) return;    // (wave-uniform) not asked: not touched
    const int ord = ts.ug.ordinal[s];
    const int nw = scene_wires(ts, s);
    if (nw == 0) {                     // (wave-uniform) nothing to decide: the scene's slots are void until it has wires, and then rebased
        uid_slots_done(ts.ug, s, lane, 0, false, ord);
        return;
    }
    const int cap = cfg.t_cap, T = live_tracks(cfg, st, s);
    const size_t base = (size_t)s * cap;
    const bool rebased = ts.ug.rebased(s);
    const double tt = t ? t[s] : (double)ord;
    const int log0 = ts.log.logged[s];

    // this lane's track ...
    int cuid = -1;
    double px = 0.0, py = 0.0;
    if (lane < T) {
        const TrackRec *rec = st.trk + base + live_slot(cfg, st, s, lane);
        cuid = rec->uid;
        px = rec->x[0]; py = rec->x[1];
    }
    // ... and this lane's slot: both old words are in registers before anything is stored
    int raw_owner = -1, s_side = 0;
    if (lane < cap) {
        raw_owner = ts.ug.owner[base + lane];
        s_side = ts.side[base + lane];
    }
    const auto [slot, fresh, release] = uid_slots_pick(cuid, raw_owner, rebased, T, cap, lane);   // (all 64 lanes)

    // the side word of this lane's TRACK comes out of its slot's lane
    const unsigned slot_w = (unsigned)__shfl(s_side, slot < 0 ? lane : slot);   // (all 64 lanes, ahead of the condition)
    const unsigned old_w = fresh ? 0u : slot_w;
    const TripWire *wt = ts.wires + (size_t)s * MMW_TRIPWIRES_MAX;
    unsigned new_w = 0u, fwd = 0u, bwd = 0u;
    for (int z0 = 0; z0 < nw; z0 += kWireChunk) {   // (uniform; wt[z] is the same address in every lane)
        // a chunk's scalar loads are all in flight before the first product.  The table always holds MMW_TRIPWIRES_MAX entries per
        // scene (zero past nw), so a chunk never reads outside it.
        double ax[kWireChunk], ay[kWireChunk], dx[kWireChunk], dy[kWireChunk], len2[kWireChunk], band[kWireChunk];
#pragma unroll
        for (int u = 0; u < kWireChunk; u++) {
            const TripWire *q = wt + z0 + u;
            ax[u] = q->ax; ay[u] = q->ay; dx[u] = q->dx; dy[u] = q->dy; len2[u] = q->len2; band[u] = q->band;
        }
#pragma unroll
        for (int u = 0; u < kWireChunk; u++) {
            const int z = z0 + u;
            const double rx = px - ax[u], ry = py - ay[u];
            const double al = rx * dx[u] + ry * dy[u];      // along the wire
            const double c = dx[u] * ry - dy[u] * rx;       // > 0: left of A -> B
            const bool inside = 0.0 <= al && al <= len2[u];   // (false for a NaN or infinite position)
            const unsigned old = (old_w >> (2 * z)) & 3u;
            const unsigned now = (!inside || z >= nw) ? 0u : c > band[u] ? kSidePos : c < -band[u] ? kSideNeg : old;
            new_w |= now << (2 * z);
            fwd |= (old == kSideNeg && now == kSidePos) ? (1u << z) : 0u;
            bwd |= (old == kSidePos && now == kSideNeg) ? (1u << z) : 0u;
        }
    }
    if (lane >= T) new_w = fwd = bwd = 0u;

    // the events: REBASED, then tracks in live order, wires ascending inside a track -- each lane's from the wave-exclusive prefix of
    // the popcounts on, by the log's append rule (mmw_evlog.hpp)
    int n_ev;
    const int at = wave_excl_sum(__popc(fwd | bwd), lane, n_ev);
    const auto ap = evlog_append(ts.log, s, log0, rebased ? 1 : 0, n_ev);
    if (rebased && lane == 0 && ap.keeps(log0)) ap.at(log0) = mmw_tripwire_event{s, -1, MMW_TW_REBASED, -1, -1, T, tt};
    {
        unsigned mask = fwd | bwd;
        int n = ap.first(at);
        while (mask) {   // (divergent: as many stores as the lane's track has crossings)
            const int z = __ffs((int)mask) - 1;
            mask &= mask - 1u;
            if (ap.keeps(n)) ap.at(n) = mmw_tripwire_event{s, cuid, ((fwd >> z) & 1u) ? MMW_TW_FORWARD : MMW_TW_BACKWARD, z, wt[z].id, lane, tt};
            n++;
        }
    }
    // the counters: lane z takes wire z's from ballots over the tracks
    if (n_ev > 0) {   // (wave-uniform)
        int f = 0, b = 0;
        for (int z = 0; z < nw; z++) {   // (uniform)
            const int fz = __popcll(__ballot((fwd >> z) & 1u)), bz = __popcll(__ballot((bwd >> z) & 1u));
            if (lane == z) { f = fz; b = bz; }
        }
        if (lane < nw && (f | b)) {
            TripCount *k = ts.count + (size_t)s * MMW_TRIPWIRES_MAX + lane;
            k->forward += f;
            k->backward += b;
        }
    }

    if (lane < T && slot >= 0) {   // (a track writes its own slot, both words: no word has two writers)
        ts.ug.owner[base + slot] = cuid;
        ts.side[base + slot] = (int32_t)new_w;
    }
    uid_slots_done(ts.ug, s, lane, base + lane, release, ord);
    evlog_commit(ts.log, s, lane, ap);
}

__global__ __launch_bounds__(256) void k_tripwire_count(DevCfg cfg, TripState ts)
{
    const auto [s, lane] = wave_scene();
    if (s >= cfg.n_scenes) return;   // (wave-uniform)
    evlog_count(ts.log, ts.sc.off, cfg.n_scenes, s, lane, scene_wires(ts, s));
}

__global__ __launch_bounds__(256) void k_tripwire_write(DevCfg cfg, TripState ts, mmw_tripwire_row *__restrict__ rows, mmw_tripwire_event *__restrict__ events,
                                                        int scene_base)
{
    if (!evlog_fits(ts.sc.totals)) return;   // (uniform over the launch) something does not fit: neither buffer, taken nor a mark is written
    const auto [s, lane] = wave_scene();
    const int S = cfg.n_scenes;
    if (s >= S) return;             // (wave-uniform)
    const int nw = scene_wires(ts, s);
    const LogWindow g = evlog_window(ts.log, s);
    const int row0 = ts.sc.off[s], ev0 = ts.sc.off[S + 1 + s];
    if (lane < nw) {   // lane z: wire z's row, and its totals become the marks
        TripCount *kp = ts.count + (size_t)s * MMW_TRIPWIRES_MAX + lane;
        const TripCount k = *kp;
        rows[row0 + lane] = mmw_tripwire_row{scene_base + s, lane, ts.wires[(size_t)s * MMW_TRIPWIRES_MAX + lane].id, k.forward, k.backward,
                                             k.forward - k.mark_forward, k.backward - k.mark_backward, g.lost};
        kp->mark_forward = k.forward;
        kp->mark_backward = k.backward;
    }
    evlog_drain(ts.log, s, lane, g, events, ev0, scene_base);
}

void launch_tripwire_zero(int n_scenes, const int32_t *flags, const TripState &ts, hipStream_t st)
{
    hipLaunchKernelGGL(k_tripwire_zero, dim3((n_scenes * MMW_TRIPWIRES_MAX + 255) / 256), dim3(256), 0, st, n_scenes, flags, ts.count);
}
void launch_tripwire_sample(const DevCfg &cfg, const DevState &s, const TripState &ts, const int32_t *flags, const double *t, hipStream_t st)
{
    hipLaunchKernelGGL(k_tripwire_sample, dim3((cfg.n_scenes + 3) / 4), dim3(256), 0, st, cfg, s, ts, flags, t);
}
void launch_tripwires(const DevCfg &cfg, const TripState &ts, mmw_tripwire_row *rows, int cap_rows, mmw_tripwire_event *events, int cap_events, int scene_base,
                      hipStream_t st)
{
    const dim3 grid((cfg.n_scenes + 3) / 4);
    hipLaunchKernelGGL(k_tripwire_count, grid, dim3(256), 0, st, cfg, ts);
    // (events <= S * depth can pass 2^31: the scan forms the totals in 64 bits and reports them saturated)
    launch_pair_scan(cfg.n_scenes, ts.sc.off, ts.sc.totals, cap_rows, cap_events, st);
    hipLaunchKernelGGL(k_tripwire_write, grid, dim3(256), 0, st, cfg, ts, rows, events, scene_base);
}

}  // namespace mmw
