// k_stance.hip -- the stance watch (mmw_stance_*): per scene zero or one rule, per live uid a class -- UPRIGHT, LOW, LYING -- from the
// head height of the posture keypoints, with hysteresis; falls and long lies as events with the track's uid in a per-scene ring.  A
// LOG: mmw_stance_sample appends behind every mmw_estimate_posture, the export drains.  Reads SceneHdr, order and of each live
// TrackRec the uid and seven keypoints; nothing of the step is touched.  No LDS, no atomics: a wave per scene, four scenes per
// workgroup, a lane per track AND per uid slot (t_cap <= 64) -- lane i holds track i's uid and keypoints, lane j slot j's words;
// uid -> slot is the one slot table's uid_slots_pick() (mmw_uidlist.hpp); the scene's rule comes through scalar loads -- s is
// wave-uniform and there is one entry per scene.
//   k_uid_rebase     (k_scan.hip) mmw_reset / mmw_reset_scenes / mmw_restore / mmw_set_stance_rules: the touched scenes' generation word
//   k_stance_zero    mmw_set_stance_rules: the listed scenes' counters and marks
//   k_stance_sample  free the slots of uids that are gone, hand free slots to the newcomers, every track's class
//   k_stance_count   rows (= scenes with a rule) and undelivered events per scene
//   k_pair_scan      (k_scan.hip) one workgroup: the two offset scans, the capacity decision, the totals
//   k_stance_write   rows, events, taken and the marks -- only if everything fits
#include <cstddef>
#include "mmw_device.hpp"
#include "mmw_uidlist.hpp"
#include "mmw_evlog.hpp"
#include "mmw_wave.hpp"
#include "mmw_kernels.hpp"

namespace mmw {

static_assert(sizeof(mmw_stance_rule) == 64 && alignof(mmw_stance_rule) == 8, "mmw_stance_rule");
static_assert(sizeof(mmw_stance_row) == 48, "mmw_stance_row");
static_assert(sizeof(mmw_stance_event) == 32 && alignof(mmw_stance_event) == 8 && offsetof(mmw_stance_event, t) == 24, "mmw_stance_event");
static_assert(sizeof(StanceRule) == 80 && sizeof(StanceCount) == 16, "the device's table entry and counters");
static_assert(MMW_STANCE_RULES_MAX == 1, "one rule per scene: the table entry of scene s is rules[s]");
static_assert(MMW_STANCE_UNKNOWN == 0 && MMW_STANCE_UPRIGHT == 1 && MMW_STANCE_LOW == 2 && MMW_STANCE_LYING == 3, "a class is two bits of a slot's word");
static_assert(MMW_TRACK_CAP_LIMIT <= 64, "one lane per track, one lane per uid slot");
static_assert(MMW_NKP == 57, "kp viewed as reshape(3, 19): row 1 the height, row 2 the depth");
constexpr int kHeadKp = 22;   // Head (joint 3), row 1

__device__ __forceinline__ int scene_rules(const StanceState &ss, int s) { return min(max(ss.n_rules[s], 0), MMW_STANCE_RULES_MAX); }

__global__ __launch_bounds__(256) void k_stance_zero(int n_scenes, const int32_t *__restrict__ flags, StanceCount *__restrict__ count)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n_scenes || !flags[s]) return;
    count[s] = StanceCount{0, 0, 0, 0};
}

__global__ __launch_bounds__(256) void k_stance_sample(DevCfg cfg, DevState st, StanceState ss, const int32_t *__restrict__ flags, const double *__restrict__ t)
{
    const auto [s, lane] = wave_scene();
    if (s >= cfg.n_scenes) return;     // (wave-uniform)
    if (flags && !flags[s]) return;    // (wave-uniform) not asked: not touched
    const int ord = ss.ug.ordinal[s];
    if (scene_rules(ss, s) == 0) {     // (wave-uniform) not watched: the scene's slots are void until it has a rule, and then rebased
        uid_slots_done(ss.ug, s, lane, 0, false, ord);
        return;
    }
    const int cap = cfg.t_cap, T = live_tracks(cfg, st, s);
    const size_t base = (size_t)s * cap;
    const bool rebased = ss.ug.rebased(s);
    const double tt = t ? t[s] : (double)ord;
    const int log0 = ss.log.logged[s];
    // the rule: the same address in every lane, so ten scalar loads
    const StanceRule *q = ss.rules + s;
    const double h_stand = q->h_stand, h_lie = q->h_lie, up_hi = q->up_hi, up_lo = q->up_lo, lie_hi = q->lie_hi, lie_lo = q->lie_lo;
    const double gap2 = q->gap2, fall_window = q->fall_window, long_lie = q->long_lie;

    // this lane's track: the uid and the seven keypoints the decision reads ...
    int cuid = -1;
    float k1 = 0.f, k2 = 0.f, k20 = 0.f, k21 = 0.f, k22 = 0.f, k39 = 0.f, k40 = 0.f;
    if (lane < T) {
        const TrackRec *rec = st.trk + base + live_slot(cfg, st, s, lane);
        cuid = rec->uid;
        k1 = rec->kp[1]; k2 = rec->kp[2];
        k20 = rec->kp[20]; k21 = rec->kp[21]; k22 = rec->kp[kHeadKp];
        k39 = rec->kp[39]; k40 = rec->kp[40];
    }
    // ... and this lane's slot: all old words are in registers before anything is stored
    int raw_owner = -1, s_word = 0;
    double s_since = 0.0, s_up = 0.0;
    if (lane < cap) {
        raw_owner = ss.ug.owner[base + lane];
        s_word = ss.word[base + lane];
        s_since = ss.t_since[base + lane];
        s_up = ss.t_upright[base + lane];
    }
    const auto [slot, fresh, release] = uid_slots_pick(cuid, raw_owner, rebased, T, cap, lane);   // (all 64 lanes)

    // the words of this lane's TRACK come out of its slot's lane (all 64 lanes, ahead of any condition)
    const int from_lane = slot < 0 ? lane : slot;
    const int slot_w = __shfl(s_word, from_lane);
    const double slot_since = __shfl(s_since, from_lane), slot_up = __shfl(s_up, from_lane);
    const int old_w = fresh ? 0 : slot_w;
    double t_since = fresh ? 0.0 : slot_since;
    double t_upright = fresh ? -__builtin_huge_val() : slot_up;

    // the decision, in the header's operation order: compares, and ONE subtraction each for the two ages
    const int old = old_w & kStanceClassMask;
    const double head = (double)k22;
    const float g0 = k1 - k2, g1 = k20 - k21, g2 = k39 - k40;
    const double sq = ((double)g0 * (double)g0 + (double)g1 * (double)g1) + (double)g2 * (double)g2;
    const bool plausible = lane < T && (head - head == 0.0) && !(sq > gap2);
    const bool a1 = head > (old == MMW_STANCE_UPRIGHT ? up_lo : old == MMW_STANCE_UNKNOWN ? h_stand : up_hi);
    const bool a0 = head > (old == MMW_STANCE_LYING ? lie_hi : old == MMW_STANCE_UNKNOWN ? h_lie : lie_lo);
    const int now = !plausible ? old : a1 ? MMW_STANCE_UPRIGHT : a0 ? MMW_STANCE_LOW : MMW_STANCE_LYING;
    const bool changed = now != old;   // (never without `plausible`)
    const double since_up = tt - t_upright;
    const bool fall = changed && now == MMW_STANCE_LYING && old != MMW_STANCE_UNKNOWN && since_up <= fall_window;
    int new_w = old_w;
    if (changed) {
        new_w = now;   // (bit 2 cleared)
        t_since = tt;
    }
    if (plausible && now == MMW_STANCE_UPRIGHT) t_upright = tt;
    const double lain = tt - t_since;
    const bool longlie = plausible && now == MMW_STANCE_LYING && !(new_w & kStanceLongLie) && lain >= long_lie;
    if (longlie) new_w |= kStanceLongLie;

    // the events: REBASED, then tracks in live order, CHANGE or FALL before LONG_LIE -- each lane's from the wave-exclusive prefix of
    // its count on, by the log's append rule (mmw_evlog.hpp)
    int n_ev;
    const int at = wave_excl_sum((changed ? 1 : 0) + (longlie ? 1 : 0), lane, n_ev);
    const auto ap = evlog_append(ss.log, s, log0, rebased ? 1 : 0, n_ev);
    if (rebased && lane == 0 && ap.keeps(log0)) ap.at(log0) = mmw_stance_event{s, -1, MMW_SEV_REBASED, 0, 0, T, tt};
    {
        int n = ap.first(at);
        if (changed) {
            if (ap.keeps(n)) ap.at(n) = mmw_stance_event{s, cuid, fall ? MMW_SEV_FALL : MMW_SEV_CHANGE, old, now, lane, tt};
            n++;
        }
        if (longlie && ap.keeps(n)) ap.at(n) = mmw_stance_event{s, cuid, MMW_SEV_LONG_LIE, MMW_STANCE_LYING, MMW_STANCE_LYING, lane, tt};
    }
    // the counters: lane 0 takes the ballots' popcounts
    const int n_fall = __popcll(__ballot(fall)), n_long = __popcll(__ballot(longlie));
    if (lane == 0 && (n_fall | n_long)) {
        StanceCount *k = ss.count + s;
        k->falls += n_fall;
        k->long_lies += n_long;
    }

    if (lane < T && slot >= 0) {   // (a track writes its own slot, all four words: no word has two writers)
        ss.ug.owner[base + slot] = cuid;
        ss.word[base + slot] = new_w;
        ss.t_since[base + slot] = t_since;
        ss.t_upright[base + slot] = t_upright;
    }
    uid_slots_done(ss.ug, s, lane, base + lane, release, ord);
    evlog_commit(ss.log, s, lane, ap);
}

__global__ __launch_bounds__(256) void k_stance_count(DevCfg cfg, StanceState ss)
{
    const auto [s, lane] = wave_scene();
    if (s >= cfg.n_scenes) return;   // (wave-uniform)
    evlog_count(ss.log, ss.sc.off, cfg.n_scenes, s, lane, scene_rules(ss, s));
}

__global__ __launch_bounds__(256) void k_stance_write(DevCfg cfg, StanceState ss, mmw_stance_row *__restrict__ rows, mmw_stance_event *__restrict__ events, int scene_base)
{
    if (!evlog_fits(ss.sc.totals)) return;   // (uniform over the launch) something does not fit: neither buffer, taken nor a mark is written
    const auto [s, lane] = wave_scene();
    const int S = cfg.n_scenes;
    if (s >= S) return;             // (wave-uniform)
    const LogWindow g = evlog_window(ss.log, s);
    const int row0 = ss.sc.off[s], ev0 = ss.sc.off[S + 1 + s];
    if (scene_rules(ss, s)) {       // (wave-uniform) lane j: slot j's owner and class; the row from four ballots
        const int cap = cfg.t_cap;
        const size_t base = (size_t)s * cap;
        const bool owned = lane < cap && !ss.ug.rebased(s) && ss.ug.owner[base + lane] != -1;   // (rebased and not yet sampled: every slot counts as free)
        const int cls = owned ? (ss.word[base + lane] & kStanceClassMask) : -1;
        const int n_up = __popcll(__ballot(cls == MMW_STANCE_UPRIGHT)), n_low = __popcll(__ballot(cls == MMW_STANCE_LOW));
        const int n_ly = __popcll(__ballot(cls == MMW_STANCE_LYING)), n_un = __popcll(__ballot(cls == MMW_STANCE_UNKNOWN));
        if (lane == 0) {            // ... and the totals become the marks
            StanceCount *kp = ss.count + s;
            const StanceCount k = *kp;
            rows[row0] = mmw_stance_row{scene_base + s, ss.rules[s].id, n_up, n_low, n_ly, n_un, k.falls, k.falls - k.mark_falls, k.long_lies,
                                        k.long_lies - k.mark_long_lies, g.lost, 0};
            kp->mark_falls = k.falls;
            kp->mark_long_lies = k.long_lies;
        }
    }
    evlog_drain(ss.log, s, lane, g, events, ev0, scene_base);
}

void launch_stance_zero(int n_scenes, const int32_t *flags, const StanceState &ss, hipStream_t st)
{
    hipLaunchKernelGGL(k_stance_zero, dim3((n_scenes + 255) / 256), dim3(256), 0, st, n_scenes, flags, ss.count);
}
void launch_stance_sample(const DevCfg &cfg, const DevState &s, const StanceState &ss, const int32_t *flags, const double *t, hipStream_t st)
{
    hipLaunchKernelGGL(k_stance_sample, dim3((cfg.n_scenes + 3) / 4), dim3(256), 0, st, cfg, s, ss, flags, t);
}
void launch_stance(const DevCfg &cfg, const StanceState &ss, mmw_stance_row *rows, int cap_rows, mmw_stance_event *events, int cap_events, int scene_base,
                   hipStream_t st)
{
    const dim3 grid((cfg.n_scenes + 3) / 4);
    hipLaunchKernelGGL(k_stance_count, grid, dim3(256), 0, st, cfg, ss);
    // (events <= S * depth can pass 2^31: the scan forms the totals in 64 bits and reports them saturated)
    launch_pair_scan(cfg.n_scenes, ss.sc.off, ss.sc.totals, cap_rows, cap_events, st);
    hipLaunchKernelGGL(k_stance_write, grid, dim3(256), 0, st, cfg, ss, rows, events, scene_base);
}

}  // namespace mmw
