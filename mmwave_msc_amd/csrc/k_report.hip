// k_report.hip -- the live-track report (mmw_report_*): compact rows of the LIVE tracks with their uids, and the difference of
// every scene's uid list against the previous report's as events.  Reads SceneHdr, order and TrackRec after the step, the way
// k_table and k_features do; nothing of the step is touched.
//   k_report_baseline  the baseline of mmw_report_enable: the uids live now
//   k_uid_rebase       (k_scan.hip) mmw_reset / mmw_reset_scenes / mmw_restore: the touched scenes' generation word
//   k_report_count     rows and events per scene: a wave per scene, a lane per track (t_cap <= 64)
//   k_pair_scan        (k_scan.hip) one workgroup: the two offset scans, the capacity decision, the totals
//   k_report_write     rows (staged in LDS, stored as contiguous 16-byte pieces), events, the new baseline -- only if everything fits
#include <cstddef>
#include "mmw_device.hpp"
#include "mmw_uidlist.hpp"
#include "mmw_math.hpp"
#include "mmw_summary.hpp"
#include "mmw_dispatch.hpp"
#include "mmw_kernels.hpp"

namespace mmw {

static_assert(sizeof(mmw_track_report) == 324 && alignof(mmw_track_report) == 4, "mmw_track_report");
static_assert(sizeof(mmw_track_event) == 16, "mmw_track_event");
static_assert(offsetof(mmw_track_report, keypoints) + sizeof(float) * MMW_NKP == sizeof(mmw_track_report), "mmw_track_report has no padding");
static_assert(MMW_TRACK_CAP_LIMIT <= 64, "one lane per track");

constexpr int kRowWords = sizeof(mmw_track_report) / 4;        // 81: odd, so the lanes of a wave fill their rows without a bank conflict
constexpr int kStageRows = 16;                                 // rows staged per pass: one pass for all but the fullest scenes
constexpr int kStageWords = kStageRows * kRowWords + 4;        // + the alignment shift (below); a multiple of 4: every wave's block starts 16-byte aligned
static_assert(kStageWords % 4 == 0, "stage blocks stay 16-byte aligned");

// A scene's uid lists, current and baseline, one entry per lane, and which entries the other list does not hold (uid_find).
// All 64 lanes of the wave call.  A scene whose generation moved since its baseline was taken has no BORN / GONE (its uids restarted).
struct SceneDiff {
    int T, Tb;                       // live tracks now / at the previous report
    int cuid, buid;                  // this lane's entry of either list (lanes past the list: -1)
    bool rebased;
    unsigned long long born, gone;   // lanes of the current list not in the baseline / of the baseline not in the current list
};
__device__ __forceinline__ SceneDiff scene_diff(const DevCfg &cfg, const DevState &st, const ReportState &rp, int s, int lane)
{
    SceneDiff d;
    d.T = live_tracks(cfg, st, s);
    d.Tb = rp.base.len(s, cfg.t_cap);
    d.rebased = rp.base.ug.rebased(s);
    d.cuid = live_uid(cfg, st, s, lane, d.T);
    d.buid = rp.base.uid(s, cfg.t_cap, lane, d.Tb);
    const bool in_base = uid_find(d.cuid, d.buid, d.Tb) >= 0, in_cur = uid_find(d.buid, d.cuid, d.T) >= 0;   // (every lane, ahead of the conditions)
    d.born = __ballot(!d.rebased && lane < d.T && !in_base);
    d.gone = __ballot(!d.rebased && lane < d.Tb && !in_cur);
    return d;
}

// mmw_report_enable: the tracks live now are the baseline -- they produce no event
__global__ __launch_bounds__(256) void k_report_baseline(DevCfg cfg, DevState st, ReportState rp)
{
    const auto [s, lane] = wave_scene();
    if (s >= cfg.n_scenes) return;   // (wave-uniform)
    const int T = live_tracks(cfg, st, s);
    rp.base.store(s, cfg.t_cap, lane, T, live_uid(cfg, st, s, lane, T));
    if (lane == 0) { rp.base.ug.gen[s] = 0; rp.base.ug.seen[s] = 0; }
}

__global__ __launch_bounds__(256) void k_report_count(DevCfg cfg, DevState st, ReportState rp)
{
    const auto [s, lane] = wave_scene();
    if (s >= cfg.n_scenes) return;   // (wave-uniform)
    const SceneDiff d = scene_diff(cfg, st, rp, s, lane);
    if (lane == 0) {
        rp.sc.off[s] = d.T;
        rp.sc.off[cfg.n_scenes + 1 + s] = d.rebased ? 1 : __popcll(d.born) + __popcll(d.gone);
    }
}

// A wave per scene, a lane per track.  A row is 324 bytes: a lane storing its own row would scatter 4-byte pieces 324 bytes apart
// over the wave.  The lanes fill their rows in LDS instead (stride 81 words, odd: no bank conflict) and the wave then stores the
// scene's rows -- contiguous in the output -- as 16-byte pieces, 1 KiB per instruction.  A row starts 4-byte aligned only, so the
// image sits in LDS shifted by the output address's offset inside its 16 bytes: the pieces are 16-byte aligned on BOTH sides, and
// the up to three words in front of the first and behind the last piece go singly.
template <bool SITE>
__global__ __launch_bounds__(256) void k_report_write(DevCfg cfg, const mmw_scene_site *__restrict__ sites, DevState st, ReportState rp,
                                                      mmw_track_report *__restrict__ rows, mmw_track_event *__restrict__ events, int scene_base)
{
    __shared__ __attribute__((aligned(16))) uint32_t stage[4][kStageWords];
    if (!rp.sc.totals[2]) return;   // (uniform over the launch) something does not fit: neither buffer, the baseline nor a generation is written
    const auto [s, lane] = wave_scene();
    const int S = cfg.n_scenes;
    if (s >= S) return;          // (wave-uniform)
    const SceneDiff d = scene_diff(cfg, st, rp, s, lane);
    const int row0 = rp.sc.off[s], ev0 = rp.sc.off[S + 1 + s];
    const unsigned long long lt = lanemask_lt();

    // events: GONE in baseline order, then BORN in current order; a rebased scene's single event instead
    if (d.rebased) {
        if (lane == 0) events[ev0] = mmw_track_event{scene_base + s, -1, MMW_EV_REBASED, d.T};
    } else {
        if ((d.gone >> lane) & 1ULL) events[ev0 + __popcll(d.gone & lt)] = mmw_track_event{scene_base + s, d.buid, MMW_EV_GONE, lane};
        if ((d.born >> lane) & 1ULL) events[ev0 + __popcll(d.gone) + __popcll(d.born & lt)] = mmw_track_event{scene_base + s, d.cuid, MMW_EV_BORN, lane};
    }

    // rows
    double m_x = cfg.m_x, m_y = cfg.m_y, m_z = cfg.m_z, fade_max = cfg.fade_max, fade_min = cfg.fade_min, fade_weight = cfg.fade_weight;
    if constexpr (SITE) {   // (s is wave-uniform: scalar loads)
        const mmw_scene_site *w = sites + s;
        m_x = w->m_x; m_y = w->m_y; m_z = w->m_z;
        fade_max = w->v_screen_fade_size_max; fade_min = w->v_screen_fade_size_min; fade_weight = w->v_screen_fade_weight;
    }
    uint32_t *lds = stage[s & 3];   // (the wave's own block)
    for (int c = 0; c < d.T; c += kStageRows) {   // (uniform)
        const int n = min(kStageRows, d.T - c);
        uint32_t *dst = reinterpret_cast<uint32_t *>(rows + row0 + c);
        const int sh = (int)((reinterpret_cast<uintptr_t>(dst) >> 2) & 3);   // words past a 16-byte boundary
        if (lane >= c && lane < c + n) {
            mmw_track_report *o = reinterpret_cast<mmw_track_report *>(lds + sh + (lane - c) * kRowWords);
            const TrackRec *rec = st.trk + (size_t)s * cfg.t_cap + live_slot(cfg, st, s, lane);
            o->scene = scene_base + s;
            o->slot = lane;
            o->uid = d.cuid;
            o->flags = (rec->is_static ? MMW_REPORT_STATIC : 0) | (((d.born >> lane) & 1ULL) ? MMW_REPORT_BORN : 0);
            summary_fields(o, rec, cfg.dx, m_x, m_y, m_z, fade_max, fade_min, fade_weight);
        }
        wave_sync();
        const int N = n * kRowWords, head = min((4 - sh) & 3, N), body = (N - head) >> 2, tail = N - head - body * 4;
        if (lane < head) dst[lane] = lds[sh + lane];
        const uint4 *src4 = reinterpret_cast<const uint4 *>(lds + sh + head);
        uint4 *dst4 = reinterpret_cast<uint4 *>(dst + head);
        for (int p = lane; p < body; p += 64) dst4[p] = src4[p];
        if (lane < tail) dst[head + body * 4 + lane] = lds[sh + head + body * 4 + lane];
        wave_sync();   // (the next pass refills the image)
    }

    // the current list is the next report's baseline (behind everything that read the old one)
    rp.base.store(s, cfg.t_cap, lane, d.T, d.cuid);
    rp.base.ug.settle(s, lane);
}

void launch_report_baseline(const DevCfg &cfg, const DevState &s, const ReportState &rp, hipStream_t st)
{
    hipLaunchKernelGGL(k_report_baseline, dim3((cfg.n_scenes + 3) / 4), dim3(256), 0, st, cfg, s, rp);
}
void launch_report(const DevCfg &cfg, const mmw_scene_site *sites, const DevState &s, const ReportState &rp, mmw_track_report *rows, int cap_rows,
                   mmw_track_event *events, int cap_events, int scene_base, hipStream_t st)
{
    const dim3 grid((cfg.n_scenes + 3) / 4);
    hipLaunchKernelGGL(k_report_count, grid, dim3(256), 0, st, cfg, s, rp);
    // (rows <= S * t_cap, events <= 2 * S * t_cap: below 2^31, so the scan's saturation at INT32_MAX never fires for a report)
    static_assert(2LL * kUpdMaxScenes * MMW_TRACK_CAP_LIMIT < (1LL << 31), "a report's totals fit an int32");
    launch_pair_scan(cfg.n_scenes, rp.sc.off, rp.sc.totals, cap_rows, cap_events, st);
    with_flag(sites != nullptr, [&](auto SITE) {
        hipLaunchKernelGGL(k_report_write<decltype(SITE)::value>, grid, dim3(256), 0, st, cfg, sites, s, rp, rows, events, scene_base);
    });
}

}  // namespace mmw
