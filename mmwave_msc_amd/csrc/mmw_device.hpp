// mmw_device.hpp -- device-side data layout shared by the HIP kernels and the C-ABI glue.
// gfx950 only (wave64, 160 KiB LDS/CU).  fp64 everywhere a decision is taken.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mmw.h"
#include "mmw_uidlist.hpp"
#include "mmw_evlog.hpp"

namespace mmw {

constexpr int kThreads = 256;       // 4 waves per workgroup, one workgroup per scene
constexpr int kWaves = kThreads / 64;
constexpr int kGateChunk = 16;      // tracks whose gate matrices sit in LDS at once
constexpr int kGateRec = 44;        // doubles per gate record: Ci[36] | log|det| | predicted position hx[6] | pad
constexpr int kLeafSize = 30;       // sklearn BallTree default leaf_size (DBSCAN passes it through)
constexpr int kSkNeighbors = 5;     // NearestNeighbors' default n_neighbors, left alone by DBSCAN.fit (sklearn/cluster/_dbscan.py:410-418):
                                    // clouds of n // 2 <= 5 points are answered by brute force, not by the tree (neighbors/_base.py:622-633)
constexpr int kMaxLeaves = 32;      // n <= 1920 -> <= 63 nodes -> <= 32 leaves
constexpr int kBigCloudMax = 30 * 64;  // = 1920: the largest cloud whose BallTree carve-up fits the LDS; larger ones (work list 2) run on slabs in global memory
constexpr int kMaxNodes = 63;

// per-scene error bits (sticky until mmw_reset)
// ERR_NONFINITE_*: apply_DBscan was reached with a NaN / an infinite value in its cloud -- sklearn's input validation raises
// ValueError there (Utils.py:272-278): "contains NaN" when any value is NaN, else "contains infinity" (oracle/c: orc_check_finite)
enum : int { ERR_SINGULAR = 1, ERR_DIVZERO = 2, ERR_CAPACITY = 4, ERR_BADCOUNT = 8, ERR_NONFINITE_NAN = 16, ERR_NONFINITE_INF = 32 };
constexpr int kDbRaised = -2;   // db_n of a frame whose apply_DBscan call "raised" (MMW_DB_RAISED; -1 = not called)

struct DevCfg {
    int32_t ring;            // FB_FRAMES_BATCH + 1
    int32_t db_min_samples;
    int32_t tr_max_tracks;
    int32_t kf_enable_est;
    int32_t model_min_input;
    int32_t dx;              // 9 / 6
    int32_t ring_rows;
    int32_t t_cap;
    int32_t max_pts;
    int32_t n_scenes;
    int32_t dense_min_units;  // Kalman kernels laid out over tracks when the context has more 4-track waves than this (mmw_kalman.hpp)
    int32_t seek_inner;       // Tracking.py:656 active: seek_inner_clusters after every associate_pointcloud (k_inner)
    int32_t db_points_thres, fb_frames_batch_static;
    int32_t big_live;        // this step's large clouds may be claimed WHILE k_track runs (side workers on, start-up frames over): they are pushed with a release; otherwise plainly, for the kernels behind k_track
    int32_t fused;           // the step is k_scene (one workgroup runs a scene's whole track(): k_scene.hip) + the worker blocks of k_post: contexts whose scenes are all resident at once
    int32_t epoch;           // number of this step (api_step.hip: counts committed steps of the context): tags the claim words of the DBSCAN queues
    int32_t var_ring, side_worker;   // side_worker: k_chain runs beside k_track on a second stream (api_step.hip); var_ring: a global ring size was changed (mmw_set_batch_size): k_track reads ring sizes from the headers
    double db_spread_thres, db_inner_eps;
    double db_z_weight, db_range_weight, db_eps;
    double tr_lifetime_dynamic, tr_lifetime_static, tr_vel_thres, tr_gate;
    double kf_q_std, kf_p_init, kf_group_disp_est_init, kf_a_n, kf_est_pointnum;
    double kf_spread_lim[6];
    double kf_a_spr;
    double intensity_mu, intensity_std;
    double s_height, tilt_cos, tilt_sin;
    double m_x, m_y, m_z, fade_max, fade_min, fade_weight;   // output step (k_table)
};

// 64 B header per scene
struct SceneHdr {
    int32_t n_tracks;
    int32_t g_len;                 // frames in the global BatchedData ring
    int32_t g_n[MMW_RING_MAX];     // rows per frame, oldest first
    int32_t g_slot[MMW_RING_MAX];  // permutation: physical slot of the k-th oldest frame
    int32_t need_db;               // set by the track kernel: run apply_DBscan this frame
    int32_t err;
    int32_t db_u;
    int32_t next_uid;              // TrackBuffer.next_track_id (Tracking.py:509,588)
    int32_t n_upd;                 // tracks after _maintain_tracks of this frame = what _update_all covers (k_track -> k_post)
    int32_t skipped;               // bit 0: the last frame was empty for this scene (k_track returned at once): its tracks are in no update list;
                                   // bits 8..15: size of the global ring after BatchedData.change_buffer_size (0 = FB_FRAMES_BATCH + 1);
                                   // bits 16..23: two per PHYSICAL slot p of the global ring -- bit 16 + 2p: the frame stored there holds a
                                   // NaN, bit 17 + 2p: an infinite value (any of the 8 columns; set by whoever writes a frame into the slot)
};
static_assert(sizeof(SceneHdr) == 64, "SceneHdr");
constexpr int kSkipRingShift = 8, kSkipRingMask = 255, kSkipNfShift = 16, kSkipNfMask = 255;
__host__ __device__ inline int hdr_ring_size(int skipped) { return (skipped >> kSkipRingShift) & kSkipRingMask; }
// bit 0: a NaN, bit 1: an infinite value among the 8 columns of one row (x, y, z, vx, vy, vz, doppler, peakVal).  One
// v_cmp_class_f64 per value; the second pass only for the (rare) row that has one.
__device__ __forceinline__ int row_nonfinite_bits(const double2 (&r)[4])
{
    constexpr int kNanInf = 0x3 | 0x4 | 0x200;   // sNaN | qNaN | -inf | +inf
    bool any = false;
#pragma unroll
    for (int u = 0; u < 4; u++) any = any || __builtin_amdgcn_class(r[u].x, kNanInf) || __builtin_amdgcn_class(r[u].y, kNanInf);
    if (!any) return 0;
    bool nan = false, inf = false;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        nan = nan || __builtin_amdgcn_class(r[u].x, 0x3) || __builtin_amdgcn_class(r[u].y, 0x3);
        inf = inf || __builtin_amdgcn_class(r[u].x, 0x204) || __builtin_amdgcn_class(r[u].y, 0x204);
    }
    return (nan ? 1 : 0) | (inf ? 2 : 0);
}
// The flags word after a frame with row bits `frame_bits` has been written into physical slot `phys`, and what the live
// frames gs[0 .. len) hold together (bit 0 NaN, bit 1 inf).
__host__ __device__ inline int nf_flags_with(int flags, int phys, int frame_bits) { return (flags & ~(3 << (2 * phys))) | ((frame_bits & 3) << (2 * phys)); }
// which ValueError sklearn raises for a cloud with these bits (NaN takes precedence)
__host__ __device__ inline int nf_error_of(int bits) { return (bits & 1) ? ERR_NONFINITE_NAN : ((bits & 2) ? ERR_NONFINITE_INF : 0); }
// What the reference divides the detected-points TLV's x, y, z by: `2 ** xyzQFormat` with the u16 Q format as a numpy int64
// (ReadDataIWR1443.py:118), which wraps -- 2^q for q <= 62, -2^63 for q = 63, 0 for q >= 64 (then x / 0 = +-inf, 0 / 0 = NaN).
__host__ __device__ inline double xyz_q_divisor(unsigned q) { return q <= 62 ? (double)(1ull << q) : (q == 63 ? -9223372036854775808.0 : 0.0); }

// The device-resident radar readers (mmw_uart_open; k_uart.hip): per scene what a ReadIWR14xx object keeps between two read()
// calls -- byteBufferLength, and the 2^15-byte byteBuffer itself in UartState::buf -- with main.py's `t` (the time of the last
// read that gave points) and the two scales of the scene's configParameters the decode needs.
constexpr int kUartBuf = MMW_UART_BUFFER;
struct UartScene {
    double t_last;
    double half_bins;      // numDopplerBins / 2 - 1
    double doppler_res;    // dopplerResolutionMps
    int32_t len;           // byteBufferLength
    int32_t reserved;
};
static_assert(sizeof(UartScene) == 32, "UartScene");
struct UartState {
    uint8_t *buf;          // [S][kUartBuf], 16-byte aligned
    UartScene *scene;      // [S]
};
// The radar log (mmw_uart_log_enable; k_uart_read<., ., LOG = true> stages, k_uart_log.hip exports): per scene the frame its last read()
// decoded, as it came off the wire -- the DataLogging.py recorder's `dataOk, frameNumber, detObj`.  A read that gives
// MMW_UART_POINTS rewrites the scene's word (all of it but `range_scale`, which the host sets) and its first `count` objects;
// every other status leaves both alone.
struct UartLogWord {
    double t;              // `now` of the read that decoded the frame
    double range_scale;    // rangeIdxToMeters (mmw_uart_log_enable / mmw_uart_open; no kernel writes it)
    uint32_t frame;        // frameNumber
    int32_t count;         // tlv_numObj (<= max_pts)
    uint32_t head;         // the TLV head word: numObj | xyzQFormat << 16
    int32_t fresh;         // 1 = not exported yet
};
static_assert(sizeof(UartLogWord) == 32, "UartLogWord");
struct UartLog {
    UartLogWord *word;     // [S], 16-byte aligned
    uint8_t *obj;          // [S][max_pts][12] the wire objects (rangeIdx, dopplerIdx, peakVal, x, y, z: six little-endian u16)
};

// One ClusterTrack.  187 doubles = 1496 B.
struct TrackRec {
    double x[9];
    double P[81];
    double centroid[6];
    double minv[6];
    double maxv[6];
    double spread[6];
    double gd[36];
    double n_est;
    double lifetime;
    int32_t point_num;
    int32_t is_static;
    int32_t ring_len;
    int32_t uid;                   // creation ordinal inside the scene (stable identity for views)
    int32_t ring_n[MMW_RING_MAX];
    int32_t ring_slot[MMW_RING_MAX];
    float kp[MMW_NKP];
    int32_t inner;                 // seek_inner_clusters state (cfg.seek_inner only): bits 0..7 = track.batch.size (what
                                   // BatchedData.change_buffer_size set, Tracking.py:60-64), bit 8 = associate_pointcloud ran this frame
};
constexpr int kInnerTouched = 256;
static_assert(sizeof(TrackRec) == 187 * 8, "TrackRec");

struct DevState {
    SceneHdr *hdr;        // [S]
    int32_t *order;       // [S][t_cap]  effective_tracks position -> physical record (always a permutation)
    TrackRec *trk;        // [S][t_cap]
    double *trk_ring;     // [S][t_cap][ring][ring_rows][8]
    double *g_ring;       // [S][ring][max_pts][8]
    const float *default_posture;  // [57]
    unsigned long long *stats;     // [kStatSlots][32] algorithmic-byte / work counters (see mmw_stats_get), summed on read-out
    int32_t *db_list;              // [4][S] scenes whose apply_DBscan the cell count could not finish this step, filled by k_track: list 3 = clouds <= 256 points (k_post), list 2 = clouds of more than kBigCloudMax points (k_dbscan_huge); rows 0 and 1 are the rings of the two queues below
    int32_t *db_count;             // [2][4] list lengths, double-buffered by step parity (list 3)
    int32_t *q;                    // [kQWords] the early queue = list 0 (n_scenes entries, 0 = empty, else scene + 1), per step parity p at
                                   // q[8p + ...]: kQCount pushes, kQHead claims, kQDone finished items of the step (reset a step ahead by
                                   // k_track); shared: q[kQStop] = last step whose k_post has begun (monotonic), q[kQTimeout];
                                   // the same three words at q[kQBig + 8p + ...] for the queue of the larger clouds (ring = list 1)
    int32_t *perm;                 // [2][S] by step parity: scene handled by unit b of k_predict / k_track / k_post, heaviest scenes (most tracks) first; k_post builds the next step's
    double *gate_buf;              // [S][t_cap][kGateRec] gate matrices of this frame, by effective_tracks position (k_predict -> k_track)
    int32_t *upd_count;            // [2][kUpdWords] by step parity: tracks in each of the kUpdShards update lists of this frame (k_track -> k_post, next k_predict)
    int32_t *upd_list;             // [2][kUpdShards][upd_region] ... and the tracks: one packed word each (upd_pack: scene, position, record slot) --
                                   // _update_all / _predict_all are laid out over the TRACKS of the context, four per wave
    int32_t *spc_count;            // [2] by step parity: scenes the next k_predict cannot take from the update lists ...
    int32_t *spc_list;             // [2][S][2] ... (scene, first new track): scenes that spawned tracks this frame
    int32_t *inner_buf;            // [S][kInnerHdr + inner_cap] seek_inner_clusters calls of the last frame (cfg.seek_inner; mmw_get_inner)
    int32_t inner_cap;             // label words per scene
    char *huge_scratch;            // [workers][huge_stride] BallTree carve-ups of the clouds of more than kBigCloudMax points (k_dbscan_huge); null when no ring of the context can hold one
    size_t huge_stride;
};
// The scratch of one live-track export's call in flight (k_report.hip, k_cloud.hip, k_skeleton.hip; scanned by k_scan.hip).  All
// device memory; nothing is kept between two calls.  What the two counts are:
//   report     rows, events          clouds     directory entries, points          skeletons  emitted entries, live tracks
//   zones      rows (defined zones), events                                        trails     directory entries, points
struct ExportScratch {
    int32_t *off;         // [2][S + 1] the two counts per scene, scanned in place into offsets; [S] = the total
    int32_t *totals;      // [4] the two totals (saturated at INT32_MAX), 1 = both fit the caller's capacities (the device's decision), 0
};
// mmw_report_enable: what the live-track report keeps between two reports (k_report.hip).  All device memory.
struct ReportState {
    UidBaseline base;     // the uids live at the previous report, and the generation they were taken in (mmw_uidlist.hpp)
    ExportScratch sc;     // rows / events of the report in flight
};
// mmw_set_zones: the zone table and what the zone export keeps between two exports (k_zone.hip).  All device memory.  A baseline of
// its own, of the report's type: reports need not be enabled, the two are consumed at different times, and mmw_set_zones bumps
// this generation alone, for the scenes it lists.
struct ZoneState {
    const mmw_zone *zones;     // [S][MMW_ZONES_MAX] the table (one copy of mmw_set_zones; read with scalar loads)
    const int32_t *n_zones;    // [S] zones defined per scene, behind the table in the same allocation
    UidBaseline base;          // the uids live at the previous successful export ...
    int32_t *base_mask;        // [S][t_cap] ... and the zones each was a member of: bit z = zone z
    ExportScratch sc;          // rows / events of the export in flight
};
// mmw_trails_enable: what the track trails keep from one mmw_trails_sample to the next (k_trail.hip).  All device memory.  A scene
// has t_cap trail SLOTS, handed out by the one slot table (UidSlots, mmw_uidlist.hpp).  The slot words are arrays over [S][t_cap]
// (lane j of a scene's wave holds slot j), 40 bytes a slot together.
struct TrailState {
    int32_t depth;             // ring entries per slot, 1 .. MMW_TRAIL_DEPTH_MAX
    mmw_trail_point *ring;     // [S][t_cap][depth] sample n (0-based) of a uid lies at n % depth
    UidSlots ug;               // the scenes' uid generation and the slot table that belongs to it: owner, call ordinal
    int32_t *total;            // [S][t_cap] samples ever taken of the slot's uid
    double *t_first;           // [S][t_cap] t of its first sample
    double *travelled;         // [S][t_cap] path length in the x/y plane over all its samples
    double *last_x, *last_y;   // [S][t_cap] the fp64 position of its newest sample
    ExportScratch sc;          // entries / points of the export in flight
};
// mmw_tripwires_enable: the wire table and what the tripwires keep from one mmw_tripwires_sample to the next (k_tripwire.hip).  All
// device memory.  A table entry is what the HOST derived of an mmw_tripwire (mmw_set_tripwires): the device takes no sqrt.  A uid's
// side word lies in the slot that the one slot table (UidSlots, mmw_uidlist.hpp) gives it.  (The member order -- the log in front,
// `side` behind `count`, the scratch in front of the slot table -- is the one that leaves the kernels' registers and the sampler's
// kernarg loads as they were, profiles/evlog_isa.txt and DESIGN.md 8m; likewise StanceState's.)
struct TripWire { double ax, ay, dx, dy, len2, band; int32_t id, pad_; };   // 56 bytes
struct TripCount { int32_t forward, backward, mark_forward, mark_backward; };   // totals since the wires were set; ... at the previous successful export
struct TripState {
    EventLog<mmw_tripwire_event> log;   // the crossings (mmw_evlog.hpp), depth 1 .. MMW_TRIPWIRE_LOG_MAX
    const TripWire *wires;     // [S][MMW_TRIPWIRES_MAX] the table (one copy of mmw_set_tripwires; read with scalar loads)
    const int32_t *n_wires;    // [S] wires defined per scene, behind the table in the same allocation
    TripCount *count;          // [S][MMW_TRIPWIRES_MAX] lane z of a scene's wave owns wire z's
    int32_t *side;             // [S][t_cap] the slot's uid's sides, two bits per wire: 0 unknown, 1 negative, 2 positive
    ExportScratch sc;          // rows / events of the export in flight
    UidSlots ug;               // the scenes' uid generation and the slot table that belongs to it: owner, call ordinal
};
// mmw_stance_enable: the rule table and what the stance watch keeps from one mmw_stance_sample to the next (k_stance.hip).  All
// device memory.  A table entry is what the HOST derived of an mmw_stance_rule (mmw_set_stance_rules): the device does no arithmetic
// on a threshold.  A uid's words lie in the slot that the one slot table (UidSlots, mmw_uidlist.hpp) gives it.
struct StanceRule { double h_stand, h_lie, up_hi, up_lo, lie_hi, lie_lo, gap2, fall_window, long_lie; int32_t id, pad_; };   // 80 bytes
struct StanceCount { int32_t falls, long_lies, mark_falls, mark_long_lies; };   // totals since the rule was set; ... at the previous successful export
constexpr int kStanceClassMask = 3, kStanceLongLie = 4;   // a slot's word: bits 0-1 the class, bit 2 "LONG_LIE given in this episode"
struct StanceState {
    EventLog<mmw_stance_event> log;   // the changes, falls and long lies (mmw_evlog.hpp), depth 1 .. MMW_STANCE_LOG_MAX
    int32_t *word;             // [S][t_cap] the slot's uid's class and episode bit
    const StanceRule *rules;   // [S][MMW_STANCE_RULES_MAX] the table (one copy of mmw_set_stance_rules; read with scalar loads)
    const int32_t *n_rules;    // [S] 0 or 1, behind the table in the same allocation
    double *t_since;           // [S][t_cap] t of the sample that entered the current class
    double *t_upright;         // [S][t_cap] t of the newest sample that classed the uid UPRIGHT, -inf if never
    StanceCount *count;        // [S] lane 0 of a scene's wave owns it
    UidSlots ug;               // the scenes' uid generation and the slot table that belongs to it: owner, call ordinal
    ExportScratch sc;          // rows / events of the export in flight
};
// mmw_heat_enable: the grid table and what the heat maps keep from one mmw_heat_sample to the next (k_heat.hip).  All device memory.
// A table entry is the caller's mmw_heat_grid as it is (the host only checks it).  The first state here that is a dense per-scene
// array: `cells` cells a scene, three arrays over [S][cells] (a wave strides over a scene's words).  A uid's last cell and time lie
// in the slot that the one slot table (UidSlots, mmw_uidlist.hpp) gives it.
struct HeatGrid { double x0, y0, cell, max_gap; int32_t nx, ny, id, pad_; };   // 48 bytes
struct HeatScene { int32_t calls, outside; double t_first, t_last; };          // since the counters last restarted (set call, CLEAR export)
struct HeatState {
    int32_t cells;             // cell capacity per scene, 1 .. MMW_HEAT_CELLS_MAX
    const HeatGrid *grids;     // [S][MMW_HEAT_GRIDS_MAX] the table (one copy of mmw_set_heat_grids; read with scalar loads)
    const int32_t *n_grids;    // [S] 0 or 1, behind the table in the same allocation
    double *dwell;             // [S][cells] time credited to the cell
    int32_t *samples;          // [S][cells] samples taken in it ...
    int32_t *visits;           // [S][cells] ... of which began a stay
    int32_t *last_cell;        // [S][t_cap] the slot's uid's cell at its newest sample, -1 = outside
    double *last_t;            // [S][t_cap] ... and that sample's t
    HeatScene *scene;          // [S] lane 0 of a scene's wave owns it
    UidSlots ug;               // the scenes' uid generation and the slot table that belongs to it: owner, call ordinal
    ExportScratch sc;          // rows / cells of the export in flight
};

// The live list of scene s, as every export walks it: T = live_tracks lanes, lane -> live_slot -> the scene's TrackRec.  Both are
// clamped into range, so a damaged state gives the same list -- report row i, cloud entry i, skeleton i -- in every export.
__device__ __forceinline__ int live_tracks(const DevCfg &cfg, const DevState &st, int s) { return min(max(st.hdr[s].n_tracks, 0), cfg.t_cap); }
__device__ __forceinline__ int live_slot(const DevCfg &cfg, const DevState &st, int s, int lane)
{
    return min(max(st.order[(size_t)s * cfg.t_cap + lane], 0), cfg.t_cap - 1);
}
// ... and this lane's live uid, -1 past the list (T = live_tracks)
__device__ __forceinline__ int live_uid(const DevCfg &cfg, const DevState &st, int s, int lane, int T)
{
    return lane < T ? st.trk[(size_t)s * cfg.t_cap + live_slot(cfg, st, s, lane)].uid : -1;
}
// The update lists (track-wise Kalman kernels).  A scene's workgroup of k_track appends its T tracks to the list of its SHARD
// (workgroup index mod shards: eight counters instead of one word that every workgroup of the launch adds to) with one atomicAdd;
// the consumers' unit w serves shard w mod shards, entries 4 (w / shards) .. + 3, so the list entry and the list's length are ONE
// round trip (the entry is read speculatively, clamped into the region) and the record's address is in the entry: two dependent
// round trips in front of a track's arithmetic where the lists "scenes by track count" of rounds 2-4 had four (bin counts, list
// entry, order[], record).
constexpr int kUpdShards = 8, kUpdWords = 16;
__host__ __device__ inline int kalman_waves_per_scene(int tr_max_tracks) { const int nq = (tr_max_tracks + 3) / 4; return nq < 1 ? 1 : nq; }
__host__ __device__ inline int upd_shards(int n_units) { return n_units < kUpdShards ? (n_units < 1 ? 1 : n_units) : kUpdShards; }
__host__ __device__ inline size_t upd_region(int n_scenes, int t_cap) { return ((size_t)(n_scenes + kUpdShards - 1) / kUpdShards + 1) * (size_t)t_cap; }
__host__ __device__ inline int upd_pack(int s, int j, int slot) { return (s << 12) | (j << 6) | slot; }   // (t_cap <= 63, n_scenes < 2^19: tracks_dense)
constexpr int kUpdMaxScenes = 1 << 19;

// Contexts of at most this many scenes run a two-launch step (mmw_kalman.hpp: pred_in_track, k_dbscan.hip: k_post takes the large
// clouds): their step is launch latency.  768 = what is resident at once with the PRED build of k_track (three workgroups
// per CU); measured 0.0777 -> 0.0705 ms at 768 scenes, 0.0937 -> 0.1128 at 1024.
constexpr int kSmallContextScenes = 768;
constexpr int kQCount = 0, kQHead = 1, kQDone = 2, kQStop = 3, kQTimeout = 4;
// The head (claim) word of a queue carries the number of the step the queue serves in its upper bits (q_tag), written when the
// queue is reset a step ahead: a claim is a compare-and-swap on tag + index, so a side-stream worker of ANOTHER step -- one that
// checked the stop epoch, was held up (six processes time-sharing the GPU: milliseconds), and looks at the queue of its parity two
// steps later -- cannot take an entry that is not its step's (it did: scripts/dual_run.py, profiles/NOTEBOOK.md round 6; the
// cloud was clustered correctly but its labels / db_n went to the OLD step's output buffers).  Consumers on the context's own
// stream run inside their step and mask the tag.
constexpr int kQTagShift = 20, kQIdxMask = (1 << kQTagShift) - 1;   // (n_scenes < 2^19 entries per step)
__host__ __device__ inline int q_tag(int epoch) { return (epoch & 0x7ff) << kQTagShift; }
constexpr int kQBig = 16;   // q[kQBig + 8p + kQCount/kQHead/kQDone]: the queue of the clouds of more than 256 points
constexpr int kQWords = 32;
constexpr int kEarlyU = 0;     // clouds of at least this many points go to the early queue (k_track.hip); a threshold above the clutter level (180) measured slower
constexpr int kInnerHdr = 2 + 16;  // calls, labels stored, rows of the first 16 calls

// n_pts[s] of a step: 1..max_pts = track() on that many points; 0 = the frame never reaches track() (offline_main.py:56
// skips empty frames); MMW_EMPTY_FRAME (-1) = track() IS called, on an empty point cloud (the reference then predicts,
// ages and expires tracks, runs _update_all and pushes an empty frame into the ring); anything else is ERR_BADCOUNT.
__device__ __forceinline__ bool frame_reaches_track(int n, int max_pts) { return n != 0 && n >= -1 && n <= max_pts; }

// Counters are spread over kStatSlots copies (one 256-byte line each, picked by scene index): thousands of
// workgroups adding to ONE address serialise in the memory-side atomic unit and that tail was longer than
// the kernels themselves.
constexpr int kStatSlots = 256;
constexpr int kStatWords = 32;
constexpr int kStatFeatBytes = 30;  // k_features: algorithmic bytes (mmw_stats_get_ext)
constexpr int kStatFeatRows = 31;   // k_features: feature tensors written
__device__ inline unsigned long long *stats_slot(const DevState &st, int scene)
{
    return st.stats ? st.stats + (size_t)(scene & (kStatSlots - 1)) * kStatWords : nullptr;
}

// One row of a frame (8 columns: x, y, z, vx, vy, vz, doppler, peakVal) into registers.  fp64 rows (mmw_step) are four
// 16-byte loads; fp32 rows (mmw_step_f32: 32 bytes per point, what a radar front end or a CSV reader produces) two, each
// value promoted to fp64 in registers -- exactly; from there on both entries run the same instructions on the same bits.
// Rows past the frame's capacity load nothing.
template <bool F32>
__device__ __forceinline__ void load_point_row(const void *frame, int i, bool valid, double2 (&r)[4])
{
    if constexpr (F32) {
        const float4 *src = reinterpret_cast<const float4 *>(frame);
        const float4 a = valid ? src[i * 2] : float4{0.f, 0.f, 0.f, 0.f}, b = valid ? src[i * 2 + 1] : float4{0.f, 0.f, 0.f, 0.f};
        r[0] = double2{(double)a.x, (double)a.y};
        r[1] = double2{(double)a.z, (double)a.w};
        r[2] = double2{(double)b.x, (double)b.y};
        r[3] = double2{(double)b.z, (double)b.w};
    } else {
        const double2 *src = reinterpret_cast<const double2 *>(frame);
#pragma unroll
        for (int u = 0; u < 4; u++) r[u] = valid ? src[i * 4 + u] : double2{0.0, 0.0};
    }
}
// start of scene s's frame: rows of 8 values, fp64 or fp32
__device__ __forceinline__ const void *frame_of(const void *pts_all, int s, int NP, bool f32)
{
    return reinterpret_cast<const char *>(pts_all) + (size_t)s * NP * (f32 ? 32 : 64);
}

__host__ __device__ inline size_t trk_ring_stride_track(const DevCfg &c) { return (size_t)c.ring * c.ring_rows * 8; }

}  // namespace mmw
