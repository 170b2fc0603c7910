// mmw_ctx.hpp -- what the api_*.hip files share: the context behind the C-ABI's opaque mmw_ctx, error reporting, the
// profiling-event bookkeeping and a few one-line helpers.  Host code only; nothing here is part of the ABI.
#pragma once

#include <cstring>
#include <string>
#include <vector>

#include "mmw_device.hpp"
#include "mmw_launch.hpp"
#include "mmw_kernels.hpp"

using namespace mmw;

struct EventPair { hipEvent_t a, b; int kid; };

// the posture CNN's shapes, floats per row: feature tensor, conv output, hidden layer -- by model: frames = 3 (define_CNN_3D,
// train.py:71-106: 960, 6144, 1536) or 1 (define_CNN, train.py:33-68: 320, 2048, 512) -- and keypoints (MMW_NKP = 57, padded);
// taps = the conv kernels' positions (3 x 3 x 3 or 3 x 3).  marsweights.model_dims is the same table in Python.
constexpr int kCnnKpPad = 64;
struct CnnDims { int per, flat, hidden, taps; };
static inline CnnDims cnn_dims(int frames) { return CnnDims{frames * 8 * 8 * 5, frames * 64 * 32, frames * 512, frames == 3 ? 27 : 9}; }

// The fp32 small chain of either model: the conv pair, then the thin Dense-1 / Dense-2 kernels, `rows` rows of feat -> kp[rows][nkp]
// through act[rows][flat] and hidden[rows][hidden]; dev_rows (device word or nullptr) = the rows that exist, as the launchers take it
static inline void launch_mars_small_f32(int frames, const float *feat, const mmw_posture_model &m, float *act, float *hidden, float *kp, int rows,
                                         hipStream_t st, const int32_t *dev_rows)
{
    const CnnDims d = cnn_dims(frames);
    launch_mars_conv_f32(frames, feat, m.conv1_w, m.conv1_b, m.conv2_w, m.conv2_b, act, rows, st, dev_rows);
    launch_mars_head_small(act, d.flat, m.dense1_w, m.dense1_ld, m.dense1_b, m.dense2_w, m.dense2_b, hidden, kp, rows, d.flat, d.hidden, MMW_NKP, st, dev_rows);
}
constexpr int kTickets = 4;
// the counters of mmw_stats_get in st.stats (the probe words of the diagnostic build lie behind them)
constexpr size_t kStatBytes = (size_t)kStatSlots * kStatWords * sizeof(unsigned long long);

// mmw_posture_attach: the model, its split Dense-1 operand and the buffers of the batched CNN chain ([cap] rows, cap a multiple of 256)
// mmw_posture_attach_models: the same with n_models models -- one split operand and one fix-up list each, everything else shared, the
// rows of a call in one band per model.  mmw_posture_attach / _frames are its one-model case.
struct PostureBatch {
    int n_models = 1;
    mmw_posture_model model[MMW_POSTURE_MODELS_MAX] = {};
    void *w16[MMW_POSTURE_MODELS_MAX] = {};   // each model's split Dense-1 operand
    int frames = 3;                   // the models: 3 = define_CNN_3D, 1 = define_CNN (= the context's ring)
    int32_t cap = 0;                  // cap_rows: the most rows one call estimates, summed over the models
    int32_t rows = 0;                 // rows of the shared buffers: pad256(cap), + 256 per model when there are several (every band starts on a multiple of 256)
    float *feat = nullptr, *hidden = nullptr, *kp = nullptr;
    int32_t *owner = nullptr, *uid = nullptr;
    int32_t *words = nullptr;         // [0] the sticky range word, [1] unused, [2 ..] a fix-up list (2 + MMW_RANGE_FIXUP_CAP) per model, then the attach-time weight check per model
    void *act16 = nullptr, *fix_scratch = nullptr;
    int32_t *h_total = nullptr;       // pinned [16]: the eligible-track total of the call in flight; several bands: totals[8] | bases[8]
    hipEvent_t total_ev = nullptr;
    // the scene -> model map (MMW_POSTURE_NONE: no model estimates the scene): device words, host mirror
    int32_t *d_map = nullptr;         // [S]
    int32_t *d_groups = nullptr;      // [16] k_feat_scan_models' totals and bases
    std::vector<int32_t> h_map;
    bool grouped = false;             // more than one model, or a scene on MMW_POSTURE_NONE: mmw_estimate_posture runs the grouped scan and a chain per band
    // the last mmw_estimate_posture: rows and first row of every band (mmw_posture_group_rows, mmw_posture_owners)
    int32_t last_total[MMW_POSTURE_MODELS_MAX] = {}, last_base[MMW_POSTURE_MODELS_MAX] = {};
};

// What the three live-track exports (mmw_report_*, mmw_clouds_*, mmw_skeletons_*), the radar log (mmw_uart_log_*) and the training samples (mmw_samples_*) keep on the host: the device scratch of the call
// in flight and the pinned counts of the outstanding calls, one slot per ticket (api_export.hip).  d_block == nullptr: not allocated.
struct ExportCtx {
    ExportScratch sc = {};
    char *d_block = nullptr;          // one allocation: [extra words of the owner | sc.off | sc.totals]
    int32_t *h_counts = nullptr;      // pinned [kTickets][4]: as ExportScratch::totals
    hipEvent_t ev[kTickets] = {nullptr, nullptr, nullptr, nullptr};
    bool issued[kTickets] = {false, false, false, false};
};

// A per-scene table of up to MAX caller entries E a scene (mmw_set_zones, mmw_set_tripwires, mmw_set_stance_rules, mmw_set_heat_grids; mmw_scene_table.hpp has the code): the
// device allocation, which holds the table as the kernels read it (entries D) and in which every set call lands as ONE copy, and
// the host mirrors of what the caller gave.  d_tab == nullptr: not allocated.
template <class E, class D, int MAX>
struct SceneTable {
    using entry = E;
    using dev_entry = D;
    static constexpr int kMax = MAX;
    char *d_tab = nullptr;            // [S][MAX] D | [S] counts | [S] the scene flags of the set call that wrote it
    std::vector<E> h_entries;         // [S][MAX] as the caller gave them, zero past a scene's count ...
    std::vector<int32_t> h_counts;    // [S] ... and the counts (the getter reads both)
    static size_t table_bytes(size_t S) { return S * MAX * sizeof(D); }
    static size_t bytes(size_t S) { return table_bytes(S) + 2 * S * sizeof(int32_t); }
    const D *entries() const { return reinterpret_cast<const D *>(d_tab); }
    const int32_t *counts(size_t S) const { return reinterpret_cast<const int32_t *>(d_tab + table_bytes(S)); }
    const int32_t *flags(size_t S) const { return counts(S) + S; }
};

struct mmw_ctx {
    mmw_config cfg;
    DevCfg dc;
    DevState st;
    int device;
    int UM;                      // ring * max_pts
    hipStream_t own_stream, stream;
    hipStream_t side_stream = nullptr;   // k_chain beside k_track (contexts with dc.side_worker)
    hipEvent_t side_gate = nullptr;      // (gate_side only) recorded on the context's stream at the head of a step: k_chain does not start before it
    int gate_side = 0;                   // mmw_config.chain_side_stream == 3
    int side_wanted = 0;                 // what the configuration / mmw_set_chain_side_stream asked for
    int fused_wanted = 0;                // the one-workgroup step (k_scene) is what this context runs unless a ring was resized or the side workers were asked for
    int side_trusted = 0;                // mmw_config.chain_side_stream == 2: the side stream is used without the concurrency check
    int side_probed = 0;                 // the side streams have been checked against the current context stream (probe_side_streams)
    int32_t *d_probe = nullptr;          // [4] flag + results of that check
    int epoch = 0;                       // step number (queue protocol of the DBSCAN workers, mmw_dbqueue.hpp)
    std::string err;
    // internal scratch
    int32_t *d_row_off = nullptr;     // [S+1]
    int32_t *h_rows = nullptr;        // pinned [kTickets]: eligible-track totals of the outstanding mmw_features_async calls
    hipEvent_t feat_ev[kTickets] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t handoff_ev = nullptr;     // mmw_stream_wait: recorded on the context's stream, waited for by the caller's
    hipEvent_t handback_ev = nullptr;    // mmw_wait_stream: recorded on the caller's stream, waited for by the context's
    int32_t feat_cap[kTickets] = {0, 0, 0, 0};
    // mmw_set_keypoints_ticket: [S] every scene's generation word (k_reset and k_snap_unpack bump it) | [kTickets][S] the words as
    // the ticket's k_features found them; feat_uid: the ticket's last mmw_features_async wrote uids, and so that snapshot
    int32_t *d_kp_gen = nullptr;
    bool feat_uid[kTickets] = {false, false, false, false};
    float *d_posture = nullptr;
    int step_parity = 0;
    int ring_frames_bound = 0;   // no scene's global ring holds more frames than this (host-side knowledge: steps since the last reset)
    // host-convenience staging (lazy): one device block in [rows | dt | n], one out [assoc | db_n | n_out | labels], their pinned
    // host mirrors, and pinned copies of the scene headers and the queue words -- mmw_frame_host moves each with ONE copy
    char *d_in = nullptr, *d_out = nullptr, *h_in = nullptr, *h_out = nullptr;
    double *d_raw = nullptr;          // [S][max_pts][8]: normalize_data's rows in the raw form of mmw_frame_host (the raw rows arrive in d_in's row area)
    SceneHdr *h_hdr = nullptr;        // pinned [S]
    int32_t *h_q = nullptr;           // pinned [kQWords]
    double *d_pts = nullptr; int32_t *d_n = nullptr; double *d_dt = nullptr;      // (views into d_in / d_out)
    int32_t *d_assoc = nullptr, *d_labels = nullptr, *d_dbn = nullptr, *d_nout = nullptr, *d_prows = nullptr;
    mmw_track_record *d_export = nullptr; int export_cap = 0;
    mmw_scene_site *d_sites = nullptr;   // [S] per-scene sites (mmw_set_sites; lazy).  Kept allocated by mmw_clear_sites ...
    int sites_on = 0;                    // ... which only turns this off: the kernels of a context without sites run again
    std::vector<mmw_scene_site> h_sites; // host mirror of d_sites while sites_on (mmw_get_sites reads it)
    char *d_snap = nullptr;           // mmw_snapshot / mmw_restore scratch (lazy): [S] scene list | [S] flags | [4] check word | [S + 2] u64 sizes | [S] directory
    // mmw_attach_posture: the model and the chain's buffers ([cap] rows: feature tensors, owners, conv output, hidden, keypoints)
    bool has_model = false;
    int model_frames = 3;             // ... 3 = define_CNN_3D, 1 = define_CNN (= the context's ring)
    mmw_posture_model model = {};
    char *d_pchain = nullptr;
    float *pc_feat = nullptr, *pc_act = nullptr, *pc_hidden = nullptr, *pc_kp = nullptr;
    int32_t *pc_owner = nullptr;
    PostureBatch *pb = nullptr;       // mmw_posture_attach (any number of scenes); independent of the one-scene chain above
    ExportCtx rep;                    // mmw_report_enable; not allocated = reports are off and nothing of them is launched
    ReportState rs = {};              // ... the report's baseline, in front of rep's scratch in rep.d_block (rs.sc = rep.sc)
    ExportCtx cloud;                  // mmw_clouds_*: allocated by the first call; not allocated = never called, nothing of it exists
    ExportCtx skel;                   // mmw_skeletons_*: allocated by the first call; not allocated = never called, nothing of it exists
    ExportCtx sample;                 // mmw_samples_*: allocated by the first call; not allocated = never called, nothing of it exists
    ExportCtx zone;                   // mmw_set_zones allocates it, mmw_clear_zones frees it; not allocated = no zone table, nothing of it is launched
    ZoneState zs = {};                // ... the zones' baseline, in front of zone's scratch in zone.d_block (zs.sc = zone.sc)
    SceneTable<mmw_zone, mmw_zone, MMW_ZONES_MAX> ztab;   // ... the zone table: what the kernels read is what the caller gave (mmw_get_zones reads the mirrors)
    ExportCtx trail;                  // mmw_trails_enable allocates it (depth 0 frees it); not allocated = trails are off, nothing of them is launched
    TrailState ts = {};               // ... the trail slots and rings, in front of trail's scratch in trail.d_block (ts.sc = trail.sc)
    ExportCtx trip;                   // mmw_tripwires_enable allocates it (log_depth 0 frees it); not allocated = tripwires are off, nothing of them is launched
    TripState tw = {};                // ... the uid slots, counters and event rings, in front of trip's scratch in trip.d_block (tw.sc = trip.sc)
    SceneTable<mmw_tripwire, TripWire, MMW_TRIPWIRES_MAX> twtab;   // ... the wire table: what the kernels read is derived on the host (mmw_get_tripwires reads the mirrors)
    ExportCtx stance;                 // mmw_stance_enable allocates it (log_depth 0 frees it); not allocated = stance is off, nothing of it is launched
    StanceState ss = {};              // ... the uid slots, counters and event rings, in front of stance's scratch in stance.d_block (ss.sc = stance.sc)
    SceneTable<mmw_stance_rule, StanceRule, MMW_STANCE_RULES_MAX> sttab;   // ... the rule table: what the kernels read is derived on the host (mmw_get_stance_rules reads the mirrors)
    ExportCtx heat;                   // mmw_heat_enable allocates it (cells 0 frees it); not allocated = heat is off, nothing of it is launched
    HeatState hs = {};                // ... the cells, uid slots and scene words, in front of heat's scratch in heat.d_block (hs.sc = heat.sc)
    SceneTable<mmw_heat_grid, HeatGrid, MMW_HEAT_GRIDS_MAX> htab;   // ... the grid table: what the kernels read is what the caller gave (mmw_get_heat_grids reads the mirrors)
    ExportCtx ulog_x;                 // mmw_uart_log_enable; not allocated = the radar log is off and mmw_uart_read launches what it always did
    UartLog ulog = {};                // ... the staged frames, in front of ulog_x's scratch in ulog_x.d_block
    std::vector<double> uart_range;   // [S] rangeIdxToMeters of the open readers (the log's range column)
    UartState uart = {};              // mmw_uart_open: the radar readers' state (uart.buf is the allocation, uart.scene lies behind the buffers); nullptr = closed
    // profiling
    unsigned prof_mask = 0;           // bit k: time kernel id k (mmw_profile_enable)
    std::vector<EventPair> pending;
    std::vector<EventPair> pool;
    double tot_ms[MMW_K_COUNT] = {0};
    int64_t launches[MMW_K_COUNT] = {0};
};

// ---- shared between the api_*.hip files, not exported ----
#pragma GCC visibility push(hidden)
int fail(mmw_ctx *ctx, int code, const char *fmt, ...);            // api_context.hip: the message into ctx->err and mmw_last_error(NULL)
int probe_side_streams(mmw_ctx *c);                                // api_context.hip
int read_headers(mmw_ctx *c, std::vector<SceneHdr> &h);            // api_query.hip
int first_scene_error(mmw_ctx *c, const SceneHdr *h, size_t n, const int32_t *q);   // api_query.hip
void posture_batch_free(PostureBatch *b);                          // api_posture.hip
void zone_free(mmw_ctx *c);                                        // api_zone.hip: table, baseline and mirrors (the caller has waited for the stream)
void tripwire_free(mmw_ctx *c);                                    // api_tripwire.hip: table, slots, counters, rings and mirrors (the caller has waited for the stream)
void stance_free(mmw_ctx *c);                                      // api_stance.hip: table, slots, counters, rings and mirrors (the caller has waited for the stream)
void heat_free(mmw_ctx *c);                                        // api_heat.hip: table, cells, slots and mirrors (the caller has waited for the stream)
void trail_free(mmw_ctx *c);                                     // api_trail.hip: slots, rings and scratch (the caller has waited for the stream)
int uart_log_rearm(mmw_ctx *c);                                    // api_uart_log.hip: every scene's log word as new, with its range scale (no-op while the log is off)
void uart_log_free(mmw_ctx *c);                                    // api_uart_log.hip: ... and the log is off (the caller has waited for the stream)
// api_export.hip: the ticketed counts of the three live-track exports (`name`: the entry the messages speak for)
int export_alloc(mmw_ctx *c, ExportCtx &x, size_t extra_words, const char *name);   // extra_words int32 in front of the scratch, at x.d_block
void export_free(ExportCtx &x);                                    // ... and x is as never allocated
int export_issue(mmw_ctx *c, ExportCtx &x, int ticket);           // behind the launch: its error, the totals into the ticket's pinned slot, the event
int export_wait(mmw_ctx *c, ExportCtx &x, int ticket, const char *name, const char *none, const int32_t **counts);   // -> the ticket's four words
// ... and the front end of the exports with two caller buffers, rows and events (mmw_report_*, mmw_zones_*, mmw_tripwires_*, mmw_stance_*; mmw_heat_*: rows and cells).
// The messages are built from the entry's words: "<entry>: <off>" while x is not allocated, "<entry>_wait: <none> outstanding under
// ticket k", and for MMW_E_CAPACITY "<entry>: n <rows> and m <second> <unfit>".  align: what both buffers must be aligned to, 0 = anything.
struct PairExport { const char *entry, *off, *none, *rows, *unfit; int align; const char *second = "events"; };   // second: the noun of the second buffer's entries
constexpr const char *kUnfitLog = "do not fit the buffers: nothing was written, nothing was taken";               // a log is drained: tripwires, stance
constexpr const char *kUnfitBaseline = "do not fit the buffers: nothing was written, the baseline is unchanged";   // two states are compared: report, zones
int pair_export_begin(mmw_ctx *c, const ExportCtx &x, const PairExport &d, const void *rows, int cap_rows, const void *events, int cap_events, int ticket);   // before the launch: enabled, capacities, pointers, alignment, ticket; device set
int pair_export_wait(mmw_ctx *c, ExportCtx &x, const PairExport &d, int ticket, int32_t *n_rows, int32_t *n_events);   // export_wait, the two counts out (either may be NULL), MMW_E_CAPACITY if the device decided so
int sample_begin(mmw_ctx *c, const ExportCtx &x, const char *entry, const char *what, const int32_t *scene_flags, const double *t);   // mmw_trails_sample / mmw_tripwires_sample / mmw_stance_sample / mmw_heat_sample: enabled, aligned, device set
int uid_rebase(mmw_ctx *c, const int32_t *dev_flags);             // the flagged scenes' uids restart: one launch for report, zones, trails, tripwires and stance, one for heat, none while all six are off
#pragma GCC visibility pop

#define HIPCHK(ctx, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(ctx, MMW_E_HIP, "%s -> %s", #expr, hipGetErrorString(e_)); } while (0)
// (a helper that has already reported through fail)
#define MMW_TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

// a timing pair for kernel id `kid`, from the pool; false (ep.kid = -1) when that id is not being timed
static inline bool prof_acquire(mmw_ctx *c, int kid, EventPair &ep)
{
    ep.kid = -1;
    if (!((c->prof_mask >> kid) & 1u)) return false;
    if (!c->pool.empty()) { ep = c->pool.back(); c->pool.pop_back(); }
    else { hipEventCreate(&ep.a); hipEventCreate(&ep.b); }
    ep.kid = kid;
    return true;
}
static inline void prof_begin(mmw_ctx *c, int kid, EventPair &ep) { if (prof_acquire(c, kid, ep)) hipEventRecord(ep.a, c->stream); }
// for an id that is exactly ONE launch: the events ride on the kernel's own packet (mmw_launch.hpp)
static inline void prof_arm(mmw_ctx *c, int kid, EventPair &ep) { if (prof_acquire(c, kid, ep)) { g_launch_prof.a = ep.a; g_launch_prof.b = ep.b; } }
static inline void prof_armed_done(mmw_ctx *c, EventPair &ep)
{
    if (ep.kid < 0) return;
    if (g_launch_prof.a) {  // nothing was launched (e.g. no large-cloud class exists): nothing to time
        g_launch_prof = LaunchProf{};
        c->pool.push_back(ep);
        return;
    }
    c->pending.push_back(ep);  // (folded by mmw_profile_get / the event-pair path)
}
static inline void prof_fold(mmw_ctx *c)
{
    for (auto &ep : c->pending) {
        hipEventSynchronize(ep.b);
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ep.a, ep.b) == hipSuccess) { c->tot_ms[ep.kid] += ms; c->launches[ep.kid]++; }
        c->pool.push_back(ep);
    }
    c->pending.clear();
}
static inline void prof_end(mmw_ctx *c, EventPair &ep)
{
    if (ep.kid < 0) return;
    hipEventRecord(ep.b, c->stream);
    c->pending.push_back(ep);
    if (c->pending.size() >= 2048) prof_fold(c);
}

// mmw_tripwires_enable / mmw_stance_enable: what the state blocks of the log consumers have in common -- the ring at the block's head,
// and behind the consumer's own int32 words, at p, the five [S] words logged | taken | gen | seen | ordinal
template <class E>
static inline void evlog_carve(EventLog<E> &log, UidSlots &ug, int32_t depth, char *block, int32_t *p, size_t S)
{
    log.depth = depth;
    log.ring = reinterpret_cast<E *>(block);
    log.logged = p;
    log.taken = p + S;
    ug.gen = p + 2 * S;
    ug.seen = p + 3 * S;
    ug.ordinal = p + 4 * S;
}

// the context's site table while one is in use (the k_*_site kernels), else nullptr
static inline const mmw_scene_site *sites_or_null(const mmw_ctx *c) { return c->sites_on ? c->d_sites : nullptr; }

// Which step a context runs is decided in ONE place: the one-workgroup step (k_scene) when it was chosen at creation and
// neither the side-stream workers are asked for (they claim scenes while the association kernel runs) nor a global ring has
// been resized (k_track's INNER instantiations read the sizes per ring).  What was ASKED for counts, not what the stream
// probe left of it: a context whose probe turned the workers off keeps the bulk kernels, as derive_dev_cfg's `can` has it.
static inline void refresh_step_kind(mmw_ctx *c) { c->dc.fused = (c->fused_wanted && !c->side_wanted && !c->dc.var_ring) ? 1 : 0; }

// Read-back into the caller's (pageable) memory of what the context's stream has written: the stream is waited for first, then the
// copy runs on it alone and is waited for.  (On the context's stream, not as a blocking hipMemcpy: that one runs on the legacy default
// stream and would also wait for whatever another runtime -- torch -- has queued there.)
static inline int d2h_after_kernels(mmw_ctx *c, void *dst, const void *src, size_t bytes)
{
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MMW_OK;
}
