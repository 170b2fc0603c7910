// api_context.hip -- the C-ABI (include/mmw.h): a context's life.  Version, default configuration, create / destroy / reset,
// the ring setters, per-scene sites, streams, device memory.  No CPU path: if HIP cannot give us a gfx950-class device,
// creation fails loudly.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <new>

#include "mmw_ctx.hpp"
#include "mmw_kalman.hpp"

thread_local LaunchProf mmw::g_launch_prof;

static thread_local std::string g_last_error;

int fail(mmw_ctx *ctx, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    g_last_error = buf;
    return code;
}

// Contexts of more than kPerSceneMaxScenes scenes run the Kalman kernels laid out over tracks and the DBSCAN chain workers on a side
// stream unless told otherwise (mmw_config.kalman_dense_min_units = 0, chain_side_stream = 0).  Round 3 had the workers from 1536
// scenes (every step recorded an event for them: 1024 / 1280 scenes 91 -> 96 us with them) and the per-scene, two-launch step up
// to 768.  Without that event (scripts/side_threshold.sh, scripts/layout_ab.py; ms per step, same box):
//   scenes                              576     640     768     896     1024    1280
//   round-3 choice, frames 20..120      -       0.0822  0.0899  0.0985  0.1108  0.1259
//   track-wise + side stream            -       0.0720  0.0809  0.0878  0.0969  0.1099
//   round-3 choice, frames 10..50       0.0646  0.0646  0.0676  0.0737  -       -
//   track-wise + side stream            0.0581  0.0599  0.0653  0.0740  -       -
// At 512 and below the one-workgroup step / the two-launch step stay ahead in the early window (0.0505 vs 0.0557 at 512).
constexpr int kPerSceneMaxScenes = 512;
constexpr int kSideWorkerMinScenes = kPerSceneMaxScenes + 1;

// The chain workers' stream.  It must not share a hardware queue with the context's stream (the HIP runtime multiplexes
// streams onto a few queues -- GPU_MAX_HW_QUEUES, 4 by default -- round-robin at creation): probe_side_streams checks that
// and re-creates a stream that does.  (A highest-priority stream gets a queue of another pool, but the context's own
// launches then start ~8 us later per step: measured, not used.)
static hipError_t create_side_streams(mmw_ctx *c)
{
    hipError_t e = hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->side_gate, hipEventDisableTiming);
    return e;
}

// 1 = a kernel on the context's stream runs while a kernel on `side` spins, 0 = it does not (shared hardware queue: a worker
// polling for k_track's pushes would keep k_track from starting until its bounded wait runs out), -1 = HIP error.
static int probe_one(mmw_ctx *c, hipStream_t side, hipStream_t other)
{
    const int polls = 1 << 12;   // a few ms at most; ~20 us when the streams are independent
    if (hipMemsetAsync(c->d_probe, 0, 4 * sizeof(int32_t), c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return -1;
    launch_probe_wait(c->d_probe, 0, polls, side);
    launch_probe_set(c->d_probe, other);
    if (hipStreamSynchronize(side) != hipSuccess || hipStreamSynchronize(other) != hipSuccess) return -1;
    int32_t w[4] = {0, 0, 0, 0};
    if (hipMemcpy(w, c->d_probe, sizeof(w), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return w[1] ? 1 : 0;
}
int probe_side_streams(mmw_ctx *c)
{
    int ok = probe_one(c, c->side_stream, c->stream);
    for (int attempt = 0; ok == 0 && attempt < 6; attempt++) {  // the next stream lands on the next hardware queue
        hipStream_t fresh = nullptr;
        if (hipStreamCreateWithFlags(&fresh, hipStreamNonBlocking) != hipSuccess) return -1;
        hipStreamSynchronize(c->side_stream);
        hipStreamDestroy(c->side_stream);
        c->side_stream = fresh;
        ok = probe_one(c, fresh, c->stream);
    }
    return ok;
}

// ---- mmw_create in four parts: argument checks, the layout (pure arithmetic), allocation, device initialisation ----
static int check_create_args(const mmw_config *cfg, int32_t n_scenes, int32_t max_pts)
{
    if (n_scenes < 1 || max_pts < 1 || max_pts > MMW_MAX_PTS_LIMIT) return fail(nullptr, MMW_E_ARG, "mmw_create: n_scenes=%d max_pts=%d out of range (max_pts <= %d)", n_scenes, max_pts, MMW_MAX_PTS_LIMIT);
    if (cfg->fb_frames_batch < 0 || cfg->fb_frames_batch + 1 > MMW_RING_MAX) return fail(nullptr, MMW_E_ARG, "FB_FRAMES_BATCH must be in [0,%d]", MMW_RING_MAX - 1);
    if (cfg->dim_x != 9 && cfg->dim_x != 6) return fail(nullptr, MMW_E_ARG, "dim_x must be 9 (CONST_ACC_MODEL) or 6 (CONST_VEL_MODEL)");
    // sklearn's parameter validation (DBSCAN._parameter_constraints, cluster/_dbscan.py:330-342: eps in (0, inf), min_samples an
    // integer >= 1): with anything else EVERY apply_DBscan call of the reference raises InvalidParameterError -- refused here
    if (!(cfg->db_eps > 0.0) || cfg->db_min_samples < 1 || (cfg->seek_inner && !(cfg->db_inner_eps > 0.0)))
        return fail(nullptr, MMW_E_ARG, "DB_EPS%s must be > 0 and DB_MIN_SAMPLES_MIN >= 1 (sklearn's DBSCAN refuses anything else)", cfg->seek_inner ? " / DB_INNER_EPS" : "");
    // (apply_DBscan has no size limit, Utils.py:250-291; here a cloud is at most the ring: MMW_RING_MAX frames of MMW_MAX_PTS_LIMIT
    //  points.  Up to 1920 points its BallTree lives in the LDS; larger ones -- only contexts with ring * max_pts > 1920 can
    //  see them -- run on slabs in global memory, k_dbscan_huge)
    const int um = (cfg->fb_frames_batch + 1) * max_pts;
    if (um > MMW_RING_MAX * MMW_MAX_PTS_LIMIT) return fail(nullptr, MMW_E_ARG, "ring*max_pts = %d exceeds %d", um, MMW_RING_MAX * MMW_MAX_PTS_LIMIT);
    return MMW_OK;
}

// What a configuration makes of a context: the kernels' DevCfg and what the context WANTS to run (refresh_step_kind and the
// stream probe decide per step what it does run).  Pure arithmetic: no HIP call but the *_lds_bytes sizing functions.  These
// choices are layout only -- results never depend on them.
struct DevPlan { DevCfg dc; int fused_wanted, side_wanted, side_trusted, gate_side; };
static int derive_dev_cfg(const mmw_config *cfg, int32_t n_scenes, int32_t max_pts, DevPlan &plan)
{
    DevCfg &d = plan.dc;
    memset(&d, 0, sizeof(d));
    const int ring = cfg->fb_frames_batch + 1;
    d.ring = ring; d.db_min_samples = cfg->db_min_samples; d.tr_max_tracks = cfg->tr_max_tracks;
    d.kf_enable_est = cfg->kf_enable_est; d.model_min_input = cfg->model_min_input; d.dx = cfg->dim_x;
    d.ring_rows = cfg->ring_rows < 64 ? 64 : cfg->ring_rows;
    d.seek_inner = cfg->seek_inner ? 1 : 0;
    d.db_points_thres = cfg->db_points_thres; d.fb_frames_batch_static = cfg->fb_frames_batch_static;
    d.db_spread_thres = cfg->db_spread_thres; d.db_inner_eps = cfg->db_inner_eps;
    // the BallTree chain workers beside k_track on a second stream: for contexts large enough that k_track is a long launch
    // (a small context's whole step is shorter than a chain), and not with seek_inner (k_inner may cancel queued scenes)
    d.side_worker = (!d.seek_inner && (cfg->chain_side_stream > 0 || (cfg->chain_side_stream == 0 && n_scenes >= kSideWorkerMinScenes))) ? 1 : 0;
    if (d.seek_inner) {
        // seek_inner_clusters clusters whole ring frames, and the first frame of a track it spawns is a cluster of up to
        // ring*max_pts rows: frames are stored whole.  A ring of size 0 would never leave add_frame's loop (Tracking.py:47-48).
        if (cfg->fb_frames_batch < 1 || cfg->fb_frames_batch_static < 1 || cfg->fb_frames_batch_static > ring)
            return fail(nullptr, MMW_E_ARG, "seek_inner: FB_FRAMES_BATCH and FB_FRAMES_BATCH_STATIC must be in [1, FB_FRAMES_BATCH + 1 = %d]", ring);
        if (d.ring_rows < ring * max_pts) d.ring_rows = ring * max_pts;
    }
    int cap = cfg->track_cap;
    if (cap <= 0) {
        const int ms = cfg->db_min_samples > 0 ? cfg->db_min_samples : 1;
        cap = (cfg->tr_max_tracks > 0 ? cfg->tr_max_tracks - 1 : 0) + (ring * max_pts) / ms + 1;
    }
    if (cap > MMW_TRACK_CAP_LIMIT) cap = MMW_TRACK_CAP_LIMIT;
    if (cap < 1) cap = 1;
    d.t_cap = cap; d.max_pts = max_pts; d.n_scenes = n_scenes;
    // layout of the Kalman kernels (mmw_kalman.hpp: tracks_dense): laid out over tracks when the context holds more
    // four-track waves than this; 0 = the default threshold (one wave per CU x 4), < 0 = always per scene
    d.dense_min_units = cfg->kalman_dense_min_units == 0 ? (n_scenes <= kPerSceneMaxScenes ? 0x7fffffff : 1024)   // (small contexts: per scene, two-launch step)
                                                         : (cfg->kalman_dense_min_units < 0 ? 0x7fffffff : cfg->kalman_dense_min_units - 1);
    if (d.seek_inner) d.dense_min_units = 0x7fffffff;  // k_inner changes a scene's track count between k_track and k_post: per-scene layout
    d.db_z_weight = cfg->db_z_weight; d.db_range_weight = cfg->db_range_weight; d.db_eps = cfg->db_eps;
    d.tr_lifetime_dynamic = cfg->tr_lifetime_dynamic; d.tr_lifetime_static = cfg->tr_lifetime_static;
    d.tr_vel_thres = cfg->tr_vel_thres; d.tr_gate = cfg->tr_gate; d.kf_q_std = cfg->kf_q_std; d.kf_p_init = cfg->kf_p_init;
    d.kf_group_disp_est_init = cfg->kf_group_disp_est_init; d.kf_a_n = cfg->kf_a_n; d.kf_est_pointnum = cfg->kf_est_pointnum;
    for (int i = 0; i < 6; i++) d.kf_spread_lim[i] = cfg->kf_spread_lim[i];
    d.kf_a_spr = cfg->kf_a_spr; d.intensity_mu = cfg->intensity_mu; d.intensity_std = cfg->intensity_std;
    d.s_height = cfg->s_height; d.tilt_cos = cfg->tilt_cos; d.tilt_sin = cfg->tilt_sin;
    d.m_x = cfg->m_x; d.m_y = cfg->m_y; d.m_z = cfg->m_z;
    d.fade_max = cfg->v_screen_fade_size_max; d.fade_min = cfg->v_screen_fade_size_min; d.fade_weight = cfg->v_screen_fade_weight;
    // The one-workgroup step (k_scene.hip): a scene's whole track() in one workgroup, for contexts whose scenes are all
    // resident at once, two workgroups per CU -- there a step is one scene's latency, and one launch boundary less is
    // what pays: measured on one box, 512 scenes x 512 points x 8 tracks 0.0617 -> 0.0588 ms per step.  (Round 3 kept the
    // two-launch step up to 256 scenes -- 0.0448 against 0.0477 ms then; round 4, scripts/fused_small.sh: 64 / 128 / 256
    // scenes x 256 points x 4 tracks 0.0355 / 0.0364 / 0.0414 two-launch against 0.0305 / 0.0313 / 0.0366 ms, 128 / 256
    // scenes x 512 x 8 equal.)  Hence "automatic" = all scenes resident at once, up to kPerSceneMaxScenes.  Not with
    // seek_inner (k_inner sits between association and update), the side-stream workers (they claim scenes while the
    // association kernel runs) or more than 63 tracks per scene (a lane per track in its maintenance step).
    const size_t sl = scene_lds_bytes(d);
    // (more than 512 points per frame: four points per thread, a register budget of one workgroup per CU -- k_scene.hip)
    const int per_cu = (sl <= 80 * 1024 && max_pts <= 512) ? 2 : (sl <= 160 * 1024 ? 1 : 0);
    const bool can = per_cu > 0 && !d.seek_inner && d.t_cap <= 63 && cfg->chain_side_stream <= 0;
    const bool want = cfg->fused_step > 0 || (cfg->fused_step == 0 && cfg->kalman_dense_min_units == 0 && n_scenes <= 256 * per_cu && n_scenes <= kPerSceneMaxScenes);
    plan.fused_wanted = d.fused = (can && want) ? 1 : 0;
    if (d.fused) { d.dense_min_units = 0x7fffffff; d.side_worker = 0; }
    plan.side_wanted = d.side_worker;
    plan.side_trusted = (d.side_worker && cfg->chain_side_stream == 2) ? 1 : 0;   // 2: taken on trust (counter collection serialises kernels: the probe would say no)
    plan.gate_side = (d.side_worker && cfg->chain_side_stream == 3) ? 1 : 0;
    return MMW_OK;
}

// sizes of the buffers that are allocated in one part of mmw_create and zero-filled in the next
static size_t trk_bytes(const DevCfg &d) { return (size_t)d.n_scenes * d.t_cap * sizeof(TrackRec); }
static size_t kp_gen_bytes(const DevCfg &d) { return (size_t)(1 + kTickets) * d.n_scenes * sizeof(int32_t); }
static size_t db_list_bytes(const DevCfg &d) { return 4 * (size_t)d.n_scenes * sizeof(int32_t); }
static size_t upd_list_bytes(const DevCfg &d) { return 2 * (size_t)kUpdShards * upd_region(d.n_scenes, d.t_cap) * sizeof(int32_t); }
static size_t inner_buf_bytes(const mmw_ctx *c) { return (size_t)c->dc.n_scenes * (size_t)(kInnerHdr + c->st.inner_cap) * sizeof(int32_t); }
constexpr size_t kStatAllocBytes = kStatBytes + (256 + 8192) * sizeof(unsigned long long);   // + probe words, workgroup times of the diagnostic build
constexpr size_t kDbCountBytes = 8 * sizeof(int32_t), kQBytes = kQWords * sizeof(int32_t), kSpcCountBytes = 2 * sizeof(int32_t), kUpdCountBytes = 2 * kUpdWords * sizeof(int32_t);

// (both parts below destroy the context before they report a failure: mmw_create just passes the code on)
#define CREATE_FAIL(c, ...) do { mmw_destroy(c); return fail(nullptr, __VA_ARGS__); } while (0)

static int create_alloc(mmw_ctx *c)
{
    const DevCfg &d = c->dc;
#ifdef MMW_DIAG_POISON   // (diagnostic build, mmw_launch.hpp: what mmw_create does not initialise reads as NaN / huge, not as whatever was there)
#define MMW_POISON_FRESH(ptr, bytes) (void)hipMemsetAsync((void *)(ptr), 0xFF, (bytes), c->own_stream)
#else
#define MMW_POISON_FRESH(ptr, bytes) ((void)0)
#endif
    // The context's stream FIRST: everything that initialises device memory below is queued on it and waited for before
    // mmw_create returns.  (Up to round 5 the zero fills were plain hipMemset calls -- work on the NULL stream, asynchronous to the
    // host for device memory -- while the context's stream is non-blocking, i.e. not ordered with the null stream: with six
    // processes on the GPU a fill could still be pending when mmw_create returned, and landed on the track records / queue words
    // AFTER the first steps had written them, or on memory mmw_destroy had already freed.  scripts/dual_run.py caught it: about
    // one fresh context in 10^4 under that load; profiles/NOTEBOOK.md round 6.)
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) CREATE_FAIL(c, MMW_E_HIP, "hipStreamCreate failed");
    c->stream = c->own_stream;
#define ALLOC(ptr, bytes)                                                                                   \
    do {                                                                                                    \
        hipError_t e_ = hipMalloc((void **)&(ptr), (bytes));                                                \
        if (e_ != hipSuccess) { int rc = fail(nullptr, MMW_E_HIP, "hipMalloc(%zu) -> %s", (size_t)(bytes), hipGetErrorString(e_)); mmw_destroy(c); return rc; } \
        MMW_POISON_FRESH(ptr, bytes);                                                                       \
    } while (0)
    const size_t S = (size_t)d.n_scenes, cap = (size_t)d.t_cap;
    ALLOC(c->st.hdr, S * sizeof(SceneHdr));
    ALLOC(c->st.order, S * cap * sizeof(int32_t));
    ALLOC(c->st.trk, trk_bytes(d));
    ALLOC(c->st.trk_ring, S * cap * (size_t)d.ring * d.ring_rows * 8 * sizeof(double));
    ALLOC(c->st.g_ring, S * (size_t)d.ring * d.max_pts * 8 * sizeof(double));
    ALLOC(c->d_posture, MMW_NKP * sizeof(float));
    ALLOC(c->d_row_off, (S + 1) * sizeof(int32_t));
    ALLOC(c->d_kp_gen, kp_gen_bytes(d));
    ALLOC(c->st.stats, kStatAllocBytes);
    ALLOC(c->st.db_list, db_list_bytes(d));
    ALLOC(c->st.db_count, kDbCountBytes);
    ALLOC(c->st.q, kQBytes);
    ALLOC(c->d_probe, 4 * sizeof(int32_t));
    ALLOC(c->st.gate_buf, S * cap * kGateRec * sizeof(double));
    ALLOC(c->st.perm, 2 * S * sizeof(int32_t));
    ALLOC(c->st.upd_count, kUpdCountBytes);
    ALLOC(c->st.upd_list, upd_list_bytes(d));
    ALLOC(c->st.spc_count, kSpcCountBytes);
    ALLOC(c->st.spc_list, 4 * S * sizeof(int32_t));
    if (d.seek_inner) {   // (else inner_buf / inner_cap stay 0: the context was value-initialised)
        c->st.inner_cap = 2 * inner_um(d);
        ALLOC(c->st.inner_buf, inner_buf_bytes(c));
    }
#undef ALLOC
#undef MMW_POISON_FRESH
    c->st.default_posture = c->d_posture;
    return MMW_OK;
}

static int create_init_device(mmw_ctx *c, int32_t n_scenes)
{
    const DevCfg &d = c->dc;
    const mmw_config *cfg = &c->cfg;
#ifdef MMW_MUTANT_NULL_STREAM_INIT
    // (diagnostic build `make DIAG=nullinit DIAGFLAGS=-DMMW_MUTANT_NULL_STREAM_INIT`, never the product: the round-5 initialisation,
    //  which scripts/dual_run.py must catch under load)
#define MMW_FILL0(ptr, bytes) hipMemset((ptr), 0, (bytes))
#else
#define MMW_FILL0(ptr, bytes) hipMemsetAsync((ptr), 0, (bytes), c->own_stream)
#endif
    if (hipMemcpyAsync(c->d_posture, cfg->default_posture, MMW_NKP * sizeof(float), hipMemcpyHostToDevice, c->own_stream) != hipSuccess ||
        MMW_FILL0(c->st.stats, kStatBytes) != hipSuccess || MMW_FILL0(c->st.db_count, kDbCountBytes) != hipSuccess ||
        MMW_FILL0(c->st.q, kQBytes) != hipSuccess || MMW_FILL0(c->st.db_list, db_list_bytes(d)) != hipSuccess ||
        MMW_FILL0(c->st.upd_count, kUpdCountBytes) != hipSuccess || MMW_FILL0(c->st.upd_list, upd_list_bytes(d)) != hipSuccess ||
        MMW_FILL0(c->st.spc_count, kSpcCountBytes) != hipSuccess || MMW_FILL0(c->st.trk, trk_bytes(d)) != hipSuccess ||
        MMW_FILL0(c->d_kp_gen, kp_gen_bytes(d)) != hipSuccess ||
        hipStreamSynchronize(c->own_stream) != hipSuccess) CREATE_FAIL(c, MMW_E_HIP, "device init failed");   // (the source of the posture copy is the context's own cfg)
    if (hipHostMalloc((void **)&c->h_rows, kTickets * sizeof(int32_t), hipHostMallocDefault) != hipSuccess) CREATE_FAIL(c, MMW_E_HIP, "hipHostMalloc failed");
    for (int k = 0; k < kTickets; k++) {
        c->h_rows[k] = 0;
        if (hipEventCreateWithFlags(&c->feat_ev[k], hipEventDisableTiming) != hipSuccess) CREATE_FAIL(c, MMW_E_HIP, "hipEventCreate failed");
    }
    if (d.side_worker && create_side_streams(c) != hipSuccess) CREATE_FAIL(c, MMW_E_HIP, "hipStreamCreate failed");
    size_t lds_b = dbscan_only_lds_bytes(c->UM);
    for (int k = 0; k < 3; k++) { const size_t v = dbscan_lds_bytes(k, c->UM, d.t_cap, cfg->db_min_samples); if (v > lds_b) lds_b = v; }
    const size_t lds_a = track_lds_bytes(d);
    if (lds_a > 160 * 1024 || lds_b > 160 * 1024) CREATE_FAIL(c, MMW_E_ARG, "LDS demand too large (track %zu B, dbscan %zu B > 160 KiB)", lds_a, lds_b);
    if (d.seek_inner) {
        if (inner_lds_demand(d) > 160 * 1024) CREATE_FAIL(c, MMW_E_ARG, "seek_inner: LDS demand too large (%zu B)", inner_lds_demand(d));
        if (prepare_inner(d) != hipSuccess) CREATE_FAIL(c, MMW_E_HIP, "hipFuncSetAttribute(k_inner) failed");
        if (MMW_FILL0(c->st.inner_buf, inner_buf_bytes(c)) != hipSuccess) CREATE_FAIL(c, MMW_E_HIP, "device init failed");
    }
#undef MMW_FILL0
    hipError_t e1 = prepare_track(d), e2 = prepare_dbscan(c->UM, d.t_cap, cfg->db_min_samples);
    if (e1 == hipSuccess && scene_lds_bytes(d) <= 160 * 1024) e1 = prepare_scene(d);
    if (e1 != hipSuccess || e2 != hipSuccess) CREATE_FAIL(c, MMW_E_HIP, "hipFuncSetAttribute(max dynamic LDS) failed: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2));
    c->st.huge_stride = dbscan_huge_slab_bytes(c->UM, d.t_cap, cfg->db_min_samples);
    if (c->st.huge_stride) {   // a ring of this context can hold a cloud the LDS cannot: one BallTree slab per worker of k_dbscan_huge
        const size_t slabs = c->st.huge_stride * (size_t)dbscan_huge_workers(n_scenes);
        if (hipMalloc((void **)&c->st.huge_scratch, slabs) != hipSuccess) CREATE_FAIL(c, MMW_E_HIP, "hipMalloc(%zu B of BallTree slabs) failed", slabs);
    }
    launch_reset(d, c->st, nullptr, c->d_kp_gen, c->stream);
    // every fill above and the reset kernel have finished before the caller sees the context
    if (hipStreamSynchronize(c->stream) != hipSuccess) CREATE_FAIL(c, MMW_E_HIP, "reset kernel failed: %s", hipGetErrorString(hipGetLastError()));
    return MMW_OK;
}

// A setter's launch over the scenes its caller flagged (NULL = every scene): the flags are staged in the feature-offset
// scratch (S + 1 words, not live between calls) and waited for, since the caller's array may go away
template <typename Launch> static int with_scene_flags(mmw_ctx *c, const int32_t *scene_flags, Launch launch)
{
    if (scene_flags) HIPCHK(c, hipMemcpyAsync(c->d_row_off, scene_flags, sizeof(int32_t) * c->dc.n_scenes, hipMemcpyHostToDevice, c->stream));
    launch(scene_flags ? c->d_row_off : nullptr);
    HIPCHK(c, hipGetLastError());
    if (scene_flags) HIPCHK(c, hipStreamSynchronize(c->stream));
    return MMW_OK;
}

// one direction of mmw_stream_wait / mmw_wait_stream: `waiter` does not go on before what `from` holds now has run
static int order_streams(mmw_ctx *c, hipEvent_t *ev, hipStream_t from, hipStream_t waiter)
{
    if (from == waiter) return MMW_OK;   // one stream: ordered as it is
    if (!*ev) HIPCHK(c, hipEventCreateWithFlags(ev, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(*ev, from));
    HIPCHK(c, hipStreamWaitEvent(waiter, *ev, 0));
    return MMW_OK;
}
static hipStream_t caller_stream(void *hip_stream) { return hip_stream == MMW_STREAM_LEGACY ? hipStreamLegacy : (hipStream_t)hip_stream; }   // (NULL is the legacy default stream already)

static mmw_scene_site site_of_config(const mmw_config &g)
{
    mmw_scene_site s;
    s.s_height = g.s_height; s.tilt_cos = g.tilt_cos; s.tilt_sin = g.tilt_sin;
    s.intensity_mu = g.intensity_mu; s.intensity_std = g.intensity_std;
    s.m_x = g.m_x; s.m_y = g.m_y; s.m_z = g.m_z;
    s.v_screen_fade_size_max = g.v_screen_fade_size_max; s.v_screen_fade_size_min = g.v_screen_fade_size_min;
    s.v_screen_fade_weight = g.v_screen_fade_weight;
    s.reserved_ = 0.0;
    return s;
}
static_assert(sizeof(mmw_scene_site) == 96, "mmw_scene_site");

// MMW_SRC_HASH: the first 16 hex digits of the SHA-256 of csrc/*.hip, csrc/*.hpp and include/mmw.h (csrc/Makefile passes it
// when this file is compiled, and this object depends on all of them): mmwave_msc_amd/_lib.py refuses a library whose
// hash is not that of the sources beside it.
#ifndef MMW_SRC_HASH
#define MMW_SRC_HASH "unhashed"
#endif
const char *mmw_version(void) { return "mmw-hip 0.4 (gfx950) src:" MMW_SRC_HASH; }

const char *mmw_kernel_name(int32_t k)
{
    static const char *names[MMW_K_COUNT] = {"k_track", "k_dbscan_big", "k_features", "k_normalize", "k_table", "k_predict", "k_post"};
    return (k >= 0 && k < MMW_K_COUNT) ? names[k] : "?";
}

int mmw_config_default(mmw_config *c)
{
    if (!c) return MMW_E_ARG;
    static const double lim[6] = {0.2, 0.2, 2, 1.2, 1.2, 0.2};
    static const float posture[MMW_NKP] = {
        0.0000f, -0.0007f, -0.0006f, -0.0038f, -0.1820f, -0.2540f, -0.2579f, 0.1830f, 0.2957f, 0.2940f,
        -0.0805f, -0.1141f, -0.1232f, -0.1358f, 0.0796f, 0.1436f, 0.1558f, 0.1720f, -0.0007f, 0.7699f,
        1.0906f, 1.4020f, 1.5513f, 1.2893f, 1.0360f, 0.7994f, 1.2865f, 1.0483f, 0.8117f, 0.7670f,
        0.3428f, 0.0000f, -0.0746f, 0.7713f, 0.3706f, -0.0128f, -0.0796f, 1.3255f, 0.0752f, 0.0533f,
        0.0203f, 0.0000f, 0.0496f, 0.1350f, 0.1303f, 0.0345f, 0.1277f, 0.1050f, 0.0392f, 0.0533f,
        0.0786f, -0.0056f, 0.0346f, -0.0007f, 0.0683f, -0.0082f, 0.0312f};
    memset(c, 0, sizeof(*c));
    c->fb_frames_batch = 2; c->db_min_samples = 35; c->tr_max_tracks = 4; c->kf_enable_est = 0;
    c->model_min_input = 0; c->dim_x = 9; c->ring_rows = 64; c->track_cap = 0; c->kalman_dense_min_units = 0;
    c->seek_inner = 0; c->chain_side_stream = 0; c->fused_step = 0; c->db_points_thres = 40; c->fb_frames_batch_static = 2; c->db_spread_thres = 0.7; c->db_inner_eps = 0.1;
    c->m_x = 0.32; c->m_y = -0.6; c->m_z = 1.3;
    c->v_screen_fade_size_max = 0.3; c->v_screen_fade_size_min = 0.2; c->v_screen_fade_weight = 0.08;
    c->db_z_weight = 0.4; c->db_range_weight = 0.03; c->db_eps = 0.3;
    c->tr_lifetime_dynamic = 3; c->tr_lifetime_static = 7; c->tr_vel_thres = 0.12; c->tr_gate = 4.5;
    c->kf_q_std = 1; c->kf_p_init = 0.1; c->kf_group_disp_est_init = 0.1; c->kf_a_n = 0.9; c->kf_est_pointnum = 10;
    memcpy(c->kf_spread_lim, lim, sizeof(lim));
    c->kf_a_spr = 0.9; c->intensity_mu = 27.0187; c->intensity_std = 70.351; c->s_height = 1.8;
    c->tilt_cos = 0.99619469809174555;   /* cos(radians(-5)) */
    c->tilt_sin = -0.087155742747658166; /* sin(radians(-5)) */
    memcpy(c->default_posture, posture, sizeof(posture));
    return MMW_OK;
}

const char *mmw_last_error(const mmw_ctx *ctx) { return ctx ? ctx->err.c_str() : g_last_error.c_str(); }

int mmw_create(const mmw_config *cfg, int32_t n_scenes, int32_t max_pts, int32_t device, mmw_ctx **out)
{
    if (!cfg || !out) return fail(nullptr, MMW_E_ARG, "mmw_create: null argument");
    *out = nullptr;
    MMW_TRY(check_create_args(cfg, n_scenes, max_pts));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(nullptr, MMW_E_NODEVICE, "no HIP device visible: libmmw_hip has no CPU path");
    if (device < 0 || device >= ndev) return fail(nullptr, MMW_E_NODEVICE, "device %d not available (%d visible)", device, ndev);
    mmw_ctx *c = new (std::nothrow) mmw_ctx();
    if (!c) return fail(nullptr, MMW_E_ARG, "out of host memory");
    c->cfg = *cfg;
    c->device = device;
    hipDeviceProp_t prop;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) { delete c; return fail(nullptr, MMW_E_HIP, "hipSetDevice / hipGetDeviceProperties(%d) -> %s", device, hipGetErrorString(e)); }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) { delete c; return fail(nullptr, MMW_E_NODEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName); }
    DevPlan plan;
    if (const int rc = derive_dev_cfg(cfg, n_scenes, max_pts, plan)) { delete c; return rc; }
    c->dc = plan.dc;
    c->UM = plan.dc.ring * max_pts;
    c->fused_wanted = plan.fused_wanted;
    c->side_wanted = plan.side_wanted;
    c->side_probed = c->side_trusted = plan.side_trusted;
    c->gate_side = plan.gate_side;
    MMW_TRY(create_alloc(c));
    MMW_TRY(create_init_device(c, n_scenes));
    *out = c;
    return MMW_OK;
}

int mmw_destroy(mmw_ctx *c)
{
    if (!c) return MMW_OK;
    hipSetDevice(c->device);
    // nothing of this context may still be running when its memory goes: the context's stream (the caller's or our own) and
    // the chain workers' side stream, which can poll the queues for a few ms after the last step
    if (c->stream) hipStreamSynchronize(c->stream);
    if (c->own_stream && c->own_stream != c->stream) hipStreamSynchronize(c->own_stream);
    if (c->side_stream) hipStreamSynchronize(c->side_stream);
    prof_fold(c);
    for (auto &ep : c->pool) { hipEventDestroy(ep.a); hipEventDestroy(ep.b); }
    void *ptrs[] = {c->st.hdr, c->st.order, c->st.trk, c->st.trk_ring, c->st.g_ring, c->d_posture, c->d_row_off, c->d_kp_gen, c->st.stats, c->st.db_list, c->st.db_count, c->st.q, c->d_probe, c->st.gate_buf, c->st.perm, c->st.upd_count, c->st.upd_list, c->st.spc_count, c->st.spc_list, c->st.inner_buf, c->d_in, c->d_out, c->d_raw, c->d_pchain,
                    c->d_export, c->st.huge_scratch, c->d_snap, c->d_sites, c->uart.buf};
    for (void *p : ptrs) if (p) hipFree(p);
    void *pinned[] = {c->h_in, c->h_out, c->h_hdr, c->h_q};
    for (void *p : pinned) if (p) hipHostFree(p);
    for (int k = 0; k < kTickets; k++) if (c->feat_ev[k]) hipEventDestroy(c->feat_ev[k]);
    if (c->handoff_ev) hipEventDestroy(c->handoff_ev);
    if (c->handback_ev) hipEventDestroy(c->handback_ev);
    if (c->h_rows) hipHostFree(c->h_rows);
    posture_batch_free(c->pb);
    export_free(c->rep);
    export_free(c->cloud);
    export_free(c->skel);
    export_free(c->sample);
    zone_free(c);
    trail_free(c);
    tripwire_free(c);
    stance_free(c);
    heat_free(c);
    uart_log_free(c);
    if (c->side_stream) hipStreamDestroy(c->side_stream);
    if (c->side_gate) hipEventDestroy(c->side_gate);
    if (c->own_stream) hipStreamDestroy(c->own_stream);
    delete c;
    return MMW_OK;
}

int mmw_reset(mmw_ctx *c)
{
    if (!c) return MMW_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    launch_reset(c->dc, c->st, nullptr, c->d_kp_gen, c->stream);
    HIPCHK(c, hipGetLastError());
    MMW_TRY(uid_rebase(c, nullptr));   // (report, zones, trails -- whichever is on: every scene's uids restart)
    c->dc.var_ring = 0;   // fresh BatchedData objects: default sizes again
    refresh_step_kind(c);
    c->ring_frames_bound = 0;
    return MMW_OK;
}

int mmw_reset_scenes(mmw_ctx *c, const int32_t *scene_flags)
{
    if (!c || !scene_flags) return fail(c, MMW_E_ARG, "mmw_reset_scenes: null argument");
    HIPCHK(c, hipSetDevice(c->device));
    int rebase_rc = MMW_OK;
    MMW_TRY(with_scene_flags(c, scene_flags, [&](const int32_t *f) {
        launch_reset(c->dc, c->st, f, c->d_kp_gen, c->stream);
        rebase_rc = uid_rebase(c, f);   // (report, zones, trails -- whichever is on: the reset scenes' uids restart)
    }));
    return rebase_rc;
}

int mmw_clear_errors(mmw_ctx *c, const int32_t *scene_flags, int32_t bits)
{
    if (!c) return MMW_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return with_scene_flags(c, scene_flags, [&](const int32_t *f) { launch_clear_errors(c->dc, c->st, f, bits, c->stream); });
}

int mmw_pop_frame(mmw_ctx *c, const int32_t *scene_flags)
{
    if (!c) return MMW_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return with_scene_flags(c, scene_flags, [&](const int32_t *f) { launch_pop_frame(c->dc, c->st, f, c->stream); });
}

int mmw_set_batch_size(mmw_ctx *c, const int32_t *scene_flags, int32_t new_size)
{
    if (!c) return MMW_E_ARG;
    // a deque(maxlen = FB_FRAMES_BATCH + 1) never holds more than that whatever `size` says; size <= 0 would never leave
    // add_frame's `while len(buffer) >= size: pop_frame()` in the reference
    if (new_size < 1) return fail(c, MMW_E_ARG, "mmw_set_batch_size: new_size = %d (BatchedData.add_frame would not terminate)", new_size);
    if (new_size > c->dc.ring) new_size = c->dc.ring;
    HIPCHK(c, hipSetDevice(c->device));
    MMW_TRY(with_scene_flags(c, scene_flags, [&](const int32_t *f) { launch_set_batch_size(c->dc, c->st, f, new_size, c->stream); }));
    c->dc.var_ring = 1;   // resized rings are k_track's (its INNER instantiations read the sizes per ring); the state layout is the same
    refresh_step_kind(c);
    return MMW_OK;
}

int mmw_set_batch_frame(mmw_ctx *c, int32_t scene, const double *rows, int32_t n)
{
    if (!c || scene < 0 || scene >= c->dc.n_scenes || n < 0 || n > c->dc.max_pts || (n > 0 && !rows)) return fail(c, MMW_E_ARG, "mmw_set_batch_frame: bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    SceneHdr h;
    MMW_TRY(d2h_after_kernels(c, &h, c->st.hdr + scene, sizeof(h)));
    h.g_len = 1;
    if (c->ring_frames_bound < 1) c->ring_frames_bound = 1;
    for (int k = 0; k < MMW_RING_MAX; k++) h.g_n[k] = 0;
    h.g_n[0] = n;
    {   // the ring's non-finite flags (SceneHdr.skipped bits 16..23): this frame's, for the slot it is written to
        int bits = 0;
        for (size_t i = 0; i < (size_t)n * 8; i++) bits |= std::isnan(rows[i]) ? 1 : (std::isinf(rows[i]) ? 2 : 0);
        const int nff = nf_flags_with((h.skipped >> kSkipNfShift) & kSkipNfMask, h.g_slot[0], bits);
        h.skipped = (h.skipped & ~(kSkipNfMask << kSkipNfShift)) | (nff << kSkipNfShift);
    }
    double *dst = c->st.g_ring + ((size_t)scene * c->dc.ring + h.g_slot[0]) * (size_t)c->dc.max_pts * 8;
    if (n > 0) HIPCHK(c, hipMemcpyAsync(dst, rows, (size_t)n * 8 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->st.hdr + scene, &h, sizeof(h), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MMW_OK;
}

// ---- per-scene sites ----
int mmw_set_sites(mmw_ctx *c, const int32_t *scenes, int32_t n, const mmw_scene_site *sites)
{
    if (!c) return fail(nullptr, MMW_E_ARG, "mmw_set_sites: null context");
    const int S = c->dc.n_scenes;
    // every check first: a refused call changes no scene's site (and does not allocate or switch the table on)
    if (n < 0 || n > S) return fail(c, MMW_E_ARG, "mmw_set_sites: n = %d, the context has %d scenes", n, S);
    if (n > 0 && !sites) return fail(c, MMW_E_ARG, "mmw_set_sites: sites is NULL with n = %d", n);
    std::vector<char> seen(scenes ? (size_t)S : 0, 0);
    for (int i = 0; i < n; i++) {
        const int s = scenes ? scenes[i] : i;
        if (s < 0 || s >= S) return fail(c, MMW_E_ARG, "mmw_set_sites: entry %d names scene %d, the context has %d scenes", i, s, S);
        if (scenes) {
            if (seen[s]) return fail(c, MMW_E_ARG, "mmw_set_sites: entry %d names scene %d a second time", i, s);
            seen[s] = 1;
        }
        // (as bits: -0.0 and NaN are not 0)
        unsigned long long r;
        memcpy(&r, &sites[i].reserved_, sizeof(r));
        if (r != 0) return fail(c, MMW_E_ARG, "mmw_set_sites: entry %d (scene %d) has a non-zero reserved_", i, s);
    }
    HIPCHK(c, hipSetDevice(c->device));
    // The new table is put together on the host (a copy of the mirror: a failure below leaves the context as it was) and
    // travels as ONE copy, ordered on the context's stream: what was queued before this call reads the old table.
    std::vector<mmw_scene_site> next = c->h_sites;
    if (!c->sites_on) next.assign((size_t)S, site_of_config(c->cfg));   // the first call, or the first after mmw_clear_sites: every scene starts from the config's own values
    for (int i = 0; i < n; i++) next[scenes ? scenes[i] : i] = sites[i];
    if (!c->d_sites) HIPCHK(c, hipMalloc((void **)&c->d_sites, sizeof(mmw_scene_site) * (size_t)S));
    HIPCHK(c, hipMemcpyAsync(c->d_sites, next.data(), sizeof(mmw_scene_site) * (size_t)S, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (`next` is pageable and goes away)
    c->h_sites.swap(next);
    c->sites_on = 1;
    return MMW_OK;
}

int mmw_get_sites(mmw_ctx *c, mmw_scene_site *out)
{
    if (!c || !out) return fail(c, MMW_E_ARG, "mmw_get_sites: null argument");
    const size_t S = (size_t)c->dc.n_scenes;
    const mmw_scene_site own = site_of_config(c->cfg);
    for (size_t i = 0; i < S; i++) out[i] = own;
    if (c->sites_on) memcpy(out, c->h_sites.data(), S * sizeof(mmw_scene_site));   // (the host mirror of the device table)
    return MMW_OK;
}

int mmw_clear_sites(mmw_ctx *c)
{
    if (!c) return fail(nullptr, MMW_E_ARG, "mmw_clear_sites: null context");
    c->sites_on = 0;   // (launches already queued carry the table's pointer: it stays allocated until mmw_destroy)
    return MMW_OK;
}

int mmw_has_sites(mmw_ctx *c)
{
    if (!c) return fail(nullptr, MMW_E_ARG, "mmw_has_sites: null context");
    return c->sites_on;
}

// ---- streams ----
int mmw_set_chain_side_stream(mmw_ctx *c, int32_t on)
{
    if (!c) return MMW_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (on && c->dc.seek_inner) return fail(c, MMW_E_ARG, "mmw_set_chain_side_stream: not with seek_inner (k_inner may cancel queued scenes)");
    if (on && !c->side_stream) HIPCHK(c, create_side_streams(c));
    c->dc.side_worker = c->side_wanted = on ? 1 : 0;   // takes effect with the next mmw_step (the queues are empty between steps)
    refresh_step_kind(c);   // the workers claim scenes while k_track runs: the bulk kernels' step
    c->side_probed = c->side_trusted;
    return MMW_OK;
}

int mmw_set_stream(mmw_ctx *c, void *s)
{
    if (!c) return MMW_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    hipStreamSynchronize(c->stream);
    c->stream = s ? (hipStream_t)s : c->own_stream;
    c->dc.side_worker = c->side_wanted;   // (checked against the new stream by the next mmw_step)
    c->side_probed = c->side_trusted;
    refresh_step_kind(c);
    return MMW_OK;
}

int mmw_synchronize(mmw_ctx *c)
{
    if (!c) return MMW_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MMW_OK;
}

int mmw_stream_wait(mmw_ctx *c, void *hip_stream)
{
    if (!c) return MMW_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return order_streams(c, &c->handoff_ev, c->stream, caller_stream(hip_stream));
}

int mmw_wait_stream(mmw_ctx *c, void *hip_stream)
{
    if (!c) return MMW_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return order_streams(c, &c->handback_ev, caller_stream(hip_stream), c->stream);
}

int mmw_side_workers(mmw_ctx *c) { return !c ? MMW_E_ARG : c->dc.side_worker ? (c->side_probed ? 1 : 2) : 0; }

int mmw_streams_concurrent(mmw_ctx *c, void *stream_a, void *stream_b)
{
    if (!c) return MMW_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const int ok = probe_one(c, (hipStream_t)stream_b, (hipStream_t)stream_a);
    if (ok < 0) return fail(c, MMW_E_HIP, "mmw_streams_concurrent: probe failed: %s", hipGetErrorString(hipGetLastError()));
    return ok;
}

// ---- device memory ----
int mmw_dev_alloc(mmw_ctx *c, size_t bytes, void **dptr)
{
    if (!c || !dptr) return MMW_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMalloc(dptr, bytes ? bytes : 8));
    return MMW_OK;
}
int mmw_dev_free(mmw_ctx *c, void *p)
{
    if (!c) return MMW_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (p) HIPCHK(c, hipFree(p));
    return MMW_OK;
}
int mmw_memcpy_h2d(mmw_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (!c) return MMW_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MMW_OK;
}
int mmw_memcpy_d2h(mmw_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (!c) return MMW_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return d2h_after_kernels(c, dst, src, bytes);
}
