// api_step.hip -- the C-ABI (include/mmw.h): a frame through the tracker.  normalize_data, TrackBuffer.track as mmw_step, the
// host-staged frame (mmw_frame_host and its kin) and the stand-alone DBSCAN.
#include "mmw_ctx.hpp"

static int normalize_impl(mmw_ctx *c, const void *raw, bool f32, const int32_t *n_raw, double *pts, int32_t *n_out)
{
    if (!c || !raw || !n_raw || !pts || !n_out) return fail(c, MMW_E_ARG, "mmw_normalize: null pointer");
    if (((uintptr_t)pts & 15) != 0) return fail(c, MMW_E_ARG, "mmw_normalize: pts must be 16-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    EventPair ep;
    prof_arm(c, MMW_K_NORMALIZE, ep);
    launch_normalize(c->dc, sites_or_null(c), raw, f32, n_raw, pts, n_out, c->stream);
    prof_armed_done(c, ep);
    HIPCHK(c, hipGetLastError());
    return MMW_OK;
}

static int step_impl(mmw_ctx *c, const void *pts, bool f32, const int32_t *n_pts, const double *dt, int32_t *assoc, int32_t *db_labels, int32_t *db_n)
{
    if (!c || !pts || !n_pts || !dt) return fail(c, MMW_E_ARG, "mmw_step: null input pointer");
    if (((uintptr_t)pts & 15) != 0) return fail(c, MMW_E_ARG, "mmw_step: pts must be 16-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    EventPair ep;
    // a cloud is the unassigned part of the ring's frames: in the first steps after a reset it cannot be larger than the
    // frames pushed so far, and the large-cloud launches are carved (LDS per workgroup -> workgroups per CU) for that bound
    if (c->ring_frames_bound < c->dc.ring) c->ring_frames_bound++;
    const int u_bound = c->ring_frames_bound * c->dc.max_pts;
    c->dc.big_live = (c->dc.side_worker && c->ring_frames_bound >= c->dc.ring) ? 1 : 0;  // (set again below if the probe turns the workers off)
    // the chain workers of this step wait on the side stream for what k_track queues.  Nothing orders them with the context's
    // stream but the queue protocol itself: they only touch scenes k_track has published, and they claim only while the stop
    // epoch says that the step in flight is THEIR step (k_chain, k_dbscan.hip) -- a launch that runs early (steps queued ahead of
    // a stalled context stream) polls and idles out, one that runs late leaves at once.
    if (c->dc.side_worker && !c->side_probed) {
        // first step on this stream set-up: the workers are only used if they really run BESIDE the context's stream
        const int ok = probe_side_streams(c);
        if (ok < 0) return fail(c, MMW_E_HIP, "side-stream probe failed: %s", hipGetErrorString(hipGetLastError()));
        c->side_probed = 1;
        if (!ok) c->dc.side_worker = c->dc.big_live = 0;
    }
    if (c->dc.side_worker && c->gate_side) {
        // No event between the two streams: the side stream paces itself -- the workers of step f leave when k_post(f) has raised
        // its stop epoch, the workers of step f + 1 start behind them and find empty queues until k_track(f + 1) pushes (idle polls
        // with s_sleep: twelve workgroups, ~70 us early in a back-to-back loop).  The event recorded at the head of every step (so
        // that they would not start early) was a marker packet on the context's stream: 7 us of idle chip per step in the
        // kernel trace (profiles/NOTEBOOK.md, round 4).  gate_side = 1 (callers with their own work on the context's stream,
        // mmw_config.chain_side_stream = 3) keeps the event.
        HIPCHK(c, hipEventRecord(c->side_gate, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->side_stream, c->side_gate, 0));
    }
    // the step number of the queue protocol counts COMMITTED steps: a step that left above (probe, gate event) has launched no
    // k_post, so no stop epoch was raised for it -- counting it would leave q[kQStop] one behind for good, and every later k_chain
    // would poll to its idle limit without ever claiming
    c->epoch++;
    c->dc.epoch = c->epoch;   // (k_track / k_scene tag the claim words of the NEXT step's queues with it: mmw_device.hpp, q_tag)
    if (c->dc.side_worker) launch_chain(c->dc, c->st, c->UM, u_bound, c->step_parity, c->epoch, db_labels, db_n, c->side_stream);
    // TrackBuffer.track (Tracking.py:683-703) = four launches on one stream:
    prof_arm(c, MMW_K_PREDICT, ep);
    launch_predict(c->dc, c->st, n_pts, dt, c->step_parity, c->stream);
    prof_armed_done(c, ep);
    prof_arm(c, MMW_K_TRACK, ep);
    if (c->dc.fused) launch_scene(c->dc, c->st, pts, f32, n_pts, dt, assoc, db_n, db_labels, c->UM, c->step_parity, c->stream);
    else launch_track(c->dc, c->st, pts, f32, n_pts, dt, assoc, db_n, db_labels, c->UM, c->step_parity, c->stream);
    prof_armed_done(c, ep);
    if (c->dc.seek_inner) launch_inner(c->dc, c->st, n_pts, db_n, c->stream);  // Tracking.py:656 active
    prof_arm(c, MMW_K_POST, ep);
    launch_post(c->dc, c->st, n_pts, c->UM, u_bound, c->step_parity, c->epoch, db_labels, db_n, c->stream);
    prof_armed_done(c, ep);
    prof_arm(c, MMW_K_DBSCAN, ep);
    launch_dbscan_big(c->dc, c->st, c->UM, u_bound, c->step_parity, db_labels, db_n, c->stream);
    launch_dbscan_huge(c->dc, c->st, c->UM, u_bound, c->step_parity, db_labels, db_n, c->stream);  // (contexts with ring * max_pts > 1920 only)
    prof_armed_done(c, ep);
    if (c->pending.size() >= 2048) prof_fold(c);
    c->step_parity ^= 1;
    HIPCHK(c, hipGetLastError());
    return MMW_OK;
}

// layout of the two staging blocks (bytes; every part 16-byte aligned)
struct StageLayout { size_t in_rows, in_dt, in_n, in_bytes, out_assoc, out_dbn, out_nout, out_prows, out_labels, out_bytes; };
static StageLayout stage_layout(const mmw_ctx *c)
{
    const size_t S = c->dc.n_scenes, NP = c->dc.max_pts;
    auto al = [](size_t v) { return (v + 15) & ~(size_t)15; };
    StageLayout L;
    L.in_dt = 0;   // [dt | n | rows]: the two small arrays in front, so that a frame's upload is ONE copy that ends with its last valid row
    L.in_n = al(S * sizeof(double));
    L.in_rows = L.in_n + al(S * sizeof(int32_t));
    L.in_bytes = L.in_rows + al(S * NP * 8 * sizeof(double));
    L.out_assoc = 0;
    L.out_dbn = al(S * NP * sizeof(int32_t));
    L.out_nout = L.out_dbn + al(S * sizeof(int32_t));
    L.out_prows = L.out_nout + al(S * sizeof(int32_t));
    L.out_labels = L.out_prows + 16;
    L.out_bytes = L.out_labels + al(S * (size_t)c->UM * sizeof(int32_t));
    return L;
}

static int ensure_host_staging(mmw_ctx *c)
{
    if (c->d_in) return MMW_OK;
    const StageLayout L = stage_layout(c);
    const size_t S = c->dc.n_scenes, NP = c->dc.max_pts;
    HIPCHK(c, hipMalloc((void **)&c->d_in, L.in_bytes));
    HIPCHK(c, hipMalloc((void **)&c->d_out, L.out_bytes));
    HIPCHK(c, hipMalloc((void **)&c->d_raw, S * NP * 8 * sizeof(double)));   // (the raw form: normalize_data's rows, what the step reads)
    HIPCHK(c, hipHostMalloc((void **)&c->h_in, L.in_bytes, hipHostMallocDefault));
    HIPCHK(c, hipHostMalloc((void **)&c->h_out, L.out_bytes, hipHostMallocDefault));
    HIPCHK(c, hipHostMalloc((void **)&c->h_hdr, S * sizeof(SceneHdr), hipHostMallocDefault));
    HIPCHK(c, hipHostMalloc((void **)&c->h_q, kQWords * sizeof(int32_t), hipHostMallocDefault));
    c->d_pts = reinterpret_cast<double *>(c->d_in + L.in_rows);
    c->d_dt = reinterpret_cast<double *>(c->d_in + L.in_dt);
    c->d_n = reinterpret_cast<int32_t *>(c->d_in + L.in_n);
    c->d_assoc = reinterpret_cast<int32_t *>(c->d_out + L.out_assoc);
    c->d_dbn = reinterpret_cast<int32_t *>(c->d_out + L.out_dbn);
    c->d_nout = reinterpret_cast<int32_t *>(c->d_out + L.out_nout);
    c->d_prows = reinterpret_cast<int32_t *>(c->d_out + L.out_prows);
    c->d_labels = reinterpret_cast<int32_t *>(c->d_out + L.out_labels);
    return MMW_OK;
}

// One frame of every scene from host memory in ONE round trip: the inputs leave as one copy from a pinned block, the kernels
// follow, the results, the scene headers (track counts, error bits) and the queue words come back as three copies into pinned
// memory, and the stream is waited for once.  (mmw_step_host used to wait four times: the step, mmw_check's two read-backs.)
static int frame_impl(mmw_ctx *c, const double *raw, const double *pts, const int32_t *n, const double *dt, double *pts_out, int32_t *n_out,
                      int32_t *assoc, int32_t *db_labels, int32_t *db_n, int32_t *n_tracks, bool posture, int32_t *posture_rows)
{
    if (!c || !n || !dt || (!raw && !pts) || (raw && pts)) return fail(c, MMW_E_ARG, "mmw_frame_host: exactly one of raw / pts, and n, dt");
    if (posture && !c->has_model) return fail(c, MMW_E_ARG, "mmw_frame_posture_host: no model attached (mmw_attach_posture)");
    HIPCHK(c, hipSetDevice(c->device));
    MMW_TRY(ensure_host_staging(c));
    const StageLayout L = stage_layout(c);
    const size_t S = c->dc.n_scenes, NP = c->dc.max_pts, UM = (size_t)c->UM;
    // rows: only the scenes' valid rows travel inside their slots (the slots are max_pts apart); small frames stay small
    const size_t row_doubles = raw ? 5 : 8;
    double *h_rows = reinterpret_cast<double *>(c->h_in + L.in_rows);
    size_t rows_span = 0;   // bytes of the row area that must be sent: up to the end of the last scene's valid rows
    for (size_t s = 0; s < S; s++) {
        const int cnt = n[s];
        if (cnt > 0 && (size_t)cnt <= NP) {
            memcpy(h_rows + s * NP * row_doubles, (raw ? raw : pts) + s * NP * row_doubles, (size_t)cnt * row_doubles * sizeof(double));
            rows_span = (s * NP + (size_t)cnt) * row_doubles * sizeof(double);
        }
    }
    memcpy(c->h_in + L.in_dt, dt, S * sizeof(double));
    memcpy(c->h_in + L.in_n, n, S * sizeof(int32_t));
    HIPCHK(c, hipMemcpyAsync(c->d_in, c->h_in, L.in_rows + rows_span, hipMemcpyHostToDevice, c->stream));   // [dt | n | rows up to the last valid one]
    double *d_rows = c->d_pts;   // what the step reads
    const int32_t *d_cnt = c->d_n;
    if (raw) {
        d_rows = c->d_raw;
        d_cnt = c->d_nout;
        MMW_TRY(normalize_impl(c, c->d_pts, false, c->d_n, d_rows, c->d_nout));   // (the raw rows sit in the row area of the upload block)
    }
    MMW_TRY(step_impl(c, d_rows, false, d_cnt, c->d_dt, c->d_assoc, c->d_labels, c->d_dbn));
    if (posture) {
        // TrackBuffer.estimate_posture behind the step, unless the frame was skipped (k_features reads the frame's row count): the
        // rows are counted on the device, every launch covers the capacity and its surplus workgroups leave on that word
        const int cap = c->dc.t_cap;
        launch_features(c->dc, sites_or_null(c), c->st, nullptr, c->pc_feat, c->pc_owner, nullptr, cap, c->stream, d_cnt, c->d_prows);
        launch_mars_small_f32(c->model_frames, c->pc_feat, c->model, c->pc_act, c->pc_hidden, c->pc_kp, cap, c->stream, c->d_prows);
        launch_set_kp(c->dc, c->st, c->pc_kp, c->pc_owner, cap, c->stream, c->d_prows);
        HIPCHK(c, hipGetLastError());
    }
    // results: [assoc | db_n | n_out | posture rows] always, the labels when asked for; headers and queue words for the error check
    const size_t head = db_labels ? L.out_bytes : L.out_labels;
    HIPCHK(c, hipMemcpyAsync(c->h_out, c->d_out, head, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_hdr, c->st.hdr, S * sizeof(SceneHdr), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_q, c->st.q, kQWords * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    double *h_pts_out = nullptr;
    if (raw && pts_out) {   // normalize_data's rows (the reference's `effective_data`): into the pinned row area, now free again
        h_pts_out = reinterpret_cast<double *>(c->h_in + L.in_rows);
        HIPCHK(c, hipMemcpyAsync(h_pts_out, d_rows, S * NP * 8 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (assoc) memcpy(assoc, c->h_out + L.out_assoc, S * NP * sizeof(int32_t));
    if (db_n) memcpy(db_n, c->h_out + L.out_dbn, S * sizeof(int32_t));
    if (n_out) memcpy(n_out, raw ? c->h_out + L.out_nout : c->h_in + L.in_n, S * sizeof(int32_t));
    if (db_labels) memcpy(db_labels, c->h_out + L.out_labels, S * UM * sizeof(int32_t));
    if (h_pts_out) memcpy(pts_out, h_pts_out, S * NP * 8 * sizeof(double));
    if (n_tracks) for (size_t s = 0; s < S; s++) n_tracks[s] = c->h_hdr[s].n_tracks;
    if (posture_rows) *posture_rows = posture ? *reinterpret_cast<const int32_t *>(c->h_out + L.out_prows) : 0;
    return first_scene_error(c, c->h_hdr, S, c->h_q);
}

int mmw_normalize(mmw_ctx *c, const double *raw, const int32_t *n_raw, double *pts, int32_t *n_out) { return normalize_impl(c, raw, false, n_raw, pts, n_out); }
int mmw_normalize_f32(mmw_ctx *c, const float *raw, const int32_t *n_raw, double *pts, int32_t *n_out) { return normalize_impl(c, raw, true, n_raw, pts, n_out); }

int mmw_normalize_tlv(mmw_ctx *c, const uint8_t *packets, size_t packets_bytes, const int64_t *tlv_offset, const mmw_uart_cfg *cfg, double *pts,
                      int32_t *n_out)
{
    if (!c || !packets || !tlv_offset || !cfg || !pts || !n_out) return fail(c, MMW_E_ARG, "mmw_normalize_tlv: null pointer");
    if (((uintptr_t)pts & 15) != 0 || ((uintptr_t)packets & 1) != 0) return fail(c, MMW_E_ARG, "mmw_normalize_tlv: pts must be 16-byte aligned, packets 2-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    EventPair ep;
    prof_arm(c, MMW_K_NORMALIZE, ep);
    static_assert(sizeof(long long) == sizeof(int64_t), "tlv offsets");
    launch_normalize_tlv(c->dc, sites_or_null(c), packets, (long long)packets_bytes, reinterpret_cast<const long long *>(tlv_offset), cfg->num_doppler_bins / 2.0 - 1,
                         cfg->doppler_resolution_mps, pts, n_out, c->stream);
    prof_armed_done(c, ep);
    HIPCHK(c, hipGetLastError());
    return MMW_OK;
}

int mmw_step(mmw_ctx *c, const double *pts, const int32_t *n_pts, const double *dt, int32_t *assoc, int32_t *db_labels, int32_t *db_n) { return step_impl(c, pts, false, n_pts, dt, assoc, db_labels, db_n); }
int mmw_step_f32(mmw_ctx *c, const float *pts, const int32_t *n_pts, const double *dt, int32_t *assoc, int32_t *db_labels, int32_t *db_n) { return step_impl(c, pts, true, n_pts, dt, assoc, db_labels, db_n); }

int mmw_frame_host(mmw_ctx *c, const double *raw, const double *pts, const int32_t *n, const double *dt, double *pts_out, int32_t *n_out,
                   int32_t *assoc, int32_t *db_labels, int32_t *db_n, int32_t *n_tracks)
{
    return frame_impl(c, raw, pts, n, dt, pts_out, n_out, assoc, db_labels, db_n, n_tracks, false, nullptr);
}

int mmw_frame_posture_host(mmw_ctx *c, const double *raw, const double *pts, const int32_t *n, const double *dt, double *pts_out, int32_t *n_out,
                           int32_t *assoc, int32_t *db_labels, int32_t *db_n, int32_t *n_tracks, int32_t *posture_rows)
{
    return frame_impl(c, raw, pts, n, dt, pts_out, n_out, assoc, db_labels, db_n, n_tracks, true, posture_rows);
}

int mmw_step_host(mmw_ctx *c, const double *pts, const int32_t *n_pts, const double *dt, int32_t *assoc, int32_t *db_labels, int32_t *db_n)
{
    if (!c || !pts || !n_pts || !dt) return fail(c, MMW_E_ARG, "mmw_step_host: null input pointer");
    return frame_impl(c, nullptr, pts, n_pts, dt, nullptr, nullptr, assoc, db_labels, db_n, nullptr, false, nullptr);
}

int mmw_dbscan(mmw_ctx *c, const double *pts, const int32_t *n, int32_t max_n, double eps, int32_t min_samples, int32_t *labels, int32_t *n_clusters)
{
    if (!c || !pts || !n || !labels) return fail(c, MMW_E_ARG, "mmw_dbscan: null pointer");
    if (max_n < 1 || max_n > c->UM) return fail(c, MMW_E_ARG, "mmw_dbscan: max_n=%d must be in [1, ring*max_pts=%d]", max_n, c->UM);
    if (!(eps > 0.0) || min_samples < 1) return fail(c, MMW_E_ARG, "mmw_dbscan: eps must be > 0 and min_samples >= 1 (sklearn's DBSCAN refuses anything else)");
    HIPCHK(c, hipSetDevice(c->device));
    launch_dbscan_only(c->dc, c->st, c->UM, pts, n, max_n, eps, min_samples, labels, n_clusters, c->stream);
    HIPCHK(c, hipGetLastError());
    return MMW_OK;
}
