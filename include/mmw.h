/*
 * mmw.h -- C-ABI of libmmw_hip.so: the MI355X (gfx950) implementation of the
 * per-frame point-cloud hot path of AsteriosPar/mmWave_MSc.
 *
 * The reference has no FFI for this path: it is plain Python
 * (`TrackBuffer.track`, `TrackBuffer.estimate_posture`, `Utils.normalize_data`,
 * `Utils.apply_DBscan`).  Each entry point below names the reference interface
 * it replaces (file:line under the reference's src/); INTEGRATION.md shows the
 * ctypes binding a reference maintainer would add.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes; no C++/torch types.
 *  - Every function returns 0 on success, <0 on error (MMW_E_*); never throws.
 *    `mmw_last_error(ctx)` returns a message (ctx may be NULL for create errors).
 *  - One context = S independent scenes (one reference TrackBuffer + global
 *    BatchedData each) resident on ONE device.  A context is used from one host
 *    thread at a time; calls are ordered on the context's HIP stream and are
 *    asynchronous unless stated ("sync").
 *  - "dev" pointers are device memory of the context's device (hipMalloc,
 *    torch.Tensor.data_ptr(), or mmw_dev_alloc); "host" pointers are host memory.
 *  - There is NO CPU fallback: creation fails if no gfx950-capable HIP device
 *    is usable.
 *  - Numerics: tracker state and every decision in fp64 (the reference's numpy
 *    dtype), features in fp32 (what Keras feeds the CNN).
 */
#ifndef MMW_H
#define MMW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMW_RING_MAX 4      /* FB_FRAMES_BATCH + 1 <= 4 */
#define MMW_NKP 57          /* 19 joints x (x,y,z)  (preprocessing.py:377) */
#define MMW_MAX_PTS_LIMIT 1024
#define MMW_TRACK_CAP_LIMIT 64
#define MMW_EMPTY_FRAME (-1) /* n_pts value: TrackBuffer.track() on an empty point cloud (0 = frame skipped) */

#define MMW_OK 0
#define MMW_E_ARG (-1)        /* bad argument / size */
#define MMW_E_SINGULAR (-2)   /* a 6x6 gate/innovation matrix was singular (numpy raises LinAlgError) */
#define MMW_E_DIVZERO (-3)    /* (N_est-1)*N == 0 in _get_Rc (Python raises ZeroDivisionError) */
#define MMW_E_CAPACITY (-4)   /* more tracks than track_cap; mmw_parse_uart_cap: a packet that reaches past the buffer's capacity */
#define MMW_E_HIP (-5)        /* HIP runtime error */
#define MMW_E_NODEVICE (-6)   /* no usable gfx950 device: the library has no CPU path */
#define MMW_E_NONFINITE (-7)  /* apply_DBscan was reached with a NaN or an infinite value in its cloud: sklearn's input validation raises
                                 ValueError there (Utils.py:272-278 -> DBSCAN.fit_predict -> check_array).  Any of the 8 columns of any row
                                 of the global ring counts; the gate never takes a point whose columns 0..5 are not finite
                                 (Tracking.py:559-563), so such rows always end up there.  The frame is in the ring, nothing was
                                 clustered or cleared -- exactly the state the exception leaves -- and the scene raises again on every
                                 frame the row is still in the ring while the trigger holds (Tracking.py:693-697) */
#define MMW_DB_RAISED (-2)    /* db_n of a scene whose apply_DBscan call of this frame raised (MMW_E_NONFINITE); -1 = not called */

/* Mirrors constants.py 1:1 (line numbers = /root/reference/src/constants.py). */
typedef struct mmw_config {
    int32_t fb_frames_batch;        /* FB_FRAMES_BATCH :66  (ring length = +1) */
    int32_t db_min_samples;         /* DB_MIN_SAMPLES_MIN :73 */
    int32_t tr_max_tracks;          /* TR_MAX_TRACKS :85 */
    int32_t kf_enable_est;          /* KF_ENABLE_EST :100 */
    int32_t model_min_input;        /* MODEL_MIN_INPUT :111 */
    int32_t dim_x;                  /* MOTION_MODEL :246 -> 9 CONST_ACC_MODEL (176-215), 6 CONST_VEL_MODEL (218-243) */
    int32_t ring_rows;              /* rows stored per frame of a per-track ring; >=64 (format_single_frame reads [:64]) */
    int32_t track_cap;              /* capacity of effective_tracks per scene; 0 = (TR_MAX_TRACKS-1)+ring*max_pts/min_samples+1, <=64 */
    double db_z_weight;             /* DB_Z_WEIGHT :70 */
    double db_range_weight;         /* DB_RANGE_WEIGHT :71 */
    double db_eps;                  /* DB_EPS :72 */
    double tr_lifetime_dynamic;     /* TR_LIFETIME_DYNAMIC :86 */
    double tr_lifetime_static;      /* TR_LIFETIME_STATIC :87 */
    double tr_vel_thres;            /* TR_VEL_THRES :88 */
    double tr_gate;                 /* TR_GATE :89 */
    double kf_q_std;                /* KF_Q_STD :93 (passed as var= to Q_discrete_white_noise :212) */
    double kf_p_init;               /* KF_P_INIT :96 */
    double kf_group_disp_est_init;  /* KF_GROUP_DISP_EST_INIT :97 */
    double kf_a_n;                  /* KF_A_N :101 */
    double kf_est_pointnum;         /* KF_EST_POINTNUM :102 */
    double kf_spread_lim[6];        /* KF_SPREAD_LIM :103 */
    double kf_a_spr;                /* KF_A_SPR :104 */
    double intensity_mu;            /* INTENSITY_MU :108 */
    double intensity_std;           /* INTENSITY_STD :109 */
    double s_height;                /* S_HEIGHT :41 */
    double tilt_cos;                /* cos(radians(S_TILT)) :42, Utils.py:315-323 */
    double tilt_sin;                /* sin(radians(S_TILT)) */
    float default_posture[MMW_NKP]; /* MODEL_DEFAULT_POSTURE :112-172 */
    int32_t kalman_dense_min_units; /* not a reference constant: layout of the Kalman kernels.  0 = automatic (laid out over tracks
                                       when the context holds more than 512 scenes and > 1024 four-track waves; smaller contexts run
                                       a two-launch step per scene), < 0 = always per scene, n > 0 = over tracks from n waves on
                                       (tests run both layouts) */
    int32_t seek_inner;             /* 0 = Tracking.py:656 stays commented out (the reference as shipped); 1 = run
                                       ClusterTrack.seek_inner_clusters (Tracking.py:409-448) after every associate_pointcloud */
    int32_t db_points_thres;        /* DB_POINTS_THRES :76   (seek_inner_clusters) */
    int32_t fb_frames_batch_static; /* FB_FRAMES_BATCH_STATIC :67 */
    int32_t chain_side_stream;      /* not a reference constant: where the small-cloud DBSCAN (pair-count screen, BallTree chain) of a
                                       frame runs.  0 = automatic (contexts of > 512 scenes: worker blocks on a second stream beside
                                       the association kernel, whatever they have not taken by its end in the post kernel), -1 = post
                                       kernel only, 1 = always with the side stream (tests run both), 2 = as 1 without the check that
                                       the side stream really runs beside the context's (profilers that serialise kernels fail it: the
                                       workers then start, find nothing to claim in time and leave -- correct, and visible as a launch),
                                       3 = as 1, and the workers of a step do not start before the step's first kernel does (an event
                                       recorded on the context's stream at the head of every step: ~7 us per step; for callers that
                                       queue their own work on the context's stream between steps -- by default the side stream paces
                                       itself by the steps' stop epochs and its workers may poll empty queues a little early) */
    double db_spread_thres;         /* DB_SPREAD_THRES :77 */
    double db_inner_eps;            /* DB_INNER_EPS :78 */
    double m_x, m_y, m_z;           /* M_X, M_Y, M_Z :31-33  monitoring point (calc_projection_points, Utils.py:180-219) */
    double v_screen_fade_size_max;  /* V_SCREEN_FADE_SIZE_MAX :48 */
    double v_screen_fade_size_min;  /* V_SCREEN_FADE_SIZE_MIN :49 */
    double v_screen_fade_weight;    /* V_SCREEN_FADE_WEIGHT :50 */
    int32_t fused_step;             /* not a reference constant: which kernels make a step.  0 = automatic: a context of <= 512 scenes
                                       whose scenes are all resident at once (two workgroups per CU up to 512 points per frame), runs
                                       TrackBuffer.track of a scene in ONE workgroup start to finish (k_scene: the step is one scene's
                                       latency there), others the bulk kernels; 1 = the one-workgroup step whenever the configuration
                                       allows it (not with seek_inner, resized rings, track_cap > 63 or the side-stream workers);
                                       -1 = never (tests run both) */
    int32_t reserved_;
} mmw_config;

/* One entry of TrackBuffer.effective_tracks (Tracking.py:139-230), flattened:
 * ClusterTrack.{state.x, state.P, cluster.*, spread_est, group_disp_est, N_est,
 * lifetime, batch (lengths), keypoints}.  P is stored 9x9 row-major (the
 * leading 6x6 block is used for CONST_VEL_MODEL). */
typedef struct mmw_track_record {
    double x[9];
    double P[81];
    double centroid[6];
    double min_vals[6];
    double max_vals[6];
    double spread_est[6];
    double group_disp_est[36];
    double n_est;
    double lifetime;
    int32_t point_num;
    int32_t is_static;              /* cluster.status: STATIC=True (Tracking.py:17,132-136) */
    int32_t ring_len;               /* len(track.batch.buffer) */
    int32_t ring_n[MMW_RING_MAX];   /* rows per frame, oldest first */
    int32_t uid;                    /* creation ordinal in its scene (TrackBuffer.next_track_id, Tracking.py:588) */
    float keypoints[MMW_NKP];
} mmw_track_record;

/* Fixed-size per-track summary exchanged between GPUs. */
typedef struct mmw_track_summary {
    int32_t scene;      /* global scene id (scene_base + local index) */
    int32_t slot;       /* position in effective_tracks */
    int32_t alive;      /* 1 if slot < n_tracks */
    int32_t is_static;
    int32_t point_num;
    float lifetime;
    float x[9];
    float centroid[6];
    float keypoints[MMW_NKP];
    /* the output step after the path, fused into the table kernel: Visualizer.calc_fade_square (Visualizer.py:14-29)
     * = Utils.calc_projection_points (Utils.py:180-219) of the head keypoint (x index 3, y index 41, z index 22)
     * relative to the track position onto the screen plane y = 0, and the side of the faded square (shrinks with
     * range, clamped to [V_SCREEN_FADE_SIZE_MIN, V_SCREEN_FADE_SIZE_MAX]).  fp64 arithmetic, rounded once. */
    float fade_x, fade_z, fade_size;
} mmw_track_summary;

typedef struct mmw_ctx mmw_ctx;

/* constants.py defaults. */
int mmw_config_default(mmw_config *cfg);

/* TrackBuffer() + BatchedData() for `n_scenes` scenes (Tracking.py:504-511, 38-41;
 * offline_main.py:32-34).  max_pts = largest point count of one frame (<= MMW_MAX_PTS_LIMIT).  apply_DBscan clusters
 * the unassigned part of the ring, up to (FB_FRAMES_BATCH + 1) * max_pts <= 4096 points: up to 1920 points its BallTree
 * lives in on-chip memory; a context whose ring can hold more additionally gets a slower global-memory path for those
 * clouds (one more launch per step, only in such contexts). */
int mmw_create(const mmw_config *cfg, int32_t n_scenes, int32_t max_pts, int32_t device, mmw_ctx **out);
int mmw_destroy(mmw_ctx *ctx);
const char *mmw_last_error(const mmw_ctx *ctx);
/* Fresh TrackBuffer/BatchedData for every scene. */
int mmw_reset(mmw_ctx *ctx);
/* ... for the scenes whose flag is non-zero only (host array of n_scenes words): how a batched caller recovers ONE scene --
 * e.g. after MMW_E_CAPACITY, which names the scene; the error bits are per scene and the other scenes' state stays valid. */
int mmw_reset_scenes(mmw_ctx *ctx, const int32_t *scene_flags);
/* The sticky error bits of every scene (host array of n_scenes words; 0 = none): 1 singular 6x6 matrix, 2 division by zero
 * in _get_Rc, 4 more tracks than track_cap (the tracks that did not fit were dropped: this scene differs from the reference
 * from then on), 8 a point count the context was not sized for, 16 / 32 apply_DBscan reached with a NaN / an infinite value
 * in its cloud (MMW_E_NONFINITE; 16 = sklearn's "contains NaN" message, which it prefers when both are present, 32 = "contains
 * infinity").  mmw_check reports the first one as its return code. */
int mmw_get_errors(mmw_ctx *ctx, int32_t *err_bits);
/* Clears the given error bits of the scenes whose flag is non-zero (host array of n_scenes words; NULL = every scene) and
 * nothing else: for errors that leave the scene's state valid -- a caller that catches the reference's ValueError
 * (MMW_E_NONFINITE) and carries on sees the same state the reference is in, and the error comes back on the next frame if
 * it still applies.  ONE flavour of MMW_E_NONFINITE does NOT leave the reference's state: with mmw_config.seek_inner, a
 * non-finite doppler / peakVal of an ASSIGNED point reaches the inner apply_DBscan (Tracking.py:440), whose ValueError leaves
 * the reference's track() in the middle of _associate_points_to_tracks -- no further track associated, no _maintain_tracks, no
 * _update_all, no add_frame --, while here only that track's inner clustering is skipped and the frame completes (db_n is then
 * NOT MMW_DB_RAISED: the frame's own call did not raise).  Like MMW_E_CAPACITY such a scene differs from the reference from
 * then on: reset it (mmw_reset_scenes), do not clear the bit and carry on. */
#define MMW_ERRBIT_SINGULAR 1
#define MMW_ERRBIT_DIVZERO 2
#define MMW_ERRBIT_CAPACITY 4
#define MMW_ERRBIT_BADCOUNT 8
#define MMW_ERRBIT_NONFINITE_NAN 16
#define MMW_ERRBIT_NONFINITE_INF 32
int mmw_clear_errors(mmw_ctx *ctx, const int32_t *scene_flags, int32_t bits);
/* BatchedData.pop_frame() (Tracking.py:66-71; its caller is preprocessing.py:264): drop the oldest frame of the global
 * ring of every scene whose flag is non-zero (host array of n_scenes words; NULL = every scene). */
int mmw_pop_frame(mmw_ctx *ctx, const int32_t *scene_flags);
/* BatchedData.change_buffer_size(new_size) (Tracking.py:60-64) on the global ring of the flagged scenes (host array of
 * n_scenes words; NULL = every scene): from the next add_frame on, frames are popped while len >= new_size.  Sizes
 * above FB_FRAMES_BATCH + 1 act like it (the reference's deque has that maxlen); new_size < 1 is MMW_E_ARG (the
 * reference's add_frame would never terminate).  mmw_reset restores the default. */
int mmw_set_batch_size(mmw_ctx *ctx, const int32_t *scene_flags, int32_t new_size);
/* BatchedData(init_data) (Tracking.py:38-41): the global ring of `scene` becomes ONE frame holding rows[n][8] (host,
 * n <= max_pts) instead of the empty frame a default BatchedData() starts with.  Sync. */
int mmw_set_batch_frame(mmw_ctx *ctx, int32_t scene, const double *rows, int32_t n);
/* ---- per-scene site parameters ----
 * A *site* is the installation a scene's radar stands in: the eleven values of mmw_config that describe the sensor mounting
 * (normalize_data: Utils.py:312-328, constants.py:41-42), the intensity scale of the feature maps (Utils.py:469,502; computed
 * per data set in preprocessing.py:291-295) and the window / monitoring point of the output step (Utils.py:180-219,
 * Visualizer.py:14-29, constants.py:31-33,48-50).  Field meaning = the mmw_config field of the same name; tilt_cos / tilt_sin
 * are taken as given, as in mmw_config (the bit-exact values are numpy's cos / sin(radians(S_TILT))).  A context starts
 * without a site table: every scene then uses the context's mmw_config and the kernels of a context that never heard of
 * sites.  While a table is in use, mmw_normalize / _f32 / _tlv, mmw_frame_host / mmw_frame_posture_host, mmw_features /
 * mmw_features_async and mmw_track_table read each scene's own site; the tracker itself (gating, Kalman, DBSCAN,
 * maintenance) keeps reading mmw_config, and so do mmw_format_frames and mmw_dbscan (utilities on caller data, not scenes).
 * A site belongs to the SLOT, not to the recording in it: mmw_reset / mmw_reset_scenes keep it, a snapshot blob does not
 * carry it, and mmw_restore leaves the destination slots' sites alone. */
typedef struct mmw_scene_site {          /* 96 bytes, all doubles */
    double s_height, tilt_cos, tilt_sin;
    double intensity_mu, intensity_std;
    double m_x, m_y, m_z;
    double v_screen_fade_size_max, v_screen_fade_size_min, v_screen_fade_weight;
    double reserved_;                    /* must be 0 */
} mmw_scene_site;
/* Give the listed scenes (host array of n indices; NULL = scenes 0 .. n-1) the sites[n] (host).  The first call allocates the
 * table and fills every scene with the config's own values; scenes never listed keep those.  Ordered on the context's
 * stream: calls issued before it use the old sites, calls after it the new.  Tracker state is not touched.  Atomic refusal
 * (MMW_E_ARG, mmw_last_error names the entry, no scene's site changes): an index out of range or listed twice, n < 0,
 * n > n_scenes, sites == NULL with n > 0, a non-zero reserved_.  The values themselves are not judged (mmw_create does not
 * judge these fields of mmw_config either).  Sync (the caller's arrays may go away). */
int mmw_set_sites(mmw_ctx *ctx, const int32_t *scenes, int32_t n, const mmw_scene_site *sites);
/* the effective site of every scene (host array of n_scenes): the config's values where none was set.  Read from the host mirror of the table: no device access. */
int mmw_get_sites(mmw_ctx *ctx, mmw_scene_site *out);
/* back to the context's config for every scene, and to the kernels of a context without sites */
int mmw_clear_sites(mmw_ctx *ctx);
/* 1 while a site table is in use, else 0 (MMW_E_ARG for a NULL context) */
int mmw_has_sites(mmw_ctx *ctx);
/* mmw_config.chain_side_stream at run time: on != 0 -> the small-cloud DBSCAN workers run on a second stream beside the
 * association kernel from the next mmw_step on, 0 -> in the post kernel only.  A caller that runs its own kernels beside
 * the tracker (the CNN of the previous frame on another stream) may prefer them off. */
int mmw_set_chain_side_stream(mmw_ctx *ctx, int32_t on);
/* Run on a caller-owned hipStream_t; NULL = the context's own (non-blocking) stream.
 * Note for callers that share device buffers with another runtime: calls on DEVICE pointers are ordered with that
 * runtime's work only if both use the same stream.  torch reports the legacy default stream as
 * torch.cuda.current_stream().cuda_stream == 0, which is NULL here, i.e. NOT torch's stream: pass MMW_STREAM_LEGACY
 * (HIP's hipStreamLegacy handle) for it, or -- better -- a torch.cuda.Stream() both sides use. */
#define MMW_STREAM_LEGACY ((void *)1)
int mmw_set_stream(mmw_ctx *ctx, void *hip_stream);
int mmw_synchronize(mmw_ctx *ctx);                                   /* sync */
/* Hand-over WITHOUT a host wait: whatever is queued on `hip_stream` after this call starts only when everything queued on the
 * context's stream so far has finished (an event recorded on the context's stream, hipStreamWaitEvent on the other).  For a
 * consumer on another stream of what the context wrote into device memory -- the RCCL all-gather of the track table on the
 * communicator's stream, a torch kernel reading mmw_features' rows.  hip_stream: a raw hipStream_t; NULL =
 * the legacy default stream (what torch reports as current_stream().cuda_stream == 0), MMW_STREAM_LEGACY the same. */
int mmw_stream_wait(mmw_ctx *ctx, void *hip_stream);
/* The other direction: whatever the context queues on ITS stream after this call starts only when everything queued on
 * `hip_stream` so far has finished.  For device buffers the context is about to REWRITE while a consumer on another stream may
 * still be reading them (the track table of the previous all-gather: write-after-read). */
int mmw_wait_stream(mmw_ctx *ctx, void *hip_stream);
int mmw_get_dims(const mmw_ctx *ctx, int32_t *n_scenes, int32_t *max_pts, int32_t *track_cap, int32_t *ring, int32_t *ring_rows);

/* Thin device-memory helpers so a ctypes host needs no HIP binding. */
int mmw_dev_alloc(mmw_ctx *ctx, size_t bytes, void **dptr);
int mmw_dev_free(mmw_ctx *ctx, void *dptr);
int mmw_memcpy_h2d(mmw_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);   /* stream-ordered, sync on return */
int mmw_memcpy_d2h(mmw_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);   /* sync */

/* Utils.normalize_data + point_transform_to_standard_axis (Utils.py:294-434):
 * raw[S][max_pts][5] = (x,y,z,doppler,peakVal) -> pts[S][max_pts][8], kept rows
 * compacted in input order; n_out[S].  All dev pointers. */
int mmw_normalize(mmw_ctx *ctx, const double *raw, const int32_t *n_raw, double *pts, int32_t *n_out);
/* The same from fp32 raw rows (20 bytes per detected object: what crosses PCIe in a host-fed loop, offline_main.py:40-57): each
 * value is promoted to fp64 as it is loaded -- exact; the IWR1443's objects are int16 counts scaled by a power of two
 * (ReadDataIWR1443.py:150-170) -- and the arithmetic is mmw_normalize's.  pts stays fp64 (normalize_data's own dtype). */
int mmw_normalize_f32(mmw_ctx *ctx, const float *raw, const int32_t *n_raw, double *pts, int32_t *n_out);

/* TrackBuffer.track(pointcloud, batch) for every scene (Tracking.py:664-703):
 *   pts[S][max_pts][8] fp64 (x,y,z,vx,vy,vz,doppler,peakVal), n_pts[S], dt[S] (= trackbuffer.dt).
 *   A scene with n_pts[s] == 0 is skipped entirely (offline_main.py:56 never calls track() on an empty frame);
 *   n_pts[s] == MMW_EMPTY_FRAME is track() called ON an empty point cloud: tracks are predicted, aged and expired,
 *   _update_all runs, an empty frame enters the ring (what the reference does when a caller does call it).
 *   dt[s] may be ANY FINITE double, per scene and per frame: zero (two frames with one timestamp) and negative (a clock that
 *   stepped back) included, as well as minutes and hours.  The predict runs with lifetime + dt (Tracking.py:372-385: F and Q
 *   are built from that sum, which may itself be zero or negative), an unassigned track's lifetime becomes lifetime + dt and
 *   the track expires when that is > its limit (Tracking.py:513-528); every layout does this arithmetic in the oracle's order,
 *   bit for bit (tests/test_gpu_dt.py).  What a NaN or infinite dt does is not pinned.
 * Outputs (dev, each may be NULL):
 *   assoc[S][max_pts]      _calc_dist_fun result: -1 = None, else index into the
 *                          track list as it was BEFORE _maintain_tracks (Tracking.py:530-574)
 *   db_labels[S][ring*max_pts], db_n[S]   sklearn labels of apply_DBscan on the global
 *                          ring (Utils.py:272-278); db_n = -1 when it was not called, MMW_DB_RAISED when
 *                          sklearn's input validation refused the cloud (MMW_E_NONFINITE). */
int mmw_step(mmw_ctx *ctx, const double *pts, const int32_t *n_pts, const double *dt,
             int32_t *assoc, int32_t *db_labels, int32_t *db_n);
/* mmw_step on fp32 rows: pts[S][max_pts][8] float (32 bytes per point, 16-byte aligned), promoted to fp64 in registers as
 * the association kernel loads them -- exact, so for rows that are fp32-representable (a CSV of the reference's logs, the
 * synthetic scenes of bench.py) every output is bit-equal to mmw_step's on the promoted rows.  Half the bytes per frame
 * over PCIe and out of HBM, and no conversion pass in front of the step. */
int mmw_step_f32(mmw_ctx *ctx, const float *pts, const int32_t *n_pts, const double *dt,
                 int32_t *assoc, int32_t *db_labels, int32_t *db_n);
/* mmw_step with host pointers (H2D, step, D2H; sync): mmw_frame_host without the normalisation. */
int mmw_step_host(mmw_ctx *ctx, const double *pts, const int32_t *n_pts, const double *dt,
                  int32_t *assoc, int32_t *db_labels, int32_t *db_n);
/* One frame of every scene from HOST memory in ONE round trip -- the body of the reference's loop (offline_main.py:40-57):
 *   raw != NULL (pts NULL): raw[S][max_pts][5] = (x, y, z, doppler, peakVal), n[S] rows each -> Utils.normalize_data -> the kept
 *                           rows -> TrackBuffer.track; a scene none of whose rows pass the scene filter is skipped
 *                           (offline_main.py:56), as is a scene with n = 0
 *   pts != NULL (raw NULL): pts[S][max_pts][8] normalised rows, n[S] as for mmw_step (0 = skipped, MMW_EMPTY_FRAME = track() on an
 *                           empty cloud)
 * dt[S] = trackbuffer.dt.  Outputs (host, each may be NULL): pts_out[S][max_pts][8] / n_out[S] = normalize_data's rows and
 * their counts (raw form; n_out = n otherwise), assoc[S][max_pts], db_labels[S][ring*max_pts], db_n[S] as mmw_step,
 * n_tracks[S] = len(effective_tracks) after the frame.  Uploads, kernels and read-backs are queued behind one another through
 * pinned staging blocks and the stream is waited for ONCE; the return code is mmw_check's (per-scene errors, first one). */
int mmw_frame_host(mmw_ctx *ctx, const double *raw, const double *pts, const int32_t *n, const double *dt, double *pts_out,
                   int32_t *n_out, int32_t *assoc, int32_t *db_labels, int32_t *db_n, int32_t *n_tracks);

/* The loop body WITH its posture estimate (offline_main.py:53-60: normalize_data, track, estimate_posture) in one round trip,
 * for the one-scene context of the drop-in's TrackBuffer.  mmw_attach_posture hands the context the define_CNN_3D model
 * (train.py:71-106, BatchNormalization folded into the Dense layers; fp32 DEVICE pointers that stay valid and unchanged in place
 * until detached with NULL): the conv kernels in Keras layout (kd,kh,kw,in,out), dense1_w[1536][dense1_ld] = Dense-1 transposed
 * (K = 6144 contiguous, Keras' Flatten order), dense2_w[57][1536].  Needs n_scenes == 1, FB_FRAMES_BATCH == 2 (the 3-frame
 * model), track_cap <= 64.
 * mmw_frame_posture_host = mmw_frame_host, and behind the step on the same stream -- unless the frame was skipped --
 * TrackBuffer.estimate_posture (Tracking.py:705-734): the feature tensors of the tracks with more than MODEL_MIN_INPUT ring
 * points, the CNN in Keras' own fp32 arithmetic (mmw_mars_conv3d's kernel, mmw_mars_head_small's kernels, with a row count
 * only the device knows) and track.keypoints = its rows.  *posture_rows (host, may be NULL) = the tracks estimated.  Still ONE
 * wait for the stream.
 * mmw_attach_posture_frames is the same entry for either model: frames = 3 IS mmw_attach_posture; frames = 1 takes the
 * single-frame model define_CNN (train.py:33-68) in the same struct -- conv kernels (kh,kw,in,out) = 720 and 4608 floats,
 * dense1_w[512][dense1_ld] with dense1_ld >= 2048, dense2_w[57][512] -- on a one-scene context with FB_FRAMES_BATCH == 0 and
 * track_cap <= 64; mmw_frame_posture_host then runs mmw_mars_conv2d's kernel in place of mmw_mars_conv3d's.  frames must be 3 or 1
 * and the context's FB_FRAMES_BATCH + 1: anything else is MMW_E_ARG with a message and nothing changed. */
typedef struct mmw_posture_model {
    const float *conv1_w, *conv1_b, *conv2_w, *conv2_b;
    const float *dense1_w;
    int64_t dense1_ld;
    const float *dense1_b, *dense2_w, *dense2_b;
} mmw_posture_model;
int mmw_attach_posture(mmw_ctx *ctx, const mmw_posture_model *model);
int mmw_attach_posture_frames(mmw_ctx *ctx, const mmw_posture_model *model, int32_t frames);
int mmw_frame_posture_host(mmw_ctx *ctx, const double *raw, const double *pts, const int32_t *n, const double *dt, double *pts_out,
                           int32_t *n_out, int32_t *assoc, int32_t *db_labels, int32_t *db_n, int32_t *n_tracks, int32_t *posture_rows);

/* The BATCHED TrackBuffer.estimate_posture (Tracking.py:705-734; the second half of the loop body, offline_main.py:57-60) for a
 * context of ANY number of scenes, with no torch tensor on the path: what posture.PosturePipeline(overlap=False) + mars.MarsCNN
 * string together in Python, as three C entries.
 * mmw_posture_attach hands the context the define_CNN_3D model (train.py:71-106) -- the SAME struct mmw_posture_model as
 * mmw_attach_posture: fp32 DEVICE pointers in Keras layout, BatchNormalization folded into the Dense layers, valid and unchanged in
 * place until detached -- and lets it allocate the chain's buffers for cap_rows rows (rounded up to 256): feature tensors, owners,
 * uids, the split activation (2 * 6144 + 256 fp16 per row), hidden, keypoints, the fix-up list and MMW_RANGE_FIXUP_SCRATCH; the
 * split-fp16 Dense-1 operand (1536 x 12288 fp16) is built once on the device (mmw_mars_split_weights).  Refused with MMW_E_ARG, a
 * message and nothing changed (an earlier model stays attached): FB_FRAMES_BATCH != 2 (the single-frame model define_CNN is not
 * served here: mmw_posture_attach_frames), cap_rows < 1, a null pointer, Dense-1 / Dense-2 not 16-byte aligned, dense1_ld < 6144 or not a multiple of 4, and a
 * conv or Dense-1 weight (conv biases included) that is not finite or of magnitude >= 65 504 -- the split arithmetic is exact inside
 * fp16's range only, and there is no silent fp32 fallback.  model == NULL detaches and frees.  Independent of mmw_attach_posture: a
 * one-scene context may hold both.  Sync.
 * mmw_estimate_posture runs, on the context's stream behind whatever was queued last (normally the frame's mmw_step): the feature
 * tensors of every track with more than MODEL_MIN_INPUT ring points (Tracking.py:718-730; each scene's own site while a site table is
 * in use) -> the host waits for the ROW COUNT only (a copy into pinned memory, not the stream: the matrix kernels need their exact
 * batch size) -> mmw_mars_conv_split's kernel -> mmw_mars_dense1_split's kernel -> mmw_mars_dense2's kernel (model.predict,
 * Tracking.py:732) -> mmw_mars_range_fixup's kernels -> track.keypoints = rows (Tracking.py:733-734, mmw_set_keypoints).  The serial
 * schedule on one stream.  *n_rows (host, may be NULL) = the tracks estimated.  No eligible track: nothing is launched behind the
 * features, returns 0.  More eligible tracks than cap_rows: MMW_E_CAPACITY, no keypoint changed.  No model attached: MMW_E_ARG.
 * Returns WITHOUT waiting for the stream: the keypoints are in place for whatever the caller queues on the context next
 * (mmw_get_tracks, mmw_track_table, the next mmw_step), as with the other asynchronous entries.
 * mmw_posture_range reads and clears this path's sticky range word -- MarsCNN.range_overflow() --: bit 0 = a sample's input or
 * activation left fp16's range and its keypoints were recomputed in fp32 (valid), bit 1 = more than MMW_RANGE_FIXUP_CAP such
 * samples in one call, the surplus keeps meaningless keypoints.  Sync.
 * mmw_posture_attach_frames is mmw_posture_attach for either model: frames = 3 IS mmw_posture_attach (same buffers, same launches,
 * same bits); frames = 1 takes the single-frame model define_CNN (train.py:33-68) on a context with FB_FRAMES_BATCH == 0, in the same
 * struct: conv kernels (kh,kw,in,out) = 720 and 4608 floats, dense1_w[512][dense1_ld] with dense1_ld >= 2048, dense2_w[57][512].  The
 * chain's buffers are sized by the model (320 floats per feature row, split activation 2 * 2048 + 256 fp16 per row, hidden 512, the
 * split Dense-1 operand 512 x 4096 fp16; MMW_RANGE_FIXUP_SCRATCH as it is), the conv weights range-checked over their 2-D sizes.
 * frames must be 3 or 1 and the context's FB_FRAMES_BATCH + 1: anything else is MMW_E_ARG with a message and nothing changed.
 * mmw_estimate_posture and mmw_posture_range run whichever model is attached: for frames = 1 mmw_mars_conv_split(frames = 1) ->
 * mmw_mars_dense1_split (k = 2048, n = 512) -> mmw_mars_dense2 (k = 512) -> mmw_mars_range_fixup_frames(frames = 1) ->
 * track.keypoints; row count, capacity, detach, sites and the range word as for the 3-frame model. */
int mmw_posture_attach(mmw_ctx *ctx, const mmw_posture_model *model, int32_t cap_rows);
int mmw_posture_attach_frames(mmw_ctx *ctx, const mmw_posture_model *model, int32_t frames, int32_t cap_rows);
int mmw_estimate_posture(mmw_ctx *ctx, int32_t *n_rows);
int mmw_posture_range(mmw_ctx *ctx, int32_t *word);
/* ---- per-scene posture models ----
 * SEVERAL models behind one mmw_estimate_posture: every scene names the model that estimates it -- the model trained on the data
 * set its site's intensity scale was computed for (mmw_set_sites), a new model on a few scenes before it gets all of them -- or
 * MMW_POSTURE_NONE: no model, its tracks keep the keypoints they have (default_posture for a track that never had any) and cost
 * no CNN row.  The models are of ONE frame count, the context's.
 * mmw_posture_attach_models: models[n_models] (1 .. MMW_POSTURE_MODELS_MAX; each as mmw_posture_attach_frames takes it and held to
 * the same rules), frames as mmw_posture_attach_frames, scene_model host [n_scenes] with entries in [-1, n_models) (NULL: every
 * scene on model 0).  Every model gets its own split Dense-1 operand (37.7 MB for the 3-frame model, 4.2 MB for the single-frame
 * one) and fix-up list; feature, activation, hidden, keypoint, owner and uid buffers are shared and hold
 * pad256(cap_rows) + 256 * n_models rows (n_models > 1), so that every model's rows start on a multiple of 256 and cap_rows keeps
 * its meaning: the most rows one call estimates, summed over the models.  Replaces whatever was attached, single or multiple.
 * Refused with MMW_E_ARG, a message that names the index of an offending model, and nothing changed (an earlier attachment stays
 * and keeps working): n_models outside 1 .. 8, a map entry outside [-1, n_models), frames, cap_rows < 1, a model
 * mmw_posture_attach_frames would refuse; MMW_E_HIP, equally atomic, for a failed allocation.  models == NULL is MMW_E_ARG:
 * mmw_posture_attach(ctx, NULL, 0) / mmw_posture_attach_frames(ctx, NULL, ..) detach either kind.  mmw_posture_attach and
 * mmw_posture_attach_frames ARE the one-model case (the map: every scene on model 0).  Sync.
 * mmw_posture_set_scene_models: the listed scenes (host array of n indices; NULL = scenes 0 .. n-1) move to model_of[n] (host).
 * The rules of mmw_set_sites: checked on the host before anything changes (an index out of range or listed twice, n < 0,
 * n > n_scenes, model_of == NULL with n > 0, an id outside [-1, n_models): MMW_E_ARG, the message names the entry, the map stays),
 * the new map travels as one copy ordered on the context's stream and holds from the next mmw_estimate_posture on.  Tracker state
 * is not touched: a track keeps the keypoints it last got (track.keypoints persists between estimates in the reference too).  The
 * map belongs to the attachment: mmw_reset / mmw_reset_scenes keep it, a snapshot blob carries neither map nor models, attaching
 * anew starts a new map.  Needs an attachment (MMW_E_ARG without one).  Sync.
 * mmw_posture_get_scene_models: the map, host [n_scenes], from its host mirror.
 * mmw_estimate_posture on such a context: the eligible tracks' rows are handed out model by model (one more one-workgroup kernel in
 * place of the scan), the host waits for every model's row count in one copy, and the chain of the CNN kernels runs once per model
 * that has rows, on that model's rows alone.  *n_rows = the rows of all models; more than cap_rows: MMW_E_CAPACITY before any CNN
 * launch, no keypoint changed; no rows anywhere: MMW_OK with 0.  mmw_posture_range is the OR over the models.  A context with ONE
 * model and every scene on it launches exactly what mmw_posture_attach's always did; with one model and scenes on
 * MMW_POSTURE_NONE it runs the model-by-model scan and one chain.
 * mmw_posture_group_rows / mmw_posture_owners report the LAST mmw_estimate_posture (a refused or empty call: no rows):
 * rows[n_models] (host) = the rows each model estimated, *n_models = their number; owner[n][2] (host, cap rows) = (scene, track
 * list position) of every estimated row, model by model and within a model by ascending scene, *n_rows = n; more rows than cap:
 * MMW_E_CAPACITY, nothing written.  mmw_posture_owners is sync.  A NULL context is MMW_E_ARG and leaves the outputs alone. */
#define MMW_POSTURE_MODELS_MAX 8
#define MMW_POSTURE_NONE      (-1)     /* a scene no model estimates */
int mmw_posture_attach_models(mmw_ctx *ctx, const mmw_posture_model *models, int32_t n_models, int32_t frames,
                              const int32_t *scene_model /* host [S]; NULL = every scene model 0 */, int32_t cap_rows);
int mmw_posture_set_scene_models(mmw_ctx *ctx, const int32_t *scenes, int32_t n, const int32_t *model_of /* host [n] */);
int mmw_posture_get_scene_models(mmw_ctx *ctx, int32_t *out /* host [S] */);
int mmw_posture_group_rows(mmw_ctx *ctx, int32_t *rows /* host [n_models] */, int32_t *n_models);
int mmw_posture_owners(mmw_ctx *ctx, int32_t *owner /* host [cap][2] */, int32_t cap, int32_t *n_rows);

/* Utils.apply_DBscan (Utils.py:250-291) on arbitrary clouds: pts[S][max_n][8], n[S]
 * -> labels[S][max_n], n_clusters[S] (dev pointers; max_n <= ring*max_pts; max_n > 1920: the global-memory path).
 * A cloud that holds a NaN or an infinite value in any of its 8 columns is refused as sklearn's input validation refuses it
 * (ValueError): its labels are not written and n_clusters[s] = -MMW_ERRBIT_NONFINITE_NAN (-16) or -MMW_ERRBIT_NONFINITE_INF (-32). */
int mmw_dbscan(mmw_ctx *ctx, const double *pts, const int32_t *n, int32_t max_n, double eps,
               int32_t min_samples, int32_t *labels, int32_t *n_clusters);

/* Feature side of TrackBuffer.estimate_posture (Tracking.py:718-730) =
 * relative_coordinates + format_single_frame (Utils.py:437-520) for every track of
 * every scene with len(batch.effective_data) > MODEL_MIN_INPUT, compacted in
 * (scene, track) order:
 *   feat[cap_rows][ring][8][8][5] fp32 (dev; [cap_rows][8][8][5] when FB_FRAMES_BATCH == 0)
 *   owner[cap_rows][2] int32 (dev) = (scene, track index)
 *   *n_rows (host) = rows written (sync).  MMW_E_CAPACITY if cap_rows is too small. */
int mmw_features(mmw_ctx *ctx, float *feat, int32_t *owner, int32_t cap_rows, int32_t *n_rows);
/* The same without the host wait, for a caller that pipelines frames (the CNN of frame f on one stream while the
 * tracker of frame f+1 runs on the context's): the rows are written behind the preceding mmw_step on the context's
 * stream, the eligible-track total follows them into pinned host memory, and mmw_features_wait(ticket) waits for THAT
 * copy only (not for the stream).  ticket in [0,4): up to four calls may be outstanding (ticket 3 is the one
 * mmw_features itself uses).  uid[cap_rows] (dev, may be NULL) receives each row's track creation ordinal
 * (mmw_track_record.uid) for mmw_set_keypoints_uid. */
int mmw_features_async(mmw_ctx *ctx, float *feat, int32_t *owner, int32_t *uid, int32_t cap_rows, int32_t ticket);
int mmw_features_wait(mmw_ctx *ctx, int32_t ticket, int32_t *n_rows);   /* waits for that ticket's total only */
/* Utils.relative_coordinates + Utils.format_single_frame (Utils.py:437-520) on caller
 * frames: frames[B][ring][64][8] fp64 (only rows [:64] matter, Utils.py:505-510),
 * counts[B][ring] valid rows (<= 0 rows: frame stays zero, Utils.py:493), ref[B][2] = (x, y)
 * subtracted from columns 0,1 -> feat[B][ring][8][8][5] fp32.  All dev pointers.
 * The 64 rows of a frame (pad rows of zeros included) are ordered by the fp64 relative x as
 * np.argsort(kind="stable") orders them: rows of equal x (-0.0 == 0.0) keep their row order, rows whose x is NaN come
 * behind all others, +inf included, in row order.  Every input row is written exactly once. */
int mmw_format_frames(mmw_ctx *ctx, const double *frames, const int32_t *counts, const double *ref, float *feat, int32_t n_items);
/* track.keypoints = frame_keypoints[i] (Tracking.py:733-734): kp[n_rows][57] fp32 dev. */
int mmw_set_keypoints(mmw_ctx *ctx, const float *kp, const int32_t *owner, int32_t n_rows);

/* The same assignment when later frames have been tracked since mmw_features_async took the rows (list positions are
 * stale then): row i goes to the track of scene owner[i][0] whose creation ordinal is uid[i]; rows of tracks that
 * have expired meanwhile are dropped, as `track.keypoints = ...` on an object no list refers to any more would be.
 * It cannot tell a uid that restarted -- mmw_reset, mmw_reset_scenes and mmw_restore start a scene's ordinals over -- from the
 * old one: rows taken before such a call go through mmw_set_keypoints_ticket. */
int mmw_set_keypoints_uid(mmw_ctx *ctx, const float *kp, const int32_t *owner, const int32_t *uid, int32_t n_rows);
/* The same for the rows mmw_features_async(ticket) wrote, with one addition: a row whose scene mmw_reset, mmw_reset_scenes or
 * mmw_restore has touched since that call is dropped -- no list refers to any track of before, whatever uid the new ones carry.
 * Every scene has a generation word that those three bump; mmw_features_async records it per ticket when uid is not NULL, and
 * the scatter compares the two.  All on the context's stream, no host wait.  MMW_E_ARG, and nothing is written: ticket outside
 * [0,4), or a ticket whose last mmw_features_async passed uid == NULL (mmw_features does), or one that was never used. */
int mmw_set_keypoints_ticket(mmw_ctx *ctx, const float *kp, const int32_t *owner, const int32_t *uid, int32_t n_rows, int32_t ticket);

/* Read-back (sync; host pointers).  Also surfaces per-scene errors recorded by
 * the kernels (returns the first one and sets the message). */
int mmw_check(mmw_ctx *ctx);
int mmw_get_num_tracks(mmw_ctx *ctx, int32_t *n_tracks /*[S]*/);
int mmw_get_tracks(mmw_ctx *ctx, mmw_track_record *out /*[S][cap]*/, int32_t cap);
int mmw_get_batch_ring(mmw_ctx *ctx, int32_t *ring_len /*[S]*/, int32_t *ring_n /*[S][MMW_RING_MAX]*/);
/* rows of frame k (oldest first) of track t of scene s: out[ring_rows][8]; *n_rows = stored rows */
int mmw_get_track_ring_frame(mmw_ctx *ctx, int32_t scene, int32_t track, int32_t k, double *out, int32_t *n_rows);
int mmw_get_batch_ring_frame(mmw_ctx *ctx, int32_t scene, int32_t k, double *out /*[max_pts][8]*/, int32_t *n_rows);

/* ClusterTrack.seek_inner_clusters (Tracking.py:409-448) runs inside mmw_step when mmw_config.seek_inner = 1, i.e. as if
 * its call site Tracking.py:656 were active: per-track ring sizes follow change_buffer_size (Tracking.py:60-64), the
 * cluster's cloud is added to the track's ring a second time, apply_DBscan(eps = DB_INNER_EPS) runs on the ring and a
 * track is appended for clusters[1] before _update_all.  Such a context stores ring frames whole (ring_rows is raised
 * to ring * max_pts); a cloud of more than min(1920, ring * ring_rows) rows, or a frame longer than ring_rows, is
 * MMW_E_CAPACITY.  This read-back (sync) returns the calls of the LAST mmw_step: n_calls[S]; rows[S][16] = points
 * clustered by each of the first 16 calls, in track-list order; labels[S][cap_labels] = their sklearn labels back to
 * back (as many as fit).  rows / labels may be NULL. */
int mmw_get_inner(mmw_ctx *ctx, int32_t *n_calls, int32_t *rows, int32_t *labels, int32_t cap_labels);

/* Per-scene track table for the multi-GPU all-gather:
 * table[S][slots] (dev), scene ids offset by scene_base.  Async. */
int mmw_track_table(mmw_ctx *ctx, mmw_track_summary *table, int32_t slots, int32_t scene_base);

/* ---- live-track report ----
 * Who is in the scenes, without reading everything back: one compact row per LIVE track -- no dead slots, 324 bytes against the
 * table's 336 per slot -- with the track's creation ordinal, and the tracks that appeared or left since the previous report as
 * events.  Rows are compacted in (scene, slot) order: scenes ascending, inside a scene effective_tracks order.  Every field a row
 * shares with mmw_track_summary equals the mmw_track_table row of that (scene, slot) from the same state bit for bit -- one
 * device function fills both, the fade square and each scene's own site (mmw_set_sites) included; uid = mmw_track_record.uid, the
 * handle mmw_set_keypoints_uid matches by: a slot moves whenever _maintain_tracks drops an earlier track, the uid never does.
 *
 * mmw_report_enable(ctx, 1) allocates the per-scene BASELINE -- the uid list [n_scenes][track_cap] of the previous report, its
 * length, a generation word -- and fills it, ordered on the context's stream, with the tracks live at that moment: those produce
 * no event (enabling again takes the baseline anew).  on = 0 waits for the stream and frees it.  A context that never enables
 * reports launches exactly what it did before reports existed.
 *
 * Events: each report compares the live uid list of every scene with its baseline -- neither list is assumed sorted -- and the
 * baseline then becomes the current list.  Events are ordered by scene; inside a scene MMW_EV_GONE first, in baseline order, then
 * MMW_EV_BORN in current order.  The report is a DIFFERENCE OF STATES, not a log: a track that was born and expired between two
 * reports appears in neither.  mmw_reset, mmw_reset_scenes and mmw_restore bump the generation of the scenes they touch (a
 * kernel of their own, launched only while reports are enabled): uids restart there, so the next report emits exactly ONE
 * MMW_EV_REBASED for such a scene and no BORN / GONE -- a uid of before never aliases one of after -- and takes the scene's
 * current tracks as its baseline; their rows are reported as always.  Row flag bit 1 is set on exactly the rows whose uid has a
 * MMW_EV_BORN in the same report.
 *
 * Capacity is decided on the DEVICE: if the live rows exceed cap_rows or the events exceed cap_events, nothing is written into
 * either buffer, the baseline and the generations stay as they were, and mmw_report_wait returns MMW_E_CAPACITY with the counts
 * needed in *n_rows / *n_events: a retry with larger buffers loses nothing.
 * mmw_report_async queues the kernels behind whatever was queued last (normally the frame's mmw_step); the two counts follow them
 * into pinned host memory, and mmw_report_wait(ticket) waits for THAT copy only, not for the stream.  ticket in [0,4): up to four
 * reports may be outstanding (ticket 3 is the one mmw_report itself uses).  rows / events: dev pointers, 4-byte aligned, scene ids
 * offset by scene_base.  MMW_E_ARG: reports not enabled, a NULL buffer with a positive cap, a negative cap, a bad ticket, a wait
 * for a ticket with no report outstanding. */
typedef struct mmw_track_report {   /* one LIVE track; 324 bytes */
    int32_t scene;      /* global scene id (scene_base + local index) */
    int32_t slot;       /* position in effective_tracks */
    int32_t uid;        /* creation ordinal in its scene (mmw_track_record.uid) */
    int32_t flags;      /* bit 0 is_static, bit 1 born since the previous report */
    int32_t point_num;
    float lifetime;
    float x[9];
    float centroid[6];
    float fade_x, fade_z, fade_size;   /* as mmw_track_summary's */
    float keypoints[MMW_NKP];
} mmw_track_report;
#define MMW_REPORT_STATIC 1
#define MMW_REPORT_BORN 2
typedef struct mmw_track_event { int32_t scene, uid, kind, slot; } mmw_track_event;
#define MMW_EV_BORN 1     /* uid is live now and was not at the previous report; slot = its position now */
#define MMW_EV_GONE 2     /* uid was live at the previous report and is not now; slot = its position then */
#define MMW_EV_REBASED 3  /* the scene was reset or restored since the previous report; uid = -1, slot = n_tracks now */
int mmw_report_enable(mmw_ctx *ctx, int32_t on);
int mmw_report_async(mmw_ctx *ctx, mmw_track_report *rows, int32_t cap_rows, mmw_track_event *events, int32_t cap_events,
                     int32_t scene_base, int32_t ticket);
int mmw_report_wait(mmw_ctx *ctx, int32_t ticket, int32_t *n_rows, int32_t *n_events);   /* waits for that ticket's counts only; either may be NULL */
int mmw_report(mmw_ctx *ctx, mmw_track_report *rows, int32_t cap_rows, mmw_track_event *events, int32_t cap_events,
               int32_t scene_base, int32_t *n_rows, int32_t *n_events);                   /* async + wait */

/* ---- live-track point clouds ----
 * Where the live tracks' points are: every track's `track.batch.effective_data` (Tracking.py:43-58 -- np.concatenate of the ring's
 * frames, what Visualizer.update_bb scatters, Visualizer.py:232-260), compacted on the device in ONE call and in the report's order,
 * so that directory entry i belongs to mmw_report row i of the same state.
 *
 * Output: a DIRECTORY of one mmw_cloud_track per entry and the points / rows of all entries, back to back.  Scenes ascend; inside a
 * scene the entries follow effective_tracks order; with MMW_CLOUD_UNASSIGNED one more entry (slot -1, uid -1) follows each scene's
 * tracks: its global ring, the unassigned points apply_DBscan clusters.  Inside an entry frames run oldest first and rows keep their
 * stored order.  The entries partition the output: first of entry i + 1 = first + count of entry i, the last one ends at *n_points.
 * mode (bits 0): MMW_CLOUD_POINTS writes mmw_cloud_point (columns 0..2 rounded once to fp32 and the index of the point's directory
 * entry), MMW_CLOUD_ROWS writes the ring rows verbatim (double[8] each: effective_data bit for bit).  Non-finite values pass through.
 *
 * `dropped`: a track frame stores min(ring_n[k], ring_rows) rows (mmw_get_dims); what the reference's effective_data holds beyond that
 * is counted here, the one declared difference.  Contexts with ring_rows = max_pts, or with seek_inner, store whole frames: 0.
 *
 * Capacity is decided on the DEVICE, as the report's: more entries than cap_tracks or more points than cap_points (totals formed in
 * 64 bits; one above INT32_MAX never fits and is reported saturated) -> nothing is written to either buffer and mmw_clouds_wait
 * returns MMW_E_CAPACITY with both counts needed.  mmw_clouds_async queues its kernels on the context's stream behind whatever was
 * queued last; the counts follow into pinned memory and mmw_clouds_wait(ticket) waits for THAT copy only.  ticket in [0,4), ticket 3
 * is mmw_clouds' own.  No enable call: the first call allocates the context's scratch, mmw_destroy frees it; a context that never
 * calls launches what it did before.  dir: dev pointer, 4-byte aligned; out: dev pointer, 16-byte aligned; scene ids are offset by
 * scene_base.  MMW_E_ARG, nothing touched: a NULL context, a NULL buffer with a positive cap, a negative cap, a mode outside
 * {0, 1, 2, 3}, a bad ticket, a misaligned buffer, a wait for a ticket with nothing outstanding. */
typedef struct mmw_cloud_track {     /* 32 bytes: one directory entry */
    int32_t scene;    /* global scene id (scene_base + local index) */
    int32_t slot;     /* position in effective_tracks; -1 = the scene's global ring (unassigned points) */
    int32_t uid;      /* mmw_track_record.uid; -1 for the global ring */
    int32_t first;    /* index of this entry's first point / row in the output */
    int32_t count;    /* points written: sum over the ring's frames of the rows it STORES */
    int32_t frames;   /* len(track.batch.buffer)  (g_len for the global ring) */
    int32_t newest;   /* rows of the newest frame among `count` (the last `newest` of the run) */
    int32_t dropped;  /* rows effective_data has in the reference that this context does not store:
                         sum of max(0, ring_n[k] - ring_rows); always 0 for the global ring */
} mmw_cloud_track;
typedef struct mmw_cloud_point { float x, y, z; int32_t track; } mmw_cloud_point;   /* 16 bytes; track = index of its directory entry */
#define MMW_CLOUD_POINTS 0      /* out = mmw_cloud_point[]: columns 0..2 rounded once to fp32 */
#define MMW_CLOUD_ROWS 1        /* out = double[][8]: the ring rows verbatim = effective_data bit for bit */
#define MMW_CLOUD_UNASSIGNED 2  /* flag bit: after a scene's tracks, one entry (slot -1) for its global ring */
int mmw_clouds_async(mmw_ctx *ctx, mmw_cloud_track *dir, int32_t cap_tracks, void *out, int32_t cap_points, int32_t mode,
                     int32_t scene_base, int32_t ticket);
int mmw_clouds_wait(mmw_ctx *ctx, int32_t ticket, int32_t *n_tracks, int32_t *n_points);   /* waits for that ticket's counts only; either may be NULL */
int mmw_clouds(mmw_ctx *ctx, mmw_cloud_track *dir, int32_t cap_tracks, void *out, int32_t cap_points, int32_t mode,
               int32_t scene_base, int32_t *n_tracks, int32_t *n_points);                   /* async + wait */

/* ---- live-track skeletons ----
 * How the live tracks stand: every track's 57 keypoints turned from their track-relative, mirrored form into the room-frame skeleton
 * that Visualizer.update_posture draws (Visualizer.py:265-307), with its plausibility check, compacted on the device in ONE call and
 * in the report's order: in MMW_SKEL_ALL entry i belongs to mmw_report row i and mmw_clouds directory entry i (without
 * MMW_CLOUD_UNASSIGNED) of the same state; `row` carries that index into MMW_SKEL_DRAWN, which leaves out the entries the check drops.
 *
 * The keypoints are 57 fp32 values kp[]; the reference views them as reshape(3, 19): row 0 = kp[0..18], row 1 = kp[19..37] (plotted
 * as height), row 2 = kp[38..56] (plotted as depth).  x is the track's fp64 state (mmw_track_record.x[0], x[1]; the same for dim_x 6
 * and 9).
 *   check   g_c = fp32(kp[19c + 1] - kp[19c + 2]) for c = 0, 1, 2 (SpineMid - Neck: one fp32 subtraction each, as numpy's on a float32
 *           array); s = g_0^2 + g_1^2 + g_2^2 in fp64, in that order (the products of fp32 values are exact there);
 *           MMW_SKEL_SKIPPED iff s > 0.25; gap = fp32(sqrt(s)).  A NaN makes the comparison false: the track is drawn, as
 *           `nan > 0.5` is false in the reference.
 *   joints  joint[j][0] = fp32(-(double)kp[j] + x[0]);  joint[j][1] = fp32((double)kp[38 + j] + x[1]);  joint[j][2] = kp[19 + j]
 *           ONE rounding each, from fp64: track.state.x[0] is a shape-(1,) fp64 array (state.x is (dim_x, 1), Tracking.py:96), so the
 *           reference's in-place `+=` on the float32 view is computed in fp64 and cast back.  Non-finite values pass through.
 * Skipped entries carry their joints all the same in MMW_SKEL_ALL.  The call is a pure function of the state and never writes it
 * (the reference's reshape is a view: it transforms track.keypoints in place each time it draws; DESIGN.md 8e lists the differences).
 * Call order: main.py:56 displays BEFORE estimate_posture (line 60) -- last frame's keypoints around this frame's position: call
 * between mmw_step and mmw_estimate_posture for that, behind mmw_estimate_posture for this frame's keypoints.
 *
 * Capacity is decided on the DEVICE, as the clouds': more entries than cap -> nothing is written and mmw_skeletons_wait returns
 * MMW_E_CAPACITY with both counts: *n_out the entries the mode needs, *n_live the live tracks (= *n_out in MMW_SKEL_ALL).
 * mmw_skeletons_async queues its kernels on the context's stream behind whatever was queued last; the counts and the fit decision
 * follow into pinned memory and mmw_skeletons_wait(ticket) waits for THAT copy only.  ticket in [0,4), ticket 3 is mmw_skeletons' own.
 * No enable call: the first call allocates the context's scratch, mmw_destroy frees it; a context that never calls launches what it
 * did before.  out: dev pointer, 16-byte aligned; scene ids are offset by scene_base.  MMW_E_ARG, nothing touched: a NULL context,
 * a negative cap, a NULL out with a positive cap, a misaligned out, a mode outside {0, 1}, a bad ticket, a wait for a ticket with
 * nothing outstanding. */
typedef struct mmw_skeleton {          /* 256 bytes, no padding */
    int32_t scene;      /* global scene id (scene_base + local index) */
    int32_t slot;       /* position in effective_tracks */
    int32_t uid;        /* mmw_track_record.uid */
    int32_t row;        /* rank of this track among ALL live tracks in (scene, slot) order: the index of its mmw_report row */
    int32_t flags;      /* bit 0 MMW_SKEL_SKIPPED: the reference's check drops this skeleton (Visualizer.py:276-278) */
    float   gap;        /* |SpineMid - Neck| as defined above */
    float   joint[19][3]; /* (x, y = depth, z = height) in the room frame: what the reference hands to plot / scatter */
    int32_t reserved_;  /* 0 */
} mmw_skeleton;
#define MMW_SKEL_SKIPPED 1
#define MMW_SKEL_ALL 0          /* mode: one entry per live track, entry i <-> report row i */
#define MMW_SKEL_DRAWN 1        /* mode: only the entries the reference draws (flag bit 0 clear), compacted, order kept */
int mmw_skeletons_async(mmw_ctx *ctx, mmw_skeleton *out, int32_t cap, int32_t mode, int32_t scene_base, int32_t ticket);
int mmw_skeletons_wait(mmw_ctx *ctx, int32_t ticket, int32_t *n_out, int32_t *n_live);   /* waits for that ticket's counts only; either may be NULL */
int mmw_skeletons(mmw_ctx *ctx, mmw_skeleton *out, int32_t cap, int32_t mode, int32_t scene_base, int32_t *n_out, int32_t *n_live);   /* async + wait */
/* host only, no context, no GPU: the 18 bones as joint index pairs ([18][2], Visualizer.py:100-119 order) and a class per joint
 * ([19]: 0 blue, 1 green, 2 red = the head, which the reference draws larger and square; Visualizer.py:122-142, 295-307).  The
 * tables are static; either pointer may be NULL. */
int mmw_skeleton_tables(const int32_t **connections, const int32_t **joint_class);

/* ---- zones ----
 * Which part of the room is occupied, by whom, and who walked in or out since the last look: per scene up to MMW_ZONES_MAX
 * axis-aligned rectangles in the scene's normalised frame, per defined zone a row of counts, and every change of a track's zone
 * membership as an event carrying the track's uid -- decided on the device from the fp64 track state, in ONE call, with a hysteresis
 * margin, so that a person standing on a boundary does not flicker between zones on the filter's jitter.
 *
 * Setting zones follows mmw_set_sites' rules.  mmw_set_zones gives scene scenes[i] (scenes == NULL: scene i) the first n_zones[i]
 * entries of zones[i][MMW_ZONES_MAX] as its zones 0 .. n_zones[i] - 1; entries past n_zones[i] are not read.  The first call
 * allocates the table -- every scene at 0 zones -- and the baseline below; scenes never listed keep what they have.  Every check is
 * made on the host before anything changes, the new table then travels as ONE copy ordered on the context's stream (exports queued
 * before the call read the old table), and the call is synchronous.  Refusal is atomic -- MMW_E_ARG, the message names the entry,
 * nothing changes, nothing is allocated: n < 0 or n > n_scenes, a NULL array with n > 0, an index out of range or listed twice,
 * n_zones[i] outside 0 .. MMW_ZONES_MAX, a NaN bound, x0 > x1 or y0 > y1, a margin that is negative or not finite, a non-zero
 * reserved_.  Infinite bounds are allowed (half planes, strips).  Zones belong to the slot, like a site: mmw_reset* keeps them, a
 * snapshot blob does not carry them (format version 1 is unchanged) and mmw_restore leaves the destination's zones alone.
 * mmw_get_zones copies the host mirror (no device access; either output may be NULL; a context without a table: 0 zones
 * everywhere, zeroed entries; entries past a scene's n_zones are zero).  mmw_clear_zones waits for the stream and frees table and
 * baseline: the context then launches exactly what a context that never had zones launches, and the export entries return
 * MMW_E_ARG again, as they do before the first mmw_set_zones.  mmw_has_zones: 1 while a table exists, else 0.
 *
 * Membership.  p = (x[0], x[1]) of the track's fp64 state (mmw_track_record.x; the same for dim_x 6 and 9).
 *   core(z) = x0 <= px && px < x1 && y0 <= py && py < y1
 *   wide(z) = the same test with x0 - margin, x1 + margin, y0 - margin, y1 + margin: ONE fp64 operation per bound
 * A track is a member of zone z now iff it was a member at the previous export and wide(z), or it was not and core(z).  "Was a
 * member": the scene's baseline, of the same generation, holds its uid with z's bit.  A NaN coordinate makes every comparison
 * false: the track is in no zone.  Zones may overlap; a track can be a member of several.
 *
 * Baseline.  Per scene the context keeps the uid list of the previous SUCCESSFUL export with a 16-bit membership mask per uid, its
 * length, and a generation and a seen-generation word: the report's mechanism, but the zones' own state -- reports need not be
 * enabled, and the two are consumed at different times.  The baseline starts empty, so a track already inside gets its
 * MMW_ZEV_ENTER at the first export: the event stream is complete, folding it gives the roster.  mmw_reset, mmw_reset_scenes and
 * mmw_restore bump the generation of the scenes they touch (uids restart there), and mmw_set_zones that of the scenes it lists
 * (their bits change meaning) -- one kernel, launched only while a table exists.  The next export of a bumped scene emits ONE
 * MMW_ZEV_REBASED (uid -1, zone -1, id -1, slot = live tracks now: every earlier membership of the scene is void), no
 * MMW_ZEV_LEAVE, evaluates membership with core alone, and emits the MMW_ZEV_ENTERs of that membership.
 *
 * Events are ordered by scene; inside a scene MMW_ZEV_REBASED first, then MMW_ZEV_LEAVE in baseline order -- zones ascending inside
 * a track, slot = the track's position then --, then MMW_ZEV_ENTER in effective_tracks order, zones ascending, slot = its position
 * now.  A baseline uid that is no longer live leaves every zone it was in.  Like the report this is a DIFFERENCE OF STATES, not a
 * log: a track that entered and left between two exports appears in neither.
 * Rows: one per DEFINED zone, in (scene, zone) order; count = members now, count_static = those with is_static, entered / left =
 * this call's MMW_ZEV_ENTER / MMW_ZEV_LEAVE events of the zone; scene is offset by scene_base, as the events' is.
 *
 * Capacity, tickets and arguments are mmw_report_*'s.  Capacity is decided on the DEVICE against both caps: if the rows exceed
 * cap_rows or the events exceed cap_events, nothing is written into either buffer, the baseline and the generations stay as they
 * were, and mmw_zones_wait returns MMW_E_CAPACITY with both counts needed: a retry with larger buffers loses nothing.
 * mmw_zones_async queues its kernels on the context's stream behind whatever was queued last (normally the frame's mmw_step); the
 * counts follow into pinned memory and mmw_zones_wait(ticket) waits for THAT copy only.  ticket in [0,4), ticket 3 is mmw_zones'
 * own.  rows / events: dev pointers, 4-byte aligned.  MMW_E_ARG, nothing touched: a NULL context, no zone table, a NULL buffer
 * with a positive cap, a negative cap, a misaligned buffer, a bad ticket, a wait for a ticket with nothing outstanding.
 * No step kernel reads any of this: a context that never defines a zone launches exactly what it did before zones existed. */
#define MMW_ZONES_MAX 16
typedef struct mmw_zone {          /* 48 bytes */
    double x0, x1, y0, y1;         /* [x0, x1) x [y0, y1) in the scene's normalised frame: the frame of mmw_track_record.x[0], x[1] */
    double margin;                 /* >= 0: hysteresis, above */
    int32_t id;                    /* the caller's label, copied into rows and events */
    int32_t reserved_;             /* must be 0 */
} mmw_zone;
typedef struct mmw_zone_row   { int32_t scene, zone, id, count, count_static, entered, left, reserved_; } mmw_zone_row;   /* 32 bytes */
typedef struct mmw_zone_event { int32_t scene, uid, kind, zone, id, slot; } mmw_zone_event;                              /* 24 bytes */
#define MMW_ZEV_ENTER 1     /* uid is a member of the zone now and was not at the previous export; slot = its position now */
#define MMW_ZEV_LEAVE 2     /* uid was a member at the previous export and is not now (or is not live any more); slot = its position then */
#define MMW_ZEV_REBASED 3   /* every earlier membership of the scene is void; uid = zone = id = -1, slot = live tracks now */
int mmw_set_zones(mmw_ctx *ctx, const int32_t *scenes, int32_t n, const int32_t *n_zones /* host [n] */, const mmw_zone *zones /* host [n][MMW_ZONES_MAX] */);
int mmw_get_zones(mmw_ctx *ctx, int32_t *n_zones /* host [S] */, mmw_zone *zones /* host [S][MMW_ZONES_MAX] */);   /* host mirror, no device access */
int mmw_clear_zones(mmw_ctx *ctx);
int mmw_has_zones(mmw_ctx *ctx);
int mmw_zones_async(mmw_ctx *ctx, mmw_zone_row *rows, int32_t cap_rows, mmw_zone_event *events, int32_t cap_events, int32_t scene_base,
                    int32_t ticket);
int mmw_zones_wait(mmw_ctx *ctx, int32_t ticket, int32_t *n_rows, int32_t *n_events);   /* waits for that ticket's counts only; either may be NULL */
int mmw_zones(mmw_ctx *ctx, mmw_zone_row *rows, int32_t cap_rows, mmw_zone_event *events, int32_t cap_events, int32_t scene_base,
              int32_t *n_rows, int32_t *n_events);                                      /* async + wait */

/* ---- trails ----
 * Where a person has been: per live uid the last `depth` positions, sampled on the device when the caller asks, with the time of the
 * first sample and the distance walked over the uid's whole life -- a path to draw and a distance, without reading the report back
 * every frame.  A TRAIL belongs to one uid of one scene: a ring of its last `depth` SAMPLES and three words that cover all of them,
 * `total`, `t_first` and `travelled`.  A sample is taken only by mmw_trails_sample, normally once behind each mmw_step.  No step
 * kernel reads or writes any of this: a context that never enables trails launches exactly what it did before trails existed.
 *
 * mmw_trails_enable(depth), depth in 1 .. MMW_TRAIL_DEPTH_MAX, allocates per scene t_cap trail slots (owner uid or -1 = free, total,
 * t_first, travelled and the last fp64 (x, y): 40 bytes), t_cap x depth ring entries of 24 bytes, and three words: a generation, the
 * generation seen and a call ordinal -- S * t_cap * (24 * depth + 40) bytes plus 12 S (t_cap = the context's track capacity: 329 MB
 * at 4096 scenes, t_cap 51, depth 64).  Every slot starts free, every word at 0; the state is ordered on the context's stream.
 * Enabling again, with any depth, starts over.  depth == 0 waits for the stream, frees the state and turns trails off (MMW_OK also
 * when they were off).  depth outside 0 .. MMW_TRAIL_DEPTH_MAX: MMW_E_ARG, nothing changed.  A failed allocation: MMW_E_HIP, nothing
 * changed -- an earlier enablement stays as it is.  Until enabled, mmw_trails_sample and the export entries return MMW_E_ARG.
 *
 * mmw_trails_sample is asynchronous: ONE kernel on the context's stream behind whatever was queued last.  Scene s is ASKED when
 * scene_flags == NULL or scene_flags[s] != 0 -- the frame's n_pts array serves as the flags (MMW_EMPTY_FRAME counts as asked: track()
 * ran).  For an asked scene, in this order:
 *   1. generation != seen: every slot of the scene is freed and seen = generation -- a uid from before a reset never aliases one
 *      from after it;
 *   2. every slot whose owner is not among the live uids is freed (trails of expired tracks are not kept);
 *   3. every live uid without a slot takes a free one (there always is one: live tracks <= t_cap; which one is not observable), with
 *      total = 0 and travelled = 0;
 *   4. every live track appends one sample:
 *        x, y, z   mmw_track_record.x[0..2] of the fp64 state, each rounded once to fp32 (the same for dim_x 6 and 9)
 *        t         t[s]; with t == NULL the scene's call ordinal as a double: the number of earlier mmw_trails_sample calls that
 *                  asked this scene since mmw_trails_enable (resets do not restart it)
 *        flags     MMW_TRAIL_STATIC | MMW_TRAIL_UPDATED as defined below
 *      total == 0: t_first = t.  Otherwise dx = x - last_x; dy = y - last_y; travelled = travelled + sqrt(dx * dx + dy * dy) -- in
 *      fp64 on the fp64 state, not on the rounded points, in exactly that operation order (no fused multiply-add: the library is
 *      built with -ffp-contract=off).  Then last = (x, y), total += 1, and the sample goes to ring position (total - 1) % depth: it
 *      overwrites the oldest.
 * Non-finite values pass through: a NaN position makes travelled NaN and it stays NaN.  A scene that is not asked is not touched
 * (nor is its ordinal).  Sampling twice without a step gives two samples.  scene_flags: dev pointer, 4-byte aligned; t: dev pointer,
 * 8-byte aligned; else MMW_E_ARG.
 *
 * mmw_trails_async / _wait is a pure function of the trail state and the live lists: it writes the caller's buffers and the
 * context's scratch, nothing else -- a refused call loses nothing, and the same state can be exported under several tickets.  One
 * directory entry per live track in the report's order (scenes ascending, then effective_tracks order): entry i belongs to
 * mmw_report row i of the same state; scene ids are offset by scene_base.  A track whose uid owns no slot (born since the last
 * sample) has count = total = 0, t_first = travelled = 0, and so has every track of a scene whose generation != seen (reset or
 * restored and not sampled since).  count = min(total, depth), cut to the NEWEST max_per_track when max_per_track > 0 (0 = all;
 * < 0: MMW_E_ARG); total, t_first and travelled are the whole trail's either way.  The entries partition `points`, as in mmw_clouds:
 * entry i owns points[first .. first + count), oldest first.
 * Capacity is decided on the DEVICE against both caps, as the clouds': totals are formed in 64 bits, saturate at INT32_MAX and then
 * never fit.  If anything does not fit, nothing is written and mmw_trails_wait returns MMW_E_CAPACITY with both counts needed.
 * mmw_trails_async queues its kernels on the context's stream; the counts follow into pinned memory and mmw_trails_wait(ticket)
 * waits for THAT copy only.  ticket in [0,4), ticket 3 is mmw_trails' own.  dir / points: dev pointers, 8-byte aligned.  MMW_E_ARG,
 * nothing touched: a NULL context, trails not enabled, a NULL buffer with a positive cap, a negative cap, a misaligned buffer, a
 * bad ticket, a wait for a ticket with nothing outstanding.
 *
 * Life cycle.  mmw_reset, mmw_reset_scenes and mmw_restore bump the generation of the scenes they touch (uids restart there) -- one
 * kernel beside the report's and the zones', launched only while trails are enabled.  mmw_destroy frees the state.  Trails are not
 * in a snapshot blob: format version 1 is unchanged and a restored scene starts new trails.  A uid sampled more than INT32_MAX
 * times is not supported. */
#define MMW_TRAIL_DEPTH_MAX 256
#define MMW_TRAIL_STATIC 1    /* point flag: is_static at the sample */
#define MMW_TRAIL_UPDATED 2   /* point flag: lifetime == 0 at the sample (the frame's points were associated) */
typedef struct mmw_trail_point { double t; float x, y, z; int32_t flags; } mmw_trail_point;   /* 24 bytes */
typedef struct mmw_trail_track {   /* 40 bytes: one directory entry */
    int32_t scene, slot, uid;      /* as mmw_track_report's: entry i belongs to mmw_report row i of the same state */
    int32_t first, count;          /* this entry's points are points[first .. first + count), oldest first */
    int32_t total;                 /* samples ever taken of this uid (count <= min(total, depth)) */
    double t_first;                /* t of the uid's first sample; 0 while total == 0 */
    double travelled;              /* path length in the x/y plane over ALL its samples, above */
} mmw_trail_track;
int mmw_trails_enable(mmw_ctx *ctx, int32_t depth);   /* 1 .. MMW_TRAIL_DEPTH_MAX; 0 = off and freed */
int mmw_trails_sample(mmw_ctx *ctx, const int32_t *scene_flags /* dev [S] or NULL */, const double *t /* dev [S] or NULL */);
int mmw_trails_async(mmw_ctx *ctx, mmw_trail_track *dir, int32_t cap_tracks, mmw_trail_point *points, int32_t cap_points,
                     int32_t max_per_track, int32_t scene_base, int32_t ticket);
int mmw_trails_wait(mmw_ctx *ctx, int32_t ticket, int32_t *n_tracks, int32_t *n_points);   /* waits for that ticket's counts only; either may be NULL */
int mmw_trails(mmw_ctx *ctx, mmw_trail_track *dir, int32_t cap_tracks, mmw_trail_point *points, int32_t cap_points,
               int32_t max_per_track, int32_t scene_base, int32_t *n_tracks, int32_t *n_points);   /* async + wait */

/* ---- tripwires ----
 * How many people walked through a door, and which way: per scene up to MMW_TRIPWIRES_MAX directed segments A -> B in the scene's
 * normalised frame, per wire the number of tracks that went across it either way, and every crossing as an event with the track's
 * uid.  The zones are a difference of states -- a track that walks through a doorway zone between two exports appears in neither
 * -- and the trails hold positions, not passages.  This is a LOG: the sides are decided on the device by mmw_tripwires_sample,
 * normally once behind each mmw_step, nothing is lost between two exports, and the export is read when the caller likes.  No step
 * kernel reads or writes any of this: a context that never enables tripwires launches exactly what it did before they existed.
 *
 * mmw_tripwires_enable(log_depth), log_depth in 1 .. MMW_TRIPWIRE_LOG_MAX, allocates the wire table (every scene at 0 wires) and per
 * scene: t_cap uid SLOTS of {owner uid or -1 = free, side word: two bits per wire, 0 unknown, 1 negative, 2 positive}; per wire the
 * int32 totals `forward` and `backward` and the two MARKS (the totals at the previous successful export); an event ring of
 * log_depth entries with the words `logged` (events ever appended) and `taken` (events handed out), event number n at n % log_depth;
 * a generation, the generation seen and a call ordinal.  Every slot starts free, every word at 0; the state is ordered on the
 * context's stream.  Enabling again, with any depth, starts over (0 wires everywhere).  log_depth == 0 waits for the stream, frees
 * the state and turns tripwires off (MMW_OK also when they were off).  log_depth outside 0 .. MMW_TRIPWIRE_LOG_MAX: MMW_E_ARG, nothing
 * changed.  A failed allocation: MMW_E_HIP, nothing changed -- an earlier enablement stays as it is.  Until enabled, every other
 * entry returns MMW_E_ARG, except mmw_get_tripwires, which reports 0 wires.
 *
 * Setting wires follows mmw_set_zones' rules.  mmw_set_tripwires gives scene scenes[i] (scenes == NULL: scene i) the first
 * n_wires[i] entries of wires[i][MMW_TRIPWIRES_MAX] as its wires 0 .. n_wires[i] - 1; entries past n_wires[i] are not read; scenes
 * never listed keep what they have.  Every check is made on the host before anything changes, the table travels as ONE copy ordered
 * on the context's stream, and the call is synchronous.  Refused as a whole (MMW_E_ARG, the message names the entry, no scene's
 * wires change): n < 0 or n > n_scenes, n_wires or wires NULL with n > 0, a scene index out of range or listed twice, n_wires[i]
 * outside 0 .. MMW_TRIPWIRES_MAX, a non-zero reserved_, a coordinate that is not finite, a margin that is negative or not finite,
 * A == B, a len2 or band (below) that is zero (band: with a margin > 0) or not finite.  For each wire the HOST derives, in exactly
 * this operation order (the library is built with -ffp-contract=off, host side included):
 *     dx = bx - ax;  dy = by - ay;  len2 = dx * dx + dy * dy;  band = margin * sqrt(len2)
 * and the device reads only ax, ay, dx, dy, len2, band and id: no device sqrt takes part in a decision.  For the listed scenes
 * the generation is bumped (their side bits change meaning), and forward, backward and the marks restart at 0, ordered on the
 * stream; the log and `taken` are kept.  Wires belong to the slot, like zones: mmw_reset* keeps wires, counters and log, a snapshot
 * blob does not carry them (format version 1 is unchanged) and mmw_restore leaves the destination's wires alone.
 * mmw_get_tripwires copies the host mirror (no device access; either output may be NULL; entries past a scene's n_wires are zero).
 *
 * mmw_tripwires_sample is asynchronous: ONE kernel on the context's stream behind whatever was queued last.  Scene flags and t are
 * mmw_trails_sample's: scene s is ASKED when scene_flags == NULL or scene_flags[s] != 0 (the frame's n_pts array serves), t == NULL
 * means the scene's call ordinal as a double -- the number of earlier mmw_tripwires_sample calls that asked this scene since
 * mmw_tripwires_enable, with or without wires.  An asked scene with 0 wires only sets seen = generation (and counts the call).  For
 * an asked scene with wires, in this order:
 *   1. generation != seen: every slot is freed, seen = generation, and ONE MMW_TW_REBASED event is appended (t of this sample);
 *   2. every slot whose owner is not among the live uids is freed;
 *   3. every live uid without a slot takes a free one with side word 0 (the trails' rule; which slot is not observable);
 *   4. for every live track, with p = (x[0], x[1]) of the fp64 state, and every defined wire in ascending order:
 *          rx = px - ax;  ry = py - ay;
 *          u = rx * dx + ry * dy;            along the wire
 *          c = dx * ry - dy * rx;            > 0: left of A -> B
 *          inside = 0 <= u && u <= len2
 *          new = !inside ? unknown : c > band ? positive : c < -band ? negative : old
 *      old = negative and new = positive: one MMW_TW_FORWARD event and forward += 1; old = positive and new = negative:
 *      MMW_TW_BACKWARD and backward += 1.  Then the side becomes `new`.
 * So a NaN or infinite coordinate makes `inside` false: the side is forgotten and there is no event.  A track that walks round an
 * end of the segment passes through `unknown` and is not counted, one that dithers inside the band is counted once at most, one
 * born beyond the wire is not counted.  Events of one call are appended in this order: REBASED first, then tracks in
 * effective_tracks order, wires ascending inside a track; each carries slot = the track's position now, t = the sample's t and the
 * scene.  If one call appends more events than log_depth, only the newest log_depth are written.  A scene that is not asked is not
 * touched.  Sampling twice without a step changes nothing the second time, except the ordinal.  scene_flags: dev pointer, 4-byte
 * aligned; t: dev pointer, 8-byte aligned; else MMW_E_ARG.
 *
 * mmw_tripwires_async / _wait export rows and events in one call, with the zones' mechanics.  Rows: one per DEFINED wire, in
 * (scene, wire) order; forward / backward are the totals since the scene's wires were last set, d_forward / d_backward those
 * totals minus the marks, lost = max(0, logged - log_depth - taken): events of the scene overwritten before an export could take
 * them, the same in each of the scene's rows -- counters never lose anything.  Events: per scene those numbered
 * max(taken, logged - log_depth) .. logged - 1, oldest first, scenes ascending; scene is offset by scene_base, as the rows' is.  On
 * success taken = logged and the marks become the totals.  A uid that crossed forward and back between two exports yields both
 * events and both counts.  Capacity is decided on the DEVICE against both caps: if anything does not fit, NOTHING is written,
 * taken and the marks stay as they were, and mmw_tripwires_wait returns MMW_E_CAPACITY with both counts needed: a retry with larger
 * buffers loses nothing.  mmw_tripwires_async queues its kernels on the context's stream; the counts follow into pinned memory
 * and mmw_tripwires_wait(ticket) waits for THAT copy only.  ticket in [0,4), ticket 3 is mmw_tripwires' own.  rows / events: dev
 * pointers, 8-byte aligned.  MMW_E_ARG, nothing touched: a NULL context, tripwires not enabled, a NULL buffer with a positive cap, a
 * negative cap, a misaligned buffer, a bad ticket, a wait for a ticket with nothing outstanding.
 *
 * Life cycle.  mmw_reset, mmw_reset_scenes and mmw_restore bump the generation of the scenes they touch (uids restart there), in
 * the one launch the report, the zones and the trails share.  mmw_destroy frees the state.  More than INT32_MAX events or crossings
 * per scene are not supported. */
#define MMW_TRIPWIRES_MAX 16
#define MMW_TRIPWIRE_LOG_MAX 4096
typedef struct mmw_tripwire {      /* 48 bytes */
    double ax, ay, bx, by;         /* A -> B in the frame of mmw_track_record.x[0], x[1] */
    double margin;                 /* >= 0, metres: half-width of the band in which a side is kept */
    int32_t id;                    /* caller's label, copied into rows and events */
    int32_t reserved_;             /* must be 0 */
} mmw_tripwire;
typedef struct mmw_tripwire_row   { int32_t scene, wire, id, forward, backward, d_forward, d_backward, lost; } mmw_tripwire_row;   /* 32 bytes */
typedef struct mmw_tripwire_event { int32_t scene, uid, kind, wire, id, slot; double t; } mmw_tripwire_event;                       /* 32 bytes */
#define MMW_TW_FORWARD 1    /* the uid went from the negative side (right of A->B) to the positive side (left) */
#define MMW_TW_BACKWARD 2
#define MMW_TW_REBASED 3    /* the scene's uids or wires are new from here on; uid = wire = id = -1, slot = live tracks then */
int mmw_tripwires_enable(mmw_ctx *ctx, int32_t log_depth);      /* 1 .. MMW_TRIPWIRE_LOG_MAX; 0 = off and freed */
int mmw_set_tripwires(mmw_ctx *ctx, const int32_t *scenes, int32_t n, const int32_t *n_wires /* host [n] */, const mmw_tripwire *wires /* host [n][MMW_TRIPWIRES_MAX] */);
int mmw_get_tripwires(mmw_ctx *ctx, int32_t *n_wires /* host [S] */, mmw_tripwire *wires /* host [S][MMW_TRIPWIRES_MAX] */);   /* host mirror, no device access */
int mmw_tripwires_sample(mmw_ctx *ctx, const int32_t *scene_flags /* dev [S] or NULL */, const double *t /* dev [S] or NULL */);
int mmw_tripwires_async(mmw_ctx *ctx, mmw_tripwire_row *rows, int32_t cap_rows, mmw_tripwire_event *events, int32_t cap_events,
                        int32_t scene_base, int32_t ticket);
int mmw_tripwires_wait(mmw_ctx *ctx, int32_t ticket, int32_t *n_rows, int32_t *n_events);   /* waits for that ticket's counts only; either may be NULL */
int mmw_tripwires(mmw_ctx *ctx, mmw_tripwire_row *rows, int32_t cap_rows, mmw_tripwire_event *events, int32_t cap_events,
                  int32_t scene_base, int32_t *n_rows, int32_t *n_events);                 /* async + wait */

/* ---- stance ----
 * Who is on the floor, since when, and did they fall: per live uid one of four classes -- MMW_STANCE_UNKNOWN, _UPRIGHT, _LOW
 * (sitting or crouched), _LYING -- decided from the head height of the posture keypoints (kp[22]: Head, row 1 = height in metres
 * above the floor), with falls and long lies as events.  The first by-uid consumer that reads mmw_track_record.kp: without it a
 * caller reads every skeleton back every frame and keeps the per-uid state on the host.  A LOG with the tripwires' mechanics: the
 * classes are decided on the device by mmw_stance_sample, normally once behind each mmw_estimate_posture, nothing is lost between
 * two exports.  No step kernel reads or writes any of this: a context that never enables stance launches exactly what it did before.
 *
 * Each scene has zero or one RULE (MMW_STANCE_RULES_MAX = 1); a scene without a rule is not watched.  mmw_stance_enable(log_depth),
 * log_depth in 1 .. MMW_STANCE_LOG_MAX, allocates the rule table (every scene at 0 rules) and per scene: t_cap uid SLOTS of {owner
 * uid or -1 = free; word: bits 0-1 the class, bit 2 "LONG_LIE given in this episode"; t_since (double): the t of the sample that
 * entered the current class; t_upright (double): the t of the newest sample that classed the uid UPRIGHT, -inf if never}; the int32
 * totals `falls` and `long_lies` and their two MARKS (the totals at the previous successful export); an event ring of log_depth
 * entries with the words `logged` and `taken`, event number n at n % log_depth; a generation, the generation seen and a call
 * ordinal.  Every slot starts free, every word at 0; the state is ordered on the context's stream.  Enabling again, with any depth,
 * starts over (0 rules everywhere).  log_depth == 0 waits for the stream, frees the state and turns stance off (MMW_OK also when it
 * was off).  log_depth outside 0 .. MMW_STANCE_LOG_MAX: MMW_E_ARG, nothing changed.  A failed allocation: MMW_E_HIP, nothing changed
 * -- an earlier enablement stays as it is.  Until enabled, every other entry returns MMW_E_ARG, except mmw_get_stance_rules, which
 * reports 0 rules.
 *
 * Setting rules follows mmw_set_tripwires' rules: mmw_set_stance_rules gives scene scenes[i] (scenes == NULL: scene i) the first
 * n_rules[i] (0 or 1) entries of rules[i][MMW_STANCE_RULES_MAX]; scenes never listed keep what they have.  Every check is made on
 * the host before anything changes, the table travels as ONE copy ordered on the context's stream, and the call is synchronous.
 * Refused as a whole (MMW_E_ARG, the message names the entry, no scene's rule changes): n < 0 or n > n_scenes, n_rules or rules NULL
 * with n > 0, a scene index out of range or listed twice, n_rules[i] outside 0 .. 1, a non-zero reserved_, an h_stand, h_lie,
 * margin, fall_window or max_gap that is not finite, a negative margin, fall_window or long_lie, a long_lie that is NaN (+inf is
 * allowed: never), max_gap <= 0, or !(lie_hi < up_lo) (below).  pad_ is not read.  For each rule the HOST derives, one fp64
 * operation each (the library is built with -ffp-contract=off, host side included):
 *     up_hi = h_stand + margin;  up_lo = h_stand - margin;  lie_hi = h_lie + margin;  lie_lo = h_lie - margin;  gap2 = max_gap * max_gap
 * and the device reads only these five and h_stand, h_lie, fall_window, long_lie and id: it takes no sqrt and does no arithmetic on
 * a threshold.  lie_hi < up_lo makes "above the upper boundary" imply "above the lower boundary" whatever the old class was.  For
 * the listed scenes the generation is bumped, and falls, long_lies and the marks restart at 0, ordered on the stream; the log and
 * `taken` are kept.  Rules belong to the slot, as wires do: mmw_reset* keeps rules, counters and log, a snapshot blob does not carry
 * them (format version 1 is unchanged) and mmw_restore leaves the destination's rules alone.  mmw_get_stance_rules copies the host
 * mirror (no device access; either output may be NULL; entries past a scene's n_rules are zero).
 *
 * mmw_stance_sample is asynchronous: ONE kernel on the context's stream behind whatever was queued last -- normally the frame's
 * mmw_estimate_posture or mmw_set_keypoints*, whose keypoints it reads.  Scene flags, t and the ordinal are mmw_tripwires_sample's.
 * An asked scene without a rule only sets seen = generation (and counts the call).  For an asked scene with a rule, in this order:
 *   1. generation != seen: every slot is freed, seen = generation, and ONE MMW_SEV_REBASED event is appended (t of this sample);
 *   2. every slot whose owner is not among the live uids is freed;
 *   3. every live uid without a slot takes a free one with word 0 and t_upright = -inf (which slot is not observable);
 *   4. for every live track, with kp[] the record's 57 fp32 keypoints, tt the sample's t and old = the slot's class:
 *          head = (double)kp[22]
 *          g_c  = fp32(kp[19c + 1] - kp[19c + 2]), c = 0, 1, 2;  s = (g_0^2 + g_1^2) + g_2^2 in fp64     (mmw_skeletons' check)
 *          plausible = (head - head == 0.0) && !(s > gap2)
 *          not plausible: nothing of the uid changes and it gets no event
 *          a1  = head > (old == UPRIGHT ? up_lo  : old == UNKNOWN ? h_stand : up_hi)
 *          a0  = head > (old == LYING   ? lie_hi : old == UNKNOWN ? h_lie   : lie_lo)
 *          new = a1 ? UPRIGHT : a0 ? LOW : LYING
 *          if new != old:
 *              kind = (new == LYING && old != UNKNOWN && tt - t_upright <= fall_window) ? FALL : CHANGE
 *              event {kind, from = old, to = new};  t_since = tt;  bit 2 cleared;  FALL: falls += 1
 *          if new == UPRIGHT: t_upright = tt
 *          if new == LYING && bit 2 clear && tt - t_since >= long_lie:
 *              event LONG_LIE {from = to = LYING};  bit 2 set;  long_lies += 1
 * So a NaN or infinite head is not plausible, a NaN s is (the reference's `nan > 0.5` is false).  The first classification of a
 * uid is a CHANGE with from = 0 and never a FALL.  A fall seen passing through LOW for a sample or two is still a FALL if the uid
 * was UPRIGHT within fall_window; a person who lies down slowly produces a CHANGE.  long_lie == 0 gives CHANGE or FALL and
 * LONG_LIE in the same sample, in that order; there is ONE LONG_LIE per episode of lying.  Events of one call are appended in this
 * order: REBASED first, then tracks in effective_tracks order, CHANGE or FALL before LONG_LIE; each carries slot = the track's
 * position now, t = the sample's t and the scene.  If one call appends more events than log_depth, only the newest log_depth are
 * written.  A scene that is not asked is not touched.  A second sample without a step changes only the ordinal -- and gives a
 * LONG_LIE if t moved on far enough.  scene_flags: dev pointer, 4-byte aligned; t: dev pointer, 8-byte aligned; else MMW_E_ARG.
 *
 * mmw_stance_async / _wait export rows and events in one call, with the tripwires' mechanics.  Rows: one per scene WITH a rule,
 * scenes ascending; upright, low, lying and unknown count the scene's owned slots by class as of the last sample (all 0 while the
 * scene is rebased and not yet sampled); falls / long_lies are the totals since the scene's rule was last set, d_falls /
 * d_long_lies those totals minus the marks, lost = max(0, logged - log_depth - taken).  Events: per scene those numbered
 * max(taken, logged - log_depth) .. logged - 1, oldest first, scenes ascending; scene is offset by scene_base, as the rows' is.  On
 * success taken = logged and the marks become the totals.  Capacity is decided on the DEVICE against both caps: if anything does
 * not fit, NOTHING is written, taken and the marks stay as they were, and mmw_stance_wait returns MMW_E_CAPACITY with both counts
 * needed: a retry with larger buffers loses nothing.  ticket in [0,4), ticket 3 is mmw_stance's own.  rows / events: dev pointers,
 * 8-byte aligned.  MMW_E_ARG, nothing touched: a NULL context, stance not enabled, a NULL buffer with a positive cap, a negative
 * cap, a misaligned buffer, a bad ticket, a wait for a ticket with nothing outstanding.
 *
 * Life cycle.  mmw_reset, mmw_reset_scenes and mmw_restore bump the generation of the scenes they touch, in the one launch the
 * report, the zones, the trails and the tripwires share.  mmw_destroy frees the state.  More than INT32_MAX events per scene are
 * not supported. */
#define MMW_STANCE_UNKNOWN 0
#define MMW_STANCE_UPRIGHT 1
#define MMW_STANCE_LOW 2        /* sitting or crouched */
#define MMW_STANCE_LYING 3
#define MMW_STANCE_RULES_MAX 1
#define MMW_STANCE_LOG_MAX 4096
typedef struct mmw_stance_rule {   /* 64 bytes */
    double h_stand;                /* head above this: UPRIGHT (metres, room height = kp[22]) */
    double h_lie;                  /* head not above this: LYING */
    double margin;                 /* >= 0: hysteresis on both heights */
    double fall_window;            /* >= 0 s: reaching LYING within this of having been UPRIGHT is a FALL */
    double long_lie;               /* >= 0 s, +inf = never: LYING this long gives ONE LONG_LIE per episode */
    double max_gap;                /* > 0: the reference's skeleton check (Visualizer.py:277 uses 0.5) */
    int32_t id;                    /* caller's label, copied into rows */
    int32_t reserved_;             /* must be 0 */
    int32_t pad_[2];               /* not read */
} mmw_stance_rule;
typedef struct mmw_stance_event { int32_t scene, uid, kind, from, to, slot; double t; } mmw_stance_event;   /* 32 bytes */
#define MMW_SEV_CHANGE 1
#define MMW_SEV_FALL 2
#define MMW_SEV_LONG_LIE 3
#define MMW_SEV_REBASED 4       /* the scene's uids or rule are new from here on; uid = -1, from = to = 0, slot = live tracks then */
typedef struct mmw_stance_row { int32_t scene, id, upright, low, lying, unknown, falls, d_falls, long_lies, d_long_lies, lost, reserved_; } mmw_stance_row;   /* 48 bytes */
int mmw_stance_enable(mmw_ctx *ctx, int32_t log_depth);         /* 1 .. MMW_STANCE_LOG_MAX; 0 = off and freed */
int mmw_set_stance_rules(mmw_ctx *ctx, const int32_t *scenes, int32_t n, const int32_t *n_rules /* host [n] */, const mmw_stance_rule *rules /* host [n][MMW_STANCE_RULES_MAX] */);
int mmw_get_stance_rules(mmw_ctx *ctx, int32_t *n_rules /* host [S] */, mmw_stance_rule *rules /* host [S][MMW_STANCE_RULES_MAX] */);   /* host mirror, no device access */
int mmw_stance_sample(mmw_ctx *ctx, const int32_t *scene_flags /* dev [S] or NULL */, const double *t /* dev [S] or NULL */);
int mmw_stance_async(mmw_ctx *ctx, mmw_stance_row *rows, int32_t cap_rows, mmw_stance_event *events, int32_t cap_events,
                     int32_t scene_base, int32_t ticket);
int mmw_stance_wait(mmw_ctx *ctx, int32_t ticket, int32_t *n_rows, int32_t *n_events);   /* waits for that ticket's counts only; either may be NULL */
int mmw_stance(mmw_ctx *ctx, mmw_stance_row *rows, int32_t cap_rows, mmw_stance_event *events, int32_t cap_events,
               int32_t scene_base, int32_t *n_rows, int32_t *n_events);                 /* async + wait */

/* ---- heat ----
 * Where in the room people spend their time: per scene zero or one GRID of nx x ny square cells in the scene's normalised frame, and
 * per cell the time live tracks spent in it (`dwell`, fp64), the samples taken in it and the visits that began in it.  The zones are
 * a few rectangles chosen in advance and the trails forget a uid when its track expires; this is the accumulation over hours, kept
 * next to the state it reads -- a few words per live track per frame -- and moved only when the caller asks for the map.  The first
 * consumer whose state is a dense per-scene array, so its export is a stream compaction: only cells with samples > 0 travel.  No step
 * kernel reads or writes any of this: a context that never enables heat launches exactly what it did before.
 *
 * mmw_heat_enable(cells), cells in 1 .. MMW_HEAT_CELLS_MAX, allocates the grid table (every scene at 0 grids) and per scene: `cells`
 * cells of {dwell fp64, samples int32, visits int32} = 16 bytes; t_cap uid SLOTS of {owner uid or -1 = free, last_cell int32, last_t
 * fp64} = 16 bytes; the scene words calls, outside (int32), t_first, t_last (fp64); a generation, the generation seen and a call
 * ordinal -- S * (16 * cells + 16 * t_cap + 36) bytes plus a table of 56 S (4096 scenes x 1024 cells: 16 B x 4 Mi cells = 67 MB, plus
 * 3.5 MB of slots at t_cap 51).  Every slot starts free, every word at 0; the state is ordered on the context's stream.  Enabling
 * again, with any capacity, starts over (0 grids everywhere).  cells == 0 waits for the stream, frees the state and turns heat off
 * (MMW_OK also when it was off).  cells outside 0 .. MMW_HEAT_CELLS_MAX: MMW_E_ARG, nothing changed.  A failed allocation: MMW_E_HIP,
 * nothing changed -- an earlier enablement stays as it is.  Until enabled, every other entry returns MMW_E_ARG, except
 * mmw_get_heat_grids, which reports 0 grids.
 *
 * Setting grids follows mmw_set_stance_rules' rules: mmw_set_heat_grids gives scene scenes[i] (scenes == NULL: scene i) the first
 * n_grids[i] (0 or 1) entries of grids[i][MMW_HEAT_GRIDS_MAX]; scenes never listed keep what they have.  Every check is made on the
 * host before anything changes, the table travels as ONE copy ordered on the context's stream, and the call is synchronous.  Refused
 * as a whole (MMW_E_ARG, the message names the entry, no scene's grid changes): n < 0 or n > n_scenes, n_grids or grids NULL with
 * n > 0, a scene index out of range or listed twice, n_grids[i] outside 0 .. 1, a non-zero reserved_, an x0, y0 or cell that is not
 * finite, cell <= 0, a max_gap that is NaN or <= 0 (+inf is allowed: every interval counts), nx < 1 or ny < 1, nx * ny (formed in 64
 * bits) above the enabled capacity.  Cell (ix, iy) covers [x0 + ix * cell, x0 + (ix + 1) * cell) x [y0 + iy * cell, ...) and has index
 * iy * nx + ix.  For the listed scenes the generation is bumped and every cell and calls, outside, t_first and t_last restart at 0,
 * ordered on the stream: the geometry changed, so old cells mean nothing.  Grids and cells belong to the slot (the room), like a
 * site: mmw_reset* and mmw_restore keep both and only bump the generation; a snapshot blob carries neither (format version 1 is
 * unchanged).  mmw_get_heat_grids copies the host mirror (no device access; either output may be NULL; entries past n_grids are zero).
 *
 * mmw_heat_sample is asynchronous: ONE kernel on the context's stream behind whatever was queued last, normally once behind each
 * mmw_step.  Scene flags, t and the ordinal are mmw_tripwires_sample's: scene s is ASKED when scene_flags == NULL or scene_flags[s]
 * != 0, and t == NULL means the scene's call ordinal as a double -- the number of earlier mmw_heat_sample calls that asked this
 * scene since mmw_heat_enable, with or without a grid.  An asked scene without a grid only sets seen = generation (and counts the
 * call).  For an asked scene with a grid, in this order:
 *   1. generation != seen: every slot is freed and seen = generation;
 *   2. every slot whose owner is not among the live uids is freed;
 *   3. every live uid without a slot takes a free one and is FRESH (which slot is not observable);
 *   4. tt = the sample's t;  calls was 0: t_first = tt;  calls += 1;  t_last = tt;
 *   5. for every live track, in effective_tracks order, with p = (x[0], x[1]) of the fp64 state:
 *          fx = (px - x0) / cell;  fy = (py - y0) / cell                  one fp64 subtraction and one fp64 division each
 *          inside = fx >= 0 && fx < (double)nx && fy >= 0 && fy < (double)ny          (a NaN makes it false)
 *          c = inside ? (int)fy * nx + (int)fx : -1
 *          c < 0: outside += 1
 *          else:  samples[c] += 1
 *                 visits[c] += 1 iff the track is fresh or last_cell != c
 *                 not fresh: dt = tt - last_t;  dwell[c] = dwell[c] + dt iff dt > 0 && dt <= max_gap
 *          last_cell = c;  last_t = tt
 * The interval since a uid's previous sample is credited to the cell it is in NOW.  Several tracks in one cell add to dwell[c] one
 * after another in list order: the fp64 sum is one defined sequence of additions (the library is built with -ffp-contract=off).  A
 * track outside the grid keeps its slot: coming back counts a visit, and the interval it was away is credited like any other.  A
 * scene that is not asked is not touched.  scene_flags: dev pointer, 4-byte aligned; t: dev pointer, 8-byte aligned; else MMW_E_ARG.
 *
 * mmw_heat_async / _wait write two buffers.  Rows: one per scene WITH a grid -- with scene_flags != NULL only those whose flag is
 * non-zero -- scenes ascending; calls and outside count the samples since the counters last restarted, t_first / t_last are the t of
 * the first and the newest of those calls (0 while calls == 0).  Cells: one mmw_heat_cell per cell of those scenes with samples > 0,
 * in (scene, cell index) order; row i owns cells[first .. first + count).  scene is offset by scene_base in both.  With mode
 * MMW_HEAT_KEEP the export is a pure function of the state: the same state can be exported under several tickets.  With
 * MMW_HEAT_CLEAR, and only when everything fitted, the exported scenes' cells and their calls, outside, t_first and t_last restart at
 * 0 behind the copy; the uid slots stay, so the next interval of somebody who is still sitting there is credited in the new window
 * and counts no new visit -- hourly maps are cut without losing a frame.  Capacity is decided on the DEVICE against both caps, as
 * the trails': totals are formed in 64 bits, saturate at INT32_MAX and then never fit; if anything does not fit, NOTHING is written,
 * nothing is cleared and mmw_heat_wait returns MMW_E_CAPACITY with both counts needed.  mmw_heat_async queues its kernels on the
 * context's stream; the counts follow into pinned memory and mmw_heat_wait(ticket) waits for THAT copy only.  ticket in [0,4),
 * ticket 3 is mmw_heat's own.  rows / cells: dev pointers, 8-byte aligned; scene_flags: dev pointer, 4-byte aligned.  MMW_E_ARG,
 * nothing touched: a NULL context, heat not enabled, a NULL buffer with a positive cap, a negative cap, a misaligned pointer, a mode
 * other than the two, a bad ticket, a wait for a ticket with nothing outstanding.
 *
 * Life cycle.  mmw_reset, mmw_reset_scenes and mmw_restore bump the generation of the scenes they touch, with the same kernel as
 * the report's, the zones', the trails', the tripwires' and stance's, launched only while heat is enabled: no interval is credited across them, no uid of before aliases one
 * of after, and the cells are kept.  mmw_destroy frees the state.  More than INT32_MAX samples per cell are not supported. */
#define MMW_HEAT_CELLS_MAX 4096
#define MMW_HEAT_GRIDS_MAX 1
typedef struct mmw_heat_grid {     /* 48 bytes */
    double x0, y0;                 /* corner of cell (0, 0) in the frame of mmw_track_record.x[0], x[1] */
    double cell;                   /* side of a cell, > 0 and finite */
    double max_gap;                /* > 0, +inf allowed: an interval longer than this is credited to nobody */
    int32_t nx, ny;                /* >= 1, nx * ny <= the enabled capacity */
    int32_t id;                    /* caller's label, copied into the row */
    int32_t reserved_;             /* must be 0 */
} mmw_heat_grid;
typedef struct mmw_heat_row  { int32_t scene, id, nx, ny, first, count, calls, outside; double t_first, t_last; } mmw_heat_row;   /* 48 bytes */
typedef struct mmw_heat_cell { int32_t scene, cell, samples, visits; double dwell; } mmw_heat_cell;                               /* 24 bytes */
#define MMW_HEAT_KEEP 0
#define MMW_HEAT_CLEAR 1
int mmw_heat_enable(mmw_ctx *ctx, int32_t cells);               /* 1 .. MMW_HEAT_CELLS_MAX per scene; 0 = off and freed */
int mmw_set_heat_grids(mmw_ctx *ctx, const int32_t *scenes, int32_t n, const int32_t *n_grids /* host [n] */, const mmw_heat_grid *grids /* host [n][MMW_HEAT_GRIDS_MAX] */);
int mmw_get_heat_grids(mmw_ctx *ctx, int32_t *n_grids /* host [S] */, mmw_heat_grid *grids /* host [S][MMW_HEAT_GRIDS_MAX] */);   /* host mirror, no device access */
int mmw_heat_sample(mmw_ctx *ctx, const int32_t *scene_flags /* dev [S] or NULL */, const double *t /* dev [S] or NULL */);
int mmw_heat_async(mmw_ctx *ctx, mmw_heat_row *rows, int32_t cap_rows, mmw_heat_cell *cells, int32_t cap_cells,
                   const int32_t *scene_flags /* dev [S] or NULL = every scene */, int32_t mode, int32_t scene_base, int32_t ticket);
int mmw_heat_wait(mmw_ctx *ctx, int32_t ticket, int32_t *n_rows, int32_t *n_cells);   /* waits for that ticket's counts only; either may be NULL */
int mmw_heat(mmw_ctx *ctx, mmw_heat_row *rows, int32_t cap_rows, mmw_heat_cell *cells, int32_t cap_cells,
             const int32_t *scene_flags, int32_t mode, int32_t scene_base, int32_t *n_rows, int32_t *n_cells);   /* async + wait */

/* Snapshot / restore of scene state (format version 1).
 *
 * A snapshot is one contiguous blob that holds the state of any subset of a context's scenes (TrackBuffer + global
 * BatchedData each) in a layout-independent, CANONICAL form: its bytes depend only on the reference-visible state, never
 * on which kernels produced it.  It can be restored into any scene slots of any context whose tracker semantics match;
 * the restored scenes then continue bit for bit as if they had never left.
 *
 *   [mmw_snapshot_header][mmw_snapshot_entry x n_scenes][section of blob scene 0][section 1] ...
 *
 * Every section starts 16-byte aligned at its entry's `offset`; sections follow each other in blob order with no gap,
 * and the last one ends at `total_bytes`.  A section holds, all little-endian, 16-byte aligned:
 *   - the scene header (64 B, MMW_SNAP_SCENE_HDR_BYTES): n_tracks, g_len, g_n[4], g_slot[4], need_db, err, db_u,
 *     next_uid, n_upd, flags -- canonical: g_slot[k] = k; need_db = db_u = n_upd = 0; flags = bits 8..15 the ring size
 *     of BatchedData.change_buffer_size (0 = FB_FRAMES_BATCH + 1), bits 16..23 two per LOGICAL frame k of the global
 *     ring (bit 16 + 2k: it holds a NaN, 17 + 2k: an infinite value), everything else 0;
 *   - n_tracks track records of MMW_SNAP_TRACK_BYTES (1496 B of state + 8 B of zeros) in effective_tracks order --
 *     canonical: ring_slot[k] = k, ring_n[k] = 0 for k >= ring_len, x / P entries beyond dim_x zero;
 *   - each track's ring frames, oldest first, min(ring_n[k], ring_rows) rows of 8 fp64 each (the rows it stores);
 *   - the global ring's frames, oldest first, g_n[k] rows of 8 fp64 each.
 * Not state (not in the blob): per-step scheduling words and lists, queue epochs and tags, statistics, profile counters,
 * the seek_inner diagnostics of mmw_get_inner.  Per-scene sites (mmw_set_sites) are not in the blob either: format version 1 is
 * unchanged, a site belongs to the slot (as an attached posture model belongs to the context) and mmw_restore leaves the
 * destination slots' sites as they are -- restored tracks arrive intact, the next frame is normalised with the destination's site.
 *
 * Ordering: mmw_snapshot / mmw_restore first wait for EVERYTHING queued on the context -- its stream and the side stream
 * of the DBSCAN chain workers, which may poll the queues for a few ms after the last step.  A caller with posture work in
 * flight on another stream (PosturePipeline) drains it first. */
#define MMW_SNAP_MAGIC "MMWSNAP"            /* 8 bytes with the terminating 0 */
#define MMW_SNAP_VERSION 1
#define MMW_SNAP_SCENE_HDR_BYTES 64
#define MMW_SNAP_TRACK_BYTES 1504
typedef struct mmw_snapshot_header {
    char magic[8];          /* MMW_SNAP_MAGIC */
    uint32_t version;       /* MMW_SNAP_VERSION */
    uint32_t header_bytes;  /* sizeof(mmw_snapshot_header) */
    uint64_t total_bytes;   /* the whole blob */
    int32_t n_scenes;       /* directory entries = sections */
    int32_t entry_bytes;    /* sizeof(mmw_snapshot_entry) */
    int32_t max_pts;        /* source context's dimensions */
    int32_t ring;
    int32_t ring_rows;
    int32_t dim_x;
    int32_t track_cap;
    int32_t reserved_;
    mmw_config config;      /* the source context's configuration, verbatim */
} mmw_snapshot_header;
typedef struct mmw_snapshot_entry {
    uint64_t offset;        /* of the section, from the blob's start (16-byte aligned) */
    uint64_t bytes;         /* of the section */
    int32_t n_tracks;
    int32_t g_len;          /* frames in the global ring */
    int32_t max_g_rows;     /* largest global-ring frame, rows */
    int32_t max_trk_rows;   /* largest track-ring frame, rows counted (ring_n; a frame stores min(ring_n, ring_rows) of them) */
    int32_t err;            /* sticky error bits (MMW_ERRBIT_*) */
    int32_t ring_size;      /* ring size of BatchedData.change_buffer_size (0 = FB_FRAMES_BATCH + 1) */
    int32_t reserved_[2];
} mmw_snapshot_entry;
typedef struct mmw_snapshot_info {
    mmw_snapshot_header header;
    const mmw_snapshot_entry *entries;   /* points into the inspected blob: [header.n_scenes] */
} mmw_snapshot_info;
/* `scenes`: host array of n distinct scene indices, NULL = all scenes in order (n is then ignored).  Blob scene i is
 * scenes[i]. */
int mmw_snapshot_size(mmw_ctx *ctx, const int32_t *scenes, int32_t n, size_t *bytes);                        /* sync */
/* writes the blob to dev_out (device memory, `cap` bytes, 16-byte aligned); *bytes = its size.  cap too small: MMW_E_ARG,
 * *bytes = the size needed, nothing written (dev_out may be NULL with cap = 0: one call that only sizes). */
int mmw_snapshot(mmw_ctx *ctx, const int32_t *scenes, int32_t n, void *dev_out, size_t cap, size_t *bytes);  /* sync */
/* blob scene i -> scene scenes[i] of this context (NULL: scene i; n must equal the blob's scene count otherwise).  Refused
 * with MMW_E_ARG before any device write (no scene changes) when: magic, version, sizes or offsets are bad; an index is
 * duplicated or out of range; any mmw_config field differs from this context's bit for bit other than track_cap,
 * ring_rows, kalman_dense_min_units, chain_side_stream, fused_step and reserved_; a scene's frames do not fit this
 * context's max_pts / ring_rows (a track frame the source stored truncated needs the same ring_rows); a scene holds more
 * tracks than this context's track_cap.  Restored scenes take their tracks from their header at the next step. */
int mmw_restore(mmw_ctx *ctx, const void *dev_blob, size_t bytes, const int32_t *scenes, int32_t n);        /* sync */
/* host only, no device: validates a blob's header and directory (the same checks as mmw_restore's, short of the target
 * context's) and describes it.  MMW_E_ARG + mmw_last_error(NULL) when it is malformed. */
int mmw_snapshot_inspect(const void *host_blob, size_t bytes, mmw_snapshot_info *out);

/* Kernel timing with hipEvents on the context's stream (bench.py roofline).
 * ids: 0 k_track (association + DBSCAN cell-count screen), 1 k_dbscan_big (BallTree DBSCAN of large clouds), 2 features,
 * 3 normalize, 4 table, 5 k_predict, 6 k_post (Kalman update + BallTree DBSCAN of small clouds). */
#define MMW_K_TRACK 0
#define MMW_K_DBSCAN 1
#define MMW_K_FEATURES 2
#define MMW_K_NORMALIZE 3
#define MMW_K_TABLE 4
#define MMW_K_PREDICT 5
#define MMW_K_POST 6
#define MMW_K_COUNT 7
/* The two Conv3D(3x3x3, same, relu) layers of define_CNN_3D (train.py:73-82) fused on the fp32 matrix
 * cores, on the current device and the given hipStream_t (NULL = default stream).  All dev pointers:
 *   feat[n][3][8][8][5]   channels-last input (what mmw_features writes)
 *   w1[3][3][3][5][16], b1[16], w2[3][3][3][16][32], b2[32]   Keras kernel layout (kd,kh,kw,in,out)
 *   out[n][3][8][8][32]   = Keras Flatten order (d,h,w,c): feed Dense-1 with Keras' weight rows. */
int mmw_mars_conv3d(void *hip_stream, const float *feat, const float *w1, const float *b1, const float *w2, const float *b2,
                    float *out, int32_t n);
/* The two Conv2D(3x3, same, relu) layers of the single-frame model define_CNN (train.py:35-44) the same way (k_mars2d.hip: fp32
 * matrix cores, fp32 throughout, the intermediate activation never leaves LDS; NaN stays NaN through the ReLUs, as Keras'):
 *   feat[n][8][8][5]   channels-last input (what mmw_features writes when FB_FRAMES_BATCH == 0)
 *   w1[3][3][5][16], b1[16], w2[3][3][16][32], b2[32]   Keras kernel layout (kh,kw,in,out)
 *   out[n][8][8][32]   = Keras Flatten order (h,w,c): feed Dense-1 with Keras' weight rows.
 * A sample only feeds its own rows of out, in an arithmetic that does not depend on n; rows past n are not written. */
int mmw_mars_conv2d(void *hip_stream, const float *feat, const float *w1, const float *b1, const float *w2, const float *b2,
                    float *out, int32_t n);

/* The two convolution layers on the fp16 matrix cores, fp32-exact by operand splitting: every fp32 value a (inputs,
 * weights, activations) is carried as hi = fp16(a), lo' = fp16((a - hi) * 2^11) and a product a.w accumulates in fp32 as
 * hi.hi + 2^-11 (hi.lo' + lo'.hi): three exact fp16 products per term, the dropped lo'.lo' term 2^-22 relative --
 * measured closer to the fp64 oracle than the fp32 kernel above.  frames = 3: define_CNN_3D's Conv3D pair
 * (train.py:73-82), feat[n][3][8][8][5], kernels (kd,kh,kw,in,out); frames = 1: define_CNN's Conv2D pair
 * (train.py:35-44), feat[n][8][8][5], kernels (kh,kw,in,out).  The activation leaves the kernel already split, for a
 * Dense-1 of the same form: out16[n][ld_out] fp16, ld_out >= 2 * frames * 2048; value j of Keras' Flatten order has its
 * hi half at (j / 32) * 64 + j % 32 and its lo' half 32 further -- runs of [hi 32 | lo' 32], one 128-byte line per
 * 32-deep step of Dense-1.  The split is exact inside fp16's range only: range_flag (device pointer, may be NULL) gets
 * bit 0 set when an input or an activation of magnitude >= 65 504 (or a non-finite input) was split -- that sample's
 * outputs are then meaningless, where Keras' fp32 would have been finite; nothing clears it but the caller. */
int mmw_mars_conv_split(void *hip_stream, int32_t frames, const float *feat, const float *w1, const float *b1, const float *w2,
                        const float *b2, void *out16, int64_t ld_out, int32_t n, int32_t *range_flag, int32_t *sample_flags);
/* ... per sample: sample_flags (device int32[2 + MMW_RANGE_FIXUP_CAP], may be NULL; zero it once) is the fix-up list: [0] counts
 * the samples whose input or activations left fp16's range (running, atomic), [2 ..] are the indices of the first
 * MMW_RANGE_FIXUP_CAP of them, in any order.
 * mmw_mars_range_fixup recomputes exactly those samples in Keras' own fp32 arithmetic and overwrites their rows of kp[n][57] --
 * all on the device and the given stream, no host wait: the listed samples' feature tensors are copied, run through the fp32
 * conv pair (mmw_mars_conv3d's kernel) and the thin Dense-1 / Dense-2 kernels of mmw_mars_head_small with a row count only the
 * device knows (workgroups past it leave at once: a frame without such samples pays four empty launches), and scattered back;
 * the list is emptied for the next call ([1] = the number taken).  More than MMW_RANGE_FIXUP_CAP flagged samples in one call:
 * bit 1 of *range_flag is raised and the surplus keeps its meaningless rows.
 * define_CNN_3D only (feat[n][3][8][8][5]); cw1 / cb1 / cw2 / cb2 = the conv kernels in Keras layout (fp32), w1[1536][ldw] /
 * bias1 / w2[57][1536] / bias2 as for mmw_mars_head_small; scratch = MMW_RANGE_FIXUP_SCRATCH bytes of device memory.
 * mmw_mars_range_fixup_frames is the same for either model: frames = 3 IS mmw_mars_range_fixup; frames = 1 repairs define_CNN's
 * samples (feat[n][8][8][5], the list of mmw_mars_conv_split(frames = 1)) with mmw_mars_conv2d's kernel, conv kernels (kh,kw,in,out),
 * w1[512][ldw] with ldw >= 2048, w2[57][512]; the same scratch size (the single-frame chain fits inside it).  Other frames: MMW_E_ARG. */
#define MMW_RANGE_FIXUP_CAP 64
#define MMW_RANGE_FIXUP_SCRATCH (512 + 64 * (960 + 6144 + 1536 + 57) * 4)
int mmw_mars_range_fixup(void *hip_stream, const float *feat, int32_t *sample_flags, int32_t n, const float *cw1, const float *cb1,
                         const float *cw2, const float *cb2, const float *w1, int64_t ldw, const float *bias1, const float *w2, const float *bias2,
                         void *scratch, float *kp, int32_t *range_flag);
int mmw_mars_range_fixup_frames(void *hip_stream, int32_t frames, const float *feat, int32_t *sample_flags, int32_t n, const float *cw1,
                                const float *cb1, const float *cw2, const float *cb2, const float *w1, int64_t ldw, const float *bias1,
                                const float *w2, const float *bias2, void *scratch, float *kp, int32_t *range_flag);
/* Dense-1 of the MARS CNN (train.py:49,87: Dense(512 k, relu); BatchNormalization folded in) on split-fp16 operands, one
 * kernel: out = relu(bias + hi . W_hi + 2^-11 (hi . W_lo' + lo' . W_hi)), fp32 accumulation and output (k_dense.hip).
 * a2 [rows_padded][lda] fp16 as mmw_mars_conv_split writes it; w2 [n][ldw] fp16 = the transposed weights (K contiguous)
 * split and interleaved the same way; bias [n], out [rows_padded][n] fp32.  rows_padded is a multiple of 256 (rows past
 * the batch may hold anything: a row only feeds its own output row), k of 32, n of 128; lda, ldw >= 2 k.  hip_stream as above. */
int mmw_mars_dense1_split(void *hip_stream, const void *a2, int64_t lda, const void *w2, int64_t ldw, const float *bias, float *out,
                          int32_t rows_padded, int32_t k, int32_t n);

/* The tile plan mmw_mars_dense1_split runs for (rows_padded, n) on the current device, host queries only (no GPU work):
 * out[0] = bands of 256 rows computed as 256 x 192 tiles (n a multiple of 192), out[1] = bands as 256 x 128 tiles, out[2] = bands
 * as 128 x 128 half tiles (the tail of the tile list: rows from (out[0] + out[1]) * 256 on), out[3] = the CU count behind the
 * split.  out[0] + out[1] + out[2] = rows_padded / 256 and one of out[0], out[1] is 0; the grids are out[0] * (n / 192),
 * out[1] * (n / 128) and 2 * out[2] * (n / 128) workgroups.  The results of mmw_mars_dense1_split do not depend on the plan. */
int mmw_mars_dense1_plan(int32_t rows_padded, int32_t n, int32_t out[4]);

/* Dense-2 of the MARS CNN at any batch size (train.py:92: Dense(57); BatchNormalization folded in), one kernel on the fp32 matrix
 * cores: kp[n_rows][57] = bias2 + hidden[n_rows][ldh] . w2[57][k]^T, fp32 fused multiply-adds in a summation order that is fixed per
 * output (the same for every row, batch size and run), fp32 out.  `hidden` is read once with 16-byte loads; rows past n_rows are
 * neither read nor written; a row only feeds its own output row.  All dev pointers; hidden and w2 16-byte aligned, k and ldh
 * multiples of 4, ldh >= k (k = 1536 for the 3-frame model, 512 for the single-frame one).  hip_stream as above. */
int mmw_mars_dense2(void *hip_stream, const float *hidden, int64_t ldh, const float *w2, const float *bias2, float *kp, int32_t n_rows,
                    int32_t k);
/* The split-fp16 operand of mmw_mars_dense1_split from fp32 weights, on the device (what mars.interleave_split builds with torch,
 * bit for bit): w[n][ldw] fp32 (K contiguous) -> w16[n][ld16] fp16, every value a carried as hi = fp16(a), lo' = fp16((a - hi) * 2^11)
 * in runs of [hi 32 | lo' 32].  k a multiple of 32, ldw >= k a multiple of 4, ld16 >= 2 k a multiple of 8, both 16-byte aligned.
 * range_flag (device pointer, may be NULL) gets bit 0 set when a value is not finite or of magnitude >= 65 504: the split is exact
 * inside fp16's range only; nothing clears it but the caller. */
int mmw_mars_split_weights(void *hip_stream, const float *w, int64_t ldw, void *w16, int64_t ld16, int32_t n, int32_t k, int32_t *range_flag);

/* The head of the MARS CNN for a SMALL batch (n_rows <= 64: one scene's tracks, TrackBuffer.estimate_posture of the offline
 * loop): Dense-1 + ReLU (train.py:49,87) and Dense-2 (train.py:54,92), both with their BatchNormalization folded in, in fp32
 * fused multiply-adds -- Keras' own arithmetic.  The weight matrix is cut along the features over the whole chip (a tile kernel
 * would stream it through one band of eight workgroups).  act[n_rows][lda] fp32 = the conv pair's output in Keras' Flatten
 * order (mmw_mars_conv3d, mmw_mars_conv2d); w1[n1][ldw] fp32 = Dense-1's weights transposed (K contiguous), bias1[n1]; w2[57][n1], bias2[57];
 * hidden[n_rows][n1] scratch; kp[n_rows][57].  All dev pointers, 16-byte aligned; k, lda, ldw multiples of 4. */
int mmw_mars_head_small(void *hip_stream, const float *act, int64_t lda, const float *w1, int64_t ldw, const float *bias1, const float *w2,
                        const float *bias2, float *hidden, float *kp, int32_t n_rows, int32_t k, int32_t n1);

/* ReadIWR14xx.read (ReadDataIWR1443.py:27-201) on a byte buffer, host only (no context, no GPU work): the input
 * step before mmw_normalize.  Looks for the LAST 8-byte magic word 02 01 04 03 06 05 08 07 in buf[0 .. len-8),
 * needs more than 16 bytes from there and at least totalPacketLen of them (little-endian u32 at offset 12; any value,
 * 0 included: the packet is complete and decoded all the same, as there).  If the header announces objects and the
 * first TLV is MMWDEMO_UART_MSG_DETECTED_POINTS (type 1), the objects (u16 count, u16 Q format, then int16 rangeIdx,
 * dopplerIdx, peakVal, x, y, z each) become raw[n][5] = (x, y, z, doppler, peakVal) -- the row layout mmw_normalize
 * takes -- with x, y, z divided by the reference's numpy-int64 `2 ** Q` (2^Q for Q <= 62, -2^63 for Q = 63, 0 for
 * Q >= 64: +-inf / NaN), doppler = dopplerIdx * doppler_resolution_mps after the reference's wrap of indices above
 * num_doppler_bins/2 - 1 (it subtracts 65535, in int16), and range_out[n] = rangeIdx * range_idx_to_meters (may be NULL).
 * cap >= len is the size of the caller's buffer: the header words, TLV head and objects the packet announces are read
 * wherever they lie in buf[0 .. cap) -- past len they are what the buffer still holds there, the reference's stale
 * bytes (a caller that keeps the reference's buffer moves the packet to buf[0] before the decode that counts) --;
 * one that reaches past cap gives MMW_E_CAPACITY (the reference raises ValueError).
 * Returns MMW_UART_POINTS (points parsed, *n_obj of them), MMW_UART_PACKET (a complete packet without: no objects
 * announced, or another TLV first), MMW_UART_NONE (no complete packet), MMW_E_ARG (bad arguments, or more than max_obj
 * objects, which the reference decodes) or MMW_E_CAPACITY.  *packet_start = the magic word (0 when there is none),
 * *packet_len = totalPacketLen (0 unless complete) tell the caller what to drop from its buffer. */
#define MMW_UART_NONE 0
#define MMW_UART_POINTS 1
#define MMW_UART_PACKET 2
typedef struct mmw_uart_cfg {
    double range_idx_to_meters;
    double doppler_resolution_mps;
    int32_t num_doppler_bins;
    int32_t reserved;
} mmw_uart_cfg;
int mmw_parse_uart_cap(const uint8_t *buf, size_t len, size_t cap, const mmw_uart_cfg *cfg, double *raw /*[max_obj][5]*/,
                       double *range_out /*[max_obj]*/, int32_t max_obj, int32_t *n_obj, uint32_t *frame_number, size_t *packet_start,
                       size_t *packet_len);
/* The first form, kept for its callers: mmw_parse_uart_cap with cap = len (nothing past len is read), returning 1 for
 * MMW_UART_POINTS, MMW_E_ARG as it does and 0 otherwise (no complete packet, one without points, or one whose words reach
 * past len).  Its *packet_len = 0 cannot tell "incomplete" from a packet that declares totalPacketLen 0: use the _cap form. */
int mmw_parse_uart(const uint8_t *buf, size_t len, const mmw_uart_cfg *cfg, double *raw /*[max_obj][5]*/, double *range_out /*[max_obj]*/,
                   int32_t max_obj, int32_t *n_obj, uint32_t *frame_number, size_t *packet_start, size_t *packet_len);

/* The batched, device-side form of that input step: the host only FINDS the packet, the GPU decodes it.
 * mmw_find_tlv (host, no GPU work) = the packet part of mmw_parse_uart_cap with cap = len -- it has no buffer history, so
 * nothing past len is read -- without decoding an object: returns 1 with *body_offset = offset from buf of the TLV BODY (u16
 * numObj, u16 xyzQFormat, numObj x six int16: rangeIdx, dopplerIdx, peakVal, x, y, z; 12 bytes per object,
 * ReadDataIWR1443.py:107-150) and *n_obj = the count it announces (the caller checks it against max_pts) when the header, the
 * body and every object it announces lie in buf[0 .. len); 0 otherwise (*body_offset = -1) -- a complete packet whose words
 * reach past len, where the reference would read stale bytes of its buffer, is refused --; MMW_E_ARG for bad arguments.
 * The packet position as mmw_parse_uart_cap gives it.
 * mmw_normalize_tlv = ReadIWR14xx.read's decode (ReadDataIWR1443.py:153-171) + Utils.normalize_data (Utils.py:342-434) for
 * every scene in ONE kernel, fused ahead of mmw_step: packets (dev) = the bytes as they arrived, all scenes' packets in one
 * buffer; tlv_offset[S] (dev) = byte offset into `packets` of each scene's TLV body (2-byte aligned), < 0 = no detected-points
 * TLV this frame (n_out = 0: mmw_step skips the scene's frame, offline_main.py:56); cfg (host) as for mmw_parse_uart_cap;
 * pts[S][max_pts][8] / n_out[S] (dev) as mmw_normalize writes them -- bit-equal to mmw_parse_uart_cap + mmw_normalize on the same
 * bytes, the Q format rule included.  12 bytes per object cross PCIe instead of 20 (fp32 raw rows) or 40 (fp64).
 * packets_bytes = the size of `packets`: nothing outside it is read, whatever the offset (INT64_MAX included).  A body that
 * does not lie inside it on a 2-byte boundary with every object it announces, or that announces more than max_pts objects
 * (mmw_parse_uart returns MMW_E_ARG for those bytes), gives n_out = MMW_BAD_FRAME: the mmw_step that follows raises the
 * scene's bad-count bit (MMW_E_ARG), the other scenes are unaffected. */
#define MMW_BAD_FRAME (-3)
int mmw_find_tlv(const uint8_t *buf, size_t len, int64_t *body_offset, int32_t *n_obj, uint32_t *frame_number, size_t *packet_start,
                 size_t *packet_len);
int mmw_normalize_tlv(mmw_ctx *ctx, const uint8_t *packets, size_t packets_bytes, const int64_t *tlv_offset, const mmw_uart_cfg *cfg, double *pts,
                      int32_t *n_out);

/* Device-resident radar readers: ReadIWR14xx.read (ReadDataIWR1443.py:27-201) + Utils.normalize_data for EVERY scene in one
 * kernel, the first line of the online loop (`dataOk, _, detObj = IWR1443.read()`, main.py:42) included.  Each scene owns
 * what a ReadIWR14xx object keeps between two calls -- the 2^15-byte byteBuffer (zeroed at open, stale bytes and all) and
 * byteBufferLength -- and main.py's `t` (44-47), on the device; the host ships whatever bytes arrived and reads nothing back.
 * mmw_uart_open: cfg[n_cfg] (host), n_cfg = 1 (every scene) or n_scenes; buffers zeroed, lengths 0, t_last = t0
 * (Tracking.py:511).  On the context's stream; calling it again replaces the state.  mmw_uart_close frees it.
 * mmw_uart_read (asynchronous, on the context's stream): chunks (dev, 4-byte aligned) = all scenes' new bytes in one buffer
 * of chunks_bytes bytes, read in whole aligned 4-byte words that hold a byte of a scene's chunk; chunk_off[S + 1] (dev) =
 * scene s's chunk is chunks[chunk_off[s] .. chunk_off[s + 1]); scene_flags[S] (dev; NULL = every scene) = the scenes that
 * read; now = the time of this call.  Every flagged scene performs exactly ONE read() with its chunk as what the port
 * delivered (an empty chunk is still a read): append if byteBufferLength + count < 2^15, cut to the LAST magic word, decode
 * one complete packet -- objects are read wherever they lie in the 2^15 bytes, past byteBufferLength they are the buffer's
 * stale bytes --, drop totalPacketLen bytes.  On dataOK the rows are normalised with the scene's mounting (its site while
 * mmw_set_sites is in use): pts[S][max_pts][8] / n_out[S] (dev) as mmw_normalize_tlv writes them, bit-equal to it on the same
 * body.  dt_out[S] (dev): on MMW_UART_POINTS now - t_last (one fp64 subtraction, main.py:45-47), and t_last = now; otherwise 0
 * and t_last stays.  n_out = 0 makes mmw_step skip the scene (main.py:44,52).  frame_number[S] (dev): the header's, 0 without
 * a complete packet.  status[S] (dev), low byte:
 *   MMW_UART_NONE / MMW_UART_POINTS / MMW_UART_PACKET  as mmw_parse_uart_cap
 *   MMW_UART_OVERFLOW  more than max_pts objects announced, which the reference decodes: the buffer is handled exactly as the
 *                      reference handles the decoded packet, the drop included; n_out = MMW_BAD_FRAME.  The ONE declared
 *                      difference of this path (radar.UartFrameParser differs from it: it raises and leaves the packet in place)
 *   MMW_UART_RAISED    the announced objects reach past byte 2^15 (mmw_parse_uart_cap: MMW_E_CAPACITY), where the reference
 *                      raises ValueError; takes precedence over OVERFLOW.  The state is as the exception leaves it: cut done,
 *                      nothing dropped.  n_out = 0, frame_number = 0
 *   MMW_UART_SKIPPED   the scene was not flagged: nothing of it is touched.  n_out = 0
 *   MMW_UART_BADCHUNK  chunk_off[s] < 0, chunk_off[s + 1] < chunk_off[s] or chunk_off[s + 1] > chunks_bytes (compared without
 *                      adding to an offset): no read() happens, the state is untouched, the other scenes are unaffected.  n_out = 0
 * bit 8, MMW_UART_CHUNK_DROPPED: the chunk did not fit (byteBufferLength + count >= 2^15) and was discarded, as there.
 * mmw_uart_get_state / mmw_uart_set_state (sync): one scene's whole byteBuffer (all 2^15 bytes), byteBufferLength
 * (0 .. 2^15 - 1) and t_last -- for tests, and to move a scene between contexts.  mmw_uart_set_time (sync): t_last = t for the
 * scenes flagged in scene_flags[S] (HOST; NULL = every scene), e.g. after mmw_reset_scenes.
 * The readers are no part of a scene's tracker state (the reference keeps them in another object): mmw_reset*, mmw_restore
 * and mmw_clear_sites leave them alone, snapshots do not hold them.  MMW_E_ARG (nothing touched) before mmw_uart_open or for
 * a NULL argument other than scene_flags. */
#define MMW_UART_OVERFLOW 3
#define MMW_UART_RAISED 4
#define MMW_UART_SKIPPED 5
#define MMW_UART_BADCHUNK 6
#define MMW_UART_CHUNK_DROPPED 256
#define MMW_UART_BUFFER 32768
int mmw_uart_open(mmw_ctx *ctx, const mmw_uart_cfg *cfg, int32_t n_cfg, double t0);
int mmw_uart_close(mmw_ctx *ctx);
int mmw_uart_read(mmw_ctx *ctx, const uint8_t *chunks, const int64_t *chunk_off, size_t chunks_bytes, const int32_t *scene_flags, double now,
                  double *pts, int32_t *n_out, double *dt_out, int32_t *status, uint32_t *frame_number);
int mmw_uart_get_state(mmw_ctx *ctx, int32_t scene, uint8_t *buf /*[MMW_UART_BUFFER]*/, int32_t *len, double *t_last);
int mmw_uart_set_state(mmw_ctx *ctx, int32_t scene, const uint8_t *buf /*[MMW_UART_BUFFER]*/, int32_t len, double t_last);
int mmw_uart_set_time(mmw_ctx *ctx, const int32_t *scene_flags, double t);

/* ---- radar log ----
 * What the readers decoded, as it came off the wire: the recorder's `dataOk, frameNumber, detObj = IWR1443.read()`
 * (DataLogging.py:30-38) for every scene in ONE call, taken from the SAME read that fed the tracker -- not from a second
 * parser on the host.  mmw_uart_log_enable(on != 0), after mmw_uart_open (before it: MMW_E_ARG): from then on mmw_uart_read
 * launches the logging twins of its kernels, which also keep each scene's last decoded frame (MMW_UART_POINTS) on the device:
 * its wire objects, frameNumber, the Q format and the `now` of that read.  Every other status leaves the scene's staged frame
 * alone; MMW_UART_OVERFLOW and MMW_UART_RAISED log nothing (the readers' declared difference).  A second read before the
 * export OVERWRITES the first frame: call mmw_uart_log after every mmw_uart_read.  on = 0 frees the log, and the context
 * launches exactly what it launched before; a context that never enables it never launches anything else.
 *
 * Output: a DIRECTORY of one mmw_uart_frame per emitted scene, scenes ascending, and their objects back to back -- entry i
 * owns rows[first .. first + count); the entries partition rows, as in mmw_clouds.  A scene is ASKED when scene_flags (dev [S])
 * is NULL or its flag is non-zero; an asked scene with a frame not exported yet and frame_number % frame_select == 0 (unsigned;
 * read_thread's FB_FRAMES_SKIP + 1; frame_select < 1 is MMW_E_ARG) is EMITTED.  count = 0 is a valid entry (dataOK with
 * tlv_numObj = 0).  A row is the reference's detObj bit for bit: x, y, z = int16 / 2 ** xyzQFormat (numpy's int64 power: inf
 * and NaN for Q >= 63 pass through), doppler and peak_val as mmw_parse_uart_cap gives them, range = rangeIdx * the scene's
 * range_idx_to_meters.  t is the `now` of the read that decoded the frame; the reference's detObj["timestamp"] is
 * round(t * 1000), which the host forms.
 * Consumed once: a successful call marks the frame of every ASKED scene exported, emitted or filtered out by frame_select;
 * scenes not asked keep theirs for a later call.
 * Capacity is decided on the DEVICE, as the clouds': more entries than cap_frames or more objects than cap_rows -> nothing is
 * written, no frame is consumed, and mmw_uart_log_wait returns MMW_E_CAPACITY with both counts needed: a retry loses nothing.
 * Tickets as mmw_clouds_* (ticket in [0,4); ticket 3 is mmw_uart_log's own).  dir: dev pointer, 8-byte aligned; rows: dev
 * pointer, 16-byte aligned; scene ids are offset by scene_base.  MMW_E_ARG, nothing touched: a NULL context, the log not
 * enabled, a NULL buffer with a positive cap, a negative cap, frame_select < 1, a bad ticket, a misaligned buffer, a wait for
 * a ticket with nothing outstanding.
 * Life cycle: mmw_uart_open called again marks every staged frame exported; mmw_uart_close and mmw_destroy free the log;
 * mmw_reset*, mmw_restore, mmw_uart_set_state and mmw_uart_set_time do not touch it. */
typedef struct mmw_uart_frame {      /* 32 bytes: one directory entry */
    int32_t scene;          /* global scene id (scene_base + local index) */
    uint32_t frame_number;  /* the packet header's frameNumber */
    int32_t first, count;   /* this frame's objects are rows[first .. first + count) */
    double t;               /* `now` of the mmw_uart_read that decoded it */
    int32_t q_format;       /* xyzQFormat as sent (u16) */
    int32_t reserved_;
} mmw_uart_frame;
typedef struct mmw_uart_object { double x, y, z, doppler, peak_val, range; } mmw_uart_object;   /* 48 bytes: one detObj row */
int mmw_uart_log_enable(mmw_ctx *ctx, int32_t on);
int mmw_uart_log_async(mmw_ctx *ctx, mmw_uart_frame *dir, int32_t cap_frames, mmw_uart_object *rows, int32_t cap_rows,
                       const int32_t *scene_flags /*dev [S] or NULL*/, int32_t frame_select, int32_t scene_base, int32_t ticket);
int mmw_uart_log_wait(mmw_ctx *ctx, int32_t ticket, int32_t *n_frames, int32_t *n_rows);   /* waits for that ticket's counts only; either may be NULL */
int mmw_uart_log(mmw_ctx *ctx, mmw_uart_frame *dir, int32_t cap_frames, mmw_uart_object *rows, int32_t cap_rows,
                 const int32_t *scene_flags /*dev [S] or NULL*/, int32_t frame_select, int32_t scene_base, int32_t *n_frames,
                 int32_t *n_rows);                                                          /* async + wait */

/* ---- training samples ----
 * The dataset side: what preprocessing.py:192-220 saves of a scene after its track(), for every scene in ONE call.  A scene gives
 * a SAMPLE when effective_tracks is not empty, effective_tracks[0].lifetime == 0 (the frame updated it) and its
 * batch.effective_data is not empty.  The sample is that track's ring, `frames = list(track.batch.buffer)`, made relative with
 * relative_coordinates(frames, track.cluster.centroid) (Utils.py:437-465: centroid[0], centroid[1] subtracted from columns 0, 1 in
 * fp64) and laid out by format_batched_frames (Utils.py:523-548): frames NEWEST first, of each its columns [0, 1, 2, 6, 7], cut to
 * its first 64 rows or padded to 64 with true zero rows (pad rows are not shifted); a frame the ring does not hold yet is 64 zero rows.
 *
 * Output: a DIRECTORY of one mmw_sample_entry per sample, scenes ascending, and out[i] = the block of entry i.
 * mode: MMW_SAMPLE_BLOCK writes double[192][5], the block bit for bit.  MMW_SAMPLE_INPUT writes float[8][8][5], what
 * format_mmwave_to_npy makes of it -- format_single_frame_mode(np.float32(block), mean, std, 1, fuse=True), Utils.py:551-572 --:
 * rows 0..63 (the newest frame), every value rounded once to fp32, intensity (I - f32(mean)) / f32(std) as two fp32 operations,
 * rows that are all zero AFTER that moved behind the others as true zero rows, then sorted by fp32 x.  np.argsort leaves ties
 * undefined; here they are ordered by (is-all-zero, row position), a stable sort of the reference's array.  mean / std: the
 * scene's site while a site table is in use (mmw_set_sites), else the context's.  | MMW_SAMPLE_ABSOLUTE: no centroid
 * subtraction, in either form (the reference's RELATIVE_ENABLED = False); the entry's centroid is filled in all the same.
 *
 * A scene is ASKED when scene_flags (dev [S]) is NULL or its flag is non-zero: pass the scenes that ran track() this frame -- the
 * library keeps nothing between calls, and a skipped scene whose position-0 track still has lifetime 0 gives its sample again
 * when asked.  A context whose ring holds more than 3 frames (fb_frames_batch > 2) is refused with MMW_E_ARG: the reference
 * raises there, frame 3 does not fit the 3 x 64 block.
 * Capacity is decided on the DEVICE, as the clouds': more samples than cap_samples -> neither buffer is written and
 * mmw_samples_wait returns MMW_E_CAPACITY with the count needed.  Tickets as mmw_clouds_* (ticket in [0,4); ticket 3 is
 * mmw_samples' own).  No enable call: the first call allocates the context's scratch, mmw_destroy frees it.  dir: dev pointer,
 * 8-byte aligned; out: dev pointer, 16-byte aligned, cap_samples blocks; scene ids are offset by scene_base.  MMW_E_ARG, nothing
 * touched: a NULL context, a NULL buffer with a positive cap, a negative cap, a mode outside {0, 1, 2, 3}, a bad ticket, a
 * misaligned buffer, a ring of more than 3 frames, a wait for a ticket with nothing outstanding. */
typedef struct mmw_sample_entry {    /* 48 bytes, no padding: one directory entry */
    int32_t scene;          /* global scene id (scene_base + local index) */
    int32_t uid;            /* mmw_track_record.uid of effective_tracks[0] */
    int32_t frames;         /* len(track.batch.buffer): 1..3 */
    int32_t reserved;       /* 0 */
    int32_t rows[3];        /* rows the reference holds in each frame, newest first (0 = absent) */
    int32_t cut;            /* rows beyond 64, summed over the frames: what the block leaves out */
    double centroid[2];     /* track.cluster.centroid[:2] */
} mmw_sample_entry;
#define MMW_SAMPLE_BLOCK 0      /* out = double[n][192][5] */
#define MMW_SAMPLE_INPUT 1      /* out = float[n][8][8][5] */
#define MMW_SAMPLE_ABSOLUTE 2   /* flag bit: no centroid subtraction */
int mmw_samples_async(mmw_ctx *ctx, mmw_sample_entry *dir, int32_t cap_samples, void *out, int32_t mode,
                      const int32_t *scene_flags /*dev [S] or NULL*/, int32_t scene_base, int32_t ticket);
int mmw_samples_wait(mmw_ctx *ctx, int32_t ticket, int32_t *n_samples);   /* waits for that ticket's count only; n_samples may be NULL */
int mmw_samples(mmw_ctx *ctx, mmw_sample_entry *dir, int32_t cap_samples, void *out, int32_t mode,
                const int32_t *scene_flags /*dev [S] or NULL*/, int32_t scene_base, int32_t *n_samples);   /* async + wait */

/* Work counters accumulated by the kernels since the last reset (sync):
 * [0] k_track algorithmic bytes  [1] k_dbscan algorithmic bytes  [2] scene-frames stepped
 * [3] apply_DBscan calls  [4] sum of U over those calls  [5] sum of tracks entering track()
 * [6] gate evaluations (points x tracks)  [7] clusters found.  Definitions: DESIGN.md §4. */
int mmw_stats_get(mmw_ctx *ctx, uint64_t *out /*[8]*/);
int mmw_stats_reset(mmw_ctx *ctx);
/* Are the chain workers in use?  0 = no (not configured, seek_inner, or the side streams turned out to share a hardware
 * queue with the context's stream: checked by the first mmw_step after mmw_create / mmw_set_stream /
 * mmw_set_chain_side_stream), 1 = yes, 2 = configured, not checked yet (no step since). */
int mmw_side_workers(mmw_ctx *ctx);
/* Do kernels queued on stream_b run while a kernel on stream_a is still running?  1 = yes, 0 = no: the HIP runtime multiplexes
 * streams onto a few hardware queues (GPU_MAX_HW_QUEUES, 4 by default, dealt round-robin at stream creation), and two streams
 * that share one execute in order.  Callers that overlap their own work with the context's (the CNN beside the tracker:
 * posture.PosturePipeline) pick their second stream with this.  Synchronises both streams; ~20 us when they are independent. */
int mmw_streams_concurrent(mmw_ctx *ctx, void *stream_a, void *stream_b);
/* Which kernels the next mmw_step launches for TrackBuffer.track (Tracking.py:683-703): 1 = the one-workgroup step (k_scene: a
 * scene's whole track() in one workgroup, then the DBSCAN worker blocks of k_post; contexts whose scenes are all resident at
 * once, mmw_config.fused_step), 2 = two launches (k_track with _predict_all at its head, k_post), 4 = the bulk kernels
 * (k_predict, k_track, k_post, k_dbscan_big).  The results do not depend on it. */
int mmw_step_kind(mmw_ctx *ctx);
/* How the batched Kalman kernels of the bulk step (k_predict, the update half of k_post) are laid out -- mmw_config.
 * kalman_dense_min_units: 1 = over the TRACKS of the context (four per wave, from the update lists k_track builds), 0 = per
 * scene (also: always with seek_inner, with track_cap > 63 and in the one-workgroup step).  The results do not depend on
 * it; the parity tests assert that the layout they asked for is the one that ran. */
int mmw_kalman_layout(mmw_ctx *ctx);
/* Diagnostic: the queue of scenes whose small-cloud DBSCAN k_track could not rule out (k_dbscan.hip), per step parity p:
 * [8p] pushed, [8p+1] claimed, [8p+2] finished this step; [3] last step whose k_post has begun, [4] waits given up (also
 * reported by mmw_check); [16 + 8p ...] the same three words for the queue of the clouds of more than 256 points.
 * Sync; does not wait for the context's stream. */
int mmw_diag_queue(mmw_ctx *ctx, int32_t *out /*[32]*/);
/* [0..7] as mmw_stats_get; [8..29] per-phase cycle sums, non-zero only in the diagnostic build
 * (make -C mmwave_msc_amd/csrc STAMPS=1), see scripts/phase_stamps.py; [30] k_features algorithmic bytes (ring rows
 * read + fp32 tensors written)  [31] feature tensors written. */
int mmw_stats_get_ext(mmw_ctx *ctx, uint64_t *out /*[32]*/);
/* on = 0: off; 1: every kernel id; otherwise a mask, bit (k + 1) selects kernel id k.  Does not synchronise. */
int mmw_profile_enable(mmw_ctx *ctx, int32_t on);
int mmw_profile_reset(mmw_ctx *ctx);
int mmw_profile_get(mmw_ctx *ctx, int32_t kernel_id, double *total_ms, int64_t *launches);   /* sync */
const char *mmw_kernel_name(int32_t kernel_id);
/* "mmw-hip <version> (gfx950) src:<hash>": <hash> = first 16 hex digits of the SHA-256 over csrc/ and
 * this header at build time (csrc/Makefile); the Python loader refuses a library built from other sources. */
const char *mmw_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MMW_H */
