// api_query.hip -- the C-ABI (include/mmw.h): reading a context.  Error checks, track counts and records, ring frames, the
// track table, the counters, per-kernel profiling and the diagnostics.
#include "mmw_ctx.hpp"
#include "mmw_kalman.hpp"

int read_headers(mmw_ctx *c, std::vector<SceneHdr> &h)
{
    HIPCHK(c, hipSetDevice(c->device));
    h.resize(c->dc.n_scenes);
    return d2h_after_kernels(c, h.data(), c->st.hdr, h.size() * sizeof(SceneHdr));
}

// the first per-scene error of a header read-back (as mmw_check reports it), or a chain worker's give-up
int first_scene_error(mmw_ctx *c, const SceneHdr *h, size_t n, const int32_t *q)
{
    for (size_t s = 0; s < n; s++) {
        const int e = h[s].err;
        if (!e) continue;
        if (e & ERR_BADCOUNT) return fail(c, MMW_E_ARG, "scene %zu: n_pts outside [0, max_pts=%d]", s, c->dc.max_pts);
        if (e & ERR_CAPACITY) return fail(c, MMW_E_CAPACITY, "scene %zu: more tracks than track_cap=%d", s, c->dc.t_cap);
        // (a zero denominator leaves inf / NaN in the track's state, which the next frames' 6x6 inversions then report as
        //  singular: when both bits are set the division came first -- as the reference's ZeroDivisionError would have)
        if (e & ERR_DIVZERO) return fail(c, MMW_E_DIVZERO, "scene %zu: (N_est-1)*N == 0 in _get_Rc / N_est == 0", s);
        if (e & ERR_SINGULAR) return fail(c, MMW_E_SINGULAR, "scene %zu: singular 6x6 gate/innovation matrix", s);
        // (the last thing track() can raise in a frame: sklearn's input validation in apply_DBscan, Utils.py:272-278.  The text is
        //  sklearn's own first line: NaN wins over infinity wherever the two sit in the cloud)
        if (e & ERR_NONFINITE_NAN) return fail(c, MMW_E_NONFINITE, "scene %zu: Input X contains NaN.", s);
        if (e & ERR_NONFINITE_INF) return fail(c, MMW_E_NONFINITE, "scene %zu: Input X contains infinity or a value too large for dtype('float64').", s);
    }
    if (q[kQTimeout] != 0) return fail(c, MMW_E_HIP, "a DBSCAN chain worker gave up waiting (%d time(s)): device hung or oversubscribed", q[kQTimeout]);
    return MMW_OK;
}

// the device keeps kStatSlots partial copies of the counters (mmw_device.hpp); the totals are formed here
static int read_stats(mmw_ctx *c, uint64_t *out, int words)
{
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<uint64_t> h(kStatBytes / sizeof(uint64_t));
    MMW_TRY(d2h_after_kernels(c, h.data(), c->st.stats, h.size() * sizeof(uint64_t)));
    for (int w = 0; w < words; w++) {
        uint64_t sum = 0;
        for (int k = 0; k < kStatSlots; k++) sum += h[(size_t)k * kStatWords + w];
        out[w] = sum;
    }
    return MMW_OK;
}

int mmw_check(mmw_ctx *c)
{
    if (!c) return MMW_E_ARG;
    std::vector<SceneHdr> h;
    MMW_TRY(read_headers(c, h));
    int32_t q[kQWords];
    MMW_TRY(d2h_after_kernels(c, q, c->st.q, sizeof(q)));
    return first_scene_error(c, h.data(), h.size(), q);
}

int mmw_get_errors(mmw_ctx *c, int32_t *err_bits)
{
    if (!c || !err_bits) return MMW_E_ARG;
    std::vector<SceneHdr> h;
    MMW_TRY(read_headers(c, h));
    for (size_t s = 0; s < h.size(); s++) err_bits[s] = h[s].err;
    return MMW_OK;
}

int mmw_get_dims(const mmw_ctx *c, int32_t *n_scenes, int32_t *max_pts, int32_t *track_cap, int32_t *ring, int32_t *ring_rows)
{
    if (!c) return MMW_E_ARG;
    if (n_scenes) *n_scenes = c->dc.n_scenes;
    if (max_pts) *max_pts = c->dc.max_pts;
    if (track_cap) *track_cap = c->dc.t_cap;
    if (ring) *ring = c->dc.ring;
    if (ring_rows) *ring_rows = c->dc.ring_rows;
    return MMW_OK;
}

int mmw_get_num_tracks(mmw_ctx *c, int32_t *n_tracks)
{
    if (!c || !n_tracks) return MMW_E_ARG;
    std::vector<SceneHdr> h;
    MMW_TRY(read_headers(c, h));
    for (size_t s = 0; s < h.size(); s++) n_tracks[s] = h[s].n_tracks;
    return MMW_OK;
}

int mmw_get_batch_ring(mmw_ctx *c, int32_t *ring_len, int32_t *ring_n)
{
    if (!c || !ring_len || !ring_n) return MMW_E_ARG;
    std::vector<SceneHdr> h;
    MMW_TRY(read_headers(c, h));
    for (size_t s = 0; s < h.size(); s++) {
        ring_len[s] = h[s].g_len;
        for (int k = 0; k < MMW_RING_MAX; k++) ring_n[s * MMW_RING_MAX + k] = k < h[s].g_len ? h[s].g_n[k] : 0;
    }
    return MMW_OK;
}

int mmw_get_tracks(mmw_ctx *c, mmw_track_record *out, int32_t cap)
{
    if (!c || !out || cap < 1) return MMW_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)c->dc.n_scenes * cap * sizeof(mmw_track_record);
    if (c->export_cap < cap) {
        if (c->d_export) hipFree(c->d_export);
        c->d_export = nullptr;
        HIPCHK(c, hipMalloc((void **)&c->d_export, bytes));
        c->export_cap = cap;
    }
    launch_export(c->dc, c->st, c->d_export, cap, c->stream);   // (writes every record, the empty ones as zeros: no memset in front)
    HIPCHK(c, hipGetLastError());
    return d2h_after_kernels(c, out, c->d_export, bytes);
}

int mmw_get_track_ring_frame(mmw_ctx *c, int32_t scene, int32_t track, int32_t k, double *out, int32_t *n_rows)
{
    if (!c || !out || !n_rows || scene < 0 || scene >= c->dc.n_scenes) return MMW_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    SceneHdr h;
    MMW_TRY(d2h_after_kernels(c, &h, c->st.hdr + scene, sizeof(h)));
    if (track < 0 || track >= h.n_tracks) return fail(c, MMW_E_ARG, "track %d out of range (%d tracks)", track, h.n_tracks);
    int32_t slot = 0;
    MMW_TRY(d2h_after_kernels(c, &slot, c->st.order + (size_t)scene * c->dc.t_cap + track, sizeof(slot)));
    TrackRec rec;
    MMW_TRY(d2h_after_kernels(c, &rec, c->st.trk + (size_t)scene * c->dc.t_cap + slot, sizeof(rec)));
    if (k < 0 || k >= rec.ring_len) return fail(c, MMW_E_ARG, "frame %d out of range (ring_len %d)", k, rec.ring_len);
    const int keep = rec.ring_n[k] < c->dc.ring_rows ? rec.ring_n[k] : c->dc.ring_rows;
    const double *src = c->st.trk_ring + ((((size_t)scene * c->dc.t_cap + slot) * c->dc.ring + rec.ring_slot[k]) * c->dc.ring_rows) * 8;
    MMW_TRY(d2h_after_kernels(c, out, src, (size_t)keep * 8 * sizeof(double)));
    *n_rows = keep;
    return MMW_OK;
}

int mmw_get_batch_ring_frame(mmw_ctx *c, int32_t scene, int32_t k, double *out, int32_t *n_rows)
{
    if (!c || !out || !n_rows || scene < 0 || scene >= c->dc.n_scenes) return MMW_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    SceneHdr h;
    MMW_TRY(d2h_after_kernels(c, &h, c->st.hdr + scene, sizeof(h)));
    if (k < 0 || k >= h.g_len) return fail(c, MMW_E_ARG, "frame %d out of range (ring_len %d)", k, h.g_len);
    const double *src = c->st.g_ring + ((size_t)scene * c->dc.ring + h.g_slot[k]) * (size_t)c->dc.max_pts * 8;
    MMW_TRY(d2h_after_kernels(c, out, src, (size_t)h.g_n[k] * 8 * sizeof(double)));
    *n_rows = h.g_n[k];
    return MMW_OK;
}

int mmw_get_inner(mmw_ctx *c, int32_t *n_calls, int32_t *rows, int32_t *labels, int32_t cap_labels)
{
    if (!c || !n_calls || cap_labels < 0) return MMW_E_ARG;
    if (!c->dc.seek_inner) return fail(c, MMW_E_ARG, "mmw_get_inner: the context was created with seek_inner = 0");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t S = c->dc.n_scenes, W = kInnerHdr + c->st.inner_cap;
    std::vector<int32_t> h(S * W);
    MMW_TRY(d2h_after_kernels(c, h.data(), c->st.inner_buf, h.size() * sizeof(int32_t)));
    for (size_t s = 0; s < S; s++) {
        const int32_t *b = h.data() + s * W;
        n_calls[s] = b[0];
        if (rows) for (int k = 0; k < 16; k++) rows[s * 16 + k] = b[2 + k];
        if (labels) {
            const int m = b[1] < cap_labels ? b[1] : cap_labels;
            memcpy(labels + s * (size_t)cap_labels, b + kInnerHdr, sizeof(int32_t) * (size_t)m);
        }
    }
    return MMW_OK;
}

int mmw_track_table(mmw_ctx *c, mmw_track_summary *table, int32_t slots, int32_t scene_base)
{
    if (!c || !table || slots < 1) return MMW_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    EventPair ep;
    prof_begin(c, MMW_K_TABLE, ep);
    launch_table(c->dc, sites_or_null(c), c->st, table, slots, scene_base, c->stream);
    prof_end(c, ep);
    HIPCHK(c, hipGetLastError());
    return MMW_OK;
}

int mmw_stats_get(mmw_ctx *c, uint64_t *out) { return (!c || !out) ? MMW_E_ARG : read_stats(c, out, 8); }
int mmw_stats_get_ext(mmw_ctx *c, uint64_t *out) { return (!c || !out) ? MMW_E_ARG : read_stats(c, out, kStatWords); }
#ifdef MMW_STAMPS
extern "C" int mmw_diag_probes(mmw_ctx *c, uint64_t *out /*[256 + 8192]*/)
{
    if (!c || !out) return MMW_E_ARG;
    return d2h_after_kernels(c, out, c->st.stats + kStatBytes / sizeof(uint64_t), (256 + 8192) * sizeof(uint64_t));
}
#endif
int mmw_step_kind(mmw_ctx *c) { return !c ? MMW_E_ARG : c->dc.fused ? 1 : (pred_in_track(c->dc) ? 2 : 4); }
int mmw_kalman_layout(mmw_ctx *c)
{
    if (!c) return MMW_E_ARG;
    return (!c->dc.fused && tracks_dense(c->dc, kalman_waves_per_scene(c->dc.tr_max_tracks))) ? 1 : 0;
}
int mmw_diag_queue(mmw_ctx *c, int32_t *out /*[32]*/)
{
    if (!c || !out) return MMW_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(out, c->st.q, kQWords * sizeof(int32_t), hipMemcpyDeviceToHost));
    return MMW_OK;
}
int mmw_stats_reset(mmw_ctx *c)
{
    if (!c) return MMW_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(c->st.stats, 0, kStatBytes, c->stream));
    return MMW_OK;
}

int mmw_profile_enable(mmw_ctx *c, int32_t on)
{
    if (!c) return MMW_E_ARG;
    c->prof_mask = (on & 1) ? ~0u : ((unsigned)on >> 1);  // no synchronisation here: mmw_profile_get folds the pending pairs
    return MMW_OK;
}
int mmw_profile_reset(mmw_ctx *c)
{
    if (!c) return MMW_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    hipStreamSynchronize(c->stream);
    prof_fold(c);
    for (int k = 0; k < MMW_K_COUNT; k++) { c->tot_ms[k] = 0; c->launches[k] = 0; }
    return MMW_OK;
}
int mmw_profile_get(mmw_ctx *c, int32_t k, double *total_ms, int64_t *launches)
{
    if (!c || k < 0 || k >= MMW_K_COUNT) return MMW_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    hipStreamSynchronize(c->stream);
    prof_fold(c);
    if (total_ms) *total_ms = c->tot_ms[k];
    if (launches) *launches = c->launches[k];
    return MMW_OK;
}

