// api_snapshot.hip -- the C-ABI (include/mmw.h): snapshot / restore of scene state (the kernels: k_snapshot.hip).
#include "mmw_ctx.hpp"

static size_t snap_align16(size_t v) { return (v + 15) & ~(size_t)15; }
static size_t snap_sections_base(int32_t n) { return snap_align16(sizeof(mmw_snapshot_header) + (size_t)n * sizeof(mmw_snapshot_entry)); }

// everything queued on the context: its stream (the caller's or its own) and the chain workers' side stream, which can poll the
// queues for a few ms after the last step (mmw_destroy waits the same way)
static int snap_drain(mmw_ctx *c)
{
    HIPCHK(c, hipSetDevice(c->device));
    if (c->stream) HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->own_stream && c->own_stream != c->stream) HIPCHK(c, hipStreamSynchronize(c->own_stream));
    if (c->side_stream) HIPCHK(c, hipStreamSynchronize(c->side_stream));
    return MMW_OK;
}

struct SnapScratch { int32_t *sel, *flags, *bad; unsigned long long *sizes; mmw_snapshot_entry *dir; };
static int snap_scratch(mmw_ctx *c, SnapScratch &x)
{
    const size_t S = c->dc.n_scenes;
    const size_t o_flags = snap_align16(S * 4), o_bad = o_flags + snap_align16(S * 4), o_sizes = o_bad + 16, o_dir = o_sizes + snap_align16((S + 2) * 8);
    if (!c->d_snap) HIPCHK(c, hipMalloc((void **)&c->d_snap, o_dir + S * sizeof(mmw_snapshot_entry)));
    x.sel = reinterpret_cast<int32_t *>(c->d_snap);
    x.flags = reinterpret_cast<int32_t *>(c->d_snap + o_flags);
    x.bad = reinterpret_cast<int32_t *>(c->d_snap + o_bad);
    x.sizes = reinterpret_cast<unsigned long long *>(c->d_snap + o_sizes);
    x.dir = reinterpret_cast<mmw_snapshot_entry *>(c->d_snap + o_dir);
    return MMW_OK;
}

// the scene list of a call: NULL = all scenes in order; else n distinct indices in [0, S)
static int snap_scene_list(mmw_ctx *c, const char *who, const int32_t *scenes, int32_t n, std::vector<int32_t> &out)
{
    const int S = c->dc.n_scenes;
    if (!scenes) {
        out.resize(S);
        for (int s = 0; s < S; s++) out[s] = s;
        return MMW_OK;
    }
    if (n < 0 || n > S) return fail(c, MMW_E_ARG, "%s: %d scenes for a context of %d", who, n, S);
    out.assign(scenes, scenes + n);
    std::vector<char> seen(S, 0);
    for (int i = 0; i < n; i++) {
        const int s = out[i];
        if (s < 0 || s >= S) return fail(c, MMW_E_ARG, "%s: scene index %d (position %d) out of range [0, %d)", who, s, i, S);
        if (seen[s]) return fail(c, MMW_E_ARG, "%s: scene index %d appears twice", who, s);
        seen[s] = 1;
    }
    return MMW_OK;
}

// header + directory of a blob of `bytes` bytes (host copies): everything that can be checked without a context
static int snap_validate(mmw_ctx *c, const mmw_snapshot_header &h, const mmw_snapshot_entry *e, size_t bytes)
{
    if (memcmp(h.magic, MMW_SNAP_MAGIC, sizeof(h.magic)) != 0) return fail(c, MMW_E_ARG, "snapshot: bad magic (not a scene snapshot)");
    if (h.version != MMW_SNAP_VERSION) return fail(c, MMW_E_ARG, "snapshot: format version %u (this library reads version %d only)", h.version, MMW_SNAP_VERSION);
    if (h.header_bytes != sizeof(mmw_snapshot_header) || h.entry_bytes != (int32_t)sizeof(mmw_snapshot_entry))
        return fail(c, MMW_E_ARG, "snapshot: header_bytes %u / entry_bytes %d (expected %zu / %zu)", h.header_bytes, h.entry_bytes, sizeof(mmw_snapshot_header), sizeof(mmw_snapshot_entry));
    if (h.total_bytes != bytes) return fail(c, MMW_E_ARG, "snapshot: total_bytes %llu but %zu bytes given", (unsigned long long)h.total_bytes, bytes);
    if (h.n_scenes < 0 || h.n_scenes > (1 << 24)) return fail(c, MMW_E_ARG, "snapshot: scene count %d", h.n_scenes);
    const size_t base = snap_sections_base(h.n_scenes);
    if (base > bytes) return fail(c, MMW_E_ARG, "snapshot: directory of %d scenes truncated (%zu of %zu bytes)", h.n_scenes, bytes, base);
    if (h.ring < 1 || h.ring > MMW_RING_MAX || h.ring != h.config.fb_frames_batch + 1 || (h.dim_x != 6 && h.dim_x != 9) || h.dim_x != h.config.dim_x ||
        h.max_pts < 1 || h.max_pts > MMW_MAX_PTS_LIMIT || h.ring_rows < 1 || h.track_cap < 1 || h.track_cap > MMW_TRACK_CAP_LIMIT)
        return fail(c, MMW_E_ARG, "snapshot: source dimensions out of range (ring %d, dim_x %d, max_pts %d, ring_rows %d, track_cap %d)", h.ring, h.dim_x,
                    h.max_pts, h.ring_rows, h.track_cap);
    size_t at = base;
    for (int i = 0; i < h.n_scenes; i++) {
        const mmw_snapshot_entry &d = e[i];
        if (d.offset != at) return fail(c, MMW_E_ARG, "snapshot: scene %d: offset %llu out of order (expected %zu)", i, (unsigned long long)d.offset, at);
        if (d.n_tracks < 0 || d.n_tracks > MMW_TRACK_CAP_LIMIT || d.g_len < 0 || d.g_len > h.ring || d.max_g_rows < 0 || d.max_g_rows > MMW_MAX_PTS_LIMIT ||
            d.max_trk_rows < 0 || d.ring_size < 0 || d.ring_size > h.ring)
            return fail(c, MMW_E_ARG, "snapshot: scene %d: directory entry out of range", i);
        const unsigned long long least = (unsigned long long)MMW_SNAP_SCENE_HDR_BYTES + (unsigned long long)d.n_tracks * MMW_SNAP_TRACK_BYTES;
        if (d.bytes < least || (d.bytes & 15) != 0 || d.bytes > bytes - at)
            return fail(c, MMW_E_ARG, "snapshot: scene %d: %llu bytes at offset %llu (blob of %zu bytes)", i, (unsigned long long)d.bytes, (unsigned long long)d.offset, bytes);
        at += d.bytes;
    }
    if (at != bytes) return fail(c, MMW_E_ARG, "snapshot: %d scenes account for %zu bytes, the blob has %zu", h.n_scenes, at, bytes);
    return MMW_OK;
}

// the mmw_config fields whose difference refuses a restore: all but track_cap, ring_rows, kalman_dense_min_units,
// chain_side_stream, fused_step and reserved_ (how the target lays its state out and which kernels it runs)
static int snap_config_compatible(mmw_ctx *c, const mmw_config &a, const mmw_config &b)
{
#define MMW_SNAP_FIELD(f) if (memcmp(&a.f, &b.f, sizeof(a.f)) != 0) return fail(c, MMW_E_ARG, "mmw_restore: mmw_config." #f " differs from this context's")
    MMW_SNAP_FIELD(fb_frames_batch); MMW_SNAP_FIELD(db_min_samples); MMW_SNAP_FIELD(tr_max_tracks); MMW_SNAP_FIELD(kf_enable_est);
    MMW_SNAP_FIELD(model_min_input); MMW_SNAP_FIELD(dim_x); MMW_SNAP_FIELD(db_z_weight); MMW_SNAP_FIELD(db_range_weight);
    MMW_SNAP_FIELD(db_eps); MMW_SNAP_FIELD(tr_lifetime_dynamic); MMW_SNAP_FIELD(tr_lifetime_static); MMW_SNAP_FIELD(tr_vel_thres);
    MMW_SNAP_FIELD(tr_gate); MMW_SNAP_FIELD(kf_q_std); MMW_SNAP_FIELD(kf_p_init); MMW_SNAP_FIELD(kf_group_disp_est_init);
    MMW_SNAP_FIELD(kf_a_n); MMW_SNAP_FIELD(kf_est_pointnum); MMW_SNAP_FIELD(kf_spread_lim); MMW_SNAP_FIELD(kf_a_spr);
    MMW_SNAP_FIELD(intensity_mu); MMW_SNAP_FIELD(intensity_std); MMW_SNAP_FIELD(s_height); MMW_SNAP_FIELD(tilt_cos);
    MMW_SNAP_FIELD(tilt_sin); MMW_SNAP_FIELD(default_posture); MMW_SNAP_FIELD(seek_inner); MMW_SNAP_FIELD(db_points_thres);
    MMW_SNAP_FIELD(fb_frames_batch_static); MMW_SNAP_FIELD(db_spread_thres); MMW_SNAP_FIELD(db_inner_eps); MMW_SNAP_FIELD(m_x);
    MMW_SNAP_FIELD(m_y); MMW_SNAP_FIELD(m_z); MMW_SNAP_FIELD(v_screen_fade_size_max); MMW_SNAP_FIELD(v_screen_fade_size_min);
    MMW_SNAP_FIELD(v_screen_fade_weight);
#undef MMW_SNAP_FIELD
    static_assert(sizeof(mmw_config) == 544, "a new mmw_config field: decide whether it refuses a restore (snap_config_compatible)");
    return MMW_OK;
}

// sizes pass + scan for the scene list `sel` (uploaded to x.sel): x.dir / x.sizes on the device, the total and the largest
// track count on the host
static int snap_measure(mmw_ctx *c, const std::vector<int32_t> &sel, SnapScratch &x, size_t *total, int *max_tracks)
{
    const int n = (int)sel.size();
    if (n > 0) HIPCHK(c, hipMemcpyAsync(x.sel, sel.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, c->stream));
    launch_snap_size(c->dc, c->st, x.sel, n, x.dir, x.sizes, snap_sections_base(n), c->stream);
    HIPCHK(c, hipGetLastError());
    unsigned long long tail[2] = {0, 0};
    MMW_TRY(d2h_after_kernels(c, tail, x.sizes + n, sizeof(tail)));
    *total = (size_t)tail[0];
    *max_tracks = (int)tail[1];
    return MMW_OK;
}

// the head of mmw_snapshot_size / mmw_snapshot: the scene list, a drained context, the scratch, the sizes
static int snap_select(mmw_ctx *c, const char *who, const int32_t *scenes, int32_t n, std::vector<int32_t> &sel, SnapScratch &x, size_t *total, int *max_tracks)
{
    MMW_TRY(snap_scene_list(c, who, scenes, n, sel));
    MMW_TRY(snap_drain(c));
    MMW_TRY(snap_scratch(c, x));
    return snap_measure(c, sel, x, total, max_tracks);
}

int mmw_snapshot_size(mmw_ctx *c, const int32_t *scenes, int32_t n, size_t *bytes)
{
    if (!c || !bytes) return fail(c, MMW_E_ARG, "mmw_snapshot_size: null argument");
    std::vector<int32_t> sel;
    SnapScratch x;
    int mt = 0;
    return snap_select(c, "mmw_snapshot_size", scenes, n, sel, x, bytes, &mt);
}

int mmw_snapshot(mmw_ctx *c, const int32_t *scenes, int32_t n, void *dev_out, size_t cap, size_t *bytes)
{
    if (!c || (!dev_out && cap) || !bytes) return fail(c, MMW_E_ARG, "mmw_snapshot: null argument");
    if (((uintptr_t)dev_out & 15) != 0) return fail(c, MMW_E_ARG, "mmw_snapshot: dev_out must be 16-byte aligned");
    std::vector<int32_t> sel;
    SnapScratch x;
    size_t total = 0;
    int mt = 0;
    MMW_TRY(snap_select(c, "mmw_snapshot", scenes, n, sel, x, &total, &mt));
    *bytes = total;
    if (total > cap) return fail(c, MMW_E_ARG, "mmw_snapshot: the blob needs %zu bytes, %zu given", total, cap);
    const int ns = (int)sel.size();
    mmw_snapshot_header h;
    memset(&h, 0, sizeof(h));
    memcpy(h.magic, MMW_SNAP_MAGIC, sizeof(h.magic));
    h.version = MMW_SNAP_VERSION;
    h.header_bytes = sizeof(mmw_snapshot_header);
    h.total_bytes = total;
    h.n_scenes = ns;
    h.entry_bytes = sizeof(mmw_snapshot_entry);
    h.max_pts = c->dc.max_pts;
    h.ring = c->dc.ring;
    h.ring_rows = c->dc.ring_rows;
    h.dim_x = c->dc.dx;
    h.track_cap = c->dc.t_cap;
    h.config = c->cfg;
    char *blob = reinterpret_cast<char *>(dev_out);
    const size_t base = snap_sections_base(ns);
    std::vector<char> head(base, 0);   // header, directory room and the zero padding in front of the first section
    memcpy(head.data(), &h, sizeof(h));
    HIPCHK(c, hipMemcpyAsync(blob, head.data(), base, hipMemcpyHostToDevice, c->stream));
    if (ns > 0) HIPCHK(c, hipMemcpyAsync(blob + sizeof(h), x.dir, (size_t)ns * sizeof(mmw_snapshot_entry), hipMemcpyDeviceToDevice, c->stream));
    launch_snap_pack(c->dc, c->st, x.sel, ns, x.dir, blob, mt, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MMW_OK;
}

int mmw_restore(mmw_ctx *c, const void *dev_blob, size_t bytes, const int32_t *scenes, int32_t n)
{
    if (!c || !dev_blob) return fail(c, MMW_E_ARG, "mmw_restore: null argument");
    if (((uintptr_t)dev_blob & 15) != 0) return fail(c, MMW_E_ARG, "mmw_restore: the blob must be 16-byte aligned");
    if (bytes < sizeof(mmw_snapshot_header)) return fail(c, MMW_E_ARG, "mmw_restore: %zu bytes cannot hold a snapshot header", bytes);
    int rc = snap_drain(c);
    if (rc) return rc;
    const char *blob = reinterpret_cast<const char *>(dev_blob);
    // header and directory to the host: everything below is decided from them (and one check kernel) before any device write
    mmw_snapshot_header h;
    MMW_TRY(d2h_after_kernels(c, &h, blob, sizeof(h)));
    if (memcmp(h.magic, MMW_SNAP_MAGIC, sizeof(h.magic)) != 0 || h.version != MMW_SNAP_VERSION || h.n_scenes < 0 ||
        snap_sections_base(h.n_scenes) > bytes)
        return snap_validate(c, h, nullptr, bytes) ? MMW_E_ARG : fail(c, MMW_E_ARG, "mmw_restore: bad header");
    std::vector<mmw_snapshot_entry> dir(h.n_scenes);
    if (h.n_scenes > 0) MMW_TRY(d2h_after_kernels(c, dir.data(), blob + sizeof(h), dir.size() * sizeof(mmw_snapshot_entry)));
    if ((rc = snap_validate(c, h, dir.data(), bytes))) return rc;
    if ((rc = snap_config_compatible(c, h.config, c->cfg))) return rc;
    std::vector<int32_t> dst;
    if (scenes && n != h.n_scenes) return fail(c, MMW_E_ARG, "mmw_restore: %d scene indices for a blob of %d scenes", n, h.n_scenes);
    if (!scenes && h.n_scenes > c->dc.n_scenes) return fail(c, MMW_E_ARG, "mmw_restore: a blob of %d scenes into a context of %d", h.n_scenes, c->dc.n_scenes);
    if ((rc = snap_scene_list(c, "mmw_restore", scenes, scenes ? n : h.n_scenes, dst))) return rc;
    if (!scenes) dst.resize(h.n_scenes);
    int max_tracks = 0, max_glen = 0, resized = 0;
    for (int i = 0; i < h.n_scenes; i++) {
        const mmw_snapshot_entry &d = dir[i];
        if (d.n_tracks > c->dc.t_cap) return fail(c, MMW_E_ARG, "mmw_restore: blob scene %d holds %d tracks, track_cap is %d", i, d.n_tracks, c->dc.t_cap);
        if (d.max_g_rows > c->dc.max_pts) return fail(c, MMW_E_ARG, "mmw_restore: blob scene %d has a frame of %d points, max_pts is %d", i, d.max_g_rows, c->dc.max_pts);
        // a track frame stores min(ring_n, ring_rows) rows: it fits if all its rows were stored and fit here, or if it was cut at the same ring_rows
        if (d.max_trk_rows > c->dc.ring_rows && h.ring_rows != c->dc.ring_rows)
            return fail(c, MMW_E_ARG, "mmw_restore: blob scene %d has a track frame of %d rows, ring_rows is %d (source %d)", i, d.max_trk_rows, c->dc.ring_rows, h.ring_rows);
        if (d.max_trk_rows > h.ring_rows && h.ring_rows != c->dc.ring_rows)
            return fail(c, MMW_E_ARG, "mmw_restore: blob scene %d has a track frame cut at the source's ring_rows %d, this context's is %d", i, h.ring_rows, c->dc.ring_rows);
        max_tracks = d.n_tracks > max_tracks ? d.n_tracks : max_tracks;
        max_glen = d.g_len > max_glen ? d.g_len : max_glen;
        if (d.ring_size) resized = 1;
    }
    SnapScratch x;
    if ((rc = snap_scratch(c, x))) return rc;
    const int ns = h.n_scenes;
    if (ns > 0) {
        // every section says what its directory entry says (nothing written yet)
        HIPCHK(c, hipMemsetAsync(x.bad, 0, sizeof(int32_t), c->stream));
        launch_snap_check(c->dc, blob, reinterpret_cast<const mmw_snapshot_entry *>(blob + sizeof(h)), ns, h.ring_rows, x.bad, c->stream);
        HIPCHK(c, hipGetLastError());
        int32_t bad = 0;
        MMW_TRY(d2h_after_kernels(c, &bad, x.bad, sizeof(bad)));
        if (bad) return fail(c, MMW_E_ARG, "mmw_restore: blob scene %d: its section disagrees with its directory entry", bad - 1);
        std::vector<int32_t> flags(c->dc.n_scenes, 0);
        for (int i = 0; i < ns; i++) flags[dst[i]] = 1;
        HIPCHK(c, hipMemcpyAsync(x.sel, dst.data(), sizeof(int32_t) * ns, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(x.flags, flags.data(), sizeof(int32_t) * flags.size(), hipMemcpyHostToDevice, c->stream));
        launch_snap_restore(c->dc, c->st, blob, reinterpret_cast<const mmw_snapshot_entry *>(blob + sizeof(h)), x.sel, x.flags, ns, max_tracks, h.ring_rows,
                            c->d_kp_gen, c->stream);
        HIPCHK(c, hipGetLastError());
        MMW_TRY(uid_rebase(c, x.flags));              // (report, zones, trails -- whichever is on: the restored scenes carry another recording's uids)
        HIPCHK(c, hipStreamSynchronize(c->stream));   // (the host vectors above go away)
    }
    // host-side bookkeeping: the large-cloud launches are carved for ring_frames_bound frames, and resized rings are k_track's
    if (c->ring_frames_bound < max_glen) c->ring_frames_bound = max_glen;
    if (resized) { c->dc.var_ring = 1; refresh_step_kind(c); }
    return MMW_OK;
}

int mmw_snapshot_inspect(const void *host_blob, size_t bytes, mmw_snapshot_info *out)
{
    if (!host_blob || !out) return fail(nullptr, MMW_E_ARG, "mmw_snapshot_inspect: null argument");
    if (bytes < sizeof(mmw_snapshot_header)) return fail(nullptr, MMW_E_ARG, "snapshot: %zu bytes cannot hold a snapshot header", bytes);
    mmw_snapshot_header h;
    memcpy(&h, host_blob, sizeof(h));
    if (memcmp(h.magic, MMW_SNAP_MAGIC, sizeof(h.magic)) != 0 || h.version != MMW_SNAP_VERSION || h.n_scenes < 0 || snap_sections_base(h.n_scenes) > bytes)
        return snap_validate(nullptr, h, nullptr, bytes) ? MMW_E_ARG : fail(nullptr, MMW_E_ARG, "snapshot: bad header");
    const mmw_snapshot_entry *e = reinterpret_cast<const mmw_snapshot_entry *>(reinterpret_cast<const char *>(host_blob) + sizeof(h));
    std::vector<mmw_snapshot_entry> dir(e, e + h.n_scenes);   // (the blob need not be 8-byte aligned)
    const int rc = snap_validate(nullptr, h, dir.data(), bytes);
    if (rc) return rc;
    out->header = h;
    out->entries = e;
    return MMW_OK;
}
