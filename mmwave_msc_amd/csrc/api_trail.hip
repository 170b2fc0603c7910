// api_trail.hip -- the C-ABI (include/mmw.h): track trails.  mmw_trails_enable owns the slots and rings, mmw_trails_sample queues
// the one kernel that appends to them, mmw_trails_async queues the export kernels of k_trail.hip and the copy of the two counts,
// mmw_trails_wait waits for that copy.
#include "mmw_ctx.hpp"

static_assert(sizeof(mmw_trail_point) == 24, "mmw_trail_point: the numpy layout of mmwave_msc_amd/_lib.py");
static_assert(sizeof(mmw_trail_track) == 40, "mmw_trail_track: the numpy layout of mmwave_msc_amd/_lib.py");

void trail_free(mmw_ctx *c)
{
    export_free(c->trail);
    c->ts = TrailState();
}

int mmw_trails_enable(mmw_ctx *c, int32_t depth)
{
    if (!c) return fail(nullptr, MMW_E_ARG, "mmw_trails_enable: null context");
    if (depth < 0 || depth > MMW_TRAIL_DEPTH_MAX) return fail(c, MMW_E_ARG, "mmw_trails_enable: depth = %d outside 0 .. %d", depth, MMW_TRAIL_DEPTH_MAX);
    HIPCHK(c, hipSetDevice(c->device));
    if (depth == 0) {
        if (!c->trail.d_block) return MMW_OK;
        HIPCHK(c, hipStreamSynchronize(c->stream));   // (a sample, an export or a rebase may still be queued on what is freed here)
        trail_free(c);
        return MMW_OK;
    }
    // The new state is allocated and cleared BEFORE the old one goes: a failure leaves an earlier enablement as it was.  One block, the
    // state in front of the scratch: [S][t_cap] t_first | travelled | last_x | last_y (fp64) | the rings | owner | total | gen | seen | ordinal
    const size_t n = (size_t)c->dc.n_scenes * c->dc.t_cap, S = c->dc.n_scenes;
    const size_t ring_bytes = n * (size_t)depth * sizeof(mmw_trail_point);
    const size_t words = (4 * n * sizeof(double) + ring_bytes) / sizeof(int32_t) + 2 * n + 3 * S;
    ExportCtx nx;
    MMW_TRY(export_alloc(c, nx, words, "mmw_trails_enable"));
    TrailState ts = {};
    ts.depth = depth;
    double *d = reinterpret_cast<double *>(nx.d_block);
    ts.t_first = d; d += n;
    ts.travelled = d; d += n;
    ts.last_x = d; d += n;
    ts.last_y = d; d += n;
    ts.ring = reinterpret_cast<mmw_trail_point *>(d);
    int32_t *p = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(d) + ring_bytes);
    ts.ug.owner = p; p += n;
    ts.total = p; p += n;
    ts.ug.gen = p; p += S;
    ts.ug.seen = p; p += S;
    ts.ug.ordinal = p;
    ts.sc = nx.sc;
    // every slot free, every word 0 (the rings need no clearing: an entry is written before `total` lets anybody read it)
    hipError_t e = hipMemsetAsync(ts.t_first, 0, 4 * n * sizeof(double), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(ts.ug.owner, 0xff, n * sizeof(int32_t), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(ts.total, 0, (n + 3 * S) * sizeof(int32_t), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // (... and whatever was queued on an earlier enablement's state has run)
    if (e != hipSuccess) {
        export_free(nx);
        return fail(c, MMW_E_HIP, "mmw_trails_enable: %s", hipGetErrorString(e));
    }
    trail_free(c);
    c->trail = nx;
    c->ts = ts;
    return MMW_OK;
}

int mmw_trails_sample(mmw_ctx *c, const int32_t *scene_flags, const double *t)
{
    if (!c) return MMW_E_ARG;
    MMW_TRY(sample_begin(c, c->trail, "mmw_trails", "trails", scene_flags, t));
    launch_trail_sample(c->dc, c->st, c->ts, scene_flags, t, c->stream);
    HIPCHK(c, hipGetLastError());
    return MMW_OK;
}

int mmw_trails_async(mmw_ctx *c, mmw_trail_track *dir, int32_t cap_tracks, mmw_trail_point *points, int32_t cap_points, int32_t max_per_track,
                     int32_t scene_base, int32_t ticket)
{
    if (!c) return MMW_E_ARG;
    if (!c->trail.d_block) return fail(c, MMW_E_ARG, "mmw_trails: trails are not enabled (mmw_trails_enable)");
    if (cap_tracks < 0 || cap_points < 0 || (cap_tracks > 0 && !dir) || (cap_points > 0 && !points))
        return fail(c, MMW_E_ARG, "mmw_trails: cap_tracks = %d, cap_points = %d with dir %s, points %s", cap_tracks, cap_points, dir ? "set" : "NULL", points ? "set" : "NULL");
    if (max_per_track < 0) return fail(c, MMW_E_ARG, "mmw_trails: max_per_track = %d is negative (0 = every point a trail holds)", max_per_track);
    if (((uintptr_t)dir & 7) != 0 || ((uintptr_t)points & 7) != 0) return fail(c, MMW_E_ARG, "mmw_trails: the buffers must be 8-byte aligned");
    if (ticket < 0 || ticket >= kTickets) return fail(c, MMW_E_ARG, "mmw_trails: ticket %d outside [0, %d)", ticket, kTickets);
    HIPCHK(c, hipSetDevice(c->device));
    launch_trails(c->dc, c->st, c->ts, dir, cap_tracks, points, cap_points, max_per_track, scene_base, c->stream);
    return export_issue(c, c->trail, ticket);
}

int mmw_trails_wait(mmw_ctx *c, int32_t ticket, int32_t *n_tracks, int32_t *n_points)
{
    if (!c) return MMW_E_ARG;
    if (!c->trail.d_block) return fail(c, MMW_E_ARG, "mmw_trails_wait: trails are not enabled (mmw_trails_enable)");
    const int32_t *h;
    MMW_TRY(export_wait(c, c->trail, ticket, "mmw_trails_wait", "no trail export", &h));
    if (n_tracks) *n_tracks = h[0];
    if (n_points) *n_points = h[1];
    if (!h[2]) return fail(c, MMW_E_CAPACITY, "mmw_trails: %d entries and %d points do not fit the buffers: nothing was written", h[0], h[1]);
    return MMW_OK;
}

int mmw_trails(mmw_ctx *c, mmw_trail_track *dir, int32_t cap_tracks, mmw_trail_point *points, int32_t cap_points, int32_t max_per_track, int32_t scene_base,
               int32_t *n_tracks, int32_t *n_points)
{
    const int rc = mmw_trails_async(c, dir, cap_tracks, points, cap_points, max_per_track, scene_base, kTickets - 1);
    return rc ? rc : mmw_trails_wait(c, kTickets - 1, n_tracks, n_points);
}
