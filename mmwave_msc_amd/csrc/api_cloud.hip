// api_cloud.hip -- the C-ABI (include/mmw.h): the live tracks' point clouds.  mmw_clouds_async queues the kernels of k_cloud.hip and
// the copy of the two counts, mmw_clouds_wait waits for that copy.  The first call allocates the context's scratch; mmw_destroy frees it.
#include "mmw_ctx.hpp"

static_assert(sizeof(mmw_cloud_track) == 32, "mmw_cloud_track: the ctypes / numpy layouts of mmwave_msc_amd/_lib.py");
static_assert(sizeof(mmw_cloud_point) == 16, "mmw_cloud_point: the ctypes / numpy layouts of mmwave_msc_amd/_lib.py");

int mmw_clouds_async(mmw_ctx *c, mmw_cloud_track *dir, int32_t cap_tracks, void *out, int32_t cap_points, int32_t mode, int32_t scene_base, int32_t ticket)
{
    if (!c) return MMW_E_ARG;
    if (cap_tracks < 0 || cap_points < 0 || (cap_tracks > 0 && !dir) || (cap_points > 0 && !out))
        return fail(c, MMW_E_ARG, "mmw_clouds: cap_tracks = %d, cap_points = %d with dir %s, out %s", cap_tracks, cap_points, dir ? "set" : "NULL", out ? "set" : "NULL");
    if (mode < 0 || mode > (MMW_CLOUD_ROWS | MMW_CLOUD_UNASSIGNED)) return fail(c, MMW_E_ARG, "mmw_clouds: mode %d outside {0, 1, 2, 3}", mode);
    if (ticket < 0 || ticket >= kTickets) return fail(c, MMW_E_ARG, "mmw_clouds: ticket %d outside [0, %d)", ticket, kTickets);
    if (((uintptr_t)out & 15) != 0 || ((uintptr_t)dir & 3) != 0) return fail(c, MMW_E_ARG, "mmw_clouds: out must be 16-byte aligned, dir 4-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->cloud.d_block) MMW_TRY(export_alloc(c, c->cloud, 0, "mmw_clouds"));
    launch_clouds(c->dc, c->st, c->cloud.sc, dir, cap_tracks, out, cap_points, mode, scene_base, c->stream);
    return export_issue(c, c->cloud, ticket);
}

int mmw_clouds_wait(mmw_ctx *c, int32_t ticket, int32_t *n_tracks, int32_t *n_points)
{
    if (!c) return MMW_E_ARG;
    const int32_t *h;
    MMW_TRY(export_wait(c, c->cloud, ticket, "mmw_clouds_wait", "nothing", &h));
    if (n_tracks) *n_tracks = h[0];
    if (n_points) *n_points = h[1];
    if (!h[2]) return fail(c, MMW_E_CAPACITY, "mmw_clouds: %d entries and %d points do not fit the buffers: nothing was written", h[0], h[1]);
    return MMW_OK;
}

int mmw_clouds(mmw_ctx *c, mmw_cloud_track *dir, int32_t cap_tracks, void *out, int32_t cap_points, int32_t mode, int32_t scene_base,
               int32_t *n_tracks, int32_t *n_points)
{
    const int rc = mmw_clouds_async(c, dir, cap_tracks, out, cap_points, mode, scene_base, kTickets - 1);
    return rc ? rc : mmw_clouds_wait(c, kTickets - 1, n_tracks, n_points);
}
