// api_cloud.hip -- the C-ABI (include/mmw.h): the live tracks' point clouds.  mmw_clouds_async queues the kernels of k_cloud.hip and
// the copy of the two counts, mmw_clouds_wait waits for that copy.  The first call allocates the context's scratch; mmw_destroy frees it.
#include <new>

#include "mmw_ctx.hpp"

static_assert(sizeof(mmw_cloud_track) == 32, "mmw_cloud_track: the ctypes / numpy layouts of mmwave_msc_amd/_lib.py");
static_assert(sizeof(mmw_cloud_point) == 16, "mmw_cloud_point: the ctypes / numpy layouts of mmwave_msc_amd/_lib.py");

void cloud_free(CloudCtx *k)
{
    if (!k) return;
    if (k->d_block) hipFree(k->d_block);
    if (k->h_counts) hipHostFree(k->h_counts);
    for (int t = 0; t < kTickets; t++) if (k->ev[t]) hipEventDestroy(k->ev[t]);
    delete k;
}

static int cloud_alloc(mmw_ctx *c)
{
    CloudCtx *k = new (std::nothrow) CloudCtx();
    if (!k) return fail(c, MMW_E_ARG, "out of host memory");
    const size_t S = c->dc.n_scenes;
    const size_t words = 2 * (S + 1) + 4;
    if (hipMalloc((void **)&k->d_block, words * sizeof(int32_t)) != hipSuccess) { cloud_free(k); return fail(c, MMW_E_HIP, "mmw_clouds: hipMalloc(%zu B) failed", words * sizeof(int32_t)); }
    int32_t *p = reinterpret_cast<int32_t *>(k->d_block);
    k->cs.off = p; p += 2 * (S + 1);
    k->cs.totals = p;
    if (hipHostMalloc((void **)&k->h_counts, kTickets * 4 * sizeof(int32_t), hipHostMallocDefault) != hipSuccess) { cloud_free(k); return fail(c, MMW_E_HIP, "mmw_clouds: hipHostMalloc failed"); }
    memset(k->h_counts, 0, kTickets * 4 * sizeof(int32_t));
    for (int t = 0; t < kTickets; t++)
        if (hipEventCreateWithFlags(&k->ev[t], hipEventDisableTiming) != hipSuccess) { cloud_free(k); return fail(c, MMW_E_HIP, "mmw_clouds: hipEventCreate failed"); }
    c->cloud = k;
    return MMW_OK;
}

int mmw_clouds_async(mmw_ctx *c, mmw_cloud_track *dir, int32_t cap_tracks, void *out, int32_t cap_points, int32_t mode, int32_t scene_base, int32_t ticket)
{
    if (!c) return MMW_E_ARG;
    if (cap_tracks < 0 || cap_points < 0 || (cap_tracks > 0 && !dir) || (cap_points > 0 && !out))
        return fail(c, MMW_E_ARG, "mmw_clouds: cap_tracks = %d, cap_points = %d with dir %s, out %s", cap_tracks, cap_points, dir ? "set" : "NULL", out ? "set" : "NULL");
    if (mode < 0 || mode > (MMW_CLOUD_ROWS | MMW_CLOUD_UNASSIGNED)) return fail(c, MMW_E_ARG, "mmw_clouds: mode %d outside {0, 1, 2, 3}", mode);
    if (ticket < 0 || ticket >= kTickets) return fail(c, MMW_E_ARG, "mmw_clouds: ticket %d outside [0, %d)", ticket, kTickets);
    if (((uintptr_t)out & 15) != 0 || ((uintptr_t)dir & 3) != 0) return fail(c, MMW_E_ARG, "mmw_clouds: out must be 16-byte aligned, dir 4-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->cloud) MMW_TRY(cloud_alloc(c));
    CloudCtx *k = c->cloud;
    launch_clouds(c->dc, c->st, k->cs, dir, cap_tracks, out, cap_points, mode, scene_base, c->stream);
    HIPCHK(c, hipGetLastError());
    // the counts and the capacity decision follow the kernels into pinned memory: mmw_clouds_wait(ticket) waits for THIS copy only
    HIPCHK(c, hipMemcpyAsync(k->h_counts + ticket * 4, k->cs.totals, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(k->ev[ticket], c->stream));
    k->issued[ticket] = true;
    return MMW_OK;
}

int mmw_clouds_wait(mmw_ctx *c, int32_t ticket, int32_t *n_tracks, int32_t *n_points)
{
    if (!c) return MMW_E_ARG;
    if (ticket < 0 || ticket >= kTickets) return fail(c, MMW_E_ARG, "mmw_clouds_wait: ticket %d outside [0, %d)", ticket, kTickets);
    CloudCtx *k = c->cloud;
    if (!k || !k->issued[ticket]) return fail(c, MMW_E_ARG, "mmw_clouds_wait: nothing outstanding under ticket %d", ticket);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipEventSynchronize(k->ev[ticket]));
    k->issued[ticket] = false;
    const int32_t *h = k->h_counts + ticket * 4;
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
