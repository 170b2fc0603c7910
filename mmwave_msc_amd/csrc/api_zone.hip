// api_zone.hip -- the C-ABI (include/mmw.h): zone occupancy.  mmw_set_zones owns the table and the baseline, mmw_zones_async queues
// the kernels of k_zone.hip and the copy of the two counts, mmw_zones_wait waits for that copy.
#include <cmath>
#include "mmw_scene_table.hpp"

static_assert(sizeof(mmw_zone) == 48, "mmw_zone: the numpy layout of mmwave_msc_amd/_lib.py");
static_assert(sizeof(mmw_zone_row) == 32, "mmw_zone_row: the numpy layout of mmwave_msc_amd/_lib.py");
static_assert(sizeof(mmw_zone_event) == 24, "mmw_zone_event: the numpy layout of mmwave_msc_amd/_lib.py");

void zone_free(mmw_ctx *c)
{
    export_free(c->zone);
    scene_table_free(c->ztab);
    c->zs = ZoneState();
}

// the baseline lies in front of the scratch, in the same device block; it starts empty, generation 0 seen
static int zone_alloc(mmw_ctx *c)
{
    const size_t S = c->dc.n_scenes, cap = c->dc.t_cap, words = 2 * S * cap + 3 * S;
    MMW_TRY(export_alloc(c, c->zone, words, "mmw_set_zones"));
    if (const int rc = scene_table_alloc(c, c->ztab, "mmw_set_zones")) {
        export_free(c->zone);
        return rc;
    }
    if (hipMemsetAsync(c->zone.d_block, 0, words * sizeof(int32_t), c->stream) != hipSuccess) {
        zone_free(c);
        return fail(c, MMW_E_HIP, "mmw_set_zones: hipMemsetAsync failed");
    }
    int32_t *p = reinterpret_cast<int32_t *>(c->zone.d_block);
    c->zs.base.base_uid = p; p += S * cap;
    c->zs.base_mask = p; p += S * cap;
    c->zs.base.base_len = p; p += S;
    c->zs.base.ug.gen = p; p += S;
    c->zs.base.ug.seen = p;
    c->zs.sc = c->zone.sc;
    c->zs.zones = c->ztab.entries();
    c->zs.n_zones = c->ztab.counts(S);
    return MMW_OK;
}

int mmw_set_zones(mmw_ctx *c, const int32_t *scenes, int32_t n, const int32_t *n_zones, const mmw_zone *zones)
{
    if (!c) return fail(nullptr, MMW_E_ARG, "mmw_set_zones: null context");
    // every check first: a refused call changes no scene's zones (and allocates nothing)
    MMW_TRY(scene_table_check<decltype(c->ztab)>(c, {"mmw_set_zones", "n_zones", "zones"}, scenes, n, n_zones, zones, [c](int i, int s, int z, const mmw_zone &q) {
        if (std::isnan(q.x0) || std::isnan(q.x1) || std::isnan(q.y0) || std::isnan(q.y1))
            return fail(c, MMW_E_ARG, "mmw_set_zones: entry %d (scene %d) zone %d has a NaN bound", i, s, z);
        if (q.x0 > q.x1 || q.y0 > q.y1) return fail(c, MMW_E_ARG, "mmw_set_zones: entry %d (scene %d) zone %d has x0 > x1 or y0 > y1", i, s, z);
        if (!(q.margin >= 0.0) || !std::isfinite(q.margin)) return fail(c, MMW_E_ARG, "mmw_set_zones: entry %d (scene %d) zone %d has a margin that is negative or not finite", i, s, z);
        if (q.reserved_ != 0) return fail(c, MMW_E_ARG, "mmw_set_zones: entry %d (scene %d) zone %d has a non-zero reserved_", i, s, z);
        return MMW_OK;
    }));
    HIPCHK(c, hipSetDevice(c->device));
    const bool fresh = !c->zone.d_block;
    if (fresh) MMW_TRY(zone_alloc(c));
    // the generation bump is of the zones' word alone: the report's baseline, the trails and the tripwires stand
    const int rc = scene_table_send(c, c->ztab, "mmw_set_zones", scenes, n, n_zones, zones, [](const mmw_zone &q) { return q; }, c->zs.base.ug.gen, [](const int32_t *) {});
    if (rc && fresh) zone_free(c);   // (the first call: as if it had never been made)
    return rc;
}

int mmw_get_zones(mmw_ctx *c, int32_t *n_zones, mmw_zone *zones)
{
    if (!c) return fail(nullptr, MMW_E_ARG, "mmw_get_zones: null context");
    scene_table_get(c->ztab, (size_t)c->dc.n_scenes, n_zones, zones);
    return MMW_OK;
}

int mmw_clear_zones(mmw_ctx *c)
{
    if (!c) return fail(nullptr, MMW_E_ARG, "mmw_clear_zones: null context");
    if (!c->zone.d_block) return MMW_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (an export or a rebase may still be queued on what is freed here)
    zone_free(c);
    return MMW_OK;
}

int mmw_has_zones(mmw_ctx *c)
{
    if (!c) return fail(nullptr, MMW_E_ARG, "mmw_has_zones: null context");
    return c->zone.d_block ? 1 : 0;
}

static const PairExport kExport = {"mmw_zones", "no zone is defined (mmw_set_zones)", "no zone export", "rows", kUnfitBaseline, 4};

int mmw_zones_async(mmw_ctx *c, mmw_zone_row *rows, int32_t cap_rows, mmw_zone_event *events, int32_t cap_events, int32_t scene_base, int32_t ticket)
{
    if (!c) return MMW_E_ARG;
    MMW_TRY(pair_export_begin(c, c->zone, kExport, rows, cap_rows, events, cap_events, ticket));
    launch_zones(c->dc, c->st, c->zs, rows, cap_rows, events, cap_events, scene_base, c->stream);
    return export_issue(c, c->zone, ticket);
}

int mmw_zones_wait(mmw_ctx *c, int32_t ticket, int32_t *n_rows, int32_t *n_events)
{
    return c ? pair_export_wait(c, c->zone, kExport, ticket, n_rows, n_events) : MMW_E_ARG;
}

int mmw_zones(mmw_ctx *c, mmw_zone_row *rows, int32_t cap_rows, mmw_zone_event *events, int32_t cap_events, int32_t scene_base, int32_t *n_rows,
              int32_t *n_events)
{
    const int rc = mmw_zones_async(c, rows, cap_rows, events, cap_events, scene_base, kTickets - 1);
    return rc ? rc : mmw_zones_wait(c, kTickets - 1, n_rows, n_events);
}
