// api_zone.hip -- the C-ABI (include/mmw.h): zone occupancy.  mmw_set_zones owns the table and the baseline, mmw_zones_async queues
// the kernels of k_zone.hip and the copy of the two counts, mmw_zones_wait waits for that copy.
#include <cmath>
#include "mmw_ctx.hpp"

static_assert(sizeof(mmw_zone) == 48, "mmw_zone: the numpy layout of mmwave_msc_amd/_lib.py");
static_assert(sizeof(mmw_zone_row) == 32, "mmw_zone_row: the numpy layout of mmwave_msc_amd/_lib.py");
static_assert(sizeof(mmw_zone_event) == 24, "mmw_zone_event: the numpy layout of mmwave_msc_amd/_lib.py");

void zone_free(mmw_ctx *c)
{
    export_free(c->zone);
    if (c->d_ztab) hipFree(c->d_ztab);
    c->d_ztab = nullptr;
    c->zs = ZoneState();
    c->h_zones.clear();
    c->h_nzones.clear();
}

// the table's allocation: [S][MMW_ZONES_MAX] mmw_zone | [S] n_zones | [S] scene flags of the mmw_set_zones call that wrote it
static size_t ztab_bytes(size_t S) { return S * MMW_ZONES_MAX * sizeof(mmw_zone) + 2 * S * sizeof(int32_t); }

// the baseline lies in front of the scratch, in the same device block; it starts empty, generation 0 seen
static int zone_alloc(mmw_ctx *c)
{
    const size_t S = c->dc.n_scenes, cap = c->dc.t_cap, words = 2 * S * cap + 3 * S;
    MMW_TRY(export_alloc(c, c->zone, words, "mmw_set_zones"));
    if (hipMalloc((void **)&c->d_ztab, ztab_bytes(S)) != hipSuccess) {
        c->d_ztab = nullptr;
        export_free(c->zone);
        return fail(c, MMW_E_HIP, "mmw_set_zones: hipMalloc(%zu B) failed", ztab_bytes(S));
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
    c->zs.zones = reinterpret_cast<const mmw_zone *>(c->d_ztab);
    c->zs.n_zones = reinterpret_cast<const int32_t *>(c->d_ztab + S * MMW_ZONES_MAX * sizeof(mmw_zone));
    c->h_zones.assign(S * MMW_ZONES_MAX, mmw_zone{});
    c->h_nzones.assign(S, 0);
    return MMW_OK;
}

int mmw_set_zones(mmw_ctx *c, const int32_t *scenes, int32_t n, const int32_t *n_zones, const mmw_zone *zones)
{
    if (!c) return fail(nullptr, MMW_E_ARG, "mmw_set_zones: null context");
    const int S = c->dc.n_scenes;
    // every check first: a refused call changes no scene's zones (and allocates nothing)
    if (n < 0 || n > S) return fail(c, MMW_E_ARG, "mmw_set_zones: n = %d, the context has %d scenes", n, S);
    if (n > 0 && (!n_zones || !zones)) return fail(c, MMW_E_ARG, "mmw_set_zones: %s is NULL with n = %d", !n_zones ? "n_zones" : "zones", n);
    std::vector<char> listed((size_t)S, 0);
    for (int i = 0; i < n; i++) {
        const int s = scenes ? scenes[i] : i;
        if (s < 0 || s >= S) return fail(c, MMW_E_ARG, "mmw_set_zones: entry %d names scene %d, the context has %d scenes", i, s, S);
        if (listed[s]) return fail(c, MMW_E_ARG, "mmw_set_zones: entry %d names scene %d a second time", i, s);
        listed[s] = 1;
        if (n_zones[i] < 0 || n_zones[i] > MMW_ZONES_MAX) return fail(c, MMW_E_ARG, "mmw_set_zones: entry %d (scene %d) has n_zones = %d, outside 0 .. %d", i, s, n_zones[i], MMW_ZONES_MAX);
        for (int z = 0; z < n_zones[i]; z++) {
            const mmw_zone &q = zones[(size_t)i * MMW_ZONES_MAX + z];
            if (std::isnan(q.x0) || std::isnan(q.x1) || std::isnan(q.y0) || std::isnan(q.y1))
                return fail(c, MMW_E_ARG, "mmw_set_zones: entry %d (scene %d) zone %d has a NaN bound", i, s, z);
            if (q.x0 > q.x1 || q.y0 > q.y1) return fail(c, MMW_E_ARG, "mmw_set_zones: entry %d (scene %d) zone %d has x0 > x1 or y0 > y1", i, s, z);
            if (!(q.margin >= 0.0) || !std::isfinite(q.margin)) return fail(c, MMW_E_ARG, "mmw_set_zones: entry %d (scene %d) zone %d has a margin that is negative or not finite", i, s, z);
            if (q.reserved_ != 0) return fail(c, MMW_E_ARG, "mmw_set_zones: entry %d (scene %d) zone %d has a non-zero reserved_", i, s, z);
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    const bool fresh = !c->zone.d_block;
    if (fresh) MMW_TRY(zone_alloc(c));
    // The new table is put together on the host (from a copy of the mirror: a failure below leaves the mirror as it was) and travels
    // as ONE copy, ordered on the context's stream: what was queued before this call reads the old table.  The listed scenes' flags
    // ride behind it, for the generation bump -- of the zones' word alone: the report's baseline and the trails stand.
    const size_t zb = (size_t)S * MMW_ZONES_MAX * sizeof(mmw_zone);
    std::vector<mmw_zone> next = c->h_zones;
    std::vector<int32_t> next_n = c->h_nzones;
    for (int i = 0; i < n; i++) {
        const size_t s = scenes ? scenes[i] : i;
        next_n[s] = n_zones[i];
        for (int z = 0; z < MMW_ZONES_MAX; z++) next[s * MMW_ZONES_MAX + z] = z < n_zones[i] ? zones[(size_t)i * MMW_ZONES_MAX + z] : mmw_zone{};
    }
    std::vector<char> stage(ztab_bytes((size_t)S));
    memcpy(stage.data(), next.data(), zb);
    memcpy(stage.data() + zb, next_n.data(), sizeof(int32_t) * (size_t)S);
    int32_t *flags = reinterpret_cast<int32_t *>(stage.data() + zb) + S;
    for (int s = 0; s < S; s++) flags[s] = listed[s];
    hipError_t e = hipMemcpyAsync(c->d_ztab, stage.data(), stage.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        launch_uid_rebase(S, c->zs.n_zones + S, UidGens{{c->zs.base.ug.gen, nullptr, nullptr}}, c->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // (`stage` is pageable and goes away)
    if (e != hipSuccess) {
        if (fresh) zone_free(c);   // (the first call: as if it had never been made)
        return fail(c, MMW_E_HIP, "mmw_set_zones: %s", hipGetErrorString(e));
    }
    c->h_zones.swap(next);
    c->h_nzones.swap(next_n);
    return MMW_OK;
}

int mmw_get_zones(mmw_ctx *c, int32_t *n_zones, mmw_zone *zones)
{
    if (!c) return fail(nullptr, MMW_E_ARG, "mmw_get_zones: null context");
    const size_t S = (size_t)c->dc.n_scenes;
    const bool have = c->zone.d_block != nullptr;
    if (n_zones) { if (have) memcpy(n_zones, c->h_nzones.data(), S * sizeof(int32_t)); else memset(n_zones, 0, S * sizeof(int32_t)); }
    if (zones) { if (have) memcpy(zones, c->h_zones.data(), S * MMW_ZONES_MAX * sizeof(mmw_zone)); else memset(zones, 0, S * MMW_ZONES_MAX * sizeof(mmw_zone)); }
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

int mmw_zones_async(mmw_ctx *c, mmw_zone_row *rows, int32_t cap_rows, mmw_zone_event *events, int32_t cap_events, int32_t scene_base, int32_t ticket)
{
    if (!c) return MMW_E_ARG;
    if (!c->zone.d_block) return fail(c, MMW_E_ARG, "mmw_zones: no zone is defined (mmw_set_zones)");
    if (cap_rows < 0 || cap_events < 0 || (cap_rows > 0 && !rows) || (cap_events > 0 && !events))
        return fail(c, MMW_E_ARG, "mmw_zones: cap_rows = %d, cap_events = %d with rows %s, events %s", cap_rows, cap_events, rows ? "set" : "NULL", events ? "set" : "NULL");
    if (((uintptr_t)rows & 3) != 0 || ((uintptr_t)events & 3) != 0) return fail(c, MMW_E_ARG, "mmw_zones: the buffers must be 4-byte aligned");
    if (ticket < 0 || ticket >= kTickets) return fail(c, MMW_E_ARG, "mmw_zones: ticket %d outside [0, %d)", ticket, kTickets);
    HIPCHK(c, hipSetDevice(c->device));
    launch_zones(c->dc, c->st, c->zs, rows, cap_rows, events, cap_events, scene_base, c->stream);
    return export_issue(c, c->zone, ticket);
}

int mmw_zones_wait(mmw_ctx *c, int32_t ticket, int32_t *n_rows, int32_t *n_events)
{
    if (!c) return MMW_E_ARG;
    if (!c->zone.d_block) return fail(c, MMW_E_ARG, "mmw_zones_wait: no zone is defined (mmw_set_zones)");
    const int32_t *h;
    MMW_TRY(export_wait(c, c->zone, ticket, "mmw_zones_wait", "no zone export", &h));
    if (n_rows) *n_rows = h[0];
    if (n_events) *n_events = h[1];
    if (!h[2]) return fail(c, MMW_E_CAPACITY, "mmw_zones: %d rows and %d events do not fit the buffers: nothing was written, the baseline is unchanged", h[0], h[1]);
    return MMW_OK;
}

int mmw_zones(mmw_ctx *c, mmw_zone_row *rows, int32_t cap_rows, mmw_zone_event *events, int32_t cap_events, int32_t scene_base, int32_t *n_rows,
              int32_t *n_events)
{
    const int rc = mmw_zones_async(c, rows, cap_rows, events, cap_events, scene_base, kTickets - 1);
    return rc ? rc : mmw_zones_wait(c, kTickets - 1, n_rows, n_events);
}
