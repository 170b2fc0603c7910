// api_tripwire.hip -- the C-ABI (include/mmw.h): tripwires.  mmw_tripwires_enable owns the table, the uid slots, the counters and
// the event rings, mmw_set_tripwires derives the table on the host, mmw_tripwires_sample queues the one kernel that decides the
// sides, mmw_tripwires_async queues the export kernels of k_tripwire.hip and the copy of the two counts, mmw_tripwires_wait waits
// for that copy.
#include <cmath>
#include "mmw_scene_table.hpp"

static_assert(sizeof(mmw_tripwire) == 48, "mmw_tripwire: the numpy layout of mmwave_msc_amd/_lib.py");
static_assert(sizeof(mmw_tripwire_row) == 32, "mmw_tripwire_row: the numpy layout of mmwave_msc_amd/_lib.py");
static_assert(sizeof(mmw_tripwire_event) == 32, "mmw_tripwire_event: the numpy layout of mmwave_msc_amd/_lib.py");

void tripwire_free(mmw_ctx *c)
{
    export_free(c->trip);
    scene_table_free(c->twtab);
    c->tw = TripState();
}

int mmw_tripwires_enable(mmw_ctx *c, int32_t log_depth)
{
    if (!c) return fail(nullptr, MMW_E_ARG, "mmw_tripwires_enable: null context");
    if (log_depth < 0 || log_depth > MMW_TRIPWIRE_LOG_MAX)
        return fail(c, MMW_E_ARG, "mmw_tripwires_enable: log_depth = %d outside 0 .. %d", log_depth, MMW_TRIPWIRE_LOG_MAX);
    HIPCHK(c, hipSetDevice(c->device));
    if (log_depth == 0) {
        if (!c->trip.d_block) return MMW_OK;
        HIPCHK(c, hipStreamSynchronize(c->stream));   // (a sample, an export or a rebase may still be queued on what is freed here)
        tripwire_free(c);
        return MMW_OK;
    }
    // The new state is allocated and cleared BEFORE the old one goes: a failure leaves an earlier enablement as it was.  One block, the
    // state in front of the scratch: [S][depth] events | [S][16] counters | [S][t_cap] owner | side | [S] logged | taken | gen | seen | ordinal
    const size_t S = c->dc.n_scenes, n = S * c->dc.t_cap;
    const size_t ring_bytes = S * (size_t)log_depth * sizeof(mmw_tripwire_event), count_bytes = S * MMW_TRIPWIRES_MAX * sizeof(TripCount);
    const size_t words = (ring_bytes + count_bytes) / sizeof(int32_t) + 2 * n + 5 * S;
    ExportCtx nx;
    MMW_TRY(export_alloc(c, nx, words, "mmw_tripwires_enable"));
    decltype(c->twtab) tab;
    if (const int rc = scene_table_alloc(c, tab, "mmw_tripwires_enable")) {
        export_free(nx);
        return rc;
    }
    TripState tw = {};
    tw.wires = tab.entries();
    tw.n_wires = tab.counts(S);
    tw.count = reinterpret_cast<TripCount *>(nx.d_block + ring_bytes);
    int32_t *p = reinterpret_cast<int32_t *>(nx.d_block + ring_bytes + count_bytes);
    tw.ug.owner = p; p += n;
    tw.side = p; p += n;
    evlog_carve(tw.log, tw.ug, log_depth, nx.d_block, p, S);
    tw.sc = nx.sc;
    // every scene at 0 wires, every slot free, every word 0 (the rings need no clearing: an entry is written before `logged` lets anybody read it)
    hipError_t e = hipMemsetAsync(tab.d_tab, 0, tab.bytes(S), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(tw.count, 0, count_bytes, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(tw.ug.owner, 0xff, n * sizeof(int32_t), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(tw.side, 0, (n + 5 * S) * sizeof(int32_t), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // (... and whatever was queued on an earlier enablement's state has run)
    if (e != hipSuccess) {
        export_free(nx);
        scene_table_free(tab);
        return fail(c, MMW_E_HIP, "mmw_tripwires_enable: %s", hipGetErrorString(e));
    }
    tripwire_free(c);
    c->trip = nx;
    c->tw = tw;
    c->twtab = std::move(tab);
    return MMW_OK;
}

// what the device reads of a wire, in the header's operation order (this file is compiled with -ffp-contract=off like the kernels)
static TripWire derive(const mmw_tripwire &w)
{
    TripWire d = {};
    d.ax = w.ax;
    d.ay = w.ay;
    d.dx = w.bx - w.ax;
    d.dy = w.by - w.ay;
    d.len2 = d.dx * d.dx + d.dy * d.dy;
    d.band = w.margin * std::sqrt(d.len2);
    d.id = w.id;
    return d;
}

int mmw_set_tripwires(mmw_ctx *c, const int32_t *scenes, int32_t n, const int32_t *n_wires, const mmw_tripwire *wires)
{
    if (!c) return fail(nullptr, MMW_E_ARG, "mmw_set_tripwires: null context");
    if (!c->trip.d_block) return fail(c, MMW_E_ARG, "mmw_set_tripwires: tripwires are not enabled (mmw_tripwires_enable)");
    // every check first: a refused call changes no scene's wires
    MMW_TRY(scene_table_check<decltype(c->twtab)>(c, {"mmw_set_tripwires", "n_wires", "wires"}, scenes, n, n_wires, wires, [c](int i, int s, int z, const mmw_tripwire &q) {
        if (q.reserved_ != 0) return fail(c, MMW_E_ARG, "mmw_set_tripwires: entry %d (scene %d) wire %d has a non-zero reserved_", i, s, z);
        if (!std::isfinite(q.ax) || !std::isfinite(q.ay) || !std::isfinite(q.bx) || !std::isfinite(q.by))
            return fail(c, MMW_E_ARG, "mmw_set_tripwires: entry %d (scene %d) wire %d has a coordinate that is not finite", i, s, z);
        if (!(q.margin >= 0.0) || !std::isfinite(q.margin))
            return fail(c, MMW_E_ARG, "mmw_set_tripwires: entry %d (scene %d) wire %d has a margin that is negative or not finite", i, s, z);
        if (q.ax == q.bx && q.ay == q.by) return fail(c, MMW_E_ARG, "mmw_set_tripwires: entry %d (scene %d) wire %d has A == B", i, s, z);
        const TripWire d = derive(q);
        if (!(d.len2 > 0.0) || !std::isfinite(d.len2)) return fail(c, MMW_E_ARG, "mmw_set_tripwires: entry %d (scene %d) wire %d has a squared length that is zero or not finite", i, s, z);
        if (!std::isfinite(d.band) || (q.margin > 0.0 && !(d.band > 0.0)))
            return fail(c, MMW_E_ARG, "mmw_set_tripwires: entry %d (scene %d) wire %d has a band (margin x length) that is zero or not finite", i, s, z);
        return MMW_OK;
    }));
    HIPCHK(c, hipSetDevice(c->device));
    // the generation bump is of the tripwires' word alone; the listed scenes' counters restart behind it
    return scene_table_send(c, c->twtab, "mmw_set_tripwires", scenes, n, n_wires, wires, derive, c->tw.ug.gen,
                            [c](const int32_t *flags) { launch_tripwire_zero(c->dc.n_scenes, flags, c->tw, c->stream); });
}

int mmw_get_tripwires(mmw_ctx *c, int32_t *n_wires, mmw_tripwire *wires)
{
    if (!c) return fail(nullptr, MMW_E_ARG, "mmw_get_tripwires: null context");
    scene_table_get(c->twtab, (size_t)c->dc.n_scenes, n_wires, wires);
    return MMW_OK;
}

int mmw_tripwires_sample(mmw_ctx *c, const int32_t *scene_flags, const double *t)
{
    if (!c) return MMW_E_ARG;
    MMW_TRY(sample_begin(c, c->trip, "mmw_tripwires", "tripwires", scene_flags, t));
    launch_tripwire_sample(c->dc, c->st, c->tw, scene_flags, t, c->stream);
    HIPCHK(c, hipGetLastError());
    return MMW_OK;
}

static const PairExport kExport = {"mmw_tripwires", "tripwires are not enabled (mmw_tripwires_enable)", "no tripwire export", "rows", kUnfitLog, 8};

int mmw_tripwires_async(mmw_ctx *c, mmw_tripwire_row *rows, int32_t cap_rows, mmw_tripwire_event *events, int32_t cap_events, int32_t scene_base, int32_t ticket)
{
    if (!c) return MMW_E_ARG;
    MMW_TRY(pair_export_begin(c, c->trip, kExport, rows, cap_rows, events, cap_events, ticket));
    launch_tripwires(c->dc, c->tw, rows, cap_rows, events, cap_events, scene_base, c->stream);
    return export_issue(c, c->trip, ticket);
}

int mmw_tripwires_wait(mmw_ctx *c, int32_t ticket, int32_t *n_rows, int32_t *n_events)
{
    return c ? pair_export_wait(c, c->trip, kExport, ticket, n_rows, n_events) : MMW_E_ARG;
}

int mmw_tripwires(mmw_ctx *c, mmw_tripwire_row *rows, int32_t cap_rows, mmw_tripwire_event *events, int32_t cap_events, int32_t scene_base, int32_t *n_rows,
                  int32_t *n_events)
{
    const int rc = mmw_tripwires_async(c, rows, cap_rows, events, cap_events, scene_base, kTickets - 1);
    return rc ? rc : mmw_tripwires_wait(c, kTickets - 1, n_rows, n_events);
}
