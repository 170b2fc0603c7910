// api_export.hip -- what mmw_report_*, mmw_clouds_* and mmw_skeletons_* share on the host (not part of the ABI): the device scratch
// that k_pair_scan works on, and the tickets -- the totals of every call follow its kernels into a pinned slot of their own, and a
// wait is for that copy only.  The argument check and the wait of the exports with a rows and an events buffer (report, zones,
// tripwires, stance).  And the generation bump of the exports that remember uids.
#include "mmw_ctx.hpp"

void export_free(ExportCtx &x)
{
    if (x.d_block) hipFree(x.d_block);
    if (x.h_counts) hipHostFree(x.h_counts);
    for (int k = 0; k < kTickets; k++) if (x.ev[k]) hipEventDestroy(x.ev[k]);
    x = ExportCtx();
}

int export_alloc(mmw_ctx *c, ExportCtx &x, size_t extra_words, const char *name)
{
    const size_t S = c->dc.n_scenes;
    const size_t words = extra_words + 2 * (S + 1) + 4;
    if (hipMalloc((void **)&x.d_block, words * sizeof(int32_t)) != hipSuccess) { export_free(x); return fail(c, MMW_E_HIP, "%s: hipMalloc(%zu B) failed", name, words * sizeof(int32_t)); }
    x.sc.off = reinterpret_cast<int32_t *>(x.d_block) + extra_words;
    x.sc.totals = x.sc.off + 2 * (S + 1);
    if (hipHostMalloc((void **)&x.h_counts, kTickets * 4 * sizeof(int32_t), hipHostMallocDefault) != hipSuccess) { export_free(x); return fail(c, MMW_E_HIP, "%s: hipHostMalloc failed", name); }
    memset(x.h_counts, 0, kTickets * 4 * sizeof(int32_t));
    for (int k = 0; k < kTickets; k++)
        if (hipEventCreateWithFlags(&x.ev[k], hipEventDisableTiming) != hipSuccess) { export_free(x); return fail(c, MMW_E_HIP, "%s: hipEventCreate failed", name); }
    return MMW_OK;
}

int export_issue(mmw_ctx *c, ExportCtx &x, int ticket)
{
    HIPCHK(c, hipGetLastError());
    // the counts and the capacity decision follow the kernels into pinned memory: export_wait(ticket) waits for THIS copy only
    HIPCHK(c, hipMemcpyAsync(x.h_counts + ticket * 4, x.sc.totals, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(x.ev[ticket], c->stream));
    x.issued[ticket] = true;
    return MMW_OK;
}

int export_wait(mmw_ctx *c, ExportCtx &x, int ticket, const char *name, const char *none, const int32_t **counts)
{
    if (ticket < 0 || ticket >= kTickets) return fail(c, MMW_E_ARG, "%s: ticket %d outside [0, %d)", name, ticket, kTickets);
    if (!x.issued[ticket]) return fail(c, MMW_E_ARG, "%s: %s outstanding under ticket %d", name, none, ticket);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipEventSynchronize(x.ev[ticket]));
    x.issued[ticket] = false;
    *counts = x.h_counts + ticket * 4;
    return MMW_OK;
}

int pair_export_begin(mmw_ctx *c, const ExportCtx &x, const PairExport &d, const void *rows, int cap_rows, const void *events, int cap_events, int ticket)
{
    if (!x.d_block) return fail(c, MMW_E_ARG, "%s: %s", d.entry, d.off);
    if (cap_rows < 0 || cap_events < 0 || (cap_rows > 0 && !rows) || (cap_events > 0 && !events))
        return fail(c, MMW_E_ARG, "%s: cap_rows = %d, cap_events = %d with rows %s, events %s", d.entry, cap_rows, cap_events, rows ? "set" : "NULL", events ? "set" : "NULL");
    if (d.align && (((uintptr_t)rows | (uintptr_t)events) & (uintptr_t)(d.align - 1)) != 0) return fail(c, MMW_E_ARG, "%s: the buffers must be %d-byte aligned", d.entry, d.align);
    if (ticket < 0 || ticket >= kTickets) return fail(c, MMW_E_ARG, "%s: ticket %d outside [0, %d)", d.entry, ticket, kTickets);
    HIPCHK(c, hipSetDevice(c->device));
    return MMW_OK;
}

int pair_export_wait(mmw_ctx *c, ExportCtx &x, const PairExport &d, int ticket, int32_t *n_rows, int32_t *n_events)
{
    const std::string name = std::string(d.entry) + "_wait";
    if (!x.d_block) return fail(c, MMW_E_ARG, "%s: %s", name.c_str(), d.off);
    const int32_t *h;
    MMW_TRY(export_wait(c, x, ticket, name.c_str(), d.none, &h));
    if (n_rows) *n_rows = h[0];
    if (n_events) *n_events = h[1];
    if (!h[2]) return fail(c, MMW_E_CAPACITY, "%s: %d %s and %d %s %s", d.entry, h[0], d.rows, h[1], d.second, d.unfit);
    return MMW_OK;
}

// What mmw_trails_sample, mmw_tripwires_sample, mmw_stance_sample and mmw_heat_sample check before they launch: `entry` ("mmw_trails") is enabled -- x is its export
// state, `what` its noun in the message -- and the two optional device arrays are aligned.  Leaves the context's device current.
int sample_begin(mmw_ctx *c, const ExportCtx &x, const char *entry, const char *what, const int32_t *scene_flags, const double *t)
{
    if (!x.d_block) return fail(c, MMW_E_ARG, "%s_sample: %s are not enabled (%s_enable)", entry, what, entry);
    if (((uintptr_t)scene_flags & 3) != 0 || ((uintptr_t)t & 7) != 0) return fail(c, MMW_E_ARG, "%s_sample: scene_flags must be 4-byte aligned, t 8-byte aligned", entry);
    HIPCHK(c, hipSetDevice(c->device));
    return MMW_OK;
}

// mmw_reset / mmw_reset_scenes / mmw_restore: uids restart in the scenes flagged in dev_flags (device, [n_scenes]; nullptr = every
// scene), so the report's baseline, the zones' memberships, the trails, the tripwires' sides, the stance classes and the heat maps' last cells of those scenes are void.  One launch for the
// five consumers of UidGens that are on, queued on the context's stream behind the kernel that emptied or refilled the scenes, and one
// for the heat maps' word while they are on (a launch takes UidGens::kMax = 5 words, and a reset is rare); nothing at all while none is.
int uid_rebase(mmw_ctx *c, const int32_t *dev_flags)
{
    const UidGens g = {{c->rep.d_block ? c->rs.base.ug.gen : nullptr, c->zone.d_block ? c->zs.base.ug.gen : nullptr, c->trail.d_block ? c->ts.ug.gen : nullptr,
                       c->trip.d_block ? c->tw.ug.gen : nullptr, c->stance.d_block ? c->ss.ug.gen : nullptr}};
    const bool five = g.gen[0] || g.gen[1] || g.gen[2] || g.gen[3] || g.gen[4];
    if (!five && !c->heat.d_block) return MMW_OK;
    if (five) launch_uid_rebase(c->dc.n_scenes, dev_flags, g, c->stream);
    if (c->heat.d_block) launch_uid_rebase(c->dc.n_scenes, dev_flags, UidGens{{c->hs.ug.gen, nullptr, nullptr, nullptr, nullptr}}, c->stream);
    HIPCHK(c, hipGetLastError());
    return MMW_OK;
}
