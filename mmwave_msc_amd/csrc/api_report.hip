// api_report.hip -- the C-ABI (include/mmw.h): the live-track report.  mmw_report_enable owns the baseline, mmw_report_async queues
// the kernels of k_report.hip and the copy of the two counts, mmw_report_wait waits for that copy.
#include <new>

#include "mmw_ctx.hpp"

static_assert(sizeof(mmw_track_report) == 324, "mmw_track_report: the ctypes / numpy layouts of mmwave_msc_amd/_lib.py");
static_assert(sizeof(mmw_track_event) == 16, "mmw_track_event: the ctypes / numpy layouts of mmwave_msc_amd/_lib.py");

void report_free(ReportCtx *r)
{
    if (!r) return;
    if (r->d_block) hipFree(r->d_block);
    if (r->h_counts) hipHostFree(r->h_counts);
    for (int k = 0; k < kTickets; k++) if (r->ev[k]) hipEventDestroy(r->ev[k]);
    delete r;
}

// mmw_reset / mmw_reset_scenes / mmw_restore: uids restart in the scenes flagged in dev_flags (device, [n_scenes]; nullptr = every
// scene).  Queued on the context's stream behind the kernel that emptied or refilled them; nothing at all while reports are off.
int report_rebase(mmw_ctx *c, const int32_t *dev_flags)
{
    if (!c->rep) return MMW_OK;
    launch_report_rebase(c->dc, c->rep->rs, dev_flags, c->stream);
    HIPCHK(c, hipGetLastError());
    return MMW_OK;
}

static int report_alloc(mmw_ctx *c)
{
    ReportCtx *r = new (std::nothrow) ReportCtx();
    if (!r) return fail(c, MMW_E_ARG, "out of host memory");
    const size_t S = c->dc.n_scenes, cap = c->dc.t_cap;
    const size_t words = S * cap + 3 * S + 2 * (S + 1) + 4;
    if (hipMalloc((void **)&r->d_block, words * sizeof(int32_t)) != hipSuccess) { report_free(r); return fail(c, MMW_E_HIP, "mmw_report_enable: hipMalloc(%zu B) failed", words * sizeof(int32_t)); }
    int32_t *p = reinterpret_cast<int32_t *>(r->d_block);
    r->rs.base_uid = p; p += S * cap;
    r->rs.base_len = p; p += S;
    r->rs.gen = p; p += S;
    r->rs.seen = p; p += S;
    r->rs.off = p; p += 2 * (S + 1);
    r->rs.totals = p;
    if (hipHostMalloc((void **)&r->h_counts, kTickets * 4 * sizeof(int32_t), hipHostMallocDefault) != hipSuccess) { report_free(r); return fail(c, MMW_E_HIP, "mmw_report_enable: hipHostMalloc failed"); }
    memset(r->h_counts, 0, kTickets * 4 * sizeof(int32_t));
    for (int k = 0; k < kTickets; k++)
        if (hipEventCreateWithFlags(&r->ev[k], hipEventDisableTiming) != hipSuccess) { report_free(r); return fail(c, MMW_E_HIP, "mmw_report_enable: hipEventCreate failed"); }
    c->rep = r;
    return MMW_OK;
}

int mmw_report_enable(mmw_ctx *c, int32_t on)
{
    if (!c) return MMW_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (!on) {
        if (!c->rep) return MMW_OK;
        HIPCHK(c, hipStreamSynchronize(c->stream));   // (a report or a rebase may still be queued on what is freed here)
        report_free(c->rep);
        c->rep = nullptr;
        return MMW_OK;
    }
    if (!c->rep) MMW_TRY(report_alloc(c));
    for (int k = 0; k < kTickets; k++) c->rep->issued[k] = false;
    launch_report_baseline(c->dc, c->st, c->rep->rs, c->stream);
    HIPCHK(c, hipGetLastError());
    return MMW_OK;
}

int mmw_report_async(mmw_ctx *c, mmw_track_report *rows, int32_t cap_rows, mmw_track_event *events, int32_t cap_events, int32_t scene_base,
                     int32_t ticket)
{
    if (!c) return MMW_E_ARG;
    if (!c->rep) return fail(c, MMW_E_ARG, "mmw_report: reports are not enabled (mmw_report_enable)");
    if (cap_rows < 0 || cap_events < 0 || (cap_rows > 0 && !rows) || (cap_events > 0 && !events))
        return fail(c, MMW_E_ARG, "mmw_report: cap_rows = %d, cap_events = %d with rows %s, events %s", cap_rows, cap_events, rows ? "set" : "NULL", events ? "set" : "NULL");
    if (((uintptr_t)rows & 3) != 0 || ((uintptr_t)events & 3) != 0) return fail(c, MMW_E_ARG, "mmw_report: the buffers must be 4-byte aligned");
    if (ticket < 0 || ticket >= kTickets) return fail(c, MMW_E_ARG, "mmw_report: ticket %d outside [0, %d)", ticket, kTickets);
    HIPCHK(c, hipSetDevice(c->device));
    ReportCtx *r = c->rep;
    launch_report(c->dc, sites_or_null(c), c->st, r->rs, rows, cap_rows, events, cap_events, scene_base, c->stream);
    HIPCHK(c, hipGetLastError());
    // the counts and the capacity decision follow the kernels into pinned memory: mmw_report_wait(ticket) waits for THIS copy only
    HIPCHK(c, hipMemcpyAsync(r->h_counts + ticket * 4, r->rs.totals, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(r->ev[ticket], c->stream));
    r->issued[ticket] = true;
    return MMW_OK;
}

int mmw_report_wait(mmw_ctx *c, int32_t ticket, int32_t *n_rows, int32_t *n_events)
{
    if (!c) return MMW_E_ARG;
    if (!c->rep) return fail(c, MMW_E_ARG, "mmw_report_wait: reports are not enabled (mmw_report_enable)");
    if (ticket < 0 || ticket >= kTickets) return fail(c, MMW_E_ARG, "mmw_report_wait: ticket %d outside [0, %d)", ticket, kTickets);
    ReportCtx *r = c->rep;
    if (!r->issued[ticket]) return fail(c, MMW_E_ARG, "mmw_report_wait: no report outstanding under ticket %d", ticket);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipEventSynchronize(r->ev[ticket]));
    r->issued[ticket] = false;
    const int32_t *h = r->h_counts + ticket * 4;
    if (n_rows) *n_rows = h[0];
    if (n_events) *n_events = h[1];
    if (!h[2]) return fail(c, MMW_E_CAPACITY, "mmw_report: %d live rows and %d events do not fit the buffers: nothing was written, the baseline is unchanged", h[0], h[1]);
    return MMW_OK;
}

int mmw_report(mmw_ctx *c, mmw_track_report *rows, int32_t cap_rows, mmw_track_event *events, int32_t cap_events, int32_t scene_base,
               int32_t *n_rows, int32_t *n_events)
{
    const int rc = mmw_report_async(c, rows, cap_rows, events, cap_events, scene_base, kTickets - 1);
    return rc ? rc : mmw_report_wait(c, kTickets - 1, n_rows, n_events);
}
