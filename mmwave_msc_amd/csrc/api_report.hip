// api_report.hip -- the C-ABI (include/mmw.h): the live-track report.  mmw_report_enable owns the baseline, mmw_report_async queues
// the kernels of k_report.hip and the copy of the two counts, mmw_report_wait waits for that copy.
#include "mmw_ctx.hpp"

static_assert(sizeof(mmw_track_report) == 324, "mmw_track_report: the ctypes / numpy layouts of mmwave_msc_amd/_lib.py");
static_assert(sizeof(mmw_track_event) == 16, "mmw_track_event: the ctypes / numpy layouts of mmwave_msc_amd/_lib.py");

// the baseline lies in front of the scratch, in the same device block
static int report_alloc(mmw_ctx *c)
{
    const size_t S = c->dc.n_scenes, cap = c->dc.t_cap;
    MMW_TRY(export_alloc(c, c->rep, S * cap + 3 * S, "mmw_report_enable"));
    int32_t *p = reinterpret_cast<int32_t *>(c->rep.d_block);
    c->rs.base.base_uid = p; p += S * cap;
    c->rs.base.base_len = p; p += S;
    c->rs.base.ug.gen = p; p += S;
    c->rs.base.ug.seen = p;
    c->rs.sc = c->rep.sc;
    return MMW_OK;
}

int mmw_report_enable(mmw_ctx *c, int32_t on)
{
    if (!c) return MMW_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (!on) {
        if (!c->rep.d_block) return MMW_OK;
        HIPCHK(c, hipStreamSynchronize(c->stream));   // (a report or a rebase may still be queued on what is freed here)
        export_free(c->rep);
        c->rs = ReportState();
        return MMW_OK;
    }
    if (!c->rep.d_block) MMW_TRY(report_alloc(c));
    for (int k = 0; k < kTickets; k++) c->rep.issued[k] = false;
    launch_report_baseline(c->dc, c->st, c->rs, c->stream);
    HIPCHK(c, hipGetLastError());
    return MMW_OK;
}

static const PairExport kExport = {"mmw_report", "reports are not enabled (mmw_report_enable)", "no report", "live rows", kUnfitBaseline, 4};

int mmw_report_async(mmw_ctx *c, mmw_track_report *rows, int32_t cap_rows, mmw_track_event *events, int32_t cap_events, int32_t scene_base,
                     int32_t ticket)
{
    if (!c) return MMW_E_ARG;
    MMW_TRY(pair_export_begin(c, c->rep, kExport, rows, cap_rows, events, cap_events, ticket));
    launch_report(c->dc, sites_or_null(c), c->st, c->rs, rows, cap_rows, events, cap_events, scene_base, c->stream);
    return export_issue(c, c->rep, ticket);
}

int mmw_report_wait(mmw_ctx *c, int32_t ticket, int32_t *n_rows, int32_t *n_events)
{
    return c ? pair_export_wait(c, c->rep, kExport, ticket, n_rows, n_events) : MMW_E_ARG;
}

int mmw_report(mmw_ctx *c, mmw_track_report *rows, int32_t cap_rows, mmw_track_event *events, int32_t cap_events, int32_t scene_base,
               int32_t *n_rows, int32_t *n_events)
{
    const int rc = mmw_report_async(c, rows, cap_rows, events, cap_events, scene_base, kTickets - 1);
    return rc ? rc : mmw_report_wait(c, kTickets - 1, n_rows, n_events);
}
