// api_stance.hip -- the C-ABI (include/mmw.h): the stance watch.  mmw_stance_enable owns the rule table, the uid slots, the counters
// and the event rings, mmw_set_stance_rules derives the table on the host, mmw_stance_sample queues the one kernel that decides the
// classes, mmw_stance_async queues the export kernels of k_stance.hip and the copy of the two counts, mmw_stance_wait waits for
// that copy.
#include <cmath>
#include "mmw_scene_table.hpp"

static_assert(sizeof(mmw_stance_rule) == 64, "mmw_stance_rule: the numpy layout of mmwave_msc_amd/_lib.py");
static_assert(sizeof(mmw_stance_row) == 48, "mmw_stance_row: the numpy layout of mmwave_msc_amd/_lib.py");
static_assert(sizeof(mmw_stance_event) == 32, "mmw_stance_event: the numpy layout of mmwave_msc_amd/_lib.py");
static_assert(sizeof(StanceRule) == 80 && sizeof(StanceCount) == 16, "the device's table entry and counters");

void stance_free(mmw_ctx *c)
{
    export_free(c->stance);
    scene_table_free(c->sttab);
    c->ss = StanceState();
}

int mmw_stance_enable(mmw_ctx *c, int32_t log_depth)
{
    if (!c) return fail(nullptr, MMW_E_ARG, "mmw_stance_enable: null context");
    if (log_depth < 0 || log_depth > MMW_STANCE_LOG_MAX)
        return fail(c, MMW_E_ARG, "mmw_stance_enable: log_depth = %d outside 0 .. %d", log_depth, MMW_STANCE_LOG_MAX);
    HIPCHK(c, hipSetDevice(c->device));
    if (log_depth == 0) {
        if (!c->stance.d_block) return MMW_OK;
        HIPCHK(c, hipStreamSynchronize(c->stream));   // (a sample, an export or a rebase may still be queued on what is freed here)
        stance_free(c);
        return MMW_OK;
    }
    // The new state is allocated and cleared BEFORE the old one goes: a failure leaves an earlier enablement as it was.  One block, the
    // state in front of the scratch, the 8-byte words first:
    // [S][depth] events | [S][t_cap] t_since | t_upright | [S] counters | [S][t_cap] owner | word | [S] logged | taken | gen | seen | ordinal
    const size_t S = c->dc.n_scenes, n = S * c->dc.t_cap;
    const size_t ring_bytes = S * (size_t)log_depth * sizeof(mmw_stance_event), time_bytes = 2 * n * sizeof(double), count_bytes = S * sizeof(StanceCount);
    const size_t words = (ring_bytes + time_bytes + count_bytes) / sizeof(int32_t) + 2 * n + 5 * S;
    ExportCtx nx;
    MMW_TRY(export_alloc(c, nx, words, "mmw_stance_enable"));
    decltype(c->sttab) tab;
    if (const int rc = scene_table_alloc(c, tab, "mmw_stance_enable")) {
        export_free(nx);
        return rc;
    }
    StanceState ss = {};
    ss.rules = tab.entries();
    ss.n_rules = tab.counts(S);
    ss.t_since = reinterpret_cast<double *>(nx.d_block + ring_bytes);
    ss.t_upright = ss.t_since + n;
    ss.count = reinterpret_cast<StanceCount *>(nx.d_block + ring_bytes + time_bytes);
    int32_t *p = reinterpret_cast<int32_t *>(nx.d_block + ring_bytes + time_bytes + count_bytes);
    ss.ug.owner = p; p += n;
    ss.word = p; p += n;
    evlog_carve(ss.log, ss.ug, log_depth, nx.d_block, p, S);
    ss.sc = nx.sc;
    // every scene at 0 rules, every slot free, every word 0 (the rings need no clearing: an entry is written before `logged` lets anybody
    // read it; a newcomer's t_upright = -inf is the sample kernel's)
    hipError_t e = hipMemsetAsync(tab.d_tab, 0, tab.bytes(S), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(ss.t_since, 0, time_bytes + count_bytes, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(ss.ug.owner, 0xff, n * sizeof(int32_t), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(ss.word, 0, (n + 5 * S) * sizeof(int32_t), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // (... and whatever was queued on an earlier enablement's state has run)
    if (e != hipSuccess) {
        export_free(nx);
        scene_table_free(tab);
        return fail(c, MMW_E_HIP, "mmw_stance_enable: %s", hipGetErrorString(e));
    }
    stance_free(c);
    c->stance = nx;
    c->ss = ss;
    c->sttab = std::move(tab);
    return MMW_OK;
}

// what the device reads of a rule: one fp64 operation each (this file is compiled with -ffp-contract=off like the kernels)
static StanceRule derive(const mmw_stance_rule &r)
{
    StanceRule d = {};
    d.h_stand = r.h_stand;
    d.h_lie = r.h_lie;
    d.up_hi = r.h_stand + r.margin;
    d.up_lo = r.h_stand - r.margin;
    d.lie_hi = r.h_lie + r.margin;
    d.lie_lo = r.h_lie - r.margin;
    d.gap2 = r.max_gap * r.max_gap;
    d.fall_window = r.fall_window;
    d.long_lie = r.long_lie;
    d.id = r.id;
    return d;
}

int mmw_set_stance_rules(mmw_ctx *c, const int32_t *scenes, int32_t n, const int32_t *n_rules, const mmw_stance_rule *rules)
{
    if (!c) return fail(nullptr, MMW_E_ARG, "mmw_set_stance_rules: null context");
    if (!c->stance.d_block) return fail(c, MMW_E_ARG, "mmw_set_stance_rules: stance is not enabled (mmw_stance_enable)");
    // every check first: a refused call changes no scene's rule
    MMW_TRY(scene_table_check<decltype(c->sttab)>(c, {"mmw_set_stance_rules", "n_rules", "rules"}, scenes, n, n_rules, rules, [c](int i, int s, int z, const mmw_stance_rule &q) {
        if (q.reserved_ != 0) return fail(c, MMW_E_ARG, "mmw_set_stance_rules: entry %d (scene %d) rule %d has a non-zero reserved_", i, s, z);
        if (!std::isfinite(q.h_stand) || !std::isfinite(q.h_lie) || !std::isfinite(q.margin) || !std::isfinite(q.fall_window) || !std::isfinite(q.max_gap))
            return fail(c, MMW_E_ARG, "mmw_set_stance_rules: entry %d (scene %d) rule %d has a height, margin, fall_window or max_gap that is not finite", i, s, z);
        if (!(q.margin >= 0.0) || !(q.fall_window >= 0.0))
            return fail(c, MMW_E_ARG, "mmw_set_stance_rules: entry %d (scene %d) rule %d has a negative margin or fall_window", i, s, z);
        if (!(q.long_lie >= 0.0)) return fail(c, MMW_E_ARG, "mmw_set_stance_rules: entry %d (scene %d) rule %d has a long_lie that is negative or NaN", i, s, z);
        if (!(q.max_gap > 0.0)) return fail(c, MMW_E_ARG, "mmw_set_stance_rules: entry %d (scene %d) rule %d has max_gap <= 0", i, s, z);
        const StanceRule d = derive(q);
        if (!(d.lie_hi < d.up_lo))
            return fail(c, MMW_E_ARG, "mmw_set_stance_rules: entry %d (scene %d) rule %d has h_lie + margin not below h_stand - margin", i, s, z);
        return MMW_OK;
    }));
    HIPCHK(c, hipSetDevice(c->device));
    // the generation bump is of the stance word alone; the listed scenes' counters restart behind it
    return scene_table_send(c, c->sttab, "mmw_set_stance_rules", scenes, n, n_rules, rules, derive, c->ss.ug.gen,
                            [c](const int32_t *flags) { launch_stance_zero(c->dc.n_scenes, flags, c->ss, c->stream); });
}

int mmw_get_stance_rules(mmw_ctx *c, int32_t *n_rules, mmw_stance_rule *rules)
{
    if (!c) return fail(nullptr, MMW_E_ARG, "mmw_get_stance_rules: null context");
    scene_table_get(c->sttab, (size_t)c->dc.n_scenes, n_rules, rules);
    return MMW_OK;
}

int mmw_stance_sample(mmw_ctx *c, const int32_t *scene_flags, const double *t)
{
    if (!c) return MMW_E_ARG;
    MMW_TRY(sample_begin(c, c->stance, "mmw_stance", "stance rules", scene_flags, t));
    launch_stance_sample(c->dc, c->st, c->ss, scene_flags, t, c->stream);
    HIPCHK(c, hipGetLastError());
    return MMW_OK;
}

static const PairExport kExport = {"mmw_stance", "stance is not enabled (mmw_stance_enable)", "no stance export", "rows", kUnfitLog, 8};

int mmw_stance_async(mmw_ctx *c, mmw_stance_row *rows, int32_t cap_rows, mmw_stance_event *events, int32_t cap_events, int32_t scene_base, int32_t ticket)
{
    if (!c) return MMW_E_ARG;
    MMW_TRY(pair_export_begin(c, c->stance, kExport, rows, cap_rows, events, cap_events, ticket));
    launch_stance(c->dc, c->ss, rows, cap_rows, events, cap_events, scene_base, c->stream);
    return export_issue(c, c->stance, ticket);
}

int mmw_stance_wait(mmw_ctx *c, int32_t ticket, int32_t *n_rows, int32_t *n_events)
{
    return c ? pair_export_wait(c, c->stance, kExport, ticket, n_rows, n_events) : MMW_E_ARG;
}

int mmw_stance(mmw_ctx *c, mmw_stance_row *rows, int32_t cap_rows, mmw_stance_event *events, int32_t cap_events, int32_t scene_base, int32_t *n_rows,
               int32_t *n_events)
{
    const int rc = mmw_stance_async(c, rows, cap_rows, events, cap_events, scene_base, kTickets - 1);
    return rc ? rc : mmw_stance_wait(c, kTickets - 1, n_rows, n_events);
}
