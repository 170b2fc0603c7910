// api_heat.hip -- the C-ABI (include/mmw.h): the dwell heat maps.  mmw_heat_enable owns the grid table, the cells, the uid slots and
// the scene words, mmw_set_heat_grids checks the grids on the host, mmw_heat_sample queues the one kernel that accumulates,
// mmw_heat_async queues the export kernels of k_heat.hip and the copy of the two counts, mmw_heat_wait waits for that copy.
#include <cmath>
#include "mmw_scene_table.hpp"

static_assert(sizeof(mmw_heat_grid) == 48, "mmw_heat_grid: the numpy layout of mmwave_msc_amd/_lib.py");
static_assert(sizeof(mmw_heat_row) == 48, "mmw_heat_row: the numpy layout of mmwave_msc_amd/_lib.py");
static_assert(sizeof(mmw_heat_cell) == 24, "mmw_heat_cell: the numpy layout of mmwave_msc_amd/_lib.py");
static_assert(sizeof(HeatGrid) == 48 && sizeof(HeatScene) == 24, "the device's table entry and scene words");

void heat_free(mmw_ctx *c)
{
    export_free(c->heat);
    scene_table_free(c->htab);
    c->hs = HeatState();
}

int mmw_heat_enable(mmw_ctx *c, int32_t cells)
{
    if (!c) return fail(nullptr, MMW_E_ARG, "mmw_heat_enable: null context");
    if (cells < 0 || cells > MMW_HEAT_CELLS_MAX) return fail(c, MMW_E_ARG, "mmw_heat_enable: cells = %d outside 0 .. %d", cells, MMW_HEAT_CELLS_MAX);
    HIPCHK(c, hipSetDevice(c->device));
    if (cells == 0) {
        if (!c->heat.d_block) return MMW_OK;
        HIPCHK(c, hipStreamSynchronize(c->stream));   // (a sample, an export or a rebase may still be queued on what is freed here)
        heat_free(c);
        return MMW_OK;
    }
    // The new state is allocated and cleared BEFORE the old one goes: a failure leaves an earlier enablement as it was.  One block, the
    // state in front of the scratch, the cells first (with cells a multiple of 4 every scene's `samples` start on 16 bytes):
    // [S][cells] dwell (fp64) | samples | visits | [S][t_cap] last_t (fp64) | [S] scene words | [S][t_cap] owner | last_cell | [S] gen | seen | ordinal
    const size_t S = c->dc.n_scenes, n = S * c->dc.t_cap, nc = S * (size_t)cells;
    const size_t cell_bytes = nc * (sizeof(double) + 2 * sizeof(int32_t)), time_bytes = n * sizeof(double), scene_bytes = S * sizeof(HeatScene);
    const size_t words = (cell_bytes + time_bytes + scene_bytes) / sizeof(int32_t) + 2 * n + 3 * S;
    ExportCtx nx;
    MMW_TRY(export_alloc(c, nx, words, "mmw_heat_enable"));
    decltype(c->htab) tab;
    if (const int rc = scene_table_alloc(c, tab, "mmw_heat_enable")) {
        export_free(nx);
        return rc;
    }
    HeatState hs = {};
    hs.cells = cells;
    hs.grids = tab.entries();
    hs.n_grids = tab.counts(S);
    hs.dwell = reinterpret_cast<double *>(nx.d_block);
    hs.samples = reinterpret_cast<int32_t *>(hs.dwell + nc);
    hs.visits = hs.samples + nc;
    hs.last_t = reinterpret_cast<double *>(nx.d_block + cell_bytes);
    hs.scene = reinterpret_cast<HeatScene *>(nx.d_block + cell_bytes + time_bytes);
    int32_t *p = reinterpret_cast<int32_t *>(nx.d_block + cell_bytes + time_bytes + scene_bytes);
    hs.ug.owner = p; p += n;
    hs.last_cell = p; p += n;
    hs.ug.gen = p; p += S;
    hs.ug.seen = p; p += S;
    hs.ug.ordinal = p;
    hs.sc = nx.sc;
    // every scene at 0 grids, every cell and word 0, every slot free
    hipError_t e = hipMemsetAsync(tab.d_tab, 0, tab.bytes(S), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(nx.d_block, 0, cell_bytes + time_bytes + scene_bytes, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(hs.ug.owner, 0xff, n * sizeof(int32_t), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(hs.last_cell, 0, (n + 3 * S) * sizeof(int32_t), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // (... and whatever was queued on an earlier enablement's state has run)
    if (e != hipSuccess) {
        export_free(nx);
        scene_table_free(tab);
        return fail(c, MMW_E_HIP, "mmw_heat_enable: %s", hipGetErrorString(e));
    }
    heat_free(c);
    c->heat = nx;
    c->hs = hs;
    c->htab = std::move(tab);
    return MMW_OK;
}

// what the device reads of a grid: the caller's values as they are
static HeatGrid as_given(const mmw_heat_grid &g)
{
    HeatGrid d = {};
    d.x0 = g.x0;
    d.y0 = g.y0;
    d.cell = g.cell;
    d.max_gap = g.max_gap;
    d.nx = g.nx;
    d.ny = g.ny;
    d.id = g.id;
    return d;
}

int mmw_set_heat_grids(mmw_ctx *c, const int32_t *scenes, int32_t n, const int32_t *n_grids, const mmw_heat_grid *grids)
{
    if (!c) return fail(nullptr, MMW_E_ARG, "mmw_set_heat_grids: null context");
    if (!c->heat.d_block) return fail(c, MMW_E_ARG, "mmw_set_heat_grids: heat maps are not enabled (mmw_heat_enable)");
    // every check first: a refused call changes no scene's grid
    const int32_t cap = c->hs.cells;
    MMW_TRY(scene_table_check<decltype(c->htab)>(c, {"mmw_set_heat_grids", "n_grids", "grids"}, scenes, n, n_grids, grids, [c, cap](int i, int s, int z, const mmw_heat_grid &q) {
        if (q.reserved_ != 0) return fail(c, MMW_E_ARG, "mmw_set_heat_grids: entry %d (scene %d) grid %d has a non-zero reserved_", i, s, z);
        if (!std::isfinite(q.x0) || !std::isfinite(q.y0) || !std::isfinite(q.cell))
            return fail(c, MMW_E_ARG, "mmw_set_heat_grids: entry %d (scene %d) grid %d has an x0, y0 or cell that is not finite", i, s, z);
        if (!(q.cell > 0.0)) return fail(c, MMW_E_ARG, "mmw_set_heat_grids: entry %d (scene %d) grid %d has cell <= 0", i, s, z);
        if (!(q.max_gap > 0.0)) return fail(c, MMW_E_ARG, "mmw_set_heat_grids: entry %d (scene %d) grid %d has a max_gap that is NaN or <= 0", i, s, z);
        if (q.nx < 1 || q.ny < 1) return fail(c, MMW_E_ARG, "mmw_set_heat_grids: entry %d (scene %d) grid %d has nx = %d, ny = %d: both must be >= 1", i, s, z, q.nx, q.ny);
        if ((long long)q.nx * (long long)q.ny > (long long)cap)
            return fail(c, MMW_E_ARG, "mmw_set_heat_grids: entry %d (scene %d) grid %d has %d x %d cells, %d are enabled (mmw_heat_enable)", i, s, z, q.nx, q.ny, cap);
        return MMW_OK;
    }));
    HIPCHK(c, hipSetDevice(c->device));
    // the generation bump is of the heat word alone; the listed scenes' cells and scene words restart behind it
    return scene_table_send(c, c->htab, "mmw_set_heat_grids", scenes, n, n_grids, grids, as_given, c->hs.ug.gen,
                            [c](const int32_t *flags) { launch_heat_zero(c->dc.n_scenes, flags, c->hs, c->stream); });
}

int mmw_get_heat_grids(mmw_ctx *c, int32_t *n_grids, mmw_heat_grid *grids)
{
    if (!c) return fail(nullptr, MMW_E_ARG, "mmw_get_heat_grids: null context");
    scene_table_get(c->htab, (size_t)c->dc.n_scenes, n_grids, grids);
    return MMW_OK;
}

int mmw_heat_sample(mmw_ctx *c, const int32_t *scene_flags, const double *t)
{
    if (!c) return MMW_E_ARG;
    MMW_TRY(sample_begin(c, c->heat, "mmw_heat", "heat maps", scene_flags, t));
    launch_heat_sample(c->dc, c->st, c->hs, scene_flags, t, c->stream);
    HIPCHK(c, hipGetLastError());
    return MMW_OK;
}

static const PairExport kExport = {"mmw_heat", "heat maps are not enabled (mmw_heat_enable)", "no heat export", "rows",
                                    "do not fit the buffers: nothing was written, nothing was cleared", 8, "cells"};

int mmw_heat_async(mmw_ctx *c, mmw_heat_row *rows, int32_t cap_rows, mmw_heat_cell *cells, int32_t cap_cells, const int32_t *scene_flags, int32_t mode,
                   int32_t scene_base, int32_t ticket)
{
    if (!c) return MMW_E_ARG;
    MMW_TRY(pair_export_begin(c, c->heat, kExport, rows, cap_rows, cells, cap_cells, ticket));
    if (((uintptr_t)scene_flags & 3) != 0) return fail(c, MMW_E_ARG, "mmw_heat: scene_flags must be 4-byte aligned");
    if (mode != MMW_HEAT_KEEP && mode != MMW_HEAT_CLEAR) return fail(c, MMW_E_ARG, "mmw_heat: mode = %d is neither MMW_HEAT_KEEP nor MMW_HEAT_CLEAR", mode);
    launch_heat(c->dc, c->hs, rows, cap_rows, cells, cap_cells, scene_flags, mode, scene_base, c->stream);
    return export_issue(c, c->heat, ticket);
}

int mmw_heat_wait(mmw_ctx *c, int32_t ticket, int32_t *n_rows, int32_t *n_cells)
{
    return c ? pair_export_wait(c, c->heat, kExport, ticket, n_rows, n_cells) : MMW_E_ARG;
}

int mmw_heat(mmw_ctx *c, mmw_heat_row *rows, int32_t cap_rows, mmw_heat_cell *cells, int32_t cap_cells, const int32_t *scene_flags, int32_t mode,
             int32_t scene_base, int32_t *n_rows, int32_t *n_cells)
{
    const int rc = mmw_heat_async(c, rows, cap_rows, cells, cap_cells, scene_flags, mode, scene_base, kTickets - 1);
    return rc ? rc : mmw_heat_wait(c, kTickets - 1, n_rows, n_cells);
}
