// k_heat.hip -- the dwell heat maps (mmw_heat_*): per scene zero or one grid of nx x ny cells, per cell the time live tracks spent in
// it, the samples taken in it and the visits that began in it; per live uid the cell and time of its previous sample.  The first
// consumer whose state is a dense per-scene array: the sampler touches a few words per live track, the export is a stream compaction
// over every cell of the exported scenes.  Reads SceneHdr, order and one line of each live TrackRec after the step; nothing of the
// step is touched.  No LDS, no atomics: a wave per scene, four scenes per workgroup.  In the sampler a lane per track AND per uid
// slot (t_cap <= 64) -- lane i holds track i's uid and cell, lane j slot j's words; uid -> slot is the one slot table's
// uid_slots_pick() (mmw_uidlist.hpp); the scene's grid comes through scalar loads.  In the export the wave strides over the scene's
// cells, 64 consecutive words a load.
//   k_uid_rebase    (k_scan.hip) mmw_reset / mmw_reset_scenes / mmw_restore / mmw_set_heat_grids: the touched scenes' generation word
//   k_heat_zero     mmw_set_heat_grids: the listed scenes' cells and scene words
//   k_heat_sample   free the slots of uids that are gone, hand free slots to the newcomers, every track's cell; tracks that share a
//                   cell are resolved inside the wave, in list order
//   k_heat_count    rows (= asked scenes with a grid) and cells with samples > 0 per scene
//   k_pair_scan     (k_scan.hip) one workgroup: the two offset scans, the capacity decision, the totals
//   k_heat_write    the row, the kept cells in cell order at base + mbcnt(ballot); MMW_HEAT_CLEAR: zeros behind them -- only if everything fits
#include <cstddef>
#include "mmw_device.hpp"
#include "mmw_uidlist.hpp"
#include "mmw_wave.hpp"
#include "mmw_kernels.hpp"

namespace mmw {

static_assert(sizeof(mmw_heat_grid) == 48 && alignof(mmw_heat_grid) == 8 && sizeof(HeatGrid) == 48, "mmw_heat_grid: the table entry is the caller's");
static_assert(offsetof(mmw_heat_grid, max_gap) == offsetof(HeatGrid, max_gap) && offsetof(mmw_heat_grid, nx) == offsetof(HeatGrid, nx) &&
              offsetof(mmw_heat_grid, id) == offsetof(HeatGrid, id), "mmw_heat_grid: the table entry is the caller's");
static_assert(sizeof(mmw_heat_row) == 48 && alignof(mmw_heat_row) == 8 && offsetof(mmw_heat_row, t_first) == 32, "mmw_heat_row");
static_assert(sizeof(mmw_heat_cell) == 24 && alignof(mmw_heat_cell) == 8 && offsetof(mmw_heat_cell, dwell) == 16, "mmw_heat_cell");
static_assert(sizeof(HeatScene) == 24, "the scene words");
static_assert(MMW_HEAT_GRIDS_MAX == 1, "one grid per scene: the table entry of scene s is grids[s]");
static_assert(MMW_HEAT_CELLS_MAX <= 4096, "a scene's kept cells stay below 2^13");
static_assert(MMW_TRACK_CAP_LIMIT <= 64, "one lane per track, one lane per uid slot");

// The cells of scene s that exist: nx * ny of its grid, 0 without one.  Clamped into the allocation, so a damaged table reads and
// writes nothing outside it.  (wave-uniform: s is)
__device__ __forceinline__ int scene_cells(const HeatState &hs, int s)
{
    if (min(max(hs.n_grids[s], 0), MMW_HEAT_GRIDS_MAX) == 0) return 0;
    const long long n = (long long)hs.grids[s].nx * (long long)hs.grids[s].ny;
    return (int)min(max(n, 0LL), (long long)hs.cells);
}

// lane k's double, k scalar: two v_readlane (uid_find's note on __shfl)
__device__ __forceinline__ double readlane_f64(double v, int k)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), k), __builtin_amdgcn_readlane(__double2loint(v), k));
}

__global__ __launch_bounds__(256) void k_heat_zero(int n_scenes, const int32_t *__restrict__ flags, HeatState hs)
{
    const auto [s, lane] = wave_scene();
    if (s >= n_scenes || !flags[s]) return;   // (wave-uniform)
    const size_t c0 = (size_t)s * hs.cells;
    for (int i = lane; i < hs.cells; i += 64) {
        hs.dwell[c0 + i] = 0.0;
        hs.samples[c0 + i] = 0;
        hs.visits[c0 + i] = 0;
    }
    if (lane == 0) hs.scene[s] = HeatScene{0, 0, 0.0, 0.0};
}

__global__ __launch_bounds__(256) void k_heat_sample(DevCfg cfg, DevState st, HeatState hs, const int32_t *__restrict__ flags, const double *__restrict__ t)
{
    const auto [s, lane] = wave_scene();
    if (s >= cfg.n_scenes) return;     // (wave-uniform)
    if (flags && !flags[s]) return;    // (wave-uniform) not asked: not touched
    const int ord = hs.ug.ordinal[s];
    const int n_cells = scene_cells(hs, s);
    if (n_cells == 0) {                // (wave-uniform) no grid: the scene's slots are void until it has one, and then rebased
        uid_slots_done(hs.ug, s, lane, 0, false, ord);
        return;
    }
    const int cap = cfg.t_cap, T = live_tracks(cfg, st, s);
    const size_t base = (size_t)s * cap, c0 = (size_t)s * hs.cells;
    const bool rebased = hs.ug.rebased(s);
    const double tt = t ? t[s] : (double)ord;
    // the grid: the same address in every lane, so scalar loads
    const HeatGrid *g = hs.grids + s;
    const double x0 = g->x0, y0 = g->y0, side = g->cell, max_gap = g->max_gap;
    const int nx = g->nx, ny = g->ny;
    const HeatScene old_words = hs.scene[s];

    // this lane's track: the uid and its cell ...
    int cuid = -1, c = -1;
    if (lane < T) {
        const TrackRec *rec = st.trk + base + live_slot(cfg, st, s, lane);
        cuid = rec->uid;
        const double fx = (rec->x[0] - x0) / side, fy = (rec->x[1] - y0) / side;
        const bool inside = fx >= 0.0 && fx < (double)nx && fy >= 0.0 && fy < (double)ny;   // (a NaN: false)
        if (inside) c = (int)fy * nx + (int)fx;
        if (c >= n_cells) c = -1;      // (never with a table the host checked)
    }
    // ... and this lane's slot: every old word is in a register before anything is stored
    int raw_owner = -1, s_cell = -1;
    double s_t = 0.0;
    if (lane < cap) {
        raw_owner = hs.ug.owner[base + lane];
        s_cell = hs.last_cell[base + lane];
        s_t = hs.last_t[base + lane];
    }
    // ... and the cell's words, in every lane that has one (lanes of one cell load the same words)
    double dwell = 0.0;
    int samples = 0, visits = 0;
    if (c >= 0) {
        dwell = hs.dwell[c0 + c];
        samples = hs.samples[c0 + c];
        visits = hs.visits[c0 + c];
    }
    const auto [slot, fresh, release] = uid_slots_pick(cuid, raw_owner, rebased, T, cap, lane);   // (all 64 lanes)

    // the words of this lane's TRACK come out of its slot's lane (all 64 lanes, ahead of any condition)
    const int from_lane = slot < 0 ? lane : slot;
    const int last_cell = __shfl(s_cell, from_lane);
    const double last_t = __shfl(s_t, from_lane);
    const bool visit = fresh || last_cell != c;
    const double dt = tt - last_t;
    const bool credit = !fresh && dt > 0.0 && dt <= max_gap;   // (a NaN dt: false)

    // Tracks that share a cell: every lane walks the T tracks in list order and takes what those of ITS cell add -- one defined
    // sequence of fp64 additions per cell --, and the first lane of a cell stores it.  k is scalar: the broadcasts are v_readlane.
    bool leader = c >= 0;
    for (int k = 0; k < T; k++) {      // (uniform)
        const int ck = __builtin_amdgcn_readlane(c, k);
        const int vk = __builtin_amdgcn_readlane((int)visit, k), qk = __builtin_amdgcn_readlane((int)credit, k);
        const double dk = readlane_f64(dt, k);
        const bool mine = c >= 0 && ck == c;
        samples += mine ? 1 : 0;
        visits += (mine && vk) ? 1 : 0;
        dwell = (mine && qk) ? dwell + dk : dwell;
        leader = (mine && k < lane) ? false : leader;
    }
    const int n_out = __popcll(__ballot(lane < T && c < 0));

    if (leader) {                      // (one lane per touched cell: no word has two writers)
        hs.dwell[c0 + c] = dwell;
        hs.samples[c0 + c] = samples;
        hs.visits[c0 + c] = visits;
    }
    if (lane < T && slot >= 0) {       // (a track writes its own slot, all three words)
        hs.ug.owner[base + slot] = cuid;
        hs.last_cell[base + slot] = c;
        hs.last_t[base + slot] = tt;
    }
    if (lane == 0) hs.scene[s] = HeatScene{old_words.calls + 1, old_words.outside + n_out, old_words.calls == 0 ? tt : old_words.t_first, tt};
    uid_slots_done(hs.ug, s, lane, base + lane, release, ord);
}

// whether the export covers scene s, and then its cells (wave-uniform)
__device__ __forceinline__ int export_cells(const HeatState &hs, const int32_t *flags, int s) { return (flags && !flags[s]) ? 0 : scene_cells(hs, s); }

__global__ __launch_bounds__(256) void k_heat_count(DevCfg cfg, HeatState hs, const int32_t *__restrict__ flags)
{
    const auto [s, lane] = wave_scene();
    if (s >= cfg.n_scenes) return;   // (wave-uniform)
    const int n = export_cells(hs, flags, s);
    const int32_t *smp = hs.samples + (size_t)s * hs.cells;
    int kept = 0;
    int i0 = 0;
    if ((hs.cells & 3) == 0) {       // (uniform over the launch) every scene's words start on 16 bytes: four a lane, 1 KiB a load
        const int4 *smp4 = reinterpret_cast<const int4 *>(smp);
        const int n4 = n >> 2;
        for (int i = lane; i - lane < n4; i += 64) {   // (uniform trip count: the ballots are of all 64 lanes)
            int4 v = make_int4(0, 0, 0, 0);
            if (i < n4) v = smp4[i];
            kept += __popcll(__ballot(v.x > 0)) + __popcll(__ballot(v.y > 0)) + __popcll(__ballot(v.z > 0)) + __popcll(__ballot(v.w > 0));
        }
        i0 = n4 << 2;
    }
    for (int i = i0 + lane; i - lane < n; i += 64) {
        const int v = i < n ? smp[i] : 0;
        kept += __popcll(__ballot(v > 0));
    }
    if (lane == 0) {
        hs.sc.off[s] = n > 0 ? 1 : 0;
        hs.sc.off[cfg.n_scenes + 1 + s] = kept;
    }
}

template <bool CLEAR>
__global__ __launch_bounds__(256) void k_heat_write(DevCfg cfg, HeatState hs, mmw_heat_row *__restrict__ rows, mmw_heat_cell *__restrict__ cells,
                                                    const int32_t *__restrict__ flags, int scene_base)
{
    if (!hs.sc.totals[2]) return;    // (uniform over the launch) something does not fit: neither buffer is written, nothing is cleared
    const auto [s, lane] = wave_scene();
    const int S = cfg.n_scenes;
    if (s >= S) return;              // (wave-uniform)
    const int n = export_cells(hs, flags, s);
    if (n == 0) return;              // (wave-uniform) no row
    const int row0 = hs.sc.off[s], first = hs.sc.off[S + 1 + s];
    const size_t c0 = (size_t)s * hs.cells;
    const unsigned long long below = (1ull << lane) - 1ull;
    int run = first;                 // (scalar: the ballots' popcounts)
    for (int i = lane; i - lane < n; i += 64) {   // (uniform trip count)
        const int smp = i < n ? hs.samples[c0 + i] : 0;
        const bool keep = smp > 0;
        const unsigned long long b = __ballot(keep);
        if (keep) {                  // a kept cell lands behind the kept cells before it: cell order without a sort
            cells[run + __popcll(b & below)] = mmw_heat_cell{scene_base + s, i, smp, hs.visits[c0 + i], hs.dwell[c0 + i]};
            if (CLEAR) {             // (a cell without a sample holds zeros already)
                hs.samples[c0 + i] = 0;
                hs.visits[c0 + i] = 0;
                hs.dwell[c0 + i] = 0.0;
            }
        }
        run += __popcll(b);
    }
    if (lane == 0) {
        const HeatGrid *g = hs.grids + s;
        const HeatScene w = hs.scene[s];
        rows[row0] = mmw_heat_row{scene_base + s, g->id, g->nx, g->ny, first, run - first, w.calls, w.outside, w.t_first, w.t_last};
        if (CLEAR) hs.scene[s] = HeatScene{0, 0, 0.0, 0.0};
    }
}

void launch_heat_zero(int n_scenes, const int32_t *flags, const HeatState &hs, hipStream_t st)
{
    hipLaunchKernelGGL(k_heat_zero, dim3((n_scenes + 3) / 4), dim3(256), 0, st, n_scenes, flags, hs);
}
void launch_heat_sample(const DevCfg &cfg, const DevState &s, const HeatState &hs, const int32_t *flags, const double *t, hipStream_t st)
{
    hipLaunchKernelGGL(k_heat_sample, dim3((cfg.n_scenes + 3) / 4), dim3(256), 0, st, cfg, s, hs, flags, t);
}
void launch_heat(const DevCfg &cfg, const HeatState &hs, mmw_heat_row *rows, int cap_rows, mmw_heat_cell *cells, int cap_cells, const int32_t *scene_flags,
                 int mode, int scene_base, hipStream_t st)
{
    const dim3 grid((cfg.n_scenes + 3) / 4);
    hipLaunchKernelGGL(k_heat_count, grid, dim3(256), 0, st, cfg, hs, scene_flags);
    // (cells <= S * MMW_HEAT_CELLS_MAX can pass 2^31: the scan forms the totals in 64 bits and reports them saturated)
    launch_pair_scan(cfg.n_scenes, hs.sc.off, hs.sc.totals, cap_rows, cap_cells, st);
    if (mode == MMW_HEAT_CLEAR) hipLaunchKernelGGL(k_heat_write<true>, grid, dim3(256), 0, st, cfg, hs, rows, cells, scene_flags, scene_base);
    else hipLaunchKernelGGL(k_heat_write<false>, grid, dim3(256), 0, st, cfg, hs, rows, cells, scene_flags, scene_base);
}

}  // namespace mmw
