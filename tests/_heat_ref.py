"""A numpy restatement of the heat maps' rules (include/mmw.h, section "heat") for tests/test_gpu_heat.py and
tests/test_heat_exports.py: applied to the state read back with `tracks()` / `num_tracks()`, carrying its own grids, cells, uid
memory and scene words.  Positions, times and `dwell` are Python floats (IEEE fp64): one subtraction and one division per
coordinate, one subtraction per interval, one addition per credited interval, in the header's order -- tracks in list order."""
import numpy as np

from mmwave_msc_amd import _lib


def cell_of(grid, px, py):
    """The header's cell index of position (px, py), -1 outside; `grid` a HEAT_GRID_DTYPE entry (or a mapping of its fields)."""
    x0, y0, side, nx, ny = float(grid["x0"]), float(grid["y0"]), float(grid["cell"]), int(grid["nx"]), int(grid["ny"])
    with np.errstate(all="ignore"):
        fx = float((np.float64(px) - np.float64(x0)) / np.float64(side))
        fy = float((np.float64(py) - np.float64(y0)) / np.float64(side))
    inside = fx >= 0.0 and fx < float(nx) and fy >= 0.0 and fy < float(ny)
    return int(fy) * nx + int(fx) if inside else -1


class HeatRef:
    """The heat state of S scenes: per scene a grid or None, `cells` cells of (dwell, samples, visits), {uid: [last_cell, last_t]}, the
    scene words, a generation that `rebase` and `set_grids` move, and the call ordinal.  It also tallies what a run held."""

    def __init__(self, n_scenes, t_cap, cells):
        assert 1 <= cells <= _lib.HEAT_CELLS_MAX
        self.S, self.t_cap, self.cells = n_scenes, t_cap, cells
        self.grid = [None] * n_scenes
        self.dwell = np.zeros((n_scenes, cells), np.float64)
        self.samples = np.zeros((n_scenes, cells), np.int32)
        self.visits = np.zeros((n_scenes, cells), np.int32)
        self.mem = [dict() for _ in range(n_scenes)]
        self.bumped = np.zeros(n_scenes, bool)
        self.ordinal = np.zeros(n_scenes, np.int64)
        self.calls = np.zeros(n_scenes, np.int32)
        self.outside = np.zeros(n_scenes, np.int32)
        self.t_first = np.zeros(n_scenes, np.float64)
        self.t_last = np.zeros(n_scenes, np.float64)
        self.tally = dict(shared=0, shared_max=0, credited=0, gap_refused=0, dt_not_positive=0, revisit=0, expired=0, fresh=0, outside=0)

    def _zero(self, s):
        self.dwell[s], self.samples[s], self.visits[s] = 0.0, 0, 0
        self.calls[s], self.outside[s], self.t_first[s], self.t_last[s] = 0, 0, 0.0, 0.0

    def set_grids(self, scenes, n_grids, grids):
        """What an ACCEPTED mmw_set_heat_grids does: the listed scenes' grid, their cells and words at 0, their generation moved."""
        for i, s in enumerate(scenes):
            g = grids[i, 0] if int(n_grids[i]) else None
            assert g is None or int(g["nx"]) * int(g["ny"]) <= self.cells
            self.grid[s] = None if g is None else g.copy()
            self._zero(s)
            self.bumped[s] = True

    def rebase(self, scenes=None):
        self.bumped[slice(None) if scenes is None else list(scenes)] = True

    def sample(self, tracks, ntr, flags=None, t=None):
        for s in range(self.S):
            if flags is not None and int(flags[s]) == 0:
                continue
            g = self.grid[s]
            if g is None:                                                        # asked without a grid: seen = generation, the call counts
                self.bumped[s] = False
                self.mem[s] = {}
                self.ordinal[s] += 1
                continue
            if self.bumped[s]:                                                   # 1.
                self.mem[s] = {}
                self.bumped[s] = False
            T = int(ntr[s])
            assert T <= self.t_cap
            live = [int(tracks[s, j]["uid"]) for j in range(T)]
            for uid in [u for u in self.mem[s] if u not in live]:                # 2.
                del self.mem[s][uid]
                self.tally["expired"] += 1
            tt = float(t[s]) if t is not None else float(self.ordinal[s])
            if self.calls[s] == 0:                                               # 4.
                self.t_first[s] = tt
            self.calls[s] += 1
            self.t_last[s] = tt
            max_gap = float(g["max_gap"])
            seen_cells = {}
            for j in range(T):                                                   # 5. (3.: a uid without memory is fresh)
                rec = tracks[s, j]
                uid = int(rec["uid"])
                c = cell_of(g, float(rec["x"][0]), float(rec["x"][1]))
                fresh = uid not in self.mem[s]
                self.tally["fresh"] += fresh
                if c < 0:
                    self.outside[s] += 1
                    self.tally["outside"] += 1
                else:
                    seen_cells[c] = seen_cells.get(c, 0) + 1
                    self.samples[s, c] += 1
                    if fresh or self.mem[s][uid][0] != c:
                        self.visits[s, c] += 1
                        self.tally["revisit"] += not fresh                   # (a known uid came in from another cell or from outside)
                    if not fresh:
                        dt = tt - self.mem[s][uid][1]
                        if dt > 0.0 and dt <= max_gap:
                            self.dwell[s, c] = float(self.dwell[s, c]) + dt
                            self.tally["credited"] += 1
                        elif dt > 0.0:
                            self.tally["gap_refused"] += 1
                        else:
                            self.tally["dt_not_positive"] += 1
                self.mem[s][uid] = [c, tt]
            for n in seen_cells.values():
                self.tally["shared"] += n > 1
                self.tally["shared_max"] = max(self.tally["shared_max"], n)
            self.ordinal[s] += 1

    def export(self, scene_base=0, scenes=None, clear=False):
        """(rows HEAT_ROW_DTYPE, cells HEAT_CELL_DTYPE) of an export of this state that fits; clear=True restarts what it exported."""
        rows, cells = [], []
        for s in range(self.S):
            g = self.grid[s]
            if g is None or (scenes is not None and s not in scenes):
                continue
            n = int(g["nx"]) * int(g["ny"])
            kept = np.flatnonzero(self.samples[s, :n] > 0)
            rows.append((scene_base + s, int(g["id"]), int(g["nx"]), int(g["ny"]), len(cells), len(kept), int(self.calls[s]), int(self.outside[s]),
                         float(self.t_first[s]), float(self.t_last[s])))
            cells.extend((scene_base + s, int(c), int(self.samples[s, c]), int(self.visits[s, c]), float(self.dwell[s, c])) for c in kept)
            if clear:
                self._zero(s)
        return np.array(rows, _lib.HEAT_ROW_DTYPE).reshape(-1), np.array(cells, _lib.HEAT_CELL_DTYPE).reshape(-1)
