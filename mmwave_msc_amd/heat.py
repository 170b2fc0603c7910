"""Dwell heat maps on the host side: small helpers on the two arrays of `SceneBatch.heat_host` / `mmw_heat_*` (include/mmw.h,
section "heat") -- `rows`, a `_lib.HEAT_ROW_DTYPE` row per scene with a grid, and `cells`, a `_lib.HEAT_CELL_DTYPE` entry per cell
with samples > 0, in (scene, cell) order; row i owns cells[first : first + count].  No GPU.

Cell index c of an nx x ny grid is column c % nx of row c // nx: a dense map is an (ny, nx) array, y down the rows."""
from __future__ import annotations

import numpy as np

from . import _lib

FIELDS = ("dwell", "samples", "visits")
_FIELD_DTYPE = {"dwell": np.float64, "samples": np.int64, "visits": np.int64}


def _arrays(rows, cells):
    return (np.asarray(rows, dtype=_lib.HEAT_ROW_DTYPE).reshape(-1), np.asarray(cells, dtype=_lib.HEAT_CELL_DTYPE).reshape(-1))


def row_of(rows, scene: int):
    """The row of `scene` (as exported: scene_base included); KeyError if the export holds none."""
    r = np.asarray(rows, dtype=_lib.HEAT_ROW_DTYPE).reshape(-1)
    at = np.flatnonzero(r["scene"] == int(scene))
    if len(at) == 0:
        raise KeyError(f"heat: no row of scene {scene} in this export")
    return r[at[0]]


def dense(rows, cells, scene: int, field: str = "dwell") -> np.ndarray:
    """The (ny, nx) map of one scene: `field` ("dwell" float64, "samples" or "visits" int64) of every cell, 0 where the export holds
    no entry."""
    if field not in FIELDS:
        raise ValueError(f"heat.dense: field is one of {FIELDS}, not {field!r}")
    r, c = _arrays(rows, cells)
    row = row_of(r, scene)
    nx, ny, first, count = int(row["nx"]), int(row["ny"]), int(row["first"]), int(row["count"])
    own = c[first: first + count]
    out = np.zeros(nx * ny, _FIELD_DTYPE[field])
    out[own["cell"]] = own[field]
    return out.reshape(ny, nx)


def centres(row, grid):
    """(xs float64[nx], ys float64[ny]): the cell centres of `row`'s grid along x and y, from the `_lib.HEAT_GRID_DTYPE` entry (or a
    mapping with x0, y0 and cell) the scene was given."""
    x0, y0, side = float(grid["x0"]), float(grid["y0"]), float(grid["cell"])
    return x0 + (np.arange(int(row["nx"])) + 0.5) * side, y0 + (np.arange(int(row["ny"])) + 0.5) * side


class Accumulator:
    """Folds a sequence of clear=True exports -- windows cut without losing a frame -- into running dense maps per scene.  A scene
    whose grid shape changes starts over (its cells were zeroed on the device as well)."""

    def __init__(self):
        self.maps = {}        # scene -> {"dwell": (ny, nx) float64, "samples": int64, "visits": int64}
        self.calls = {}       # scene -> sample calls folded
        self.outside = {}     # scene -> samples that fell outside the grid
        self.t_first = {}     # scene -> t of the first call folded
        self.t_last = {}      # scene -> t of the newest
        self.windows = 0

    def add(self, rows, cells):
        r, c = _arrays(rows, cells)
        for row in r:
            s, shape = int(row["scene"]), (int(row["ny"]), int(row["nx"]))
            if s not in self.maps or self.maps[s]["dwell"].shape != shape:
                self.maps[s] = {f: np.zeros(shape, _FIELD_DTYPE[f]) for f in FIELDS}
                self.calls[s], self.outside[s] = 0, 0
                self.t_first.pop(s, None)
                self.t_last.pop(s, None)
            for f in FIELDS:
                self.maps[s][f] += dense(r, c, s, f)
            if int(row["calls"]) > 0:
                self.t_first.setdefault(s, float(row["t_first"]))
                self.t_last[s] = float(row["t_last"])
            self.calls[s] += int(row["calls"])
            self.outside[s] += int(row["outside"])
        self.windows += 1
        return self

    def dense(self, scene: int, field: str = "dwell") -> np.ndarray:
        return self.maps[int(scene)][field]
