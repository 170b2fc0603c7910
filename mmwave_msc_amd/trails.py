"""Track trails on the host side: small helpers on the two arrays of `SceneBatch.trails_host` / `mmw_trails_*` (include/mmw.h,
section "trails") -- `dir`, a `_lib.TRAIL_TRACK_DTYPE` entry per live track, and `points`, their `_lib.TRAIL_POINT_DTYPE` samples
back to back, oldest first.  No GPU.

`dir["travelled"]` is the distance over the uid's whole life, summed in fp64 on the device; `window_length` is the length of what
was exported, from the rounded points -- the two differ once a trail is longer than its ring, or was cut by `last`."""
from __future__ import annotations

import numpy as np

from . import _lib


def _arrays(dir, points):
    return (np.asarray(dir, dtype=_lib.TRAIL_TRACK_DTYPE).reshape(-1), np.asarray(points, dtype=_lib.TRAIL_POINT_DTYPE).reshape(-1))


def split(dir, points) -> list:
    """One view of `points` per directory entry: entry i's samples, oldest first (empty for a track never sampled)."""
    d, p = _arrays(dir, points)
    return [p[int(e["first"]): int(e["first"]) + int(e["count"])] for e in d]


def window_length(dir, points) -> np.ndarray:
    """float32[n]: per entry the path length in the x/y plane of its EXPORTED points, in fp32 arithmetic on the fp32 points (0 for
    fewer than two)."""
    out = np.zeros(len(np.asarray(dir).reshape(-1)), np.float32)
    for i, tr in enumerate(split(dir, points)):
        if len(tr) > 1:
            dx, dy = np.diff(tr["x"]), np.diff(tr["y"])
            out[i] = np.sqrt(dx * dx + dy * dy, dtype=np.float32).sum(dtype=np.float32)
    return out


def age(dir, points) -> np.ndarray:
    """float64[n]: per entry its newest exported sample's `t` minus `t_first` (0 for a track never sampled)."""
    d, _ = _arrays(dir, points)
    out = np.zeros(len(d), np.float64)
    for i, tr in enumerate(split(dir, points)):
        if len(tr):
            out[i] = tr["t"][-1] - d["t_first"][i]
    return out
