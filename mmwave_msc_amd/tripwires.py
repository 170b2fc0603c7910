"""Tripwires on the host side: `Tally`, the fold of the event log of `SceneBatch.tripwires_host` / `mmw_tripwires_*`
(include/mmw.h, section "tripwires"), and `sides`, the header's side arithmetic in numpy, for placing wires.

The log is complete as long as no row reports `lost`: every crossing the device counted is one event.  Counts are kept per
(scene, id) -- `id` is the caller's label, so several wires with one id (a polyline doorway) fold into one counter."""
from __future__ import annotations

import numpy as np

from . import _lib


class Tally:
    """{(scene, id): forward / backward counts}, and per (scene, id) the uids that went forward and have not come back, kept
    current by `apply(events)`.  `scene` is the events' scene id (`scene_base` included)."""

    def __init__(self):
        self.forward = {}
        self.backward = {}
        self.inside = {}

    def apply(self, events) -> "Tally":
        """Fold one export's events (a `_lib.TRIPWIRE_EVENT_DTYPE` array, or rows with its fields), in order.  FORWARD adds the uid
        to the (scene, id)'s set, BACKWARD takes it out (a uid that was not in it -- it went forward before the log began -- only
        counts); REBASED empties every set of its scene: the uids that follow name other tracks.  The counts go on.  Any other
        kind raises ValueError."""
        for e in np.asarray(events, dtype=_lib.TRIPWIRE_EVENT_DTYPE).reshape(-1):
            scene, uid, kind = int(e["scene"]), int(e["uid"]), int(e["kind"])
            if kind == _lib.TW_REBASED:
                for key in [k for k in self.inside if k[0] == scene]:
                    del self.inside[key]
                continue
            key = (scene, int(e["id"]))
            if kind == _lib.TW_FORWARD:
                self.forward[key] = self.forward.get(key, 0) + 1
                self.inside.setdefault(key, set()).add(uid)
            elif kind == _lib.TW_BACKWARD:
                self.backward[key] = self.backward.get(key, 0) + 1
                self.inside.get(key, set()).discard(uid)
            else:
                raise ValueError(f"Tally: event kind {kind}")
        return self

    def counts(self) -> dict:
        """{(scene, id): (forward, backward, net = forward - backward)} of every (scene, id) that saw a crossing."""
        keys = sorted(set(self.forward) | set(self.backward))
        return {k: (self.forward.get(k, 0), self.backward.get(k, 0), self.forward.get(k, 0) - self.backward.get(k, 0)) for k in keys}

    def net(self, scene: int, id: int) -> int:
        return self.forward.get((scene, id), 0) - self.backward.get((scene, id), 0)

    def went_forward(self, scene: int, id: int) -> frozenset:
        """The uids that crossed (scene, id) forward and not back since the scene's last REBASED."""
        return frozenset(self.inside.get((scene, id), ()))


def sides(wires, x, y):
    """(u, c, inside) of the points (x, y) against `wires` (a `_lib.TRIPWIRE_DTYPE` array of any shape), in the header's operation
    order: u = rx * dx + ry * dy along the wire, c = dx * ry - dy * rx (> 0: left of A -> B), inside = 0 <= u <= len2.  x and y
    broadcast against the wires' shape.  A track is on the positive side where inside and c > margin * sqrt(len2), on the negative
    where inside and c < -margin * sqrt(len2)."""
    w = np.asarray(wires, dtype=_lib.TRIPWIRE_DTYPE)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    dx, dy = w["bx"] - w["ax"], w["by"] - w["ay"]
    len2 = dx * dx + dy * dy
    with np.errstate(invalid="ignore", over="ignore"):
        rx, ry = x - w["ax"], y - w["ay"]
        u = rx * dx + ry * dy
        c = dx * ry - dy * rx
        inside = (0.0 <= u) & (u <= len2)
    return u, c, inside
