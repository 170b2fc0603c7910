"""Zone occupancy on the host side: `Roster`, the fold of the event stream of `SceneBatch.zones_host` / `mmw_zones_*`
(include/mmw.h, section "zones").

The stream is complete -- a track already inside a zone gets its ENTER at the first export, a track that expires LEAVEs every zone
it was in, and a scene whose memberships became void (reset, restore, new zones) says so with one REBASED before its ENTERs -- so
folding every export's events in order gives, after each export, exactly who is in which zone.  Dwell times are the caller's: note the
clock at ENTER and LEAVE."""
from __future__ import annotations

import numpy as np

from . import _lib


class Roster:
    """{(scene, zone): set of uid}, kept current by `apply(events)`.  `scene` is the events' scene id (`scene_base` included), `zone`
    the zone's index in its scene; `ids[(scene, zone)]` is the caller's label the events carried."""

    def __init__(self):
        self.members = {}
        self.ids = {}

    def apply(self, events) -> "Roster":
        """Fold one export's events (a `_lib.ZONE_EVENT_DTYPE` array, or rows with its fields), in order.  REBASED empties every
        zone of its scene; a LEAVE of a uid the roster does not hold, or an ENTER of one it holds, means events were skipped or
        applied twice and raises ValueError."""
        for e in np.asarray(events, dtype=_lib.ZONE_EVENT_DTYPE).reshape(-1):
            scene, uid, kind, zone = int(e["scene"]), int(e["uid"]), int(e["kind"]), int(e["zone"])
            if kind == _lib.ZEV_REBASED:
                for key in [k for k in self.members if k[0] == scene]:
                    del self.members[key]
                continue
            key = (scene, zone)
            self.ids[key] = int(e["id"])
            inside = self.members.setdefault(key, set())
            if kind == _lib.ZEV_ENTER:
                if uid in inside:
                    raise ValueError(f"Roster: uid {uid} enters zone {zone} of scene {scene} twice")
                inside.add(uid)
            elif kind == _lib.ZEV_LEAVE:
                if uid not in inside:
                    raise ValueError(f"Roster: uid {uid} leaves zone {zone} of scene {scene} without having entered")
                inside.remove(uid)
                if not inside:
                    del self.members[key]
            else:
                raise ValueError(f"Roster: event kind {kind}")
        return self

    def occupied(self) -> dict:
        """{(scene, zone): frozenset of uid} of the zones that hold somebody."""
        return {k: frozenset(v) for k, v in self.members.items() if v}

    def count(self, scene: int, zone: int) -> int:
        return len(self.members.get((scene, zone), ()))

    def zones_of(self, scene: int, uid: int) -> list:
        """The zones of `scene` that hold `uid`, ascending."""
        return sorted(z for (s, z), v in self.members.items() if s == scene and uid in v)
