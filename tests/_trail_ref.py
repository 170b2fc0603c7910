"""A numpy restatement of the trails' rules (include/mmw.h, section "trails") for tests/test_gpu_trails.py and
tests/test_trail_exports.py: applied to the state read back with `tracks()` / `num_tracks()`, carrying its own trail state.  The
points are `np.float32(...)` of the fp64 state, `travelled` is Python floats and `math.sqrt`, in the header's operation order."""
import math

import numpy as np

from mmwave_msc_amd import _lib


class _Trail:
    __slots__ = ("slot", "total", "t_first", "travelled", "last", "ring")

    def __init__(self, slot):
        self.slot, self.total, self.t_first, self.travelled, self.last, self.ring = slot, 0, 0.0, 0.0, None, []


class TrailRef:
    """The trail state of S scenes: per scene {uid: _Trail}, a generation that `rebase` moves, and the call ordinal.  It also
    tallies what a run held: ring wraps, trails that went on while the uid's list position changed, slots a newcomer reused."""

    def __init__(self, n_scenes, t_cap, depth):
        assert 1 <= depth <= _lib.TRAIL_DEPTH_MAX
        self.S, self.t_cap, self.depth = n_scenes, t_cap, depth
        self.trails = [dict() for _ in range(n_scenes)]
        self.bumped = np.zeros(n_scenes, bool)
        self.ordinal = np.zeros(n_scenes, np.int64)
        self.pos = [dict() for _ in range(n_scenes)]        # uid -> list position at its previous sample
        self.used = [set() for _ in range(n_scenes)]        # slots that ever held a trail since the scene's last rebase
        self.wraps = self.moved = self.reused = 0

    def rebase(self, scenes=None):
        self.bumped[slice(None) if scenes is None else list(scenes)] = True

    def sample(self, tracks, ntr, flags=None, t=None):
        for s in range(self.S):
            if flags is not None and int(flags[s]) == 0:
                continue
            if self.bumped[s]:                                                   # 1.
                self.trails[s], self.pos[s], self.used[s] = {}, {}, set()
                self.bumped[s] = False
            T = int(ntr[s])
            assert T <= self.t_cap
            live = [int(tracks[s, j]["uid"]) for j in range(T)]
            for uid in [u for u in self.trails[s] if u not in live]:             # 2.
                del self.trails[s][uid]
                self.pos[s].pop(uid, None)
            free = sorted(set(range(self.t_cap)) - {tr.slot for tr in self.trails[s].values()})
            for uid in live:                                                     # 3. (which slot is not observable: the lowest free one here)
                if uid not in self.trails[s]:
                    slot = free.pop(0)
                    self.reused += slot in self.used[s]
                    self.used[s].add(slot)
                    self.trails[s][uid] = _Trail(slot)
            tt = float(t[s]) if t is not None else float(self.ordinal[s])
            for j in range(T):                                                   # 4.
                rec = tracks[s, j]
                tr = self.trails[s][int(rec["uid"])]
                x, y, z = float(rec["x"][0]), float(rec["x"][1]), float(rec["x"][2])
                fl = (_lib.TRAIL_STATIC if int(rec["is_static"]) != 0 else 0) | (_lib.TRAIL_UPDATED if float(rec["lifetime"]) == 0.0 else 0)
                if tr.total == 0:
                    tr.t_first = tt
                else:
                    dx, dy = x - tr.last[0], y - tr.last[1]
                    tr.travelled = tr.travelled + math.sqrt(dx * dx + dy * dy)
                    self.moved += self.pos[s].get(int(rec["uid"]), j) != j
                tr.last = (x, y)
                tr.total += 1
                with np.errstate(over="ignore", invalid="ignore"):
                    point = (tt, np.float32(x), np.float32(y), np.float32(z), fl)
                if len(tr.ring) == self.depth:
                    tr.ring.pop(0)
                    self.wraps += 1
                tr.ring.append(point)
                self.pos[s][int(rec["uid"])] = j
            self.ordinal[s] += 1

    def export(self, tracks, ntr, last=0, scene_base=0):
        """(dir TRAIL_TRACK_DTYPE, points TRAIL_POINT_DTYPE) of an export of this state; it changes nothing."""
        assert last >= 0
        dir_, points = [], []
        for s in range(self.S):
            for j in range(int(ntr[s])):
                uid = int(tracks[s, j]["uid"])
                tr = None if self.bumped[s] else self.trails[s].get(uid)
                if tr is None:
                    dir_.append((scene_base + s, j, uid, len(points), 0, 0, 0.0, 0.0))
                    continue
                ring = tr.ring[-last:] if last > 0 else tr.ring
                dir_.append((scene_base + s, j, uid, len(points), len(ring), tr.total, tr.t_first, tr.travelled))
                points.extend(ring)
        return np.array(dir_, _lib.TRAIL_TRACK_DTYPE).reshape(-1), np.array(points, _lib.TRAIL_POINT_DTYPE).reshape(-1)
