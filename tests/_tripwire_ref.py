"""A numpy restatement of the tripwires' rules (include/mmw.h, section "tripwires") for tests/test_gpu_tripwires.py: applied to the
state read back with `tracks()` / `num_tracks()` after each step, carrying its own wires, sides, counters and log.  The arithmetic
is Python floats and `math.sqrt` in the header's operation order (no fused multiply-add anywhere), so every decision and every
exported field is compared by its bytes."""
import math

import numpy as np

from mmwave_msc_amd import _lib
from tests._evlog_ref import EventLogRef

UNKNOWN, NEGATIVE, POSITIVE = 0, 1, 2


def derive(w):
    """(ax, ay, dx, dy, len2, band, id) of one wire given as a TRIPWIRE_DTYPE record or a tuple (ax, ay, bx, by, margin, id)."""
    ax, ay, bx, by, margin, wid = (float(w[0]), float(w[1]), float(w[2]), float(w[3]), float(w[4]), int(w[5]))
    dx = bx - ax
    dy = by - ay
    len2 = dx * dx + dy * dy
    band = margin * math.sqrt(len2)
    return ax, ay, dx, dy, len2, band, wid


class TripRef:
    """The tripwire state of S scenes.  It also tallies what a run held: forward and backward crossings, sides the band alone
    kept (inside, a known old side, c within [-band, band]), and passages through `unknown` that ended on the other side."""

    def __init__(self, n_scenes, t_cap, depth):
        self.S, self.t_cap, self.depth = n_scenes, t_cap, depth
        self.wires = [[] for _ in range(n_scenes)]
        self.sides = [dict() for _ in range(n_scenes)]          # uid -> [side] * 16
        self.forward = np.zeros((n_scenes, 16), np.int64)
        self.backward = np.zeros((n_scenes, 16), np.int64)
        self.mark_f = np.zeros((n_scenes, 16), np.int64)
        self.mark_b = np.zeros((n_scenes, 16), np.int64)
        self.evlog = EventLogRef(n_scenes, depth, _lib.TRIPWIRE_LOG_MAX)
        self.logged = self.evlog.logged                         # (the same array: the tests read it)
        self.bumped = np.zeros(n_scenes, bool)
        self.ordinal = np.zeros(n_scenes, np.int64)
        self.n_forward = self.n_backward = self.n_kept = 0

    def set_wires(self, scenes, n_wires, wires):
        """As mmw_set_tripwires after its checks: (n_wires, wires) is `_lib.make_tripwires`' pair, entry i for scenes[i]."""
        for i, s in enumerate(scenes):
            self.wires[s] = [derive(wires[i, k].tolist()) for k in range(int(n_wires[i]))]
            self.bumped[s] = True
            self.forward[s] = self.backward[s] = self.mark_f[s] = self.mark_b[s] = 0

    def rebase(self, scenes=None):
        self.bumped[slice(None) if scenes is None else list(scenes)] = True

    def sample(self, tracks, ntr, flags=None, t=None):
        for s in range(self.S):
            if flags is not None and int(flags[s]) == 0:
                continue
            tt = float(t[s]) if t is not None else float(self.ordinal[s])
            self.ordinal[s] += 1
            if not self.wires[s]:
                self.bumped[s] = False
                continue
            T = int(ntr[s])
            assert T <= self.t_cap
            if self.bumped[s]:                                                   # 1.
                self.sides[s] = {}
                self.bumped[s] = False
                self.evlog.append(s, (s, -1, _lib.TW_REBASED, -1, -1, T, tt))
            live = [int(tracks[s, j]["uid"]) for j in range(T)]
            for uid in [u for u in self.sides[s] if u not in live]:              # 2.
                del self.sides[s][uid]
            for uid in live:                                                     # 3.
                self.sides[s].setdefault(uid, [UNKNOWN] * 16)
            for j in range(T):                                                   # 4.
                rec = tracks[s, j]
                px, py = float(rec["x"][0]), float(rec["x"][1])
                side = self.sides[s][int(rec["uid"])]
                for z, (ax, ay, dx, dy, len2, band, wid) in enumerate(self.wires[s]):
                    rx = px - ax
                    ry = py - ay
                    u = rx * dx + ry * dy
                    c = dx * ry - dy * rx
                    inside = 0.0 <= u and u <= len2
                    old = side[z]
                    if not inside:
                        new = UNKNOWN
                    elif c > band:
                        new = POSITIVE
                    elif c < -band:
                        new = NEGATIVE
                    else:
                        new = old
                        self.n_kept += old != UNKNOWN
                    if old == NEGATIVE and new == POSITIVE:
                        self.forward[s, z] += 1
                        self.n_forward += 1
                        self.evlog.append(s, (s, int(rec["uid"]), _lib.TW_FORWARD, z, wid, j, tt))
                    elif old == POSITIVE and new == NEGATIVE:
                        self.backward[s, z] += 1
                        self.n_backward += 1
                        self.evlog.append(s, (s, int(rec["uid"]), _lib.TW_BACKWARD, z, wid, j, tt))
                    side[z] = new
                for z in range(len(self.wires[s]), 16):
                    side[z] = UNKNOWN

    def peek(self, scene_base=0):
        """(rows TRIPWIRE_ROW_DTYPE, events TRIPWIRE_EVENT_DTYPE) of an export of this state; it changes nothing."""
        rows, events = [], []
        for s in range(self.S):
            ev, lost = self.evlog.window(s, scene_base)
            for z, w in enumerate(self.wires[s]):
                f, b = int(self.forward[s, z]), int(self.backward[s, z])
                rows.append((scene_base + s, z, w[6], f, b, f - int(self.mark_f[s, z]), b - int(self.mark_b[s, z]), lost))
            events += ev
        return np.array(rows, _lib.TRIPWIRE_ROW_DTYPE).reshape(-1), np.array(events, _lib.TRIPWIRE_EVENT_DTYPE).reshape(-1)

    def export(self, scene_base=0):
        """... and a successful one: taken = logged, the marks become the totals."""
        out = self.peek(scene_base)
        self.evlog.commit()
        self.mark_f[:], self.mark_b[:] = self.forward, self.backward
        return out
