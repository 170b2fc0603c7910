"""The per-scene event log of the tripwires and the stance watch (csrc/mmw_evlog.hpp), restated once for tests/_tripwire_ref.py and
tests/_stance_ref.py: a ring of `depth` events per scene that drops the oldest, `logged` and `taken`, the window an export hands out
and the commit of a successful one.  An event is a tuple whose first field is the LOCAL scene index."""
import numpy as np


class EventLogRef:
    def __init__(self, n_scenes, depth, depth_max):
        assert 1 <= depth <= depth_max
        self.depth = depth
        self.log = [[] for _ in range(n_scenes)]                # per scene the newest `depth` events, oldest first
        self.logged, self.taken = np.zeros(n_scenes, np.int64), np.zeros(n_scenes, np.int64)   # events ever appended / handed out

    def append(self, s, ev):
        self.log[s] = (self.log[s] + [ev])[-self.depth:]
        self.logged[s] += 1

    def window(self, s, scene_base=0):
        """(events, lost) of an export of scene s: events first .. first + n - 1 with the caller's scene index, and how many were
        overwritten before it came; it changes nothing."""
        logged, taken = int(self.logged[s]), int(self.taken[s])
        first = max(taken, logged - self.depth)
        n, lost = logged - first, max(0, logged - self.depth - taken)
        return [(scene_base + e[0],) + e[1:] for e in self.log[s][len(self.log[s]) - n:]], lost

    def commit(self):
        """... and a successful one: everything logged is taken."""
        self.taken[:] = self.logged
