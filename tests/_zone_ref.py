"""A numpy restatement of the zone export's rules (include/mmw.h, section "zones") for tests/test_gpu_zones.py: applied to the state
read back with `tracks()` / `num_tracks()`, carrying its own baseline.  Everything it returns is integers."""
import numpy as np

from mmwave_msc_amd import _lib


def core(z, px, py):
    with np.errstate(invalid="ignore"):
        return bool(z["x0"] <= px and px < z["x1"] and z["y0"] <= py and py < z["y1"])


def wide(z, px, py):
    m = np.float64(z["margin"])
    with np.errstate(invalid="ignore"):   # (one fp64 operation per bound)
        return bool(np.float64(z["x0"]) - m <= px and px < np.float64(z["x1"]) + m and np.float64(z["y0"]) - m <= py and py < np.float64(z["y1"]) + m)


class ZoneRef:
    """The exporter's state: the zone table, and per scene the baseline (uid list in order, a set of zones per uid) and whether its
    generation moved since."""

    def __init__(self, n_scenes):
        self.S = n_scenes
        self.nz = np.zeros(n_scenes, np.int32)
        self.zones = np.zeros((n_scenes, _lib.ZONES_MAX), _lib.ZONE_DTYPE)
        self.base = [[] for _ in range(n_scenes)]        # [(uid, frozenset of zones)]
        self.bumped = np.zeros(n_scenes, bool)
        self.held = 0                                     # memberships kept by the margin alone (wide, not core, was a member)

    def set_zones(self, n_zones, zones, scenes=None):
        scenes = range(len(n_zones)) if scenes is None else scenes
        for i, s in enumerate(scenes):
            self.nz[s] = n_zones[i]
            self.zones[s] = zones[i]
            self.bumped[s] = True

    def rebase(self, scenes=None):
        self.bumped[slice(None) if scenes is None else list(scenes)] = True

    def membership(self):
        """{(scene, zone): set of uid} of the baseline."""
        out = {}
        for s in range(self.S):
            for uid, zs in self.base[s]:
                for z in zs:
                    out.setdefault((s, z), set()).add(uid)
        return out

    def export(self, tracks, ntr, scene_base=0, commit=True):
        """(rows, events) of an export of this state; `commit=False`: a look that leaves the baseline alone (a refused export)."""
        rows, events = [], []
        new_base = []
        held = 0
        for s in range(self.S):
            T, nz = int(ntr[s]), int(self.nz[s])
            rebased = bool(self.bumped[s])
            before = {} if rebased else dict(self.base[s])
            if rebased:
                events.append((scene_base + s, -1, _lib.ZEV_REBASED, -1, -1, T))
            cur = []
            for j in range(T):
                t = tracks[s, j]
                uid, px, py = int(t["uid"]), t["x"][0], t["x"][1]
                was = before.get(uid, frozenset())
                now = set()
                for z in range(nz):
                    zz = self.zones[s, z]
                    if z in was:
                        if wide(zz, px, py):
                            now.add(z)
                            held += 0 if core(zz, px, py) else 1
                    elif core(zz, px, py):
                        now.add(z)
                cur.append((uid, frozenset(now), bool(t["is_static"])))
            live = {uid: now for uid, now, _ in cur}
            left = np.zeros(_lib.ZONES_MAX, np.int64)
            entered = np.zeros(_lib.ZONES_MAX, np.int64)
            if not rebased:
                for pos, (uid, was) in enumerate(self.base[s]):
                    for z in sorted(was - live.get(uid, frozenset())):
                        events.append((scene_base + s, uid, _lib.ZEV_LEAVE, z, int(self.zones[s, z]["id"]), pos))
                        left[z] += 1
            for pos, (uid, now, _) in enumerate(cur):
                for z in sorted(now - before.get(uid, frozenset())):
                    events.append((scene_base + s, uid, _lib.ZEV_ENTER, z, int(self.zones[s, z]["id"]), pos))
                    entered[z] += 1
            for z in range(nz):
                rows.append((scene_base + s, z, int(self.zones[s, z]["id"]), sum(z in now for _, now, _ in cur),
                             sum(z in now and st for _, now, st in cur), int(entered[z]), int(left[z]), 0))
            new_base.append([(uid, now) for uid, now, _ in cur])
        if commit:
            self.base = new_base
            self.bumped[:] = False
            self.held += held
        return np.array(rows, _lib.ZONE_ROW_DTYPE).reshape(-1), np.array(events, _lib.ZONE_EVENT_DTYPE).reshape(-1)
