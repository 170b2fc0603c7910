"""The stance watch on the host side: `Watch`, the fold of the event log of `SceneBatch.stance_host` / `mmw_stance_*`
(include/mmw.h, section "stance"), and `classify`, the header's decision in numpy, for choosing a rule's heights.

The log is complete as long as no row reports `lost`: every change of class the device saw is one event."""
from __future__ import annotations

import numpy as np

from . import _lib

UNKNOWN, UPRIGHT, LOW, LYING = _lib.STANCE_UNKNOWN, _lib.STANCE_UPRIGHT, _lib.STANCE_LOW, _lib.STANCE_LYING


class Watch:
    """{(scene, uid): (class, since)} of every uid the log has classed, the uids that are down (LYING) and those that are alarmed
    (a FALL or a LONG_LIE since they last left LYING), kept current by `apply(events)`.  `scene` is the events' scene id
    (`scene_base` included).  A uid that expires stays as it was last seen until its scene is REBASED or `forget` drops it: the
    log has no event for an expiry (the report's events do)."""

    def __init__(self):
        self.state = {}
        self.alarmed_ = set()
        self.falls = 0
        self.long_lies = 0

    def apply(self, events) -> "Watch":
        """Fold one export's events (a `_lib.STANCE_EVENT_DTYPE` array, or rows with its fields), in order.  CHANGE and FALL set
        the uid's class to `to` since the event's t; a FALL alarms the uid, a LONG_LIE too; leaving LYING ends the alarm.  REBASED
        empties its scene: the uids that follow name other tracks.  Any other kind raises ValueError."""
        for e in np.asarray(events, dtype=_lib.STANCE_EVENT_DTYPE).reshape(-1):
            scene, uid, kind = int(e["scene"]), int(e["uid"]), int(e["kind"])
            key = (scene, uid)
            if kind == _lib.SEV_REBASED:
                for k in [k for k in self.state if k[0] == scene]:
                    del self.state[k]
                self.alarmed_ = {k for k in self.alarmed_ if k[0] != scene}
            elif kind in (_lib.SEV_CHANGE, _lib.SEV_FALL):
                to = int(e["to"])
                self.state[key] = (to, float(e["t"]))
                if to != LYING:
                    self.alarmed_.discard(key)
                if kind == _lib.SEV_FALL:
                    self.alarmed_.add(key)
                    self.falls += 1
            elif kind == _lib.SEV_LONG_LIE:
                self.state.setdefault(key, (LYING, float(e["t"])))
                self.alarmed_.add(key)
                self.long_lies += 1
            else:
                raise ValueError(f"Watch: event kind {kind}")
        return self

    def forget(self, scene: int, uid: int) -> None:
        """Drop a uid that is gone (an EV_GONE of the report)."""
        self.state.pop((scene, uid), None)
        self.alarmed_.discard((scene, uid))

    def down(self) -> frozenset:
        """The (scene, uid) whose class is LYING."""
        return frozenset(k for k, (cls, _) in self.state.items() if cls == LYING)

    def alarmed(self) -> frozenset:
        """The (scene, uid) that fell or have lain longer than their rule's long_lie, and have not got up since."""
        return frozenset(self.alarmed_)


def classify(rule, kp, old=UNKNOWN):
    """(new class, plausible) of keypoints `kp` (float32[..., 57]) for a uid whose class was `old` (an int or an array that
    broadcasts against kp's leading shape) under `rule` (a `_lib.STANCE_RULE_DTYPE` record, or a dict / tuple as
    `_lib.make_stance_rules` takes), in the header's operation order.  Where the keypoints are not plausible the class stays `old`."""
    if not (isinstance(rule, np.void) or (isinstance(rule, np.ndarray) and rule.dtype == _lib.STANCE_RULE_DTYPE)):
        rule = _lib.make_stance_rules([[rule]])[1][0, 0]
    r = {f: np.float64(np.asarray(rule[f]).reshape(-1)[0]) for f in _lib.STANCE_FIELDS[:6]}
    up_hi, up_lo = r["h_stand"] + r["margin"], r["h_stand"] - r["margin"]
    lie_hi, lie_lo = r["h_lie"] + r["margin"], r["h_lie"] - r["margin"]
    gap2 = r["max_gap"] * r["max_gap"]
    kp = np.asarray(kp, np.float32)
    old = np.broadcast_to(np.asarray(old, np.int32), kp.shape[:-1])
    with np.errstate(invalid="ignore", over="ignore"):
        head = kp[..., 22].astype(np.float64)
        g = [(kp[..., 19 * c + 1] - kp[..., 19 * c + 2]).astype(np.float64) for c in range(3)]   # (fp32 differences)
        s = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
        plausible = (head - head == 0.0) & ~(s > gap2)
        a1 = head > np.where(old == UPRIGHT, up_lo, np.where(old == UNKNOWN, r["h_stand"], up_hi))
        a0 = head > np.where(old == LYING, lie_hi, np.where(old == UNKNOWN, r["h_lie"], lie_lo))
    new = np.where(a1, UPRIGHT, np.where(a0, LOW, LYING)).astype(np.int32)
    new = np.where(plausible, new, old).astype(np.int32)
    return (int(new), bool(plausible)) if new.ndim == 0 else (new, plausible)
