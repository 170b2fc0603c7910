"""A numpy restatement of the stance watch's rules (include/mmw.h, section "stance") for tests/test_gpu_stance.py: applied to the
state read back with `tracks()` / `num_tracks()` after each step, carrying its own rules, slots, counters and log.  The decision is
compares of fp64 values and one subtraction for each of the two ages, in the header's operation order; the squared gap is three
products of fp32 differences widened to fp64 -- Python floats, no fused multiply-add anywhere -- so every decision and every exported
field is compared by its bytes.

The slots are modelled as the slot table hands them out (mmw_uidlist.hpp: the r-th newcomer, in live order, takes the r-th free
slot), not because a slot is visible in the export -- it is not -- but so that the tallies can say when a newborn took the slot of a
uid that expired while LYING.

`planted(scene, uid, frame)` is the seeded script the tests plant keypoints from."""
import collections

import numpy as np

from mmwave_msc_amd import _lib
from tests._evlog_ref import EventLogRef

UNKNOWN, UPRIGHT, LOW, LYING = 0, 1, 2, 3
NKP, HEAD = 57, 22
F32 = np.float32


def derive(r):
    """What the device reads of a rule given as a STANCE_RULE_DTYPE record: one fp64 operation each."""
    h_stand, h_lie, margin, max_gap = float(r["h_stand"]), float(r["h_lie"]), float(r["margin"]), float(r["max_gap"])
    return dict(h_stand=h_stand, h_lie=h_lie, up_hi=h_stand + margin, up_lo=h_stand - margin, lie_hi=h_lie + margin, lie_lo=h_lie - margin,
                gap2=max_gap * max_gap, fall_window=float(r["fall_window"]), long_lie=float(r["long_lie"]), id=int(r["id"]))


def gap_s(kp):
    """s of the skeleton check: g_c = fp32(kp[19c + 1] - kp[19c + 2]); (g_0^2 + g_1^2) + g_2^2 in fp64."""
    kp = np.asarray(kp, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        g = [float(F32(kp[19 * c + 1]) - F32(kp[19 * c + 2])) for c in range(3)]
    return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]


class StanceRef:
    def __init__(self, n_scenes, t_cap, depth):
        self.S, self.t_cap, self.depth = n_scenes, t_cap, depth
        self.rules = [None] * n_scenes
        self.owner = np.full((n_scenes, t_cap), -1, np.int64)
        self.word = np.zeros((n_scenes, t_cap), np.int64)        # bits 0-1 the class, bit 2 LONG_LIE given
        self.t_since = np.zeros((n_scenes, t_cap))
        self.t_upright = np.full((n_scenes, t_cap), -np.inf)
        self.lay_expired = np.zeros((n_scenes, t_cap), bool)     # (for the tallies only)
        self.falls = np.zeros(n_scenes, np.int64)
        self.long_lies = np.zeros(n_scenes, np.int64)
        self.mark_f = np.zeros(n_scenes, np.int64)
        self.mark_l = np.zeros(n_scenes, np.int64)
        self.evlog = EventLogRef(n_scenes, depth, _lib.STANCE_LOG_MAX)
        self.logged = self.evlog.logged                         # (the same array: the tests read it)
        self.bumped = np.zeros(n_scenes, bool)
        self.ordinal = np.zeros(n_scenes, np.int64)
        self.tally = collections.Counter()

    def set_rules(self, scenes, n_rules, rules):
        """As mmw_set_stance_rules after its checks: (n_rules, rules) is `_lib.make_stance_rules`' pair, entry i for scenes[i]."""
        for i, s in enumerate(scenes):
            self.rules[s] = derive(rules[i, 0]) if int(n_rules[i]) else None
            self.bumped[s] = True
            self.falls[s] = self.long_lies[s] = self.mark_f[s] = self.mark_l[s] = 0

    def rebase(self, scenes=None):
        self.bumped[slice(None) if scenes is None else list(scenes)] = True

    def cls(self, s, uid):
        """The class of a live uid as of the last sample."""
        j = int(np.flatnonzero(self.owner[s] == uid)[0])
        return int(self.word[s, j]) & 3

    def sample(self, tracks, ntr, flags=None, t=None):
        for s in range(self.S):
            if flags is not None and int(flags[s]) == 0:
                continue
            tt = float(t[s]) if t is not None else float(self.ordinal[s])
            self.ordinal[s] += 1
            q = self.rules[s]
            if q is None:
                self.bumped[s] = False
                self.tally["asked_without_rule"] += 1
                continue
            T = int(ntr[s])
            assert T <= self.t_cap
            owner, word = self.owner[s], self.word[s]
            if self.bumped[s]:                                                   # 1.
                owner[:] = -1
                self.lay_expired[s] = False
                self.bumped[s] = False
                self.evlog.append(s, (s, -1, _lib.SEV_REBASED, 0, 0, T, tt))
            live = [int(tracks[s, j]["uid"]) for j in range(T)]
            for j in range(self.t_cap):                                          # 2.
                if owner[j] != -1 and int(owner[j]) not in live:
                    owner[j] = -1
                    self.lay_expired[s, j] = (int(word[j]) & 3) == LYING     # (the slot of a uid that expired while LYING)
            for uid in live:                                                     # 3. (the r-th newcomer takes the r-th free slot)
                if uid not in owner:
                    j = int(np.flatnonzero(owner == -1)[0])
                    self.tally["slot_reused_after_lying"] += bool(self.lay_expired[s, j])
                    self.lay_expired[s, j] = False
                    owner[j] = uid
                    word[j] = 0
                    self.t_since[s, j] = 0.0
                    self.t_upright[s, j] = -np.inf
            for i in range(T):                                                   # 4.
                kp = np.asarray(tracks[s, i]["keypoints"], F32)
                uid = live[i]
                j = int(np.flatnonzero(owner == uid)[0])
                old, bit = int(word[j]) & 3, int(word[j]) & 4
                head = float(kp[HEAD])
                sq = gap_s(kp)
                finite = head - head == 0.0                                      # (inf - inf is NaN: not == 0.0)
                if not finite or sq > q["gap2"]:
                    self.tally["implausible_head" if not finite else "implausible_gap"] += 1
                    continue
                a1 = head > (q["up_lo"] if old == UPRIGHT else q["h_stand"] if old == UNKNOWN else q["up_hi"])
                a0 = head > (q["lie_hi"] if old == LYING else q["h_lie"] if old == UNKNOWN else q["lie_lo"])
                new = UPRIGHT if a1 else LOW if a0 else LYING
                # what the margin alone decided: the class a newcomer with this head would get is another one
                if old == UPRIGHT and new == UPRIGHT and not head > q["h_stand"]:
                    self.tally["kept_upright_by_margin"] += 1
                if old != UPRIGHT and old != UNKNOWN and new != UPRIGHT and head > q["h_stand"]:
                    self.tally["kept_below_upright_by_margin"] += 1
                if old == LYING and new == LYING and head > q["h_lie"]:
                    self.tally["kept_lying_by_margin"] += 1
                if old != LYING and old != UNKNOWN and new != LYING and not head > q["h_lie"]:
                    self.tally["kept_above_lying_by_margin"] += 1
                if new != old:
                    fall = new == LYING and old != UNKNOWN and tt - self.t_upright[s, j] <= q["fall_window"]
                    self.evlog.append(s, (s, uid, _lib.SEV_FALL if fall else _lib.SEV_CHANGE, old, new, i, tt))
                    self.t_since[s, j] = tt
                    bit = 0
                    if fall:
                        self.falls[s] += 1
                        self.tally["fall_from_upright" if old == UPRIGHT else "fall_through_low"] += 1
                    elif old == UNKNOWN:
                        self.tally["first_" + ("", "upright", "low", "lying")[new]] += 1
                    else:
                        self.tally["change_between_known"] += 1
                        self.tally["lay_down_slowly"] += new == LYING
                if new == UPRIGHT:
                    self.t_upright[s, j] = tt
                if new == LYING and not bit and tt - self.t_since[s, j] >= q["long_lie"]:
                    self.evlog.append(s, (s, uid, _lib.SEV_LONG_LIE, LYING, LYING, i, tt))
                    bit = 4
                    self.long_lies[s] += 1
                    self.tally["long_lie"] += 1
                elif new == LYING and bit and tt - self.t_since[s, j] >= q["long_lie"]:
                    self.tally["long_lie_not_repeated"] += 1
                word[j] = new | bit

    def peek(self, scene_base=0):
        """(rows STANCE_ROW_DTYPE, events STANCE_EVENT_DTYPE) of an export of this state; it changes nothing."""
        rows, events = [], []
        for s in range(self.S):
            q = self.rules[s]
            ev, lost = self.evlog.window(s, scene_base)
            if q is not None:
                owned = (self.owner[s] != -1) & (not self.bumped[s])
                n = [int((owned & ((self.word[s] & 3) == c)).sum()) for c in (UPRIGHT, LOW, LYING, UNKNOWN)]
                f, l = int(self.falls[s]), int(self.long_lies[s])
                rows.append((scene_base + s, q["id"], n[0], n[1], n[2], n[3], f, f - int(self.mark_f[s]), l, l - int(self.mark_l[s]), lost, 0))
            events += ev
        return np.array(rows, _lib.STANCE_ROW_DTYPE).reshape(-1), np.array(events, _lib.STANCE_EVENT_DTYPE).reshape(-1)

    def export(self, scene_base=0):
        """... and a successful one: taken = logged, the marks become the totals."""
        out = self.peek(scene_base)
        self.evlog.commit()
        self.mark_f[:], self.mark_l[:] = self.falls, self.long_lies
        return out


# ---- the planting script ----------------------------------------------------------------------------------------------------------
# Heads for the rule h_stand 1.25, h_lie 0.5, margin 0.125 (up_hi 1.375, up_lo 1.125, lie_hi 0.625, lie_lo 0.375), all dyadic:
U, M, L = 1.5, 0.875, 0.25                 # plainly UPRIGHT, LOW, LYING
U_KEEP, M_KEEP_UP = 1.1875, 1.3125         # between up_lo and h_stand: an UPRIGHT stays; between h_stand and up_hi: a LOW stays
L_KEEP, M_KEEP_LIE = 0.5625, 0.4375        # between h_lie and lie_hi: a LYING stays; between lie_lo and h_lie: a LOW stays
NAN, GAP = "nan", "gap"                    # a NaN head; a plain UPRIGHT head with g = (0.75, 0, 0): s = 0.5625 > 0.25
SCRIPTS = (
    (U, U, L, L, L, L, L, L, U, U, L, L),                              # falls from UPRIGHT, lies long (one LONG_LIE, then none), gets up, falls
    (U, M, L, L, U, M, L, L, L, L, L, L),                              # falls through ONE LOW sample: tt - t_upright == fall_window exactly
    (U, M, M, L, L, M, U, U, M, M, L, L),                              # lies down slowly: LYING three samples after UPRIGHT is a CHANGE
    (U, U_KEEP, M, M_KEEP_UP, U, L, L_KEEP, M, M_KEEP_LIE, M, U, U),   # every margin, both ways
    (U, NAN, U, GAP, L, NAN, L, GAP, L, L, L, L),                      # samples that are not plausible change nothing
    (L, L, L, L, L, L, L, L, L, L, L, L),                              # found lying, never gets up
    (M, M, L_KEEP, M, U, M, M, M_KEEP_LIE, L, L, M, M),                # found LOW
)


def planted(scene, uid, frame):
    """The 57 keypoints planted for (scene, uid) behind frame `frame`: zeros but the head height (kp[22]) and, for GAP, kp[1]."""
    v = SCRIPTS[(scene + 2 * uid) % len(SCRIPTS)][(frame + scene // len(SCRIPTS)) % 12]
    kp = np.zeros(NKP, F32)
    if v == NAN:
        kp[HEAD] = np.nan
    elif v == GAP:
        kp[HEAD], kp[1] = U, 0.75
    else:
        kp[HEAD] = v
    return kp
