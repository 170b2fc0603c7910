"""A numpy restatement of the deferred keypoint scatter (`mmw_set_keypoints_uid` / `mmw_set_keypoints_ticket`, include/mmw.h)
for tests/test_gpu_kp_scatter.py and tests/test_kp_scatter_ref.py: applied to the structured arrays `tracks()` and `num_tracks()`
return, carrying its own per-scene generation and per-ticket snapshots of it.  Nothing is computed: a row's 57 floats are copied
or they are not."""
import numpy as np

TICKETS = 4   # kTickets (csrc/mmw_ctx.hpp)


class TicketError(ValueError):
    """What the library answers with MMW_E_ARG: a ticket outside [0, 4), never taken, or last taken without uids."""


class KpScatterRef:
    def __init__(self, n_scenes):
        self.S = n_scenes
        self.gen = np.zeros(n_scenes, np.int64)
        self.snap = [None] * TICKETS          # per ticket: the generations its rows were taken in, or None (no rows with uids)
        self.dropped = {"scene": 0, "stranger": 0, "generation": 0}   # what a run held, by reason
        self.landed = 0

    def rebase(self, scenes=None):
        """`reset` (scenes=None), `reset_scenes`, `restore`: the touched scenes' uids start over."""
        self.gen[slice(None) if scenes is None else list(scenes)] += 1

    def take(self, ticket, with_uid=True):
        """`features_async(ticket=...)`; with_uid=False: the call passed uid = NULL (`mmw_features` does, on the last ticket)."""
        if not 0 <= ticket < TICKETS:
            raise TicketError(ticket)
        self.snap[ticket] = self.gen.copy() if with_uid else None

    def scatter(self, tracks, ntr, kp, owner, uid, ticket=None):
        """`tracks` with the rows applied, in order (a copy; the argument is left alone).  ticket=None: the uid form, which knows
        no generation."""
        if ticket is not None and (not 0 <= ticket < TICKETS or self.snap[ticket] is None):
            raise TicketError(ticket)
        out = np.ascontiguousarray(tracks).view(np.uint8).copy().view(tracks.dtype)   # (as bytes: a record's padding travels too)
        kp = np.asarray(kp, np.float32).reshape(-1, out.dtype["keypoints"].shape[0])
        owner = np.asarray(owner).reshape(-1, 2)
        for i in range(len(kp)):
            s, u = int(owner[i, 0]), int(uid[i])
            if not 0 <= s < self.S:
                self.dropped["scene"] += 1
                continue
            if ticket is not None and self.snap[ticket][s] != self.gen[s]:
                self.dropped["generation"] += 1
                continue
            hit = [j for j in range(min(int(ntr[s]), out.shape[1])) if int(out[s, j]["uid"]) == u]
            if not hit:
                self.dropped["stranger"] += 1
                continue
            out[s, hit[0]]["keypoints"] = kp[i]
            self.landed += 1
        return out
