"""tests/_kp_scatter_ref.py, the restatement tests/test_gpu_kp_scatter.py compares the keypoint scatter kernel with, on a hand-made
table (no GPU): a row that matches, a stranger uid, a scene index out of range, a scene whose generation moved, a ticket retaken."""
import numpy as np
import pytest

from tests._kp_scatter_ref import KpScatterRef, TicketError

NKP = 57
# what the restatement reads, and three fields it must not touch; with padding, as mmw_track_record has
DT = np.dtype([("x", "f8", (9,)), ("is_static", "i1"), ("uid", "i4"), ("keypoints", "f4", (NKP,)), ("n_est", "f8")], align=True)
assert DT.itemsize > 9 * 8 + 1 + 4 + NKP * 4 + 8


def _table():
    """3 scenes x 4 positions: scene 0 holds uids 5, 2, 9 (not in uid order), scene 1 holds uid 0, scene 2 is empty; every dead
    position carries uid 2 as well, to be found by a restatement that looks past n_tracks."""
    t = np.full((3, 4 * DT.itemsize), 0xAB, np.uint8).view(DT)   # (the padding too)
    t["n_est"], t["is_static"] = 0.5, 1
    t["uid"] = 2
    t["uid"][0, :3] = (5, 2, 9)
    t["uid"][1, 0] = 0
    t["x"] = np.arange(3 * 4 * 9).reshape(3, 4, 9)
    t["keypoints"] = -1.0
    return t, np.array([3, 1, 0], np.int32)


def _kp(n):
    return (64.0 * np.arange(n)[:, None] + np.arange(NKP)[None, :]).astype(np.float32)


def _only_changed(before, after, cells):
    want = before.view(np.uint8).copy().view(DT)   # (as bytes: the padding too)
    for (s, j), row in cells.items():
        want[s, j]["keypoints"] = row
    assert after.tobytes() == want.tobytes()


def test_match_stranger_and_bad_scene():
    t, ntr = _table()
    ref = KpScatterRef(3)
    kp = _kp(7)
    owner = np.array([(0, 63), (0, -5), (1, 0), (0, 0), (2, 0), (-1, 0), (3, 0)], np.int32)   # (the second column is not read)
    uid = np.array([9, 5, 0, 7, 2, 5, 5], np.int32)
    keep = t.view(np.uint8).copy()
    out = ref.scatter(t, ntr, kp, owner, uid)
    assert t.tobytes() == keep.tobytes()                       # the argument is left alone
    _only_changed(t, out, {(0, 2): kp[0], (0, 0): kp[1], (1, 0): kp[2]})
    # uid 7 is nowhere; uid 2 of scene 2 sits past its n_tracks = 0; scenes -1 and 3 do not exist
    assert ref.dropped == {"scene": 2, "stranger": 2, "generation": 0} and ref.landed == 3


def test_rows_apply_in_order():
    t, ntr = _table()
    kp = _kp(2)
    out = KpScatterRef(3).scatter(t, ntr, kp, [(0, 0), (0, 0)], [2, 2])
    _only_changed(t, out, {(0, 1): kp[1]})


def test_generation_moved_and_ticket_retaken():
    t, ntr = _table()
    ref = KpScatterRef(3)
    kp = _kp(2)
    owner, uid = np.array([(0, 0), (1, 0)], np.int32), np.array([2, 0], np.int32)
    ref.take(0)
    ref.rebase([1])
    out = ref.scatter(t, ntr, kp, owner, uid, ticket=0)
    _only_changed(t, out, {(0, 1): kp[0]})                       # scene 1 moved on: its row is dropped, the same uid live or not
    assert ref.dropped["generation"] == 1
    out = ref.scatter(t, ntr, kp, owner, uid)                    # the uid form knows no generation
    _only_changed(t, out, {(0, 1): kp[0], (1, 0): kp[1]})
    ref.take(1)                                                  # a second ticket, taken after the rebase: lands ...
    _only_changed(t, ref.scatter(t, ntr, kp, owner, uid, ticket=1), {(0, 1): kp[0], (1, 0): kp[1]})
    _only_changed(t, ref.scatter(t, ntr, kp, owner, uid, ticket=0), {(0, 1): kp[0]})   # ... while ticket 0 still does not,
    ref.take(0)                                                  # until it is retaken
    _only_changed(t, ref.scatter(t, ntr, kp, owner, uid, ticket=0), {(0, 1): kp[0], (1, 0): kp[1]})
    ref.rebase()                                                 # every scene
    _only_changed(t, ref.scatter(t, ntr, kp, owner, uid, ticket=0), {})
    _only_changed(t, ref.scatter(t, ntr, kp, owner, uid, ticket=1), {})


def test_tickets_refused():
    t, ntr = _table()
    ref = KpScatterRef(3)
    kp, owner, uid = _kp(1), [(0, 0)], [2]
    for bad in (-1, 4):
        with pytest.raises(TicketError):
            ref.scatter(t, ntr, kp, owner, uid, ticket=bad)
        with pytest.raises(TicketError):
            ref.take(bad)
    with pytest.raises(TicketError):
        ref.scatter(t, ntr, kp, owner, uid, ticket=2)            # never taken
    ref.take(2)
    ref.scatter(t, ntr, kp, owner, uid, ticket=2)
    ref.take(2, with_uid=False)                                  # retaken without uids: nothing to scatter by
    with pytest.raises(TicketError):
        ref.scatter(t, ntr, kp, owner, uid, ticket=2)
