"""The deferred keypoint scatter on the GPU: `mmw_set_keypoints_uid` and `mmw_set_keypoints_ticket` (k_set_kp_uid, csrc/k_misc.hip),
which write the keypoint rows `mmw_features_async` took one or two frames earlier into the tracks that still exist.

Expected values come from tests/_kp_scatter_ref.py, a numpy restatement applied to the state read back with `tracks()` /
`num_tracks()`.  Payloads are exactly representable and unique per element, kp[i, e] = 64 i + e (+ 64 * a base per scatter), and
what is compared is ALL fields of EVERY record of EVERY scene as bytes: a row that is misrouted, or a store past the 57 keypoints,
shows wherever it lands.  No two rows of one call name the same track (which of two writers wins is unspecified).

1-3  the kernel's edges: the ballot search over a 64-track list in reversed uid order with a match at position 63, strangers and
     scene indices out of range, row counts around the 4-rows-per-block launch, a list compacted between take and scatter;
4-6  the ticket form: rows of a scene that `reset`, `reset_scenes` or `restore` touched since the ticket's `features_async` are
     dropped -- the scene's uids start over, and the same uid is (and is asserted to be) live again under another track;
7    the pipeline built on it against the frame-synchronous loop across a mid-run `reset_scenes` / `restore` that is not drained.
"""
import functools

import numpy as np
import pytest

from tests._kp_scatter_ref import KpScatterRef

pytestmark = pytest.mark.gpu

NKP = 57
INT32_MAX = 2 ** 31 - 1
N = 96
TOUCHED = (0, 7)


def _kp(n, base=0):
    return (64.0 * (base + np.arange(n))[:, None] + np.arange(NKP)[None, :]).astype(np.float32)


def _state(sb):
    return sb.num_tracks(), sb.tracks()


def _same(got, want, ctx=None):
    """Every field of every record of every scene, as bytes."""
    assert got.dtype == want.dtype and got.shape == want.shape
    for s in range(got.shape[0]):
        if got[s].tobytes() != want[s].tobytes():
            bad = [(j, k) for j in range(got.shape[1]) for k in got.dtype.names if got[s, j][k].tobytes() != want[s, j][k].tobytes()]
            raise AssertionError((ctx, "scene", s, "(position, field) that differ:", bad[:8]))


def _scatter(sb, kp, owner, uid, n=None, ticket=None):
    """Upload the rows and scatter the first n of them: the uid form, or the ticket form; waits."""
    n = len(kp) if n is None else n
    kp, owner, uid = (np.ascontiguousarray(a, dtype=t) for a, t in ((kp, np.float32), (owner, np.int32), (uid, np.int32)))
    p = [sb.buf(name, max(a.nbytes, 8)).upload(a).ptr for name, a in (("sc_kp", kp), ("sc_owner", owner), ("sc_uid", uid))]
    if ticket is None:
        sb.set_keypoints_uid_dev(p[0], p[1], p[2], n)
    else:
        sb.set_keypoints_ticket_dev(p[0], p[1], p[2], n, ticket)
    sb.synchronize()


def _take(sb, ticket, tag=""):
    """features_async(ticket) into buffers of this ticket's own -> (owner[n, 2], uid[n]) as the device wrote them."""
    cap = sb.S * sb.track_cap
    b_f = sb.buf("tk_feat" + tag, cap * sb.ring * 64 * 5 * 4)
    b_o = sb.buf("tk_owner" + tag, cap * 8)
    b_u = sb.buf("tk_uid" + tag, cap * 4)
    sb.features_async(b_f.ptr, b_o.ptr, b_u.ptr, cap, ticket=ticket)
    n = sb.features_wait(ticket)
    return b_o.download((n, 2), np.int32), b_u.download((n,), np.int32)


# ---- 1, 2: a planted scene of 64 tracks -------------------------------------------------------------------------------------
def _planted():
    """2 scenes, track_cap 64: scene 0 holds 64 live tracks under uids 63 .. 0 (tests/_snap_plant.py), scene 1 what four frames left."""
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    from tests._report_scenes import scenario
    from tests._snap_plant import plant_tracks
    sb = SceneBatch(_lib.default_config(tr_max_tracks=64, db_min_samples=12, track_cap=64, tr_lifetime_dynamic=100.0, tr_lifetime_static=100.0), 2, N)
    assert sb.track_cap == 64
    pts, cnt, dts = scenario()
    for f in range(4):
        sb.step_host(pts[f, :2].astype(np.float64), cnt[f, :2], dts[f, :2])
    assert (sb.num_tracks() >= 1).all()
    plant_tracks(sb, 0, list(range(63, -1, -1)))
    ntr, trk = _state(sb)
    assert ntr[0] == 64 and trk[0]["uid"].tolist() == list(range(63, -1, -1)) and 1 <= ntr[1] < 64
    return sb


def _rows_of_planted(trk, ntr, seed):
    """(owner, uid): scene 0's 64 uids in a shuffled order; between them, from row 1 on after every second one, the live tracks of
    scene 1, three strangers (uid 64, -1, INT32_MAX) and two scene indices out of range (-1 and S = 2).  owner[:, 1] is garbage."""
    rng = np.random.default_rng(seed)
    main = [(0, int(u)) for u in rng.permutation(64)]
    extra = [(1, int(u)) for u in trk[1, : ntr[1]]["uid"]] + [(0, 64), (0, -1), (1, INT32_MAX), (-1, 0), (2, 0)]
    rows = []
    while main or extra:
        rows += [main.pop(0)] if main else []
        rows += [extra.pop(0)] if extra else []
        rows += [main.pop(0)] if main else []
    owner = np.array([(s, g) for (s, _), g in zip(rows, rng.integers(-2 ** 31, 2 ** 31, len(rows)))], np.int32)
    return owner, np.array([u for _, u in rows], np.int32)


@pytest.mark.parametrize("form", ["uid", "ticket"])
def test_64_tracks_in_reversed_order_strangers_and_scenes_out_of_range(form):
    sb = _planted()
    ref = KpScatterRef(2)
    ntr, before = _state(sb)
    owner, uid = _rows_of_planted(before, ntr, 1)
    kp = _kp(len(owner))
    ticket = None
    if form == "ticket":
        ticket = 1
        _take(sb, ticket)
        ref.take(ticket)
    _scatter(sb, kp, owner, uid, ticket=ticket)
    after = sb.tracks()
    _same(after, ref.scatter(before, ntr, kp, owner, uid, ticket=ticket))
    assert ref.landed == 64 + ntr[1] and ref.dropped == {"scene": 2, "stranger": 3, "generation": 0}
    i0 = int(np.flatnonzero((owner[:, 0] == 0) & (uid == 0))[0])
    assert np.array_equal(after[0, 63]["keypoints"], kp[i0])     # the match at list position 63
    assert np.array_equal(sb.num_tracks(), ntr)
    sb.check()
    sb.close()


@pytest.mark.parametrize("n_rows", [0, 1, 3, 4, 5, 67])
def test_row_counts_around_the_four_row_block(n_rows):
    """A block of 256 threads takes four rows: 1 and 3 leave the only block partial, 5 and 67 the last one; the rows behind n_rows,
    which are uploaded too, must not be read.  0 rows with NULL pointers is a no-op."""
    sb = _planted()
    ntr, before = _state(sb)
    owner, uid = _rows_of_planted(before, ntr, 2)
    assert len(owner) >= 67 + 3 and (n_rows < 3 or len(set(owner[:3, 0])) == 2)      # rows behind the count; two scenes in the first block
    kp = _kp(len(owner))
    if n_rows == 0:
        assert sb.L.mmw_set_keypoints_uid(sb.h, None, None, None, 0) == 0
        sb.synchronize()
        _same(sb.tracks(), before, "NULL")
    _scatter(sb, kp, owner, uid, n=n_rows)
    ref = KpScatterRef(2)
    _same(sb.tracks(), ref.scatter(before, ntr, kp[:n_rows], owner[:n_rows], uid[:n_rows]), n_rows)
    assert ref.landed + sum(ref.dropped.values()) == n_rows
    sb.check()
    sb.close()


# ---- 3: rows taken before a track expires, scattered after the list was compacted ------------------------------------------------
@pytest.mark.parametrize("form", ["uid", "ticket"])
def test_rows_taken_before_an_expiry_scattered_after_the_list_was_compacted(form):
    """5 scenes of tests/_report_scenes.py (targets that leave, lifetimes of three frames): rows taken behind frame 7, scattered behind
    frame 10.  Followed through the C oracle, four tracks that had a row are gone by then and four have moved to another position."""
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    from tests._report_scenes import CFG_KW, scenario
    S, F1, F2 = 5, 7, 10
    pts, cnt, dts = scenario()
    sb = SceneBatch(_lib.default_config(**CFG_KW), S, N)
    ref = KpScatterRef(S)
    for f in range(F1 + 1):
        sb.step_host(pts[f, :S].astype(np.float64), cnt[f, :S], dts[f, :S])
    owner, uid = _take(sb, 0)
    ref.take(0)
    for f in range(F1 + 1, F2 + 1):
        sb.step_host(pts[f, :S].astype(np.float64), cnt[f, :S], dts[f, :S])
    ntr, before = _state(sb)
    now = {(s, int(before[s, j]["uid"])): j for s in range(S) for j in range(ntr[s])}
    moved = sum(1 for (s, j), u in zip(owner, uid) if (int(s), int(u)) in now and now[(int(s), int(u))] != j)
    gone = sum(1 for (s, j), u in zip(owner, uid) if (int(s), int(u)) not in now)
    assert moved >= 1 and gone >= 1, (moved, gone)
    kp = _kp(len(owner))
    ticket = 0 if form == "ticket" else None
    _scatter(sb, kp, owner, uid, ticket=ticket)
    _same(sb.tracks(), ref.scatter(before, ntr, kp, owner, uid, ticket=ticket))
    assert ref.dropped == {"scene": 0, "stranger": gone, "generation": 0} and ref.landed == len(owner) - gone
    sb.check()
    sb.close()


# ---- 4-6: the generation ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _walkers(n_scenes, n_frames):
    """Two targets a scene, in view throughout: a track each from the first frame on, in the first frame after a reset again."""
    from mmwave_msc_amd.synth import make_batch
    out = make_batch(range(4100, 4100 + n_scenes), n_frames, N, 2)
    for a in out:
        a.setflags(write=False)
    return out


def _ctx8(**kw):
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    return SceneBatch(_lib.default_config(tr_max_tracks=4, db_min_samples=12, **kw), 8, N)


def _step(sb, f):
    pts, cnt, dts = _walkers(8, 8)
    sb.step_host(pts[f].astype(np.float64), cnt[f], dts[f])


def _mask(scenes, S=8):
    m = np.zeros(S, np.int32)
    m[list(scenes)] = 1
    return m


@pytest.mark.parametrize("how", ["reset_scenes", "restore", "reset"])
def test_rows_of_a_scene_touched_since_the_ticket_are_dropped(how):
    sb = _ctx8()
    ref = KpScatterRef(8)
    for f in range(4):
        _step(sb, f)
    owner, uid = _take(sb, 0)
    ref.take(0)
    assert all((owner[:, 0] == s).sum() >= 1 for s in range(8)) and (uid == 0).sum() == 8
    touched = range(8) if how == "reset" else TOUCHED
    if how == "restore":       # a blob of the very same scenes: every uid a row names is live again, in the very same record
        was = sb.tracks()
        sb.restore(sb.snapshot(scenes=list(TOUCHED)), scenes=list(TOUCHED))
        _same(sb.tracks(), was)
    else:
        if how == "reset":
            sb.reset()
        else:
            sb.reset_scenes(_mask(TOUCHED))
        assert (sb.num_tracks()[list(touched)] == 0).all()
        _step(sb, 4)            # ... until the touched scenes hold a track of uid 0 again
    ref.rebase(None if how == "reset" else TOUCHED)
    ntr, before = _state(sb)
    in_touched = np.isin(owner[:, 0], list(touched))
    for s in touched:
        assert 0 in before[s, : ntr[s]]["uid"].tolist(), s
    alias = sum(1 for (s, _), u in zip(owner[in_touched], uid[in_touched]) if int(u) in before[s, : ntr[s]]["uid"].tolist())
    assert alias >= len(touched)   # rows the uid form would write into a track of after
    kp = _kp(len(owner))
    _scatter(sb, kp, owner, uid, ticket=0)
    after = sb.tracks()
    _same(after, ref.scatter(before, ntr, kp, owner, uid, ticket=0), how)
    for s in touched:
        assert after[s].tobytes() == before[s].tobytes(), s
    assert ref.dropped == {"scene": 0, "stranger": 0, "generation": int(in_touched.sum())} and ref.landed == int((~in_touched).sum())
    assert ref.landed > 0 or how == "reset"
    sb.check()
    sb.close()


def test_two_tickets_in_flight_around_one_reset_scenes():
    sb = _ctx8()
    ref = KpScatterRef(8)
    for f in range(4):
        _step(sb, f)
    owner0, uid0 = _take(sb, 0, "0")
    ref.take(0)
    sb.reset_scenes(_mask(TOUCHED))
    ref.rebase(TOUCHED)
    for f in range(4, 7):
        _step(sb, f)
    owner1, uid1 = _take(sb, 1, "1")
    ref.take(1)
    ntr, before = _state(sb)
    in_touched1 = np.isin(owner1[:, 0], TOUCHED)
    assert in_touched1.sum() >= 2 and np.isin(owner0[:, 0], TOUCHED).sum() >= 2
    kp1 = _kp(len(owner1), base=1000)
    _scatter(sb, kp1, owner1, uid1, ticket=1)                       # taken after the reset: the touched scenes' rows land
    after1 = sb.tracks()
    _same(after1, ref.scatter(before, ntr, kp1, owner1, uid1, ticket=1), "ticket 1")
    assert ref.landed == len(owner1) and ref.dropped["generation"] == 0
    kp0 = _kp(len(owner0), base=2000)
    _scatter(sb, kp0, owner0, uid0, ticket=0)                       # taken before it: they do not
    after0 = sb.tracks()
    _same(after0, ref.scatter(after1, ntr, kp0, owner0, uid0, ticket=0), "ticket 0")
    assert ref.dropped["generation"] == int(np.isin(owner0[:, 0], TOUCHED).sum())
    for s in TOUCHED:
        assert after0[s].tobytes() == after1[s].tobytes()
    owner2, uid2 = _take(sb, 0, "0")                                # ticket 0 retaken: lands
    ref.take(0)
    kp2 = _kp(len(owner2), base=3000)
    landed = ref.landed
    _scatter(sb, kp2, owner2, uid2, ticket=0)
    _same(sb.tracks(), ref.scatter(after0, ntr, kp2, owner2, uid2, ticket=0), "ticket 0 retaken")
    assert ref.landed - landed == len(owner2) == len(owner1)
    sb.check()
    sb.close()


def test_tickets_that_hold_no_uid_rows_are_refused_and_write_nothing():
    from mmwave_msc_amd import _lib
    sb = _ctx8()
    for f in range(4):
        _step(sb, f)
    owner, uid = _take(sb, 1)
    ntr, before = _state(sb)
    kp = _kp(len(owner))
    assert len(owner) >= 8

    def refused(ticket):
        with pytest.raises(_lib.MmwError) as e:
            _scatter(sb, kp, owner, uid, ticket=ticket)
        assert e.value.code == _lib.E_ARG
        sb.synchronize()
        _same(sb.tracks(), before, ticket)

    refused(-1)
    refused(4)
    refused(2)                                                      # never used
    feat_h, owner_h = sb.features_host()                            # mmw_features: ticket 3, without uids
    assert np.array_equal(owner_h, owner)
    refused(3)
    cap = sb.S * sb.track_cap
    sb.features_async(sb.buf("tk_feat", 0).ptr, sb.buf("tk_owner", 0).ptr, None, cap, ticket=1)   # ticket 1 retaken with uid = NULL
    assert sb.features_wait(1) == len(owner)
    refused(1)
    _take(sb, 1)                                                    # ... and with uids again: accepted
    _scatter(sb, kp, owner, uid, ticket=1)
    ref = KpScatterRef(8)
    ref.take(1)
    _same(sb.tracks(), ref.scatter(before, ntr, kp, owner, uid, ticket=1))
    assert ref.landed == len(owner)
    sb.check()
    sb.close()


# ---- 7: the pipeline against the frame-synchronous loop across a reset / restore in mid-flight ------------------------------------
P_S, P_K, P_MIN, P_SCENES = 6, 6, 100, (1, 4)
# MODEL_MIN_INPUT = 100 on these scenes (about 43 points a target a frame): a track is eligible once its ring holds three frames.
# reset_scenes before frame 6, frames 6 and 7 follow: the reborn tracks hold one, then two frames.  restore before frame 6 of a
# blob taken behind frame 0 (one frame in every ring), frame 6 follows: two frames.  Both are asserted on the C oracle below.
P_FRAMES = {"reset_scenes": 8, "restore": 7}


def _oracle_eligible(how):
    """Per touched scene: the list positions oracle.c_oracle's features() takes in every frame the scene lives through."""
    from oracle import c_oracle as co
    pts, cnt, dts = _walkers(P_S, 8)
    cfg = co.default_config(tr_max_tracks=4, db_min_samples=12, model_min_input=P_MIN)
    out = {}
    for s in P_SCENES:
        orc, per = co.OracleScene(cfg, N), {}
        for f in range(P_FRAMES[how]):
            if f == P_K:
                orc = co.OracleScene(cfg, N)
                if how == "restore":
                    orc.track(pts[0, s, : cnt[0, s]].astype(np.float64), float(dts[0, s]))
            orc.track(pts[f, s, : cnt[f, s]].astype(np.float64), float(dts[f, s]))
            per[f] = (orc.features()[1].tolist(), orc.n_tracks)
        out[s] = per
    return out


def _pipeline_loop(how, schedule):
    """schedule: "sync" (estimate_posture completes before the next track()), "serial" / "overlap" (PosturePipeline)."""
    import torch
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    from mmwave_msc_amd.mars import MarsCNN, random_keras_weights
    from mmwave_msc_amd.posture import PosturePipeline
    pts, cnt, dts = _walkers(P_S, 8)
    dev = torch.device("cuda", 0)
    model = MarsCNN.from_keras_weights(random_keras_weights(3, 3)).to("cuda:0")
    sb = SceneBatch(_lib.default_config(tr_max_tracks=4, db_min_samples=12, model_min_input=P_MIN), P_S, N, device=0)
    pipe = PosturePipeline(sb, model, P_S * sb.track_cap, overlap=(schedule == "overlap")) if schedule != "sync" else None
    with torch.cuda.stream(pipe.A if pipe else torch.cuda.current_stream(dev)):
        d_pts = torch.from_numpy(np.array(pts)).to(dev).double()
        d_cnt = torch.from_numpy(np.array(cnt)).to(dev)
        d_dt = torch.from_numpy(np.array(dts)).to(dev)
    torch.cuda.synchronize()
    blob = None
    for f in range(P_FRAMES[how]):
        if f == P_K:                                                # not drained: up to two frames' rows are in flight
            if how == "restore":
                sb.restore(blob, scenes=list(P_SCENES))
            else:
                sb.reset_scenes(_mask(P_SCENES, P_S))
        sb.step_dev(d_pts[f].data_ptr(), d_cnt[f].data_ptr(), d_dt[f].data_ptr())
        if pipe:
            pipe.after_step()
        else:
            sb.synchronize()
            feat, owner = sb.features_host()
            if len(owner):
                sb.set_keypoints_host(model.predict_numpy(feat), owner)
        if f == 0 and how == "restore":
            blob = sb.snapshot(scenes=list(P_SCENES))
    if pipe:
        pipe.close()
    sb.check()
    ntr = sb.num_tracks()
    trk = sb.tracks(cap=max(int(ntr.max()), 1))
    posture = np.array(list(sb.cfg.default_posture), np.float32)
    sb.close()
    torch.cuda.synchronize()
    return ntr, trk, posture


@functools.lru_cache(maxsize=None)
def _sync_loop(how):
    return _pipeline_loop(how, "sync")


@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("how", ["reset_scenes", "restore"])
def test_pipeline_equals_synchronous_loop_across_a_reset_in_mid_flight(how, overlap):
    """Rows of frames 4 and 5 are in flight when scenes 1 and 4 are reset (or restored to their state behind frame 0): the track that
    carries uid 0 afterwards is another one (or the same one of another time) and is never eligible itself, so it must end with
    `default_posture` -- not with the keypoints the CNN computed for the uid 0 of before."""
    elig = _oracle_eligible(how)
    for s in P_SCENES:
        assert 0 in elig[s][P_K - 2][0] and 0 in elig[s][P_K - 1][0], (s, elig[s])            # uid 0 of before: rows in flight
        for f in range(P_K, P_FRAMES[how]):
            assert elig[s][f][1] >= 1 and 0 not in elig[s][f][0], (s, f, elig[s])             # uid 0 of after: never a row
    n2, t2, posture = _sync_loop(how)
    n1, t1, _ = _pipeline_loop(how, "overlap" if overlap else "serial")
    assert np.array_equal(n1, n2) and (n1 >= 2).all()
    for s in range(P_S):
        a, b = t1[s, : n1[s]], t2[s, : n2[s]]
        assert np.array_equal(a["uid"], b["uid"]) and np.array_equal(a["x"], b["x"]), s
        assert np.allclose(a["keypoints"], b["keypoints"], rtol=0, atol=1e-6), (s, np.abs(a["keypoints"] - b["keypoints"]).max(axis=1))
    for s in P_SCENES:
        for t in (t1, t2):
            assert t[s, 0]["uid"] == 0 and t[s, 0]["keypoints"].tobytes() == posture.tobytes(), s
    others = [s for s in range(P_S) if s not in P_SCENES]
    assert all((t1[s, : n1[s]]["keypoints"] != posture).any() for s in others)               # the CNN did run for the scenes left alone
