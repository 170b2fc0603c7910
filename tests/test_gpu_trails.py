"""Track trails (mmw_trails_*, include/mmw.h) on the GPU: per live uid a ring of its last `depth` sampled positions, the time of
its first sample and the distance it walked.

Expected values come from tests/_trail_ref.py, a numpy restatement of the header's rules applied to the state read back with
`tracks()` / `num_tracks()` after each step; it carries its own trail state.  Every field is compared exactly, floats by their
bytes.  `travelled` is the exception: it must lie within total * 2**-52 * |want| of the restatement's and be NaN where the
restatement's is.  That bound is derived, not measured: the two sides run the same fp64 operations in the same order (the library is
built with -ffp-contract=off) except for sqrt, where the device's may differ from the correctly rounded one by an ulp, i.e. by at
most 2**-52 relative; each of the at most `total` samples adds one such term, every term is non-negative, so the sum only grows and
each term's error is at most 2**-52 of the final sum.  The tests print how many values were bit-equal.  The scenario is
tests/_report_scenes.py's (24 scenes x 96 points x 12 frames: tracks are born, walk and expire inside the run)."""
import numpy as np
import pytest

from tests._feature_run import BASE, S2, TrailRun, cut, nothing_else_moves, same_trails, step, step_empty
from tests._layouts import make_checked
from tests._report_scenes import CFG_KW, F, N, S, scenario
from tests._snap_plant import directory, plant_state, record_at
from tests._trail_ref import TrailRef

pytestmark = pytest.mark.gpu


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["per_scene", "one_workgroup"])
def test_depth_4_sampled_and_exported_after_every_step(layout):
    sb = make_checked(S, N, layout, **CFG_KW)
    sb.enable_report()
    run = TrailRun(sb, 4)
    pts, cnt, dts = scenario()
    d_flags, d_t = sb.alloc(S * 4), sb.alloc(S * 8)
    clock = np.zeros(S)
    for f in range(F):
        run.step(f)
        clock = clock + dts[f]
        # the frame's n_pts array is the flags: a scene without a frame is not sampled
        d_flags.upload(cnt[f]); d_t.upload(clock)
        sb.sample_trails_dev(d_flags.ptr, d_t.ptr)
        run.ref.sample(sb.tracks(), sb.num_tracks(), flags=cnt[f], t=clock)
        dir_, points = run.compare((layout, f))
        rows, _ = sb.report_host(scene_base=BASE)
        for k in ("scene", "slot", "uid"):
            assert np.array_equal(dir_[k], rows[k]), (f, k)
        assert int(dir_["count"].sum()) == len(points) and (dir_["count"] == np.minimum(dir_["total"], 4)).all()
    sb.check()
    for b in (d_flags, d_t):
        b.free()
    sb.close()
    tally = dict(wraps=run.ref.wraps, moved=run.ref.moved, reused=run.ref.reused)
    print("trail tallies", layout, tally, "travelled bit-equal", run.equal, "of", run.seen)
    assert tally["wraps"] >= 1 and tally["moved"] >= 1 and tally["reused"] >= 1, tally


# 2 ------------------------------------------------------------------------------------------------------------------------
def test_scene_flags_call_ordinals_and_the_trimmed_export():
    sb = make_checked(S, N, "per_scene", **CFG_KW)
    run = TrailRun(sb, 4)
    for f in range(F):
        run.step(f)
        run.sample(scenes=[s for s in range(S) if not (f % 2 == 1 and s % 3 == 0)])   # (t = NULL: the scenes' call ordinals)
        run.compare(f)
    assert run.ref.ordinal.tolist() == [F - F // 2 if s % 3 == 0 else F for s in range(S)]
    full_d, full_p = run.compare("full")
    last_d, last_p = run.compare("last 2", last=2)
    assert (full_d["count"] > 2).any() and len(last_p) < len(full_p)
    for k in ("scene", "slot", "uid", "total", "t_first", "travelled"):
        assert last_d[k].tobytes() == full_d[k].tobytes(), k
    assert np.array_equal(last_d["count"], np.minimum(full_d["count"], 2))
    from mmwave_msc_amd import trails
    for a, b in zip(trails.split(last_d, last_p), trails.split(full_d, full_p)):
        assert a.tobytes() == b[-2:].tobytes()
    # the points' t are ordinals: whole numbers, ascending inside a trail, and a scene left out every other frame has seen fewer
    assert (full_p["t"] == np.floor(full_p["t"])).all() and all((np.diff(v["t"]) > 0).all() for v in trails.split(full_d, full_p))
    print("travelled bit-equal", run.equal, "of", run.seen)
    sb.close()


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_capacity_is_decided_on_the_device_and_the_export_consumes_nothing():
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import MmwError
    sb = make_checked(S2, N, "per_scene", **CFG_KW)
    run = TrailRun(sb, 4, cut(S2))
    for f in range(8):
        run.step(f)
        run.sample(t=np.full(S2, 0.25 * f))
    want_d, want_p = run.ref.export(sb.tracks(), sb.num_tracks())
    n_t, n_p = len(want_d), len(want_p)
    assert n_t >= S2 and n_p > n_t
    sent_d, sent_p = np.full(n_t * 40 + 64, 0xA5, np.uint8), np.full(n_p * 24 + 64, 0x5A, np.uint8)
    b_d, b_p = sb.alloc(sent_d.nbytes).upload(sent_d), sb.alloc(sent_p.nbytes).upload(sent_p)
    for t, (cap_t, cap_p) in enumerate(((n_t, n_p - 1), (n_t - 1, n_p), (0, 0))):
        sb.trails_dev(b_d.ptr if cap_t else None, cap_t, b_p.ptr if cap_p else None, cap_p, 0, t)
        with pytest.raises(MmwError) as ei:
            sb.trails_wait(t)
        assert ei.value.code == _lib.E_CAPACITY and ei.value.needed == (n_t, n_p), (t, ei.value.needed)
        assert np.array_equal(b_d.download(sent_d.shape, np.uint8), sent_d) and np.array_equal(b_p.download(sent_p.shape, np.uint8), sent_p)
    # nothing was consumed: the full export is the restatement's, and nothing is written past the counts
    sb.trails_dev(b_d.ptr, n_t, b_p.ptr, n_p, 0, 0)
    assert sb.trails_wait(0) == (n_t, n_p)
    got = (b_d.download((n_t,), _lib.TRAIL_TRACK_DTYPE), b_p.download((n_p,), _lib.TRAIL_POINT_DTYPE))
    same_trails(got, (want_d, want_p), "exact caps")
    assert np.array_equal(b_d.download(sent_d.shape, np.uint8)[n_t * 40:], sent_d[n_t * 40:])
    assert np.array_equal(b_p.download(sent_p.shape, np.uint8)[n_p * 24:], sent_p[n_p * 24:])
    run.compare("after the refusals", scene_base=0)
    # the same state under three tickets before any wait: three equal results
    bufs = [(sb.alloc(n_t * 40), sb.alloc(n_p * 24)) for _ in range(3)]
    for t, (bd, bp) in enumerate(bufs):
        sb.trails_dev(bd.ptr, n_t, bp.ptr, n_p, 0, t, BASE)
    for t in (2, 0, 1):
        assert sb.trails_wait(t) == (n_t, n_p)
    outs = [bd.download((n_t,), _lib.TRAIL_TRACK_DTYPE).tobytes() + bp.download((n_p,), _lib.TRAIL_POINT_DTYPE).tobytes() for bd, bp in bufs]
    assert outs[0] == outs[1] == outs[2]
    same_trails((np.frombuffer(outs[0][: n_t * 40], _lib.TRAIL_TRACK_DTYPE), np.frombuffer(outs[0][n_t * 40:], _lib.TRAIL_POINT_DTYPE)),
                run.ref.export(sb.tracks(), sb.num_tracks(), scene_base=BASE), "tickets")
    # the argument checks: nothing is queued, the message names the entry
    for bad in (lambda: sb.trails_dev(None, 1, b_p.ptr, n_p), lambda: sb.trails_dev(b_d.ptr, -1, b_p.ptr, n_p),
                lambda: sb.trails_dev(b_d.ptr + 4, n_t, b_p.ptr, n_p), lambda: sb.trails_dev(b_d.ptr, n_t, b_p.ptr + 4, n_p),
                lambda: sb.trails_dev(b_d.ptr, n_t, b_p.ptr, n_p, -1), lambda: sb.trails_dev(b_d.ptr, n_t, b_p.ptr, n_p, 0, 4),
                lambda: sb.trails_wait(1), lambda: sb.sample_trails_dev(b_d.ptr + 2, None)):
        with pytest.raises(MmwError) as ei:
            bad()
        assert ei.value.code == _lib.E_ARG
    run.compare("after the refused arguments")
    for b in [b_d, b_p] + [x for p in bufs for x in p]:
        b.free()
    sb.close()


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_reset_and_restore_end_the_trails_of_their_scenes_only():
    S4, reset, restored = 8, (1, 5), (2, 6)
    sb = make_checked(S4, N, "per_scene", **CFG_KW)
    run = TrailRun(sb, 4, cut(S4))
    blob = None
    for f in range(7):
        run.step(f)
        run.sample(t=np.full(S4, 0.5 * f))
        run.compare(f)
        if f == 3:
            blob = sb.snapshot(list(restored))
    before, _ = run.compare("before")
    sb.reset_scenes(np.isin(np.arange(S4), reset))
    sb.restore(blob, scenes=list(restored))
    run.ref.rebase(reset + restored)
    d, p = run.compare("voided")                      # before the next sample call: exactly those scenes' entries are empty
    touched = np.isin(d["scene"] - BASE, reset + restored)
    assert touched.any() and not d["total"][touched].any() and not d["count"][touched].any()
    assert not d["t_first"][touched].any() and not d["travelled"][touched].any()
    assert (d["total"][~touched] > 0).all() and (~touched).sum() >= 4
    keep = ~np.isin(before["scene"] - BASE, reset + restored)
    for k in d.dtype.names:                            # the other scenes' entries are what they were, bit for bit (but `first`)
        assert k == "first" or d[k][~touched].tobytes() == before[k][keep].tobytes(), k
    assert not np.isin(d["scene"] - BASE, reset).any() and np.isin(d["scene"] - BASE, restored).any()   # (a reset scene holds nobody)
    run.step(7)
    run.sample(t=np.full(S4, 3.5))
    d, p = run.compare("after")
    touched = np.isin(d["scene"] - BASE, reset + restored)
    assert np.isin(d["scene"] - BASE, reset).any(), "the reset scenes spawned no track in the next frame"
    assert (d["total"][touched] == 1).all() and (d["t_first"][touched] == 3.5).all() and not d["travelled"][touched].any()
    assert (d["total"][~touched] > 1).any()
    # mmw_reset: every scene
    sb.reset()
    run.ref.rebase()
    d, p = run.compare("reset")
    assert len(d) == 0 and len(p) == 0
    run.step(0)
    run.sample()
    d, _ = run.compare("after reset")
    assert len(d) and (d["total"] == 1).all() and (d["t_first"] == 8.0).all()    # (t = NULL: eight earlier calls; resets do not restart the ordinal)
    print("travelled bit-equal", run.equal, "of", run.seen)
    sb.close()


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_planted_positions_walk_overflow_signed_zero_and_nan():
    """Four tracks' states written through a snapshot blob (tests/_snap_plant.py's plant_state: x at REC_X, P at REC_P, the lifetime
    at REC_LIFETIME of a track's record), ONE restore -- a restore ends the scene's trails --, then the tracker itself moves them: a
    step on an empty frame predicts x += (lifetime + dt) * v, exactly for these values, and its Kalman update (towards the old
    centroid) leaves x alone because the planted covariance is zero and stays zero with kf_q_std = 0: the gain is 0."""
    kw = dict(CFG_KW, tr_lifetime_dynamic=100.0, tr_lifetime_static=100.0, kf_q_std=0.0)
    sb = make_checked(S2, N, "per_scene", **kw)
    data = cut(S2)
    for f in range(4):
        step(sb, f, data)
    assert (sb.num_tracks() >= 1).all()
    blob = bytearray(sb.snapshot())
    ents = directory(blob)
    WALK, BIG, NEG, NAN = 0, 1, 2, 3                  # the scene whose track 0 carries each plant
    plants = {WALK: [0.0, 0.0, 1.0, 3.0, 4.0, 0.0], BIG: [1e39, 2.0, 1.0, 0.0, 0.0, 0.0], NEG: [-0.0, 1.0, -0.0, 0.0, 0.0, 0.0],
              NAN: [0.0, 0.0, 1.0, np.nan, 0.0, 0.0]}
    for sc, x in plants.items():
        plant_state(blob, record_at(ents, sc), x)
    sb.restore(bytes(blob))
    run = TrailRun(sb, 8, data)

    def entry(d, sc):
        return d[(d["scene"] == BASE + sc) & (d["slot"] == 0)][0]

    seen = []
    for k, dt in enumerate((None, 1.0, 0.0)):   # sample; step dt = 1; sample; sample again; step dt = 0 (the lifetime is 1 by then); sample
        if dt is not None:
            step_empty(sb, dt)
        run.sample(t=np.full(S2, float(k)))
        d, p = run.compare(("planted", k))
        seen.append((d, p))
        if k == 1:
            run.sample(t=np.full(S2, 1.5))
            seen.append(run.compare(("planted", "twice")))
    from mmwave_msc_amd import trails
    walk = [entry(d, WALK) for d, _ in seen]
    assert [w["total"] for w in walk] == [1, 2, 3, 4]
    assert [w["travelled"].tobytes() for w in walk] == [np.float64(v).tobytes() for v in (0.0, 5.0, 5.0, 10.0)]
    d, p = seen[-1]
    parts = dict((int(e["scene"]) - BASE, v) for e, v in zip(d, trails.split(d, p)) if e["slot"] == 0)
    assert parts[WALK]["x"].tolist() == [0.0, 3.0, 3.0, 6.0] and parts[WALK]["y"].tolist() == [0.0, 4.0, 4.0, 8.0]
    assert parts[WALK]["t"].tolist() == [0.0, 1.0, 1.5, 2.0] and entry(d, WALK)["t_first"] == 0.0
    assert (parts[BIG]["x"] == np.inf).all() and np.isfinite(entry(d, BIG)["travelled"]) and entry(d, BIG)["travelled"] == 0.0
    first = seen[0][1][entry(seen[0][0], NEG)["first"]]
    assert first["x"] == 0.0 and np.signbit(first["x"]) and np.signbit(first["z"]) and not np.signbit(first["y"])
    nan = [entry(dd, NAN) for dd, _ in seen]
    assert nan[0]["travelled"] == 0.0 and all(np.isnan(v["travelled"]) for v in nan[1:]), [v["travelled"] for v in nan]
    assert not np.isnan(parts[NAN]["x"][0]) and np.isnan(parts[NAN]["x"][1:]).all()
    sb.close()


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_depth_1_depth_256_and_the_refused_depths():
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import MmwError
    data = cut(2)
    for depth in (1, _lib.TRAIL_DEPTH_MAX):
        sb = make_checked(2, N, "per_scene", **CFG_KW)
        with pytest.raises(MmwError) as ei:       # before enabling, every other entry is refused
            sb.sample_trails()
        assert ei.value.code == _lib.E_ARG
        run = TrailRun(sb, depth, data)
        for f in range(F):
            run.step(f)
            run.sample(t=np.full(2, 0.125 * f))
            d, p = run.compare((depth, f))
            assert (d["count"] == np.minimum(d["total"], depth)).all()
            if f == 5:
                for bad in (_lib.TRAIL_DEPTH_MAX + 1, -1):
                    with pytest.raises(MmwError) as ei:
                        sb.enable_trails(bad)
                    assert ei.value.code == _lib.E_ARG     # ... and the earlier enablement goes on working (the frames that follow)
        assert d["total"].max() > 1
        if depth == 1:
            # enabling again starts over
            sb.enable_trails(3)
            run.ref = TrailRef(2, sb.track_cap, 3)
            d, _ = run.compare("enabled again")
            assert len(d) and not d["total"].any()
            run.sample()
            d, _ = run.compare("enabled again, sampled")
            assert (d["total"] == 1).all() and not d["t_first"].any()
        sb.enable_trails(0)
        b = sb.alloc(64)
        for entry in (lambda: sb.sample_trails(), lambda: sb.trails_dev(b.ptr, 1, b.ptr, 1), lambda: sb.trails_wait(0), lambda: sb.trails_host()):
            with pytest.raises(MmwError) as ei:
                entry()
            assert ei.value.code == _lib.E_ARG
        sb.enable_trails(0)      # (off already: MMW_OK)
        step(sb, 0, data)       # the context steps on, and resets launch nothing of the trails
        sb.reset()
        b.free()
        sb.close()
        print("depth", depth, "travelled bit-equal", run.equal, "of", run.seen)


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_trails_leave_the_tracker_alone():
    a = make_checked(S2, N, "per_scene", **CFG_KW)
    b = make_checked(S2, N, "per_scene", **CFG_KW)
    data = cut(S2)
    a.enable_trails(4)

    def drive(f):
        a.sample_trails()
        a.trails_host()

    nothing_else_moves(a, b, data, F, drive)
    a.close(); b.close()


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_more_than_32_live_tracks_in_one_scene():
    """track_cap = 64 with 36 targets in scene 0 (lanes and trail slots past 32: the upper half of the 64-bit ballots) and 5 in
    scene 1; depth 2 over 5 frames wraps the rings."""
    from tests._grid_scenes import many_tracks
    sb, pts, n_s, n_pts, frames, _ = many_tracks("track_cap_64")
    run = TrailRun(sb, 2)
    most = 0
    for f in range(frames):
        sb.step_host(pts[f].astype(np.float64), np.full(n_s, n_pts, np.int32), np.full(n_s, 0.1))
        run.sample(t=np.full(n_s, 0.1 * f))
        d, _ = run.compare(f)
        most = max(most, int(sb.num_tracks().max()))
    assert most > 32 and run.ref.wraps >= 1, (most, run.ref.wraps)
    assert (d["slot"] > 32).any() and (d["total"][d["slot"] > 32] > 1).any()
    print("travelled bit-equal", run.equal, "of", run.seen)
    sb.check()
    sb.close()
