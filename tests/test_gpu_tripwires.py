"""Tripwires (mmw_tripwires_*, include/mmw.h) on the GPU: per scene up to 16 directed segments, per wire the tracks that went
across it either way, and every crossing as an event with the track's uid in a per-scene log.

Expected values come from tests/_tripwire_ref.py, a numpy restatement of the header's rules applied to the state read back with
`tracks()` / `num_tracks()` after each step; it carries its own wires, sides, counters and log.  Every field of every row and event
is compared by its bytes -- there is no tolerance anywhere: the device takes no sqrt, and both sides run the same fp64 products
and sums in the same order (the library is built with -ffp-contract=off).  The scenario is tests/_report_scenes.py's (24 scenes x 96
points x 12 frames: tracks are born, walk and expire inside the run).

The planted tests write track states into a snapshot blob (tests/_snap_plant.py's plant_state: x at REC_X, P at REC_P, the lifetime
at REC_LIFETIME of a track's record) and restore it ONCE; then steps on empty frames move the tracks: predict is
x += (lifetime + dt) * v with lifetime += dt, so the multiplier of step k is the running sum L_k of the dts given so far -- any
sequence of non-zero L_k, negative ones included, by giving dt_k = L_k - L_(k-1) -- and the Kalman update leaves x alone because
the planted covariance is zero and stays zero with kf_q_std = 0.  Every planted value is a small dyadic number: each product and
sum below is exact, and the positions are asserted as read back."""
import numpy as np
import pytest

from tests._feature_run import BASE, REPORT, S2, TRACKS, TrailRun, TripRun, cut, n_kind, nothing_else_moves, same_pair, settled, step
from tests._layouts import make_checked
from tests._report_scenes import CFG_KW, F, N, S, coming_and_going, scenario, strips, wires16
from tests._snap_plant import FAR, directory, dts as _dts, plant_state, record_at
from tests._tripwire_ref import TripRef

pytestmark = pytest.mark.gpu


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["per_scene", "one_workgroup"])
def test_scenario_sampled_and_exported_after_every_step(layout):
    """16 wires per scene from (c, 8) to (c, 0), c = -2 + 0.25 k, margin 0.03, log depth 64.  Through the C oracle, identities
    matched by continuity, this scenario holds 15 forward and 18 backward crossings and 70 sides kept by the band, in 17 of the 24
    scenes (31 / 35 crossings at margin 0): the floors asserted on the restatement are a third of that."""
    from mmwave_msc_amd.tripwires import Tally
    sb = make_checked(S, N, layout, **CFG_KW)
    run = TripRun(sb, 64)
    run.set_wires(wires16(S))
    pts, cnt, dts = scenario()
    d_flags, d_t = sb.alloc(S * 4), sb.alloc(S * 8)
    clock = np.zeros(S)
    tally = Tally()
    for f in range(F):
        run.step(f)
        clock = clock + dts[f]
        # the frame's n_pts array is the flags: a scene without a frame is not sampled
        d_flags.upload(cnt[f]); d_t.upload(clock)
        sb.sample_tripwires_dev(d_flags.ptr, d_t.ptr)
        run.ref.sample(sb.tracks(), sb.num_tracks(), flags=cnt[f], t=clock)
        rows, events = run.compare((layout, f))
        tally.apply(events)
        assert len(rows) == 16 * S and not rows["lost"].any()
    sb.check()
    for b in (d_flags, d_t):
        b.free()
    sb.close()
    ref = run.ref
    figures = dict(forward=ref.n_forward, backward=ref.n_backward, kept=ref.n_kept, scenes=int(((ref.forward + ref.backward).sum(axis=1) > 0).sum()))
    print("tripwire tallies", layout, figures)
    # the fold of the GPU's events = the restatement's totals = the rows' totals
    want = {(BASE + s, 100 + k): (int(ref.forward[s, k]), int(ref.backward[s, k]), int(ref.forward[s, k] - ref.backward[s, k]))
            for s in range(S) for k in range(16) if ref.forward[s, k] or ref.backward[s, k]}
    assert tally.counts() == want
    from_rows = {(int(r["scene"]), int(r["id"])): (int(r["forward"]), int(r["backward"]), int(r["forward"] - r["backward"])) for r in rows
                 if r["forward"] or r["backward"]}
    assert from_rows == want
    assert figures["forward"] >= 5 and figures["backward"] >= 5 and figures["kept"] >= 20, figures


# 2 ------------------------------------------------------------------------------------------------------------------------
def _planted(plants, n_scenes=S2, depth=8):
    """A context whose scene sc's track 0 is plants[sc] = [px, py, pz, vx, vy, vz] with zero covariance and lifetime 0 (one restore),
    tripwires enabled behind it.  -> (run, blob, entries)"""
    sb = settled(lambda sb, data: sb, n_scenes, long_lived=True, kf_q_std=0.0)
    blob = bytearray(sb.snapshot())
    ents = directory(blob)
    for sc, x in plants.items():
        plant_state(blob, record_at(ents, sc), x)
    sb.restore(bytes(blob))
    return TripRun(sb, depth, cut(n_scenes)), blob, ents


def test_planted_positions_band_edges_ends_u_turns_and_non_finite():
    from mmwave_msc_amd import _lib
    Fw, Bw = _lib.TW_FORWARD, _lib.TW_BACKWARD
    e = 2.0 ** -50
    door = (0.0, -4.0, 0.0, 4.0)                     # dx = 0, dy = 8, len2 = 64: u = 8 (py + 4), c = -8 px; band = 8 margin
    # scene: [x of track 0], its wires, the multipliers of the seven steps, the positions the eight samples see, (sample, kind, wire)
    cases = {
        # c == 0 with margin 0 keeps the side (samples 1, 5); c == -band / c == band exactly keep it (wire 1 at samples 2, 6), the next step flips
        0: ([-0.5, 0.0, 1.0, 0.25, 0.0, 0.0], [door + (0.0,), door + (0.25,)], [2, 1, 1, -1, -1, -1, -1],
            [(-0.5, 0.0), (0.0, 0.0), (0.25, 0.0), (0.5, 0.0), (0.25, 0.0), (0.0, 0.0), (-0.25, 0.0), (-0.5, 0.0)],
            [(2, Bw, 0), (3, Bw, 1), (6, Fw, 0), (7, Fw, 1)]),
        # a U-turn inside the band (samples 1 .. 4) gives no event; a full pass gives one (BACKWARD: positive -> negative), dithering in the band behind it none, the pass back FORWARD (scene 3: FORWARD, then BACKWARD)
        1: ([-0.5, 0.0, 1.0, 0.125, 0.0, 0.0], [door + (0.25,)], [3, 2, -2, -3, 8, -3, -5],
            [(-0.5, 0.0), (-0.125, 0.0), (0.125, 0.0), (-0.125, 0.0), (-0.5, 0.0), (0.5, 0.0), (0.125, 0.0), (-0.5, 0.0)],
            [(5, Bw, 0), (7, Fw, 0)]),
        # u == 0 (wire 0, sample 1) and u == len2 (wire 2, sample 2) are inside: the side is known and the crossing counts; wire 1 starts
        # 2**-50 later and wire 3 ends 2**-50 earlier: there the track is outside at that sample, the side unknown, and nothing is counted
        2: ([0.0, 3.0, 1.0, 1.0, -2.0, 0.0], [(1.0, 0.0, 5.0, 0.0), (1.0 + e, 0.0, 5.0, 0.0), (-2.0, 0.0, 2.0, 0.0), (-2.0, 0.0, 2.0 - e, 0.0)],
            [1, 1, 1, 1, 1, 1, 1], [(float(k), 3.0 - 2.0 * k) for k in range(8)], [(2, Bw, 0), (2, Bw, 2)]),
        # positive (sample 0), beyond the end B (1: u = 80 > 64), back inside on the negative side (2: u == len2): through `unknown`, no event;
        # then a pass either way, and once more beyond the end and back (6, 7): no event
        3: ([-1.0, 0.0, 1.0, 1.0, 2.0, 0.0], [door + (0.0,)], [3, -1, -2, 1, 1, 1, -1],
            [(-1.0, 0.0), (2.0, 6.0), (1.0, 4.0), (-1.0, 0.0), (0.0, 2.0), (1.0, 4.0), (2.0, 6.0), (1.0, 4.0)],
            [(3, Fw, 0), (5, Bw, 0)]),
        # an infinite coordinate (sample 0), and a NaN from the first step on (inf - centroid times a zero gain): never inside, no event
        4: ([np.inf, 0.0, 1.0, 0.0, 0.0, 0.0], [door + (0.0,)], [1, 1, 1, 1, 1, 1, 1], None, []),
    }
    run, _, _ = _planted({sc: c[0] for sc, c in cases.items()})
    sb = run.sb
    run.set_wires([c[1] for c in cases.values()])
    dts = _dts([c[2] for c in cases.values()])
    uid0 = None
    seen = {sc: [] for sc in cases}
    for k in range(8):
        if k:
            run.step_empty(dts[k - 1])
        trk = sb.tracks()
        if uid0 is None:
            uid0 = [int(trk["uid"][sc, 0]) for sc in cases]
        assert [int(trk["uid"][sc, 0]) for sc in cases] == uid0
        for sc, c in cases.items():
            pos = (float(trk["x"][sc, 0, 0]), float(trk["x"][sc, 0, 1]))
            if c[3] is not None:
                assert pos == c[3][k], (sc, k, pos)
            elif k == 0:
                assert np.isinf(pos[0])
            else:
                assert np.isnan(pos[0]), (k, pos)
        run.sample(t=float(k))
        rows, events = run.compare(("planted", k))
        if k == 2:                                     # two samples without a step add nothing
            run.sample(t=2.5)
            again = run.compare(("planted", "twice"))
            assert len(again[1]) == 0 and not again[0]["d_forward"].any() and not again[0]["d_backward"].any()
            assert again[0]["forward"].tobytes() == rows["forward"].tobytes() and again[0]["backward"].tobytes() == rows["backward"].tobytes()
        for ev in events:
            sc = int(ev["scene"]) - BASE
            if ev["kind"] != _lib.TW_REBASED and int(ev["uid"]) == uid0[sc]:
                assert ev["slot"] == 0 and ev["t"] == float(k)
                seen[sc].append((k, int(ev["kind"]), int(ev["wire"])))
    for sc, c in cases.items():
        assert seen[sc] == c[4], (sc, seen[sc])
    sb.close()


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_it_is_a_log_forward_and_back_between_two_exports():
    """Export every third frame: the planted track of scene 0 crosses the far wire forward and comes back between two exports --
    both events are delivered and d_forward == d_backward == 1 (no other track comes near that wire).  A difference of states
    would show nothing."""
    from mmwave_msc_amd import _lib
    run, _, _ = _planted({0: [FAR + 0.5, 0.0, 1.0, 1.0, 0.0, 0.0]})        # c = -8 (px - 100): negative side
    sb = run.sb
    run.set_wires([[(FAR, -4.0, FAR, 4.0, 0.0, 55)]] + [[]] * (S2 - 1))
    run.sample(t=0.0)
    rows, events = run.compare("first")
    assert [int(e["kind"]) for e in events] == [_lib.TW_REBASED] and rows["forward"].tolist() == [0]
    t = 0.0
    for trio, (steps, end, totals) in enumerate((((-1, 1, 1), FAR + 1.5, (1, 1)), ((-2, 2, -1), FAR + 0.5, (2, 2)))):
        for L in steps:                                # px: 99.5 (FORWARD), back beyond the wire (BACKWARD), and one step more
            run.step_empty(_one_dt(run, L))
            t += 1.0
            run.sample(t=t)
        assert [float(v) for v in sb.tracks()["x"][0, 0, :2]] == [end, 0.0]
        rows, events = run.compare(("every third frame", trio))
        assert (events["scene"] == BASE).all()
        assert [(int(e["kind"]), int(e["id"]), int(e["slot"]), float(e["t"])) for e in events] == [(_lib.TW_FORWARD, 55, 0, t - 2.0), (_lib.TW_BACKWARD, 55, 0, t - 1.0)]
        assert (int(rows["forward"][0]), int(rows["backward"][0])) == totals
        assert (int(rows["d_forward"][0]), int(rows["d_backward"][0]), int(rows["lost"][0])) == (1, 1, 0)
    sb.close()


def _one_dt(run, L):
    """The dt that makes the next step's multiplier L in every scene (the run keeps the running sum)."""
    prev = getattr(run, "_L", 0.0)
    run._L = float(L)
    return np.full(run.sb.S, float(L) - prev)


@pytest.mark.parametrize("depth", [1, 2])
def test_log_depth_1_and_2_three_wires_crossed_in_one_step(depth):
    """One track crosses three parallel wires in ONE step: only the newest `depth` events are written, `lost` says how many were
    not, and the counters still say 3."""
    from mmwave_msc_amd import _lib
    run, _, _ = _planted({0: [FAR - 0.5, 0.0, 1.0, 3.0, 0.0, 0.0]}, depth=depth)
    sb = run.sb
    run.set_wires([[(FAR + k, -4.0, FAR + k, 4.0, 0.0, 60 + k) for k in range(3)]] + [[]] * (S2 - 1))
    run.sample(t=0.0)
    rows, events = run.compare("first")
    assert [int(e["kind"]) for e in events] == [_lib.TW_REBASED] and not rows["lost"].any()
    run.step_empty(_one_dt(run, 1))
    assert float(sb.tracks()["x"][0, 0, 0]) == FAR + 2.5
    run.sample(t=1.0)
    rows, events = run.compare("three in one step")
    assert rows["backward"].tolist() == [1, 1, 1] and rows["d_backward"].tolist() == [1, 1, 1] and not rows["forward"].any()
    assert rows["lost"].tolist() == [3 - depth] * 3
    assert [(int(e["kind"]), int(e["wire"]), int(e["id"])) for e in events] == [(_lib.TW_BACKWARD, k, 60 + k) for k in range(3 - depth, 3)]
    run.sample(t=2.0)
    rows, events = run.compare("nothing new")
    assert len(events) == 0 and not rows["lost"].any() and rows["backward"].tolist() == [1, 1, 1] and not rows["d_backward"].any()
    sb.close()


def test_depth_log_max_the_refused_depths_and_enabling_again():
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import MmwError
    data = cut(2)
    sb = make_checked(2, N, "per_scene", **CFG_KW)
    b = sb.alloc(64)
    entries = (lambda: sb.sample_tripwires(), lambda: sb.tripwires_async(b.ptr, 1, b.ptr, 1), lambda: sb.tripwires_wait(0), lambda: sb.tripwires_host(),
               lambda: sb.set_tripwires(wires16(2)))

    def all_refused():
        for entry in entries:
            with pytest.raises(MmwError) as ei:
                entry()
            assert ei.value.code == _lib.E_ARG
        assert not sb.tripwires()[0].any() and sb.tripwires()[1].tobytes() == bytes(2 * 16 * 48)   # (mmw_get_tripwires: 0 wires)
    all_refused()                                  # before enabling
    run = TripRun(sb, _lib.TRIPWIRE_LOG_MAX, data)
    run.set_wires(wires16(2))
    for f in range(F):
        run.step(f)
        run.sample(t=0.125 * f)
        if f % 4 == 3:
            run.compare(("depth 4096", f))
        if f == 5:
            for bad in (_lib.TRIPWIRE_LOG_MAX + 1, -1):
                with pytest.raises(MmwError) as ei:
                    sb.enable_tripwires(bad)
                assert ei.value.code == _lib.E_ARG     # ... and the earlier enablement goes on working (the frames that follow)
    assert run.ref.logged.sum() >= 2
    # enabling again starts over: no wires, no counts, an empty log
    sb.enable_tripwires(3)
    run.ref = TripRef(2, sb.track_cap, 3)
    assert not sb.tripwires()[0].any()
    rows, events = run.compare("enabled again")
    assert len(rows) == 0 and len(events) == 0
    run.set_wires(wires16(2))
    run.sample()
    rows, events = run.compare("enabled again, sampled")
    assert len(rows) == 32 and [int(e["kind"]) for e in events] == [_lib.TW_REBASED] * 2 and not events["t"].any()
    sb.enable_tripwires(0)
    all_refused()
    sb.enable_tripwires(0)      # (off already: MMW_OK)
    step(sb, 0, data)          # the context steps on, and resets launch nothing of the tripwires
    sb.reset()
    b.free()
    sb.close()


# 4 ------------------------------------------------------------------------------------------------------------------------
def _settled(n_scenes=S2, frames=8, depth=64):
    def make(sb, data):
        run = TripRun(sb, depth, data)
        run.set_wires(wires16(n_scenes))
        return run
    return settled(make, n_scenes, frames, each_frame=lambda run, f: run.sample(t=0.25 * f))


def test_capacity_is_decided_on_the_device_and_a_refused_export_takes_nothing():
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import MmwError
    run = _settled()
    sb = run.sb
    want_r, want_e = run.ref.peek()
    n_r, n_e = len(want_r), len(want_e)
    assert n_r == 16 * S2 and n_e > S2, (n_r, n_e)       # (a REBASED per scene and some crossings)
    sent_r, sent_e = np.full(n_r * 32 + 64, 0xA5, np.uint8), np.full(n_e * 32 + 64, 0x5A, np.uint8)
    b_r, b_e = sb.alloc(sent_r.nbytes).upload(sent_r), sb.alloc(sent_e.nbytes).upload(sent_e)
    for t, (cap_r, cap_e) in enumerate(((n_r, n_e - 1), (n_r - 1, n_e), (0, 0))):
        sb.tripwires_async(b_r.ptr if cap_r else None, cap_r, b_e.ptr if cap_e else None, cap_e, 0, t)
        with pytest.raises(MmwError) as ei:
            sb.tripwires_wait(t)
        assert ei.value.code == _lib.E_CAPACITY and ei.value.needed == (n_r, n_e), (t, ei.value.needed)
        assert np.array_equal(b_r.download(sent_r.shape, np.uint8), sent_r) and np.array_equal(b_e.download(sent_e.shape, np.uint8), sent_e)
    # `taken` and the marks stand: the retry returns what the first call would have, and nothing is written past the counts
    sb.tripwires_async(b_r.ptr, n_r, b_e.ptr, n_e, 0, 0)
    assert sb.tripwires_wait(0) == (n_r, n_e)
    same_pair((b_r.download((n_r,), _lib.TRIPWIRE_ROW_DTYPE), b_e.download((n_e,), _lib.TRIPWIRE_EVENT_DTYPE)), run.ref.export(), "exact caps")
    assert (want_r["d_forward"] + want_r["d_backward"]).sum() > 0
    assert np.array_equal(b_r.download(sent_r.shape, np.uint8)[n_r * 32:], sent_r[n_r * 32:])
    assert np.array_equal(b_e.download(sent_e.shape, np.uint8)[n_e * 32:], sent_e[n_e * 32:])
    rows, events = run.compare("after the export")        # taken = logged, the marks are the totals
    assert len(events) == 0 and not rows["d_forward"].any() and not rows["d_backward"].any()
    assert rows["forward"].tobytes() == want_r["forward"].tobytes()
    for b in (b_r, b_e):
        b.free()
    sb.close()


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_reset_restore_and_set_tripwires_rebase_their_scenes_only():
    from mmwave_msc_amd import _lib
    S4, reset, restored, rewired = 8, (1, 5), (2, 6), (3,)
    sb = make_checked(S4, N, "per_scene", **CFG_KW)
    run = TripRun(sb, 64, cut(S4))
    run.set_wires(wires16(S4))
    blob = None
    for f in range(7):
        run.step(f)
        run.sample(t=0.5 * f)
        rows, _ = run.compare(f)
        if f == 3:
            blob = sb.snapshot(list(restored))
    before = rows
    assert (before["forward"] + before["backward"]).sum() > 0
    sb.reset_scenes(np.isin(np.arange(S4), reset))
    sb.restore(blob, scenes=list(restored))
    run.ref.rebase(reset + restored)
    nw, wt = wires16(1, margin=0.125)
    run.set_wires((nw, wt), scenes=list(rewired))
    rows, events = run.compare("before the next sample")     # nothing is logged until a sample asks the scene; scene 3's counters restarted
    assert len(events) == 0
    hit = np.isin(rows["scene"] - BASE, rewired)
    assert not rows["forward"][hit].any() and not rows["backward"][hit].any()
    assert rows["forward"][~hit].tobytes() == before["forward"][~hit].tobytes() and rows["backward"][~hit].tobytes() == before["backward"][~hit].tobytes()
    run.step(7)
    run.sample(t=3.5)
    rows, events = run.compare("after")
    touched = reset + restored + rewired
    reb = events[events["kind"] == _lib.TW_REBASED]
    assert sorted((reb["scene"] - BASE).tolist()) == sorted(touched) and (reb["t"] == 3.5).all()
    for sc in touched:                                         # ... at its place in the log: the first of the scene's events of this sample
        mine = events[events["scene"] == BASE + sc]
        assert mine["kind"][0] == _lib.TW_REBASED and (mine["kind"][1:] != _lib.TW_REBASED).all()
        assert (mine["uid"][0], mine["wire"][0], mine["id"][0], mine["slot"][0]) == (-1, -1, -1, int(sb.num_tracks()[sc]))
    keep = ~np.isin(rows["scene"] - BASE, rewired)
    assert (rows["forward"][keep] >= before["forward"][keep]).all() and (rows["backward"][keep] >= before["backward"][keep]).all()
    # mmw_reset: every scene
    sb.reset()
    run.ref.rebase()
    run.step(0)
    run.sample(t=4.0)
    rows, events = run.compare("after reset")
    assert n_kind(events, _lib.TW_REBASED) == S4
    sb.close()


def test_a_uid_restored_on_the_other_side_gives_no_crossing():
    """The planted track of scene 0 stands on the negative side of the far wire; the scene is reset and restored with the same uid
    number on the positive side: a REBASED, no FORWARD, counters at 0.  (Without the rebase this is a crossing.)"""
    from mmwave_msc_amd import _lib
    run, blob, ents = _planted({0: [FAR + 0.5, 0.0, 1.0, 0.0, 0.0, 0.0]})
    sb = run.sb
    run.set_wires([[(FAR, -4.0, FAR, 4.0, 0.0, 9)]] + [[]] * (S2 - 1))
    run.sample(t=0.0)
    run.compare("negative side")
    uid = int(sb.tracks()["uid"][0, 0])
    assert run.ref.sides[0][uid][0] == 1                      # (the restatement's: negative)
    plant_state(blob, record_at(ents, 0), [FAR - 0.5, 0.0, 1.0, 0.0, 0.0, 0.0])
    sb.reset_scenes(np.arange(S2) == 0)
    sb.restore(bytes(blob))                                    # (every scene of the blob: scene 0's track 0 on the other side)
    run.ref.rebase()
    assert int(sb.tracks()["uid"][0, 0]) == uid and float(sb.tracks()["x"][0, 0, 0]) == FAR - 0.5
    run.sample(t=1.0)
    rows, events = run.compare("positive side")
    assert [int(e["kind"]) for e in events] == [_lib.TW_REBASED] and not rows["forward"].any() and not rows["backward"].any()
    assert run.ref.sides[0][uid][0] == 2
    sb.close()


# 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["track_cap_40", "track_cap_64"])
def test_many_tracks_and_all_16_wires(shape):
    """The track_cap = 40 grid scenes of the skeleton tests, and the report's track_cap = 64 scene with 36 targets (lanes and uid
    slots past 32: the upper half of the 64-bit ballots); 16 long wires across the grid."""
    from tests._grid_scenes import many_tracks
    sb, pts, n_s, n_pts, frames, floor = many_tracks(shape)
    run = TripRun(sb, 256)
    run.set_wires(wires16(n_s, margin=0.01, y0=40.0, y1=-40.0, x0=-6.0, pitch=0.75))
    most = 0
    for f in range(frames):
        sb.step_host(pts[f].astype(np.float64), np.full(n_s, n_pts, np.int32), np.full(n_s, 0.1))
        run.sample(t=0.1 * f)
        rows, events = run.compare(f)
        most = max(most, int(sb.num_tracks().max()))
    known = sum(1 for s in range(n_s) for side in run.ref.sides[s].values() if any(side))
    print("many tracks", shape, "most", most, "uids with a known side", known, "crossings", run.ref.n_forward, run.ref.n_backward)
    assert most > floor and known > floor, (most, known)
    assert len(rows) == 16 * n_s
    sb.check()
    sb.close()


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_1027_scenes_the_scan_loop_a_short_last_block_and_scenes_without_wires():
    """More than 1024 scenes: two scenes per thread of the scan workgroup; 1027 = 256 blocks of four waves and one of three.  Every
    fourth scene has no wire: no row, no event."""
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    Sn, Nn, Fn = 1027, 32, 5
    pts, cnt, dts = coming_and_going(Sn, Nn, Fn)
    sb = SceneBatch(_lib.default_config(**CFG_KW), Sn, Nn)
    run = TripRun(sb, 16, (pts, cnt, dts))
    with_wires = [s for s in range(Sn) if s % 4 != 3]
    run.set_wires(wires16(len(with_wires)), scenes=with_wires)
    for f in range(Fn):
        run.step(f)
        if f == 3:
            sb.reset_scenes(np.isin(np.arange(Sn) % 64, (1, 3)))    # scenes without a wire among them: nothing at all
            run.ref.rebase([s for s in range(Sn) if s % 64 in (1, 3)])
        run.sample(t=0.5 * f)
        rows, events = run.compare(f)
        assert len(rows) == 16 * len(with_wires) and set((rows["scene"] - BASE).tolist()) == set(with_wires)
        assert not np.isin((events["scene"] - BASE) % 4, (3,)).any()
        if f == 0:
            assert n_kind(events, _lib.TW_REBASED) == len(with_wires)
        if f == 3:
            assert n_kind(events, _lib.TW_REBASED) == len([s for s in with_wires if s % 64 == 1])
    print("1027 scenes: forward, backward, kept", run.ref.n_forward, run.ref.n_backward, run.ref.n_kept)
    assert run.ref.n_forward + run.ref.n_backward > 0
    assert (run.ref.logged[Sn - 3:] > 0).any(), "the last, short block logged something"
    sb.close()


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_two_tickets_around_a_step():
    from mmwave_msc_amd import _lib
    frames = 8
    ra, rb = _settled(frames=frames - 2), _settled(frames=frames - 2)
    a, b = ra.sb, rb.sb
    pts, cnt, dts = ra.data
    for run in (ra, rb):                        # (nothing was exported yet: the first ticket takes the log of the frames so far)
        run.step(frames - 2)
        run.sample(t=10.0)
    want0 = rb.compare("first", scene_base=0)
    rb.step(frames - 1)
    rb.sample(t=11.0)
    want1 = rb.compare("second", scene_base=0)
    print("two tickets: events", len(want0[1]), len(want1[1]))
    cap_r, cap_e = 16 * S2, 64 * S2
    d_pts = a.alloc(pts[frames - 1].size * 8).upload(pts[frames - 1].astype(np.float64))
    d_cnt, d_dt = a.alloc(S2 * 4).upload(cnt[frames - 1]), a.alloc(S2 * 8).upload(dts[frames - 1])
    d_t = a.alloc(S2 * 8).upload(np.full(S2, 11.0))
    r0, e0, r1, e1 = a.alloc(cap_r * 32), a.alloc(cap_e * 32), a.alloc(cap_r * 32), a.alloc(cap_e * 32)
    a.synchronize()
    a.tripwires_async(r0.ptr, cap_r, e0.ptr, cap_e, 0, 0)
    a.step_dev(d_pts.ptr, d_cnt.ptr, d_dt.ptr)
    a.sample_tripwires_dev(None, d_t.ptr)
    a.tripwires_async(r1.ptr, cap_r, e1.ptr, cap_e, 0, 1)
    assert a.tripwires_wait(1) == (len(want1[0]), len(want1[1]))
    assert a.tripwires_wait(0) == (len(want0[0]), len(want0[1]))
    for (rbuf, ebuf), (wr, we) in (((r0, e0), want0), ((r1, e1), want1)):
        assert rbuf.download((len(wr),), _lib.TRIPWIRE_ROW_DTYPE).tobytes() == wr.tobytes()
        assert ebuf.download((len(we),), _lib.TRIPWIRE_EVENT_DTYPE).tobytes() == we.tobytes()
    # the second delivered only what the first had not taken: its events are all of the second sample
    assert len(want0[1]) >= S2 and (want0[1]["t"] <= 10.0).all() and (want1[1]["t"] == 11.0).all()
    with pytest.raises(_lib.MmwError) as ei:
        a.tripwires_wait(0)
    assert ei.value.code == _lib.E_ARG
    a.check()
    for buf in (d_pts, d_cnt, d_dt, d_t, r0, e0, r1, e1):
        buf.free()
    a.close(); b.close()


# 9 ------------------------------------------------------------------------------------------------------------------------
def _refusals(n_scenes):
    """(scenes, n, n_wires, wires) argument sets mmw_set_tripwires must refuse; None = a NULL pointer."""
    from mmwave_msc_amd import _lib
    ok = (-1.0, 8.0, -1.0, 0.0, 0.1, 5)

    def one(**fields):
        nw, wt = _lib.make_tripwires([[ok, ok]])
        for fld, v in fields.items():
            wt[0, 1][fld] = v
        return None, 1, nw, wt
    two = _lib.make_tripwires([[ok], [ok]])
    many = _lib.make_tripwires([[ok]] * (n_scenes + 1))
    single = _lib.make_tripwires([[ok]])
    return {
        "index out of range": (np.array([0, n_scenes], np.int32), 2) + two,
        "negative index": (np.array([-1, 0], np.int32), 2) + two,
        "listed twice": (np.array([1, 1], np.int32), 2) + two,
        "n < 0": (None, -1) + two,
        "n > n_scenes": (None, n_scenes + 1) + many,
        "NULL n_wires": (None, 1, None, single[1]),
        "NULL wires": (None, 1, single[0], None),
        "n_wires 17": (None, 1, np.array([17], np.int32), single[1]),
        "n_wires -1": (None, 1, np.array([-1], np.int32), single[1]),
        "reserved_": one(reserved_=1),
        "NaN ax": one(ax=np.nan), "infinite by": one(by=np.inf), "infinite bx": one(bx=-np.inf), "NaN ay": one(ay=np.nan),
        "negative margin": one(margin=-0.01), "infinite margin": one(margin=np.inf), "NaN margin": one(margin=np.nan),
        "A == B": one(bx=-1.0, by=8.0),
        "len2 overflows": one(ay=1e200, by=-1e200),
        "len2 underflows to zero": one(ay=0.0, by=1e-200),
        "band overflows": one(margin=1e308),
        "band underflows to zero": one(margin=5e-324, ay=0.0, by=0.25),
    }


def test_refused_arguments_touch_nothing():
    from mmwave_msc_amd import _lib
    run = _settled(frames=4)
    sb = run.sb
    buf = sb.alloc(4096)
    L = sb.L

    def set_raw(scenes, n, nw, wt):
        return L.mmw_set_tripwires(sb.h, None if scenes is None else scenes.ctypes.data, n, None if nw is None else nw.ctypes.data,
                                   None if wt is None else wt.ctypes.data)
    run.step(4)
    run.sample(t=9.0)                                 # nothing was exported yet: the log and the counters hold something when the refusals come
    before = sb.tripwires()
    for name, args in _refusals(S2).items():
        assert set_raw(*args) == _lib.E_ARG, name
        assert "mmw_set_tripwires" in _lib.last_error(sb.h), name
        after = sb.tripwires()
        assert np.array_equal(after[0], before[0]) and after[1].tobytes() == before[1].tobytes(), name
    msg = set_raw(*_refusals(S2)["A == B"]), _lib.last_error(sb.h)
    assert "entry 0" in msg[1] and "wire 1" in msg[1], msg
    # a margin of 0 and entries past n_wires that would be refused are accepted -- and undone again below
    nw_ok, wt_ok = _lib.make_tripwires([[(0.0, 0.0, 0.0, 1.0)]])
    wt_ok[0, 1]["ax"], wt_ok[0, 1]["reserved_"] = np.nan, 9     # past n_wires: not read
    assert set_raw(None, 1, nw_ok, wt_ok) == 0
    assert sb.tripwires()[0][0] == 1 and sb.tripwires()[1][0, 1:].tobytes() == bytes(15 * 48)
    run.ref.set_wires([0], nw_ok, wt_ok)
    nw, wt = wires16(1)
    run.set_wires((nw, wt), scenes=[0])
    # refused sample and export arguments: nothing queued, no ticket left behind, nothing taken
    sent = np.full(4096, 0x3C, np.uint8)
    buf.upload(sent)
    for bad in (lambda: sb.tripwires_async(buf.ptr, -1, buf.ptr, 1), lambda: sb.tripwires_async(buf.ptr, 1, buf.ptr, -1),
                lambda: sb.tripwires_async(None, 1, buf.ptr, 1), lambda: sb.tripwires_async(buf.ptr, 1, None, 1),
                lambda: sb.tripwires_async(buf.ptr + 4, 1, buf.ptr, 1), lambda: sb.tripwires_async(buf.ptr, 1, buf.ptr + 4, 1),
                lambda: sb.tripwires_async(buf.ptr, 1, buf.ptr, 1, 0, 4), lambda: sb.tripwires_async(buf.ptr, 1, buf.ptr, 1, 0, -1),
                lambda: sb.tripwires_wait(4), lambda: sb.tripwires_wait(-1), lambda: sb.tripwires_wait(0),
                lambda: sb.sample_tripwires_dev(buf.ptr + 2, None), lambda: sb.sample_tripwires_dev(None, buf.ptr + 4),
                lambda: sb.enable_tripwires(-1), lambda: sb.enable_tripwires(_lib.TRIPWIRE_LOG_MAX + 1)):
        with pytest.raises(_lib.MmwError) as ei:
            bad()
        assert ei.value.code == _lib.E_ARG
    for t in range(4):
        with pytest.raises(_lib.MmwError):
            sb.tripwires_wait(t)
    sb.synchronize()
    assert np.array_equal(buf.download(sent.shape, np.uint8), sent)
    # wire table, counters and log are what the restatement says they are: the events of sample 9.0 are still to be had
    rows, events = run.compare("after the refusals")
    assert len(events) >= S2 and (events["t"] == 0.0).sum() >= S2      # (the REBASED of the first sample among them)
    run.step(5)
    run.sample(t=10.0)
    run.compare("one more frame")
    buf.free()
    sb.check()
    sb.close()


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_nothing_else_moves():
    """A context that enables, sets, samples and exports tripwires ends the run with the snapshot bytes, report, zones and trails of
    one that never did, and both launched the same step kernels the same number of times (mmw_profile_get)."""
    from mmwave_msc_amd import _lib
    a = make_checked(S2, N, "per_scene", **CFG_KW)
    b = make_checked(S2, N, "per_scene", **CFG_KW)
    data = cut(S2)
    for sb in (a, b):
        sb.profile(True)
        sb.enable_report()
        sb.set_zones(strips(S2))
        sb.enable_trails(4)
    run = TripRun(a, 64, data)
    run.set_wires(wires16(S2))
    n_events = []

    def drive(f):
        run.sample(t=0.25 * f)
        n_events.append(len(run.compare(f)[1]))
        if f == 4:
            for sb in (a, b):
                sb.reset_scenes(np.arange(S2) == 1)
            run.ref.rebase([1])

    nothing_else_moves(a, b, data, 8, drive, both=lambda sb, f: sb.sample_trails(t=0.25 * f),
                       each_frame=TRACKS + REPORT + (lambda sb: sb.zones_host(), lambda sb: sb.trails_host()), at_end=(lambda sb: sb.snapshot(),))
    assert sum(n_events) > S2
    counts = [(a.profile_get(k)[1], b.profile_get(k)[1]) for k in range(_lib.K_COUNT)]
    print("kernel launches (with tripwires, without)", counts)
    assert all(x == y for x, y in counts) and sum(y for _, y in counts) > 0, counts
    a.check(); b.check()
    a.close(); b.close()


# 11 -----------------------------------------------------------------------------------------------------------------------
def test_trails_and_tripwires_keep_separate_slot_tables():
    """Both samplers run the one slot code (UidSlots, csrc/mmw_uidlist.hpp), each on a table of its own; a mix-up of the two shows
    only when both are enabled and the tables differ.  The report scenario cut to 6 scenes, trails of depth 4 beside 16 wires a
    scene and a log of 64: tripwires are sampled in every scene after every frame, trails in every scene after the even frames and
    in the even scenes only after the odd ones, and scene 1 is reset in front of frame 6.  Both exports are compared after every
    frame as tests/test_gpu_trails.py and this file compare them.  Driven from the C oracle on the same cut (identities by
    continuity), the restatements see 6 trail slots reused, 8 forward and 2 backward crossings, and 6 scene-frames after which the
    two consumers hold different uid sets; the run counts as not vacuous with one of each."""
    from mmwave_msc_amd import _lib
    Sn = 6
    data = cut(Sn)
    sb = make_checked(Sn, N, "per_scene", **CFG_KW)
    trails = TrailRun(sb, 4, data)
    wires = TripRun(sb, 64, data)
    wires.set_wires(wires16(Sn))
    even = [s for s in range(Sn) if s % 2 == 0]
    n_crossings = n_differ = 0
    for f in range(F):
        if f == 6:
            sb.reset_scenes(np.arange(Sn) == 1)
            trails.ref.rebase([1])
            wires.ref.rebase([1])
        wires.step(f)
        clock = np.full(Sn, 0.25 * f)
        trails.sample(t=clock, scenes=even if f % 2 else None)
        wires.sample(t=clock)
        trails.compare(("trails", f))
        _, events = wires.compare(("tripwires", f))
        n_crossings += n_kind(events, _lib.TW_FORWARD) + n_kind(events, _lib.TW_BACKWARD)
        n_differ += sum(set(trails.ref.trails[s]) != set(wires.ref.sides[s]) for s in range(Sn))
    sb.check()
    sb.close()
    figures = dict(reused=trails.ref.reused, crossings=n_crossings, differ=n_differ)
    print("two slot tables", figures, "travelled bit-equal", trails.equal, "of", trails.seen)
    assert n_crossings == wires.ref.n_forward + wires.ref.n_backward
    assert figures["reused"] >= 1 and figures["crossings"] >= 1 and figures["differ"] >= 1, figures
