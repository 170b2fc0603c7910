"""Zone occupancy (mmw_set_zones / mmw_zones_*, include/mmw.h) on the GPU: per defined zone a row of counts, and every change of a
track's zone membership since the previous export as an event with the track's uid.

Expected values come from tests/_zone_ref.py, a numpy restatement of the header's rules applied to the state read back with
`tracks()` / `num_tracks()` after each step; it carries its own baseline.  Everything is integers: rows and events are compared
exactly, field by field.  The scenario is tests/_report_scenes.py's (24 scenes x 96 points x 12 frames: tracks are born, walk and
expire inside the run)."""
import numpy as np
import pytest

from tests._feature_run import BASE, REPORT, S2, TRACKS, cut, export_and_compare, n_kind, nothing_else_moves, same_records, settled, step
from tests._layouts import make_checked
from tests._report_scenes import CFG_KW, F, N, S, coming_and_going, strips
from tests._snap_plant import REC_X, directory, plant_word, record_at
from tests._zone_ref import ZoneRef

pytestmark = pytest.mark.gpu


def _roster_equals(roster, ref, scene_base=BASE):
    want = {(s + scene_base, z): frozenset(u) for (s, z), u in ref.membership().items()}
    assert roster.occupied() == want, (roster.occupied(), want)


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["per_scene", "one_workgroup"])
def test_strips_rows_and_events_after_every_step(layout):
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.zones import Roster
    sb = make_checked(S, N, layout, **CFG_KW)
    assert not sb.has_zones
    nz, zt = strips(S)
    sb.set_zones((nz, zt))
    assert sb.has_zones
    got_n, got_z = sb.zones()
    assert np.array_equal(got_n, nz) and got_z.tobytes() == zt.tobytes()
    ref, roster = ZoneRef(S), Roster()
    ref.set_zones(nz, zt)
    tally = dict(enter_live=0, leave_live=0, enter_newborn=0, leave_expired=0, track_frames=0)
    for f in range(F):
        step(sb, f)
        before = [{u for u, _ in b} for b in ref.base]
        rows, events = export_and_compare(sb, ref, f)
        roster.apply(events)
        _roster_equals(roster, ref)
        now = [{u for u, _ in b} for b in ref.base]
        # what the run holds, from the uids read back (the reference side: `events` equals the restatement's)
        for e in events:
            s, u = int(e["scene"]) - BASE, int(e["uid"])
            if e["kind"] == _lib.ZEV_ENTER:
                tally["enter_live" if u in before[s] else "enter_newborn"] += 1
            elif e["kind"] == _lib.ZEV_LEAVE:
                tally["leave_live" if u in now[s] else "leave_expired"] += 1
        tally["track_frames"] += int(sb.num_tracks().sum())
        assert n_kind(events, _lib.ZEV_REBASED) == (S if f == 0 else 0), f   # (mmw_set_zones listed every scene)
        assert len(rows) == 16 * S and int(rows["count"].sum()) == sum(len(v) for v in roster.occupied().values())
    sb.check()
    sb.close()
    tally["held_by_margin"] = ref.held
    print("zone tallies", layout, tally)
    assert tally["enter_live"] >= 20 and tally["leave_live"] >= 8 and tally["held_by_margin"] >= 8, tally
    assert tally["enter_newborn"] >= 30 and tally["leave_expired"] >= 20, tally


# 2 ------------------------------------------------------------------------------------------------------------------------
def _record_positions():
    """Pass 1: the first five scenes without zones; per frame (uid[S2][T], x[S2][T][2], num_tracks)."""
    sb = make_checked(S2, N, "per_scene", **CFG_KW)
    data, rec = cut(S2), []
    for f in range(F):
        step(sb, f, data)
        trk, ntr = sb.tracks(), sb.num_tracks()
        rec.append((trk["uid"].copy(), trk["x"][:, :, :2].copy(), ntr.copy()))
    sb.close()
    return rec


def _margin_candidates(rec, margin):
    """(scene, uid, axis, f0, f, bound_leaves, bound_holds): a track whose coordinate at frame f lies more than `margin` above the one at
    f0, with an upper bound b for which fl(b + margin) == p(f) exactly, and one for which it is one ulp above."""
    out = []
    for s in range(S2):
        for f in range(1, F):
            uid_f, x_f, n_f = rec[f]
            for j in range(int(n_f[s])):
                for f0 in range(f):
                    uid_0, x_0, n_0 = rec[f0]
                    hit = [i for i in range(int(n_0[s])) if uid_0[s, i] == uid_f[s, j]]
                    if not hit:
                        continue
                    for a in (0, 1):
                        p, p0 = np.float64(x_f[s, j, a]), np.float64(x_0[s, hit[0], a])
                        if not (np.isfinite(p) and np.isfinite(p0)):
                            continue
                        up = np.nextafter(p, np.inf)
                        leaves = [b for b in (p - margin, np.nextafter(p - margin, np.inf), np.nextafter(p - margin, -np.inf)) if b + margin == p]
                        holds = [b for b in (up - margin, np.nextafter(up - margin, np.inf), np.nextafter(up - margin, -np.inf)) if b + margin == up]
                        if leaves and holds and p0 < leaves[0] and p0 < holds[0]:
                            out.append((s, int(uid_f[s, j]), a, f0, f, leaves[0], holds[0]))
    return out


def test_exact_bounds_margin_identity_and_non_finite_positions():
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.zones import Roster
    E, L, R = _lib.ZEV_ENTER, _lib.ZEV_LEAVE, _lib.ZEV_REBASED
    margin = 0.25
    rec = _record_positions()
    cands = _margin_candidates(rec, margin)
    print("margin candidates", len(cands), cands[:4])
    assert cands, "no track of the five scenes moves more than the margin along an axis between two frames it is live in"
    s, uid, a, f0, f, b_leaves, b_holds = cands[0]
    uid_f, x_f, n_f = rec[f]
    j = [i for i in range(int(n_f[s])) if uid_f[s, i] == uid][0]
    px, py = np.float64(x_f[s, j, 0]), np.float64(x_f[s, j, 1])
    p = (px, py)[a]
    # the identities the expectations below rest on
    assert np.float64(b_leaves) + np.float64(margin) == p and np.float64(b_holds) + np.float64(margin) == np.nextafter(p, np.inf)
    inf = np.inf

    def upper(b, mg):   # a zone bounded from above at b along axis a only
        return (-inf, b, -inf, inf, mg) if a == 0 else (-inf, inf, -inf, b, mg)
    zones = [(px, inf, -inf, inf, 0.0, 50),          # 0: px == x0 -> in
             (-inf, px, -inf, inf, 0.0, 51),         # 1: px == x1 -> out
             (-inf, inf, py, inf, 0.0, 52),          # 2: py == y0 -> in
             (-inf, inf, -inf, py, 0.0, 53),         # 3: py == y1 -> out
             upper(b_leaves, margin) + (54,),        # 4: member since f0, fl(bound + margin) == p -> leaves
             upper(b_holds, margin) + (55,)]         # 5: member since f0, fl(bound + margin) one ulp above p -> held
    sb = make_checked(S2, N, "per_scene", **CFG_KW)
    nz, zt = _lib.make_zones([zones])
    sb.set_zones((nz, zt), scenes=[s])
    ref, roster = ZoneRef(S2), Roster()
    ref.set_zones(nz, zt, scenes=[s])
    data = cut(S2)
    got = {}
    for k in range(f + 1):
        step(sb, k, data)
        if k in (f0, f):
            trk = sb.tracks()
            assert trk["uid"].tobytes() == rec[k][0].tobytes() and trk["x"][:, :, :2].tobytes() == rec[k][1].tobytes(), "the two passes differ"
            got[k] = export_and_compare(sb, ref, k)
            roster.apply(got[k][1])
    ev0 = [(int(e["uid"]), int(e["kind"]), int(e["zone"])) for e in got[f0][1] if e["scene"] == s + BASE]
    ev1 = [(int(e["uid"]), int(e["kind"]), int(e["zone"])) for e in got[f][1] if e["scene"] == s + BASE]
    assert (uid, E, 4) in ev0 and (uid, E, 5) in ev0, ev0
    assert (uid, L, 4) in ev1 and (uid, L, 5) not in ev1, ev1
    assert roster.zones_of(s + BASE, uid) == [0, 2, 5], roster.zones_of(s + BASE, uid)
    assert ref.held >= 1

    # NaN, +inf and -0.0 positions, planted in a snapshot blob and restored: x[0] of track t of a section (tests/_snap_plant.py: REC_X)
    ntr = sb.num_tracks()
    spots = [(sc, t) for sc in range(S2) for t in range(int(ntr[sc]))]
    assert len(spots) >= 3, ntr
    blob = bytearray(sb.snapshot())
    ents = directory(blob)
    assert len(ents) == S2
    planted = dict(zip(spots[:3], (np.nan, np.inf, -0.0)))
    for (sc, t), v in planted.items():
        plant_word(blob, record_at(ents, sc, t) + REC_X, v)
    sb.restore(bytes(blob))
    nz2, zt2 = _lib.make_zones([[(-inf, inf, -inf, inf, 0.0, 60), (0.0, inf, -inf, inf, 0.0, 61), (-inf, 0.0, -inf, inf, 0.0, 62),
                                 (-5.0, 1e300, -inf, inf, 0.5, 63)]] * S2)
    sb.set_zones((nz2, zt2))
    ref.rebase()
    ref.set_zones(nz2, zt2)
    trk = sb.tracks()
    (s_nan, t_nan), (s_inf, t_inf), (s_neg, t_neg) = spots[:3]
    assert np.isnan(trk["x"][s_nan, t_nan, 0]) and trk["x"][s_inf, t_inf, 0] == np.inf
    assert trk["x"][s_neg, t_neg, 0] == 0.0 and np.signbit(trk["x"][s_neg, t_neg, 0])
    rows, events = export_and_compare(sb, ref, "planted")
    assert n_kind(events, R) == S2 and n_kind(events, L) == 0
    assert n_kind(events, E) == len(events) - S2 > 0
    roster = Roster().apply(events)
    assert roster.zones_of(s_nan + BASE, int(trk["uid"][s_nan, t_nan])) == []          # NaN: every comparison is false
    assert roster.zones_of(s_inf + BASE, int(trk["uid"][s_inf, t_inf])) == []          # +inf < x1 is false for x1 = +inf and for a finite x1
    assert roster.zones_of(s_neg + BASE, int(trk["uid"][s_neg, t_neg])) == [0, 1, 3]   # -0.0 >= 0.0, and -0.0 < 0.0 is false
    sb.close()


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_export_every_third_frame_gives_the_net_difference():
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.zones import Roster
    sb = make_checked(S, N, "per_scene", **CFG_KW)
    nz, zt = strips(S)
    sb.set_zones((nz, zt))
    ref, roster = ZoneRef(S), Roster()
    ref.set_zones(nz, zt)
    seen_uids, event_uids = set(), set()
    for f in range(F):
        step(sb, f)
        ntr, trk = sb.num_tracks(), sb.tracks()
        seen_uids |= {(s, int(trk["uid"][s, j])) for s in range(S) for j in range(int(ntr[s]))}
        if f % 3 == 2:
            rows, events = export_and_compare(sb, ref, f)
            roster.apply(events)
            _roster_equals(roster, ref)
            event_uids |= {(int(e["scene"]) - BASE, int(e["uid"])) for e in events if e["kind"] != _lib.ZEV_REBASED}
    # a difference of states: the restatement saw nothing but the four exported states, and every event names a track of the run
    assert event_uids and event_uids <= seen_uids, (len(event_uids), len(seen_uids))
    sb.close()


# 4 ------------------------------------------------------------------------------------------------------------------------
def _settled(n_scenes=S2, frames=8):
    """A context after `frames` frames with the strips defined and nothing exported yet, and the restatement for it."""
    sb = settled(lambda sb, data: sb, n_scenes, frames)
    data = cut(n_scenes)
    nz, zt = strips(n_scenes)
    sb.set_zones((nz, zt))
    ref = ZoneRef(n_scenes)
    ref.set_zones(nz, zt)
    return sb, ref, data


def test_capacity_is_decided_on_the_device_and_a_refused_export_loses_nothing():
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import MmwError
    sb, ref, data = _settled()
    twin, _, _ = _settled()
    want_rows, want_events = ref.export(sb.tracks(), sb.num_tracks(), commit=False)
    n_rows, n_events = len(want_rows), len(want_events)
    assert n_rows == 16 * S2 and n_events > S2
    sent_r, sent_e = np.full(n_rows * 32 + 64, 0xA5, np.uint8), np.full(n_events * 24 + 64, 0x5A, np.uint8)
    b_r, b_e = sb.alloc(sent_r.nbytes).upload(sent_r), sb.alloc(sent_e.nbytes).upload(sent_e)
    for t, (cap_r, cap_e) in enumerate(((n_rows, n_events - 1), (n_rows - 1, n_events), (0, 0))):
        sb.zones_async(b_r.ptr if cap_r else None, cap_r, b_e.ptr if cap_e else None, cap_e, 0, t)
        with pytest.raises(MmwError) as ei:
            sb.zones_wait(t)
        assert ei.value.code == _lib.E_CAPACITY and ei.value.needed == (n_rows, n_events), (t, ei.value.needed)
        assert np.array_equal(b_r.download(sent_r.shape, np.uint8), sent_r) and np.array_equal(b_e.download(sent_e.shape, np.uint8), sent_e)
    # the retry returns what a twin that was never refused returns, now and after the next frame
    sb.zones_async(b_r.ptr, n_rows, b_e.ptr, n_events, 0, 0)
    assert sb.zones_wait(0) == (n_rows, n_events)
    t_rows, t_events = twin.zones_host()
    same_records(t_rows, want_rows, "twin", "rows")
    same_records(t_events, want_events, "twin", "events")
    assert b_r.download((n_rows,), _lib.ZONE_ROW_DTYPE).tobytes() == t_rows.tobytes()
    assert b_e.download((n_events,), _lib.ZONE_EVENT_DTYPE).tobytes() == t_events.tobytes()
    assert np.array_equal(b_r.download(sent_r.shape, np.uint8)[n_rows * 32:], sent_r[n_rows * 32:])      # nothing past the rows
    assert np.array_equal(b_e.download(sent_e.shape, np.uint8)[n_events * 24:], sent_e[n_events * 24:])  # ... or the events
    for c in (sb, twin):
        step(c, 8, data)
    a_rows, a_events = sb.zones_host()
    t_rows, t_events = twin.zones_host()
    assert a_rows.tobytes() == t_rows.tobytes() and a_events.tobytes() == t_events.tobytes()
    assert n_kind(a_events, _lib.ZEV_REBASED) == 0
    for b in (b_r, b_e):
        b.free()
    sb.close(); twin.close()


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_reset_restore_and_set_zones_rebase_their_scenes_only():
    from mmwave_msc_amd import _lib
    R = _lib.ZEV_REBASED
    sb = make_checked(S2, N, "per_scene", **CFG_KW)
    data = cut(S2)
    nz, zt = strips(S2)
    sb.set_zones((nz, zt))
    ref = ZoneRef(S2)
    ref.set_zones(nz, zt)

    def rebased_scenes(events):
        return sorted(int(e["scene"]) - BASE for e in events if e["kind"] == R)

    f, elsewhere = 0, 0
    for _ in range(5):
        step(sb, f, data); f += 1
        export_and_compare(sb, ref, f)
    # reset_scenes
    sb.reset_scenes(np.isin(np.arange(S2), (1, 3)))
    ref.rebase((1, 3))
    step(sb, f, data); f += 1
    _, events = export_and_compare(sb, ref, "reset_scenes")
    assert rebased_scenes(events) == [1, 3]
    elsewhere += sum(e["kind"] != R and int(e["scene"]) - BASE not in (1, 3) for e in events)
    # restore: scene 0's state into scene 2
    sb.restore(sb.snapshot([0]), scenes=[2])
    ref.rebase((2,))
    step(sb, f, data); f += 1
    _, events = export_and_compare(sb, ref, "restore")
    assert rebased_scenes(events) == [2]
    elsewhere += sum(e["kind"] != R and int(e["scene"]) - BASE != 2 for e in events)
    assert np.array_equal(sb.zones()[0], nz) and sb.zones()[1].tobytes() == zt.tobytes()    # zones belong to the slot
    # set_zones on one scene
    nz4, zt4 = _lib.make_zones([[(-1.0, 1.0, 0.0, 4.0, 0.1, 444), (-3.0, 3.0, 4.0, np.inf, 0.1, 445)]])
    sb.set_zones((nz4, zt4), scenes=[4])
    ref.set_zones(nz4, zt4, scenes=[4])
    step(sb, f, data); f += 1
    rows, events = export_and_compare(sb, ref, "set_zones")
    assert rebased_scenes(events) == [4] and len(rows) == 16 * (S2 - 1) + 2
    elsewhere += sum(e["kind"] != R and int(e["scene"]) - BASE != 4 for e in events)
    assert elsewhere > 0   # ... and ordinary events in the scenes that were not rebased
    # reset(): every scene, and the zones stay
    sb.reset()
    ref.rebase()
    rows, events = export_and_compare(sb, ref, "reset")
    assert rebased_scenes(events) == list(range(S2)) and len(events) == S2 and (events["slot"] == 0).all()
    assert len(rows) == 16 * (S2 - 1) + 2 and not rows["count"].any()
    step(sb, 0, data)
    _, events = export_and_compare(sb, ref, "after reset")
    assert rebased_scenes(events) == []
    sb.close()


# 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["track_cap_40", "track_cap_64"])
def test_many_tracks_and_all_16_overlapping_zones(shape):
    """The track_cap = 40 grid scenes of the skeleton tests (lanes past 16 in both scenes), and the report's track_cap = 64 scene with 36
    targets (lanes past 32); 16 zones that overlap, so that tracks sit in several at once."""
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.zones import Roster
    from tests._grid_scenes import many_tracks
    sb, pts, n_s, n_pts, frames, floor = many_tracks(shape)
    nz, zt = _lib.make_zones([[(-6.0 + 0.5 * k, -1.5 + 0.5 * k, 0.5 + 0.25 * k, np.inf, 0.1, 100 * s + k) for k in range(16)] for s in range(n_s)])
    sb.set_zones((nz, zt))
    ref, roster = ZoneRef(n_s), Roster()
    ref.set_zones(nz, zt)
    most = 0
    for f in range(frames):
        sb.step_host(pts[f].astype(np.float64), np.full(n_s, n_pts, np.int32), np.full(n_s, 0.1))
        rows, events = export_and_compare(sb, ref, f)
        roster.apply(events)
        most = max(most, int(sb.num_tracks().max()))
    _roster_equals(roster, ref)
    assert most > floor, most
    ntr, trk = sb.num_tracks(), sb.tracks()
    several = [len(roster.zones_of(BASE + s, int(trk["uid"][s, j]))) for s in range(n_s) for j in range(int(ntr[s]))]
    assert max(several) >= 4 and sum(v >= 2 for v in several) > floor // 2, several
    assert (rows["count"] > 0).sum() >= 16, rows["count"]
    sb.check()
    sb.close()


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_1027_scenes_the_scan_loop_a_short_last_block_and_scenes_without_zones():
    """More than 1024 scenes: two scenes per thread of the scan workgroup; 1027 = 256 blocks of four waves and one of three.  Every
    other scene has no zone: no row, and only its REBASED after a reset."""
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    Sn, Nn, Fn = 1027, 32, 5
    pts, cnt, dts = coming_and_going(Sn, Nn, Fn)
    sb = SceneBatch(_lib.default_config(**CFG_KW), Sn, Nn)
    with_zones = list(range(0, Sn, 2))
    nz, zt = strips(len(with_zones))
    sb.set_zones((nz, zt), scenes=with_zones)
    ref = ZoneRef(Sn)
    ref.set_zones(nz, zt, scenes=with_zones)
    n_enter = n_leave = 0
    for f in range(Fn):
        step(sb, f, (pts, cnt, dts))
        if f == 3:
            sb.reset_scenes(np.isin(np.arange(Sn) % 64, (1, 2)))    # scenes without a zone among them: a REBASED and nothing else
            ref.rebase([s for s in range(Sn) if s % 64 in (1, 2)])
        rows, events = export_and_compare(sb, ref, f)
        assert len(rows) == 16 * len(with_zones) and set(rows["scene"] - BASE) == set(with_zones)
        n_enter += n_kind(events, _lib.ZEV_ENTER)
        n_leave += n_kind(events, _lib.ZEV_LEAVE)
        if f == 3:
            assert n_kind(events, _lib.ZEV_REBASED) == len([s for s in range(Sn) if s % 64 in (1, 2)])
    ntr = sb.num_tracks()
    assert ntr[Sn - 1] or ntr[Sn - 2] or ntr[Sn - 3], "the last, short block holds tracks"
    assert (events["scene"] - BASE >= Sn - 3).any() or (rows["count"][rows["scene"] - BASE >= Sn - 3] > 0).any()
    print("1027 scenes: enter, leave", n_enter, n_leave)
    assert n_enter > Sn // 4 and n_leave > 0, (n_enter, n_leave)
    sb.close()


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_two_tickets_around_a_step():
    from mmwave_msc_amd import _lib
    frames = 8
    a, _, data = _settled(frames=frames - 2)
    b, _, _ = _settled(frames=frames - 2)
    pts, cnt, dts = data
    for sb in (a, b):
        assert len(sb.zones_host()[1]) > 0
        step(sb, frames - 2, data)
    want0 = b.zones_host()
    step(b, frames - 1, data)
    want1 = b.zones_host()
    print("two tickets: events", len(want0[1]), len(want1[1]))
    assert want0[0].tobytes() + want0[1].tobytes() != want1[0].tobytes() + want1[1].tobytes()   # the two exports differ: an order mix-up shows
    cap_r, cap_e = 16 * S2, 64 * S2
    d_pts = a.alloc(pts[frames - 1].size * 8).upload(pts[frames - 1].astype(np.float64))
    d_cnt, d_dt = a.alloc(S2 * 4).upload(cnt[frames - 1]), a.alloc(S2 * 8).upload(dts[frames - 1])
    r0, e0, r1, e1 = a.alloc(cap_r * 32), a.alloc(cap_e * 24), a.alloc(cap_r * 32), a.alloc(cap_e * 24)
    a.synchronize()
    a.zones_async(r0.ptr, cap_r, e0.ptr, cap_e, 0, 0)
    a.step_dev(d_pts.ptr, d_cnt.ptr, d_dt.ptr)
    a.zones_async(r1.ptr, cap_r, e1.ptr, cap_e, 0, 1)
    assert a.zones_wait(1) == (len(want1[0]), len(want1[1]))
    assert a.zones_wait(0) == (len(want0[0]), len(want0[1]))
    for (rb, eb), (wr, we) in (((r0, e0), want0), ((r1, e1), want1)):
        assert rb.download((len(wr),), _lib.ZONE_ROW_DTYPE).tobytes() == wr.tobytes()
        assert eb.download((len(we),), _lib.ZONE_EVENT_DTYPE).tobytes() == we.tobytes()
    with pytest.raises(_lib.MmwError) as ei:
        a.zones_wait(0)
    assert ei.value.code == _lib.E_ARG
    a.check()
    for buf in (d_pts, d_cnt, d_dt, r0, e0, r1, e1):
        buf.free()
    a.close(); b.close()


# 9 ------------------------------------------------------------------------------------------------------------------------
def _refusals(n_scenes):
    """(scenes, n, n_zones, zones) argument sets mmw_set_zones must refuse; None = a NULL pointer."""
    from mmwave_msc_amd import _lib
    ok = (-1.0, 1.0, 0.0, 2.0, 0.1, 5)

    def one(**fields):
        nz, zt = _lib.make_zones([[ok, ok]])
        for fld, v in fields.items():
            zt[0, 1][fld] = v
        return None, 1, nz, zt
    two = _lib.make_zones([[ok], [ok]])
    many = _lib.make_zones([[ok]] * (n_scenes + 1))
    bad_count = _lib.make_zones([[ok]])
    out = {
        "index out of range": (np.array([0, n_scenes], np.int32), 2) + two,
        "negative index": (np.array([-1, 0], np.int32), 2) + two,
        "listed twice": (np.array([1, 1], np.int32), 2) + two,
        "n < 0": (None, -1) + two,
        "n > n_scenes": (None, n_scenes + 1) + many,
        "NULL n_zones": (None, 1, None, bad_count[1]),
        "NULL zones": (None, 1, bad_count[0], None),
        "n_zones 17": (None, 1, np.array([17], np.int32), bad_count[1]),
        "n_zones -1": (None, 1, np.array([-1], np.int32), bad_count[1]),
        "NaN bound x0": one(x0=np.nan), "NaN bound y1": one(y1=np.nan),
        "x0 > x1": one(x0=1.5), "y0 > y1": one(y0=2.5),
        "negative margin": one(margin=-0.01), "infinite margin": one(margin=np.inf), "NaN margin": one(margin=np.nan),
        "reserved_": one(reserved_=1),
    }
    return out


def test_refused_arguments_touch_nothing():
    from mmwave_msc_amd import _lib
    sb = make_checked(S2, N, "per_scene", **CFG_KW)
    data = cut(S2)
    for f in range(4):
        step(sb, f, data)
    buf = sb.alloc(4096)
    L = sb.L

    def set_raw(scenes, n, nz, zt):
        return L.mmw_set_zones(sb.h, None if scenes is None else scenes.ctypes.data, n, None if nz is None else nz.ctypes.data,
                               None if zt is None else zt.ctypes.data)

    def exports_refused():
        for call in (lambda: sb.zones_async(buf.ptr, 1, buf.ptr, 1), lambda: sb.zones_wait(0), lambda: sb.zones_host()):
            with pytest.raises(_lib.MmwError) as ei:
                call()
            assert ei.value.code == _lib.E_ARG
    # before any mmw_set_zones: the exports are refused, a refused first call allocates nothing
    exports_refused()
    for name, args in _refusals(S2).items():
        assert set_raw(*args) == _lib.E_ARG, name
        assert "mmw_set_zones" in _lib.last_error(sb.h), name
        assert not sb.has_zones, name
    exports_refused()
    assert not sb.zones()[0].any() and sb.zones()[1].tobytes() == bytes(S2 * 16 * 48)
    # with a table: every refusal leaves table, baseline and generations as they were
    nz, zt = strips(S2)
    sb.set_zones((nz, zt))
    ref = ZoneRef(S2)
    ref.set_zones(nz, zt)
    export_and_compare(sb, ref, "first")
    before = sb.zones()
    for name, args in _refusals(S2).items():
        assert set_raw(*args) == _lib.E_ARG, name
        after = sb.zones()
        assert np.array_equal(after[0], before[0]) and after[1].tobytes() == before[1].tobytes(), name
    msg_entry = set_raw(*_refusals(S2)["x0 > x1"]), _lib.last_error(sb.h)
    assert "entry 0" in msg_entry[1] and "zone 1" in msg_entry[1], msg_entry
    # infinite bounds, an empty zone and entries past n_zones that would be refused are all accepted -- and undone again below
    nz_ok, zt_ok = _lib.make_zones([[(-np.inf, np.inf, -np.inf, np.inf), (1.0, 1.0, 2.0, 2.0)]])
    zt_ok[0, 2]["x0"], zt_ok[0, 2]["reserved_"] = np.nan, 9     # past n_zones: not read
    assert set_raw(None, 1, nz_ok, zt_ok) == 0
    assert sb.zones()[0][0] == 2 and sb.zones()[1][0, 2:].tobytes() == bytes(14 * 48)
    sb.set_zones((nz[:1], zt[:1]))
    ref.rebase((0,))
    # refused export arguments: nothing queued, no ticket left behind, no baseline consumed
    sent = np.full(4096, 0x3C, np.uint8)
    buf.upload(sent)
    for bad in (lambda: sb.zones_async(buf.ptr, -1, buf.ptr, 1), lambda: sb.zones_async(buf.ptr, 1, buf.ptr, -1),
                lambda: sb.zones_async(None, 1, buf.ptr, 1), lambda: sb.zones_async(buf.ptr, 1, None, 1),
                lambda: sb.zones_async(buf.ptr + 2, 1, buf.ptr, 1), lambda: sb.zones_async(buf.ptr, 1, buf.ptr + 1, 1),
                lambda: sb.zones_async(buf.ptr, 1, buf.ptr, 1, 0, 4), lambda: sb.zones_async(buf.ptr, 1, buf.ptr, 1, 0, -1),
                lambda: sb.zones_wait(4), lambda: sb.zones_wait(-1), lambda: sb.zones_wait(0)):
        with pytest.raises(_lib.MmwError) as ei:
            bad()
        assert ei.value.code == _lib.E_ARG
    for t in range(4):
        with pytest.raises(_lib.MmwError):
            sb.zones_wait(t)
    sb.synchronize()
    assert np.array_equal(buf.download(sent.shape, np.uint8), sent)
    step(sb, 4, data)
    export_and_compare(sb, ref, "after the refusals")
    # mmw_clear_zones: as before the first mmw_set_zones; a new table starts from an empty baseline
    sb.clear_zones()
    assert not sb.has_zones and not sb.zones()[0].any()
    exports_refused()
    sb.clear_zones()
    sb.set_zones((nz, zt))
    ref = ZoneRef(S2)
    ref.set_zones(nz, zt)
    export_and_compare(sb, ref, "after clear")
    buf.free()
    sb.check()
    sb.close()


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_nothing_else_moves():
    a = make_checked(S2, N, "per_scene", **CFG_KW)
    b = make_checked(S2, N, "per_scene", **CFG_KW)
    data = cut(S2)
    for sb in (a, b):
        sb.enable_report()
    a.set_zones(strips(S2))
    ref = ZoneRef(S2)
    ref.set_zones(*strips(S2))
    n_events = []

    def ring_frames(sb):
        """Every frame of the global ring and of every live track's ring."""
        (glen, _), ntr, ring_len = sb.batch_ring(), sb.num_tracks(), sb.tracks()["ring_len"]
        return [[sb.batch_ring_frame(s, k) for k in range(int(glen[s]))] +
                [sb.track_ring_frame(s, j, k) for j in range(int(ntr[s])) for k in range(int(ring_len[s, j]))] for s in range(S2)]

    nothing_else_moves(a, b, data, 8, lambda f: n_events.append(len(export_and_compare(a, ref, f)[1])),
                       each_frame=TRACKS + REPORT + (lambda sb: sb.skeletons_host(), lambda sb: sb.batch_ring()), at_end=(ring_frames,))
    assert sum(n_events) > 3 * S2
    a.check(); b.check()
    a.close(); b.close()
