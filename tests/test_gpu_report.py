"""The live-track report (mmw_report_*, include/mmw.h) on the GPU: compact rows of the live tracks with their uids, and the
tracks that appeared or left since the previous report as events.

Rows are checked against what the library already reports about the same state -- `track_table_host` (bit for bit: one device
function fills both), `tracks()["uid"]`, `num_tracks()` -- and events against a host-side difference of consecutive uid lists.
The scenario (tests/_report_scenes.py) has been run through the C oracle: track counts rise and fall, and some scene gains and
loses a track in the same frame; the tests assert positive BORN and GONE counts so that they cannot pass vacuously."""
import numpy as np
import pytest

from tests._feature_run import step
from tests._layouts import LAYOUTS, make_checked
from tests._report_scenes import CFG_KW, F, N, S, as_tuples, host_events, scenario, uid_lists

pytestmark = pytest.mark.gpu

SHARED = ("scene", "slot", "point_num", "lifetime", "x", "centroid", "keypoints", "fade_x", "fade_z", "fade_size")


def _batch(n_scenes=S, max_pts=N, **kw):
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    return SceneBatch(_lib.default_config(**{**CFG_KW, **kw}), n_scenes, max_pts)


def _check_rows(sb, rows, events, scene_base=0):
    """Rows against num_tracks(), tracks() and the track table of the same state."""
    from mmwave_msc_amd import _lib
    ntr, trk = sb.num_tracks(), sb.tracks()
    table = sb.track_table_host(sb.track_cap, scene_base)
    assert len(rows) == int(ntr.sum())
    want = [(s, j) for s in range(sb.S) for j in range(int(ntr[s]))]
    assert [(int(r["scene"]) - scene_base, int(r["slot"])) for r in rows] == want   # (scene, slot) order, no dead slot
    if not want:
        return
    ss, jj = np.array(want).T
    alive = table[ss, jj]
    assert (alive["alive"] == 1).all() and int(table["alive"].sum()) == len(rows)
    for f in SHARED:
        assert rows[f].tobytes() == np.ascontiguousarray(alive[f]).tobytes(), f
    assert np.array_equal(rows["flags"] & _lib.REPORT_STATIC, alive["is_static"])
    assert np.array_equal(rows["uid"], trk["uid"][ss, jj])
    born = {(int(e["scene"]), int(e["uid"])) for e in events if e["kind"] == _lib.EV_BORN}
    flagged = {(int(r["scene"]), int(r["uid"])) for r in rows if r["flags"] & _lib.REPORT_BORN}
    assert flagged == born
    assert not (rows["flags"] & ~(_lib.REPORT_STATIC | _lib.REPORT_BORN)).any()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_rows_and_events_after_every_step(layout):
    from mmwave_msc_amd import _lib
    sb = make_checked(S, N, layout, **CFG_KW)
    sb.enable_report()
    prev = [[] for _ in range(S)]
    n_born = n_gone = n_both = 0
    for f in range(F):
        step(sb, f)
        rows, events = sb.report_host(scene_base=100)
        _check_rows(sb, rows, events, scene_base=100)
        cur = uid_lists(sb)
        assert as_tuples(events) == host_events(prev, cur, scene_base=100), f
        kinds = {}
        for e in events:
            kinds.setdefault(int(e["scene"]), set()).add(int(e["kind"]))
        n_born += int((events["kind"] == _lib.EV_BORN).sum())
        n_gone += int((events["kind"] == _lib.EV_GONE).sum())
        n_both += sum(1 for k in kinds.values() if {_lib.EV_BORN, _lib.EV_GONE} <= k)
        prev = cur
    sb.check()
    sb.close()
    assert n_born > S and n_gone > 0 and n_both > 0, (n_born, n_gone, n_both)


def test_a_report_every_third_frame_is_the_net_difference():
    from mmwave_msc_amd import _lib
    sb = _batch()
    sb.enable_report()
    prev = [[] for _ in range(S)]
    n_born = n_gone = 0
    for f in range(F):
        step(sb, f)
        cur = uid_lists(sb)
        if f % 3 != 2:
            continue
        rows, events = sb.report_host()
        _check_rows(sb, rows, events)
        assert as_tuples(events) == host_events(prev, cur), f
        n_born += int((events["kind"] == _lib.EV_BORN).sum())
        n_gone += int((events["kind"] == _lib.EV_GONE).sum())
        prev = cur   # (a difference of states, not a log: a track born and gone between two reports is in neither)
    sb.close()
    assert n_born > 0 and n_gone > 0, (n_born, n_gone)


def test_capacity_is_decided_on_the_device_and_a_retry_loses_nothing():
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import MmwError
    a, b = _batch(), _batch()
    for sb in (a, b):
        sb.enable_report()
        for f in range(6):
            step(sb, f)
    b._export_caps["report"] = (S * b.track_cap, 2 * S * b.track_cap)   # (the twin is never refused)
    want_rows, want_events = b.report_host()
    n_r, n_e = len(want_rows), len(want_events)
    assert n_r > 0 and n_e > 0
    rdt, edt = _lib.TRACK_REPORT_DTYPE, _lib.TRACK_EVENT_DTYPE
    sent_r, sent_e = np.full(n_r * rdt.itemsize, 0xA5, np.uint8), np.full(n_e * edt.itemsize, 0x5A, np.uint8)
    b_r, b_e = a.alloc(sent_r.nbytes).upload(sent_r), a.alloc(sent_e.nbytes).upload(sent_e)
    # sizing call: no buffers at all
    a.report_async(None, 0, None, 0, 0, 0)
    with pytest.raises(MmwError) as ei:
        a.report_wait(0)
    assert ei.value.code == _lib.E_CAPACITY and ei.value.needed == (n_r, n_e)
    for cap_r, cap_e in ((n_r - 1, n_e), (n_r, n_e - 1)):
        a.report_async(b_r.ptr, cap_r, b_e.ptr, cap_e, 0, 1)
        with pytest.raises(MmwError) as ei:
            a.report_wait(1)
        assert ei.value.code == _lib.E_CAPACITY and ei.value.needed == (n_r, n_e)
        assert np.array_equal(b_r.download(sent_r.shape, np.uint8), sent_r)
        assert np.array_equal(b_e.download(sent_e.shape, np.uint8), sent_e)
    # with room: what the twin that was never refused got -- the baseline and the generations were left alone
    a.report_async(b_r.ptr, n_r, b_e.ptr, n_e, 0, 2)
    assert a.report_wait(2) == (n_r, n_e)
    assert b_r.download((n_r,), rdt).tobytes() == want_rows.tobytes()
    assert b_e.download((n_e,), edt).tobytes() == want_events.tobytes()
    # ... and both carry on alike
    for sb in (a, b):
        step(sb, 6)
    ra, ea = a.report_host()
    rb, eb = b.report_host()
    assert ra.tobytes() == rb.tobytes() and ea.tobytes() == eb.tobytes() and len(ea) > 0
    b_r.free(); b_e.free()
    a.close(); b.close()


def test_reset_and_restore_rebase_their_scenes():
    from mmwave_msc_amd import _lib
    sb = _batch()
    sb.enable_report()
    blob = None
    for f in range(6):
        step(sb, f)
        if f == 3:
            blob = sb.snapshot([7])
            snap_uids = uid_lists(sb)[7]
        sb.report_host()
    assert snap_uids, "scene 7 holds a track at frame 3"
    before = uid_lists(sb)
    mask = np.zeros(S, bool)
    mask[[2, 5]] = True
    sb.reset_scenes(mask)
    sb.restore(blob, [9])
    rows, events = sb.report_host()
    cur = uid_lists(sb)
    assert cur[2] == [] and cur[5] == [] and cur[9] == snap_uids
    _check_rows(sb, rows, events)
    # those three scenes, and only those: exactly one REBASED each (slot = tracks now), no BORN / GONE; nothing else moved
    assert as_tuples(events) == [(2, -1, _lib.EV_REBASED, 0), (5, -1, _lib.EV_REBASED, 0), (9, -1, _lib.EV_REBASED, len(snap_uids))]
    assert as_tuples(events) == host_events(before, cur, rebased=(2, 5, 9))
    # the reports after that are ordinary: uids restarted at 0 in the reset scenes, and uid 0 is BORN only where it is a new track
    prev = cur
    born0 = set()
    for f in range(6, F):
        step(sb, f)
        rows, events = sb.report_host()
        cur = uid_lists(sb)
        _check_rows(sb, rows, events)
        assert as_tuples(events) == host_events(prev, cur), f
        assert not (events["kind"] == _lib.EV_REBASED).any()
        born0 |= {int(e["scene"]) for e in events if e["kind"] == _lib.EV_BORN and e["uid"] == 0}
        prev = cur
    assert born0 and born0 <= {2, 5}, born0
    # mmw_reset: every scene
    sb.reset()
    rows, events = sb.report_host()
    assert len(rows) == 0 and as_tuples(events) == [(s, -1, _lib.EV_REBASED, 0) for s in range(S)]
    rows, events = sb.report_host()
    assert len(rows) == 0 and len(events) == 0
    sb.close()


def test_rows_use_each_scenes_own_site():
    from mmwave_msc_amd import _lib
    sb = _batch()
    rng = np.random.default_rng(11)
    sites = _lib.make_sites(sb.cfg, S, m_x=rng.uniform(-1, 1, S), m_y=rng.uniform(-1.5, -0.2, S), m_z=rng.uniform(0.8, 1.8, S),
                            v_screen_fade_size_max=rng.uniform(0.3, 0.5, S), v_screen_fade_size_min=rng.uniform(0.05, 0.2, S),
                            v_screen_fade_weight=rng.uniform(0.02, 0.2, S))
    sb.enable_report()
    for f in range(6):
        step(sb, f)
    sb.report_host()                    # (takes the events: the reports below carry no BORN flag)
    plain_rows, _ = sb.report_host()
    sb.set_sites(sites)
    rows, events = sb.report_host()
    assert len(events) == 0 and len(rows) > S // 2
    _check_rows(sb, rows, events)   # (fade_x / fade_z / fade_size against k_table_site's)
    assert not np.array_equal(rows["fade_x"], plain_rows["fade_x"]) and not np.array_equal(rows["fade_size"], plain_rows["fade_size"])
    assert np.array_equal(rows["keypoints"], plain_rows["keypoints"]) and np.array_equal(rows["uid"], plain_rows["uid"])
    sb.clear_sites()
    rows, _ = sb.report_host()
    assert rows.tobytes() == plain_rows.tobytes()
    sb.close()


def test_two_reports_outstanding_across_two_steps():
    """No host wait between step, report, step, report: the tickets' counts and buffers equal the synchronous sequence's.  The row
    buffers start 4 and 8 bytes past a 16-byte boundary (rows are 4-byte aligned only)."""
    from mmwave_msc_amd import _lib
    pts, cnt, dts = scenario()
    a, b = _batch(), _batch()
    for sb in (a, b):
        sb.enable_report()
        for f in range(4):
            step(sb, f)
        sb.report_host()
    want = []
    for f in (4, 5):
        step(b, f)
        want.append(b.report_host())
    rdt, edt = _lib.TRACK_REPORT_DTYPE, _lib.TRACK_EVENT_DTYPE
    cap = S * a.track_cap
    d_pts = [a.alloc(pts[f].size * 8).upload(pts[f].astype(np.float64)) for f in (4, 5)]
    d_cnt = [a.alloc(S * 4).upload(cnt[f]) for f in (4, 5)]
    d_dt = [a.alloc(S * 8).upload(dts[f]) for f in (4, 5)]
    b_r = [a.alloc(cap * rdt.itemsize + 16) for _ in range(2)]
    b_e = [a.alloc(2 * cap * edt.itemsize) for _ in range(2)]
    a.synchronize()
    for k in range(2):
        a.step_dev(d_pts[k].ptr, d_cnt[k].ptr, d_dt[k].ptr)
        a.report_async(b_r[k].ptr + 4 * (k + 1), cap, b_e[k].ptr, 2 * cap, 0, k)
    for k in range(2):
        n_r, n_e = a.report_wait(k)
        assert (n_r, n_e) == (len(want[k][0]), len(want[k][1]))
        raw = b_r[k].download((cap * rdt.itemsize + 16,), np.uint8)
        rows = raw[4 * (k + 1): 4 * (k + 1) + n_r * rdt.itemsize].view(rdt)
        events = b_e[k].download((2 * cap,), edt)[:n_e]
        assert rows.tobytes() == want[k][0].tobytes() and events.tobytes() == want[k][1].tobytes()
    assert len(want[0][1]) + len(want[1][1]) > 0
    a.check()
    for d in d_pts + d_cnt + d_dt + b_r + b_e:
        d.free()
    a.close(); b.close()


def test_reports_leave_the_scene_state_alone():
    a, b = _batch(), _batch()
    a.enable_report()
    for f in range(8):
        for sb in (a, b):
            step(sb, f)
        a.report_host()
    assert a.snapshot() == b.snapshot()
    a.close(); b.close()


def test_1027_scenes_the_scan_loop_and_a_short_last_block():
    """More than 1024 scenes: two scenes per thread of the scan workgroup; 1027 = 256 blocks of four waves and one of three."""
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.synth import make_scene
    S2, N2, F2 = 1027, 32, 5
    pts = np.zeros((F2, S2, N2, 8), np.float32)
    cnt = np.zeros((F2, S2), np.int32)
    dts = np.zeros((F2, S2))
    for s in range(S2):
        presence = np.ones((F2, 1), bool)
        presence[: s % 3] = False            # arrives at frame 0, 1 or 2
        presence[2 + s % 3:] = s % 5 != 0    # one scene in five: leaves again
        pts[:, s], cnt[:, s], dts[:, s] = make_scene(7000 + s, F2, N2, 1, presence=presence)
    sb = _batch(S2, N2)
    sb.enable_report()
    prev = [[] for _ in range(S2)]
    n_born = 0
    for f in range(F2):
        step(sb, f, (pts, cnt, dts))
        rows, events = sb.report_host()
        cur = uid_lists(sb)
        _check_rows(sb, rows, events)
        assert as_tuples(events) == host_events(prev, cur), f
        n_born += int((events["kind"] == _lib.EV_BORN).sum())
        prev = cur
    assert cur[S2 - 1] or cur[S2 - 2] or cur[S2 - 3], "the last, short block holds tracks"
    assert n_born > S2 // 2, n_born
    sb.close()


def test_more_than_32_live_tracks_in_one_scene():
    """track_cap = 64 and 36 targets in scene 0: every lane of the wave's lower half and some of the upper hold a track, and the rows
    of the scene take three staging passes."""
    from mmwave_msc_amd import _lib
    from tests._grid_scenes import grid_scene as _grid_scene
    S3, N3, F3 = 2, 1024, 5
    kw = dict(tr_max_tracks=40, db_min_samples=12, track_cap=64)
    from mmwave_msc_amd.batch import SceneBatch
    sb = SceneBatch(_lib.default_config(**kw), S3, N3)
    assert sb.track_cap == 64
    pts = np.stack([_grid_scene(4700, F3, N3, 36), _grid_scene(4701, F3, N3, 5)], axis=1)
    cnt = np.full((F3, S3), N3, np.int32)
    dts = np.full((F3, S3), 0.1)
    sb.enable_report()
    prev = [[] for _ in range(S3)]
    most = 0
    for f in range(F3):
        step(sb, f, (pts, cnt, dts))
        rows, events = sb.report_host()
        cur = uid_lists(sb)
        _check_rows(sb, rows, events)
        assert as_tuples(events) == host_events(prev, cur), f
        most = max(most, len(cur[0]))
        prev = cur
    sb.check()
    sb.close()
    assert most > 32, most


def test_not_enabled_is_refused_and_enable_disable_enable_works():
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import MmwError
    sb = _batch()
    buf = sb.alloc(4096)
    for call in (lambda: sb.report_async(buf.ptr, 1, buf.ptr, 1), lambda: sb.report_wait(0), lambda: sb.report_host()):
        with pytest.raises(MmwError) as ei:
            call()
        assert ei.value.code == _lib.E_ARG
    for f in range(3):
        step(sb, f)
    sb.enable_report()
    for bad in (lambda: sb.report_async(None, 1, buf.ptr, 1), lambda: sb.report_async(buf.ptr, 1, None, 1), lambda: sb.report_async(buf.ptr, -1, buf.ptr, 1),
                lambda: sb.report_async(buf.ptr, 1, buf.ptr, -1), lambda: sb.report_async(buf.ptr, 1, buf.ptr, 1, 0, 4), lambda: sb.report_async(buf.ptr, 1, buf.ptr, 1, 0, -1),
                lambda: sb.report_wait(4), lambda: sb.report_wait(1)):
        with pytest.raises(MmwError) as ei:
            bad()
        assert ei.value.code == _lib.E_ARG
    rows, events = sb.report_host()
    assert len(rows) == int(sb.num_tracks().sum()) > 0 and len(events) == 0   # the tracks live at enable time produce no event
    sb.enable_report(False)
    with pytest.raises(MmwError) as ei:
        sb.report_host()
    assert ei.value.code == _lib.E_ARG
    step(sb, 3)
    step(sb, 4)
    sb.enable_report(False)   # (off twice is fine)
    sb.enable_report()
    rows, events = sb.report_host()
    _check_rows(sb, rows, events)
    assert len(events) == 0
    step(sb, 5)
    prev = [[int(u) for u in rows["uid"][rows["scene"] == s]] for s in range(S)]
    rows, events = sb.report_host()
    assert as_tuples(events) == host_events(prev, uid_lists(sb))
    buf.free()
    sb.close()
