"""The scan step the three live-track exports share (k_pair_scan, csrc/k_scan.hip) where its shape matters: more than 1024
scenes -- two scenes per thread of the scan workgroup with a ragged tail, and a short last block in the count kernels -- for the
clouds and the skeletons (the report has test_gpu_report.test_1027_scenes_the_scan_loop_and_a_short_last_block), and ONE scene,
where only thread 0 of the scan has work and thread 1023 writes the totals, for all three.

The skeletons hand the scan their counts in the order (emitted, live) and read the offsets back in that order; MMW_SKEL_DRAWN
with some tracks skipped makes the two arrays differ, so an exchange on one side only cannot pass.

The saturation of the totals at INT32_MAX is not reached here: it takes more than 2^31 points in one context."""
import numpy as np
import pytest

from tests._report_scenes import CFG_KW

pytestmark = pytest.mark.gpu

S2, N2, F2 = 1027, 32, 5


def _batch(n_scenes, max_pts):
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    return SceneBatch(_lib.default_config(**CFG_KW), n_scenes, max_pts)


@pytest.fixture(scope="module")
def big():
    """1027 scenes of one target each after five frames, the staggered presence of the report's 1027-scene test: a target arrives
    at frame 0, 1 or 2 and one in five leaves again.  Reports enabled before the first step.  Shared: the tests leave the tracker's state
    alone (the skeleton test plants keypoints, which nothing else here reads)."""
    from mmwave_msc_amd.synth import make_scene
    pts = np.zeros((F2, S2, N2, 8), np.float32)
    cnt = np.zeros((F2, S2), np.int32)
    dts = np.zeros((F2, S2))
    for s in range(S2):
        presence = np.ones((F2, 1), bool)
        presence[: s % 3] = False
        presence[2 + s % 3:] = s % 5 != 0
        pts[:, s], cnt[:, s], dts[:, s] = make_scene(7000 + s, F2, N2, 1, presence=presence)
    sb = _batch(S2, N2)
    sb.enable_report()
    for f in range(F2):
        sb.step_host(pts[f].astype(np.float64), cnt[f], dts[f])
    ntr = sb.num_tracks()
    assert ntr[S2 - 3:].any(), "the last, short block holds tracks"
    assert int((ntr > 0).sum()) > S2 // 2, "most scenes hold a track"
    yield sb
    sb.close()


def _concat(frames):
    return np.concatenate([np.zeros((0, 8))] + [np.asarray(a, np.float64).reshape(-1, 8) for a in frames])


def test_clouds_at_1027_scenes_against_the_getters_and_the_report(big):
    sb = big
    rep, _ = sb.report_host(scene_base=3)
    d, rows = sb.clouds_host(rows=True, unassigned=True, scene_base=3)
    print("entries", len(d), "rows", len(rows), "report rows", len(rep))
    # every entry starts where the previous one ended: `first` is the running sum of the counts, over all 1027 scenes
    ends = np.concatenate([[0], np.cumsum(d["count"].astype(np.int64))])
    assert np.array_equal(d["first"], ends[:-1]) and int(ends[-1]) == len(rows) > 0
    # the directory lines up with the report: the tracks' entries are its rows, and every scene closes with its global ring
    tracked = d[d["slot"] >= 0]
    assert len(tracked) == len(rep) == int(sb.num_tracks().sum()) and len(d) == len(rep) + S2
    for k in ("scene", "slot", "uid"):
        assert np.array_equal(tracked[k], rep[k]), k
    assert np.array_equal(d["scene"][d["slot"] < 0], 3 + np.arange(S2))
    assert (np.diff(d["scene"]) >= 0).all()
    assert (tracked["scene"] >= 3 + S2 - 3).any(), "the last, short block holds tracks"
    # the rows are what the library's own getters return, frame by frame
    ln, _ = sb.batch_ring()
    for e in d:
        s, j = int(e["scene"]) - 3, int(e["slot"])
        if j < 0:
            want = _concat([sb.batch_ring_frame(s, k) for k in range(int(ln[s]))])
            assert int(e["frames"]) == int(ln[s]), s
        else:
            want = _concat([sb.track_ring_frame(s, j, k) for k in range(int(e["frames"]))])
        assert int(e["count"]) == len(want), (s, j)
        assert rows[e["first"]: e["first"] + e["count"]].tobytes() == want.tobytes(), (s, j)


def test_skeletons_drawn_at_1027_scenes_keep_their_report_rows(big):
    from mmwave_msc_amd import _lib
    sb = big
    ntr = sb.num_tracks()
    owner = np.array([(s, j) for s in range(S2) for j in range(int(ntr[s]))], np.int32).reshape(-1, 2)
    # every third scene's first track fails the reference's check (SpineMid - Neck = 1 > 0.5), every other track passes it (0)
    wide = (owner[:, 0] % 3 == 0) & (owner[:, 1] == 0)
    kp = np.random.default_rng(8700).uniform(-1.0, 2.0, size=(len(owner), 57)).astype(np.float32)
    for c in range(3):
        kp[:, 19 * c + 1] = kp[:, 19 * c + 2]
    kp[wide, 1] = kp[wide, 2] + np.float32(1.0)
    sb.set_keypoints_host(kp, owner)
    rep, _ = sb.report_host()
    every = sb.skeletons_host()
    assert len(every) == len(rep) == len(owner) and np.array_equal(every["row"], np.arange(len(rep)))
    for k in ("scene", "slot", "uid"):
        assert np.array_equal(every[k], rep[k]), k
    assert np.array_equal((every["flags"] & _lib.SKEL_SKIPPED) != 0, wide)
    keep = ~wide
    b = sb.alloc(len(every) * 256)
    sb.skeletons_dev(b.ptr, int(keep.sum()), _lib.SKEL_DRAWN, 1)       # exactly the room the emitted entries need
    n_out, n_live = sb.skeletons_wait(1)
    print("n_out", n_out, "n_live", n_live)
    assert n_live == len(rep) and n_out == int(keep.sum()) and 0 < n_out < n_live
    got = b.download((n_out,), _lib.SKELETON_DTYPE)
    b.free()
    assert np.array_equal(got["row"], np.flatnonzero(keep))            # `row` is the entry's index in the SKEL_ALL output
    assert got.tobytes() == every[keep].tobytes()
    assert sb.skeletons_host(drawn=True).tobytes() == got.tobytes()
    # the two scanned arrays differ: an emitted entry's position falls behind its report row from the first skipped track on
    assert (got["row"] > np.arange(n_out)).sum() > n_out // 2


# ---- one scene ---------------------------------------------------------------------------------------------------------
def _exports(sb):
    """(name, item sizes, issue(ptr0, cap0, ptr1, cap1, ticket), wait) of the three exports; the skeletons have one buffer."""
    from mmwave_msc_amd import _lib
    return (
        ("report", (324, 16), lambda p0, c0, p1, c1, t: sb.report_async(p0, c0, p1, c1, 0, t), sb.report_wait),
        ("clouds", (32, 64), lambda p0, c0, p1, c1, t: sb.clouds_dev(p0, c0, p1, c1, _lib.CLOUD_ROWS, t), sb.clouds_wait),
        ("skeletons", (256, 0), lambda p0, c0, p1, c1, t: sb.skeletons_dev(p0, c0, _lib.SKEL_ALL, t), sb.skeletons_wait),
    )


@pytest.mark.parametrize("tracks", [False, True], ids=["no_track", "one_track"])
def test_one_scene_through_all_three_exports(tracks):
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import MmwError
    from mmwave_msc_amd.synth import make_scene
    sb = _batch(1, N2)
    sb.enable_report()
    if tracks:
        pts, cnt, dts = make_scene(7001, F2, N2, 1)
        for f in range(F2):
            sb.step_host(pts[f][None].astype(np.float64), cnt[f: f + 1], dts[f: f + 1])
    n_trk = int(sb.num_tracks()[0])
    assert (n_trk > 0) == tracks
    room = 128   # (a track's cloud is at most ring x 32 = 96 rows)
    for name, items, issue, wait in _exports(sb):
        sent = [np.full(max(room * it, 16), 0xA5 + k, np.uint8) for k, it in enumerate(items)]
        bufs = [sb.alloc(a.nbytes).upload(a) for a in sent]
        if not tracks:
            # nothing to report: (0, 0) with and without buffers, and not a byte is written
            issue(None, 0, None, 0, 0)
            assert wait(0) == (0, 0), name
            issue(bufs[0].ptr, room, bufs[1].ptr, room, 1)
            assert wait(1) == (0, 0), name
        else:
            issue(None, 0, None, 0, 0)                                   # sizing call: refused, with the counts needed
            with pytest.raises(MmwError) as ei:
                wait(0)
            need = ei.value.needed
            print(name, "needed", need)
            assert ei.value.code == _lib.E_CAPACITY and need[0] > 0 and max(need) <= room, (name, need)
            assert need[0] == n_trk and (name != "skeletons" or need[1] == n_trk), (name, need)
            issue(bufs[0].ptr, need[0] - 1, bufs[1].ptr, need[1], 1)     # one entry short: refused alike
            with pytest.raises(MmwError) as ei:
                wait(1)
            assert ei.value.code == _lib.E_CAPACITY and ei.value.needed == need, name
        for b, a in zip(bufs, sent):
            assert np.array_equal(b.download(a.shape, np.uint8), a), name
        if tracks:
            issue(bufs[0].ptr, need[0], bufs[1].ptr, need[1], 2)         # with exactly the room: the same counts
            assert wait(2) == need, name
            head = bufs[0].download((need[0] * items[0],), np.uint8).view(np.int32).reshape(need[0], -1)
            assert (head[:, 0] == 0).all() and np.array_equal(head[:, 1], np.arange(n_trk)), name   # scene 0, slots in order
            for b, a, it, n in zip(bufs, sent, items, need):
                assert np.array_equal(b.download(a.shape, np.uint8)[n * it:], a[n * it:]), name      # nothing past the entries
        for b in bufs:
            b.free()
    sb.close()


# ---- the host wrappers' growth path ------------------------------------------------------------------------------------
def test_every_host_export_grows_once_and_returns_what_an_unrefused_twin_returns():
    """report_host, clouds_host, skeletons_host and radar_log_host share one issue / wait / grow / retry helper.  Context A starts
    with room for ONE entry in every buffer, so each export is refused once (E_CAPACITY with the counts needed) and asked again;
    its twin B, fed the same frames and the same radar bytes, has ample room and is never refused.  A returns B's arrays byte for
    byte -- the refused call wrote, consumed and rebased nothing --, A's capacities end up as the counts returned, B's never moved."""
    from mmwave_msc_amd import radar
    from tests import _rows_ref as rr
    from tests._report_scenes import scenario
    S, N, F = 4, 96, 6
    pts, cnt, dts = scenario(n_scenes=S, n_pts=N)   # (its 12 frames: the third target's arrival needs 9; the first six are stepped)
    rng = np.random.default_rng(61)
    objects = (5, 1, 17, 9)
    chunks = []
    for s in range(S):
        raw = np.column_stack([rng.uniform(-3, 3, N), rng.uniform(0.2, 7, N), rng.uniform(-1.5, 0.8, N),
                               rng.integers(-12, 13, N) * rr.CFGP["dopplerResolutionMps"], rng.integers(0, 4000, N)])
        body = radar.encode_tlv_bodies(raw, objects[s], 9, rr.CFGP["dopplerResolutionMps"])
        chunks.append(rr.uart_packet(s + 1, body.tobytes(), objects[s]))
    a, b = _batch(S, N), _batch(S, N)
    for sb in (a, b):
        sb.enable_report()
        sb.open_radars(rr.CFGP, t0=0.0)
        sb.enable_radar_log()
        for f in range(F):
            sb.step_host(pts[f].astype(np.float64), cnt[f], dts[f])
        sb.read_radars(chunks, now=1.0)
    ample = {"report": (256, 512), "clouds": (256, 16384), "skeletons": (256,), "radar_log": (64, 4096)}
    assert sorted(a._export_caps) == sorted(ample)
    a._export_caps = {k: (1,) * len(v) for k, v in ample.items()}
    b._export_caps = dict(ample)
    calls = {"report": lambda sb: sb.report_host(), "clouds": lambda sb: sb.clouds_host(unassigned=True),
             "skeletons": lambda sb: (sb.skeletons_host(),), "radar_log": lambda sb: sb.radar_log_host()}
    for name, call in calls.items():
        got, want = call(a), call(b)
        print(name, [len(w) for w in want])
        assert len(got) == len(want) == len(ample[name]), name
        for g, w in zip(got, want):
            assert len(w) > 0 and g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), name
        assert max(len(w) for w in want) > 1, name                       # (room for one entry was too little: A was refused)
        assert a._export_caps[name] == tuple(len(g) for g in got), (name, a._export_caps[name])
        assert b._export_caps[name] == ample[name], (name, b._export_caps[name])
    a.close(); b.close()
