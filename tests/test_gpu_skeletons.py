"""The live tracks' skeletons (mmw_skeletons_*, include/mmw.h) on the GPU: every track's keypoints as the room-frame skeleton of
Visualizer.update_posture, with its plausibility check, in one call and in the report's (scene, slot) order.

Expected values come from tests/_skeleton_ref.py, a numpy restatement of the semantics in include/mmw.h applied to state read back
through `tracks()` and `report_host()`.  No live run of the reference's Visualizer pins it -- it imports Qt, pyqtgraph and
matplotlib; the pin is the five numpy lines of update_posture (Visualizer.py:274-283) as read.  Flags, gap and all 57 joint
words are compared bit for bit (as uint32); only where a test plants a NaN is "NaN where NaN is expected" accepted for that word,
since neither numpy nor the header defines a NaN's payload.

The scenario is tests/_report_scenes.py's cut to its first five scenes (the last workgroup of four scenes is ragged).  Through the
C oracle none of its 24 scenes holds 0 tracks in frames 0 .. 7 (every scene keeps a track from frame 0 on), so the empty scene the
parity test must meet is made with `reset_scenes` on scene 2 after frame 5: an empty scene between two populated ones."""
import numpy as np
import pytest

from tests import _skeleton_ref as ref
from tests._layouts import make_checked
from tests._report_scenes import CFG_KW, scenario

pytestmark = pytest.mark.gpu

S, N, F = 5, 96, 8
PLANT = (3, 5, 7)
EMPTIED = (5, 2)     # (frame, scene): reset after that frame's step


def _data():
    pts, cnt, dts = scenario()
    return pts[:F, :S], cnt[:F, :S], dts[:F, :S]


def _step(sb, data, f):
    pts, cnt, dts = data
    sb.step_host(pts[f].astype(np.float64), cnt[f], dts[f])


def _random_keypoints(rng, n):
    """(kp float32[n, 57], wide bool[n]): random keypoints whose SpineMid - Neck distance is below 0.45 (narrow) or above 0.55 (wide)."""
    kp = rng.uniform(-1.0, 2.0, size=(n, 57)).astype(np.float32)
    wide = rng.integers(0, 2, size=n).astype(bool)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.where(wide, rng.uniform(0.55, 1.2, size=n), rng.uniform(0.0, 0.45, size=n))
    for c in range(3):
        kp[:, 19 * c + 1] = (kp[:, 19 * c + 2].astype(np.float64) + r * d[:, c]).astype(np.float32)
    g = np.stack([kp[:, 19 * c + 1] - kp[:, 19 * c + 2] for c in range(3)], axis=1).astype(np.float64)
    gap = np.sqrt((g * g).sum(axis=1))
    assert ((gap < 0.45) | (gap > 0.55)).all() and ((gap > 0.55) == wide).all()   # (fp32 rounding moves a gap by 1e-7, not by 0.05)
    return kp, wide


def _plant(sb, rng):
    """Random keypoints on every live track; how many of either kind."""
    ntr = sb.num_tracks()
    owner = np.array([(s, j) for s in range(sb.S) for j in range(int(ntr[s]))], np.int32).reshape(-1, 2)
    kp, wide = _random_keypoints(rng, len(owner))
    sb.set_keypoints_host(kp, owner)
    return int(wide.sum()), int((~wide).sum())


def _same_bits(got, want, ctx=""):
    """Two SKELETON_DTYPE arrays byte for byte, field by field for the message."""
    assert got.dtype == want.dtype and len(got) == len(want), (ctx, len(got), len(want))
    for k in ("scene", "slot", "uid", "row", "flags", "reserved_"):
        assert np.array_equal(got[k], want[k]), (ctx, k, got[k], want[k])
    assert np.array_equal(got["gap"].view(np.uint32), want["gap"].view(np.uint32)), (ctx, "gap")
    assert np.array_equal(got["joint"].view(np.uint32), want["joint"].view(np.uint32)), (ctx, "joint")
    assert got.tobytes() == want.tobytes(), ctx


def _states(layout, dim_x, seed, scene_base=0):
    """Runs the scenario; after each planted frame yields (frame, sb, report rows, tracks, num_tracks history)."""
    sb = make_checked(S, N, layout, **dict(CFG_KW, dim_x=dim_x))
    sb.enable_report()
    data, rng = _data(), np.random.default_rng(seed)
    history, kinds = [], [0, 0]
    try:
        for f in range(F):
            _step(sb, data, f)
            if f == EMPTIED[0]:
                sb.reset_scenes(np.arange(S) == EMPTIED[1])
            history.append(sb.num_tracks().copy())
            if f in PLANT:
                w, n = _plant(sb, rng)
                kinds[0] += w
                kinds[1] += n
                rows, _ = sb.report_host(scene_base=scene_base)
                yield f, sb, rows, sb.tracks(), history, kinds
        sb.check()
    finally:
        sb.close()


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim_x", [9, 6])
@pytest.mark.parametrize("layout", ["per_scene", "one_workgroup"])
def test_all_mode_equals_the_restatement_bit_for_bit(layout, dim_x):
    n_entries = 0
    for f, sb, rows, trk, history, kinds in _states(layout, dim_x, seed=8100 + dim_x, scene_base=40):
        got = sb.skeletons_host(scene_base=40)
        sb.skeletons_dev(sb.buf("skeletons", len(rows) * 256).ptr, len(rows), 0, 0, 40)
        n_out, n_live = sb.skeletons_wait(0)
        assert n_out == n_live == len(rows) == len(got) == int(history[-1].sum()), f
        for k in ("scene", "slot", "uid"):
            assert np.array_equal(got[k], rows[k]), (f, k)
        assert np.array_equal(got["row"], np.arange(len(rows))) and (got["reserved_"] == 0).all(), f
        want = ref.expected(rows, trk, scene_base=40)
        assert np.array_equal(want["uid"], rows["uid"]), f
        _same_bits(got, want, ctx=f)
        assert np.array_equal(got["joint"][:, :, 2], rows["keypoints"][:, 19:38]), f   # the height row is the planted one, untouched
        n_entries += len(got)
    hist = np.stack(history)
    assert (hist[list(PLANT)] == 0).any(), hist                    # a scene without a track at a compared frame
    assert (np.diff(hist, axis=0) < 0).any(), hist                 # a track count falls
    assert hist[EMPTIED[0], EMPTIED[1]] == 0 and hist[EMPTIED[0], EMPTIED[1] + 1] > 0 and hist[EMPTIED[0], EMPTIED[1] - 1] > 0
    total = kinds[0] + kinds[1]
    assert total == n_entries > 2 * S and 4 * kinds[0] >= total and 4 * kinds[1] >= total, kinds


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim_x", [9, 6])
def test_drawn_mode_is_the_not_skipped_subset_in_order(dim_x):
    from mmwave_msc_amd import _lib
    fewer = 0
    for f, sb, rows, trk, history, kinds in _states("per_scene", dim_x, seed=8100 + dim_x):
        want = ref.expected(rows, trk)
        keep = (want["flags"] & _lib.SKEL_SKIPPED) == 0
        got = sb.skeletons_host(drawn=True)
        _same_bits(got, want[keep], ctx=f)
        assert np.array_equal(got["row"], np.flatnonzero(keep)), f
        b = sb.alloc(max(len(got), 1) * 256)
        sb.skeletons_dev(b.ptr, len(got), _lib.SKEL_DRAWN, 1)
        n_out, n_live = sb.skeletons_wait(1)
        assert (n_out, n_live) == (int(keep.sum()), len(rows)) and n_out < n_live, f
        assert b.download((n_out,), _lib.SKELETON_DTYPE).tobytes() == want[keep].tobytes(), f
        b.free()
        fewer += n_live - n_out
    assert fewer > 3


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_many_tracks_lanes_past_16_and_several_stores_per_scene():
    from tests._grid_scenes import grid_scene as _grid_scene
    n_s, n_pts, frames = 2, 640, 3
    sb = make_checked(n_s, n_pts, "per_scene", tr_max_tracks=28, db_min_samples=12, track_cap=40)
    assert sb.track_cap == 40
    sb.enable_report()
    pts = np.stack([_grid_scene(4300 + s, frames, n_pts, 18 + 2 * s) for s in range(n_s)], axis=1)
    for f in range(frames):
        sb.step_host(pts[f].astype(np.float64), np.full(n_s, n_pts, np.int32), np.full(n_s, 0.1))
    ntr = sb.num_tracks()
    assert (ntr > 16).all() and (ntr % 4 != 0).any(), ntr   # (the last group of four entries of a scene is ragged)
    wide, narrow = _plant(sb, np.random.default_rng(8300))
    assert wide > 4 and narrow > 4
    rows, _ = sb.report_host()
    want = ref.expected(rows, sb.tracks())
    assert len(want) == int(ntr.sum())
    _same_bits(sb.skeletons_host(), want, ctx="all")
    _same_bits(sb.skeletons_host(drawn=True), ref.drawn(want), ctx="drawn")
    assert 0 < len(ref.drawn(want)) < len(want)
    sb.check()
    sb.close()


# 4 ------------------------------------------------------------------------------------------------------------------------
def _four_tracks():
    """One scene with four live tracks (four targets of test_gpu_parity._grid_scene)."""
    from tests._grid_scenes import grid_scene as _grid_scene
    sb = make_checked(1, 160, "per_scene", tr_max_tracks=4, db_min_samples=12)
    pts = _grid_scene(4400, 2, 160, 4)
    for f in range(2):
        sb.step_host(pts[f][None].astype(np.float64), np.full(1, 160, np.int32), np.full(1, 0.1))
    assert int(sb.num_tracks()[0]) >= 3
    return sb


def test_the_boundary_and_non_finite_values():
    from mmwave_msc_amd import _lib
    sb = _four_tracks()
    kp = np.random.default_rng(8400).uniform(-1.0, 2.0, size=(3, 57)).astype(np.float32)
    kp[:, [1, 2, 20, 21, 39, 40]] = 0.0
    kp[0, 1] = 0.5                                                # differences (0.5, 0, 0): s = 0.25 is not > 0.25 -> drawn
    kp[1, 2] = -np.nextafter(np.float32(0.5), np.float32(1.0))    # (nextafter(0.5f, 1), 0, 0) -> skipped
    kp[2, 1] = np.nan                                             # column 1 of row 0: drawn; gap and joint[1][0] are NaN
    kp[0, 7], kp[1, 38 + 9], kp[2, 19 + 4] = np.inf, -np.inf, np.inf
    sb.set_keypoints_host(kp, np.array([(0, 0), (0, 1), (0, 2)], np.int32))
    sb.enable_report()
    rows, _ = sb.report_host()
    trk = sb.tracks()
    assert trk["keypoints"][0, :3].view(np.uint32).tobytes() == kp.view(np.uint32).tobytes()
    got, want = sb.skeletons_host()[:3], ref.expected(rows, trk)[:3]
    assert got["flags"].tolist() == want["flags"].tolist() == [0, _lib.SKEL_SKIPPED, 0]
    assert got["gap"][0] == np.float32(0.5) and got["gap"][1] == np.nextafter(np.float32(0.5), np.float32(1.0)) and np.isnan(got["gap"][2])
    nan_w = np.isnan(want["joint"])
    assert nan_w.sum() == 1 and nan_w[2, 1, 0] and np.array_equal(np.isnan(got["joint"]), nan_w)
    assert np.array_equal(got["joint"].view(np.uint32)[~nan_w], want["joint"].view(np.uint32)[~nan_w])
    assert np.array_equal(got["gap"][:2].view(np.uint32), want["gap"][:2].view(np.uint32))
    assert got["joint"][0, 7, 0] == -np.inf and got["joint"][1, 9, 1] == -np.inf and got["joint"][2, 4, 2] == np.inf
    # DRAWN: the boundary track and the NaN track, not the one past the boundary
    drawn = sb.skeletons_host(drawn=True)
    assert [r for r in drawn["row"].tolist() if r < 3] == [0, 2]
    sb.close()


# 5 ------------------------------------------------------------------------------------------------------------------------
def _settled(seed=8500):
    """The scenario after frame 7 with planted keypoints: (sb, report rows, expected ALL entries)."""
    sb = make_checked(S, N, "per_scene", **CFG_KW)
    data = _data()
    for f in range(F):
        _step(sb, data, f)
    _plant(sb, np.random.default_rng(seed))
    sb.enable_report()
    rows, _ = sb.report_host()
    return sb, rows, ref.expected(rows, sb.tracks())


def test_capacity_is_decided_on_the_device_and_nothing_is_written():
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import MmwError, SceneBatch
    sb, rows, want = _settled()
    n_live, want_d = len(want), ref.drawn(want)
    n_drawn = len(want_d)
    assert 0 < n_drawn < n_live
    sent = np.full(n_live * 256, 0xA5, np.uint8)
    b = sb.alloc(sent.nbytes).upload(sent)
    for mode, need, expect in ((_lib.SKEL_ALL, n_live, want), (_lib.SKEL_DRAWN, n_drawn, want_d)):
        sb.skeletons_dev(b.ptr, need - 1, mode, 0)
        with pytest.raises(MmwError) as ei:
            sb.skeletons_wait(0)
        assert ei.value.code == _lib.E_CAPACITY and ei.value.needed == (need, n_live)
        assert np.array_equal(b.download(sent.shape, np.uint8), sent)
        sb.skeletons_dev(b.ptr, need, mode, 1)
        assert sb.skeletons_wait(1) == (need, n_live)
        assert b.download((need,), _lib.SKELETON_DTYPE).tobytes() == expect.tobytes()
        assert np.array_equal(b.download(sent.shape, np.uint8)[need * 256:], sent[need * 256:])   # nothing past the entries
        b.upload(sent)
    sb.skeletons_dev(None, 0, _lib.SKEL_ALL, 2)              # sizing call: no buffer at all
    with pytest.raises(MmwError) as ei:
        sb.skeletons_wait(2)
    assert ei.value.code == _lib.E_CAPACITY and ei.value.needed == (n_live, n_live)
    b.free()
    sb.close()
    fresh = SceneBatch(_lib.default_config(**CFG_KW), S, N)   # no track at all: nothing, and no error
    fresh.skeletons_dev(None, 0, _lib.SKEL_DRAWN, 0)
    assert fresh.skeletons_wait(0) == (0, 0)
    assert len(fresh.skeletons_host()) == 0
    fresh.close()


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_two_tickets_around_a_step():
    from mmwave_msc_amd import _lib
    a = make_checked(S, N, "per_scene", **CFG_KW)
    b = make_checked(S, N, "per_scene", **CFG_KW)
    data = _data()
    pts, cnt, dts = data
    for sb in (a, b):
        for f in range(F - 1):
            _step(sb, data, f)
        _plant(sb, np.random.default_rng(8600))
    want0 = b.skeletons_host()
    _step(b, data, F - 1)
    want1 = b.skeletons_host()
    assert len(want0) and len(want1) and want0.tobytes() != want1.tobytes()
    cap = S * a.track_cap
    d_pts = a.alloc(pts[F - 1].size * 8).upload(pts[F - 1].astype(np.float64))
    d_cnt, d_dt = a.alloc(S * 4).upload(cnt[F - 1]), a.alloc(S * 8).upload(dts[F - 1])
    out0, out1 = a.alloc(cap * 256), a.alloc(cap * 256)
    a.synchronize()
    a.skeletons_dev(out0.ptr, cap, _lib.SKEL_ALL, 0)
    a.step_dev(d_pts.ptr, d_cnt.ptr, d_dt.ptr)
    a.skeletons_dev(out1.ptr, cap, _lib.SKEL_ALL, 1)
    assert a.skeletons_wait(1) == (len(want1), len(want1))
    assert a.skeletons_wait(0) == (len(want0), len(want0))
    assert out0.download((len(want0),), _lib.SKELETON_DTYPE).tobytes() == want0.tobytes()
    assert out1.download((len(want1),), _lib.SKELETON_DTYPE).tobytes() == want1.tobytes()
    with pytest.raises(_lib.MmwError) as ei:
        a.skeletons_wait(0)
    assert ei.value.code == _lib.E_ARG
    a.check()
    for buf in (d_pts, d_cnt, d_dt, out0, out1):
        buf.free()
    a.close(); b.close()


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_touch_nothing():
    from mmwave_msc_amd import _lib
    sb, rows, want = _settled()
    sent = np.full(len(want) * 256 + 16, 0x3C, np.uint8)
    b = sb.alloc(sent.nbytes).upload(sent)
    L, cap = sb.L, len(want)
    assert L.mmw_skeletons_async(None, b.ptr, cap, 0, 0, 0) == _lib.E_ARG
    assert L.mmw_skeletons(None, b.ptr, cap, 0, 0, None, None) == _lib.E_ARG
    for bad in (lambda: sb.skeletons_dev(b.ptr, -1), lambda: sb.skeletons_dev(None, 1), lambda: sb.skeletons_dev(b.ptr + 4, cap),
                lambda: sb.skeletons_dev(b.ptr, cap, 2), lambda: sb.skeletons_dev(b.ptr, cap, -1),
                lambda: sb.skeletons_dev(b.ptr, cap, 0, 4), lambda: sb.skeletons_dev(b.ptr, cap, 0, -1),
                lambda: sb.skeletons_wait(4), lambda: sb.skeletons_wait(-1), lambda: sb.skeletons_wait(0)):
        with pytest.raises(_lib.MmwError) as ei:
            bad()
        assert ei.value.code == _lib.E_ARG
    for t in range(3):   # no refused call left a ticket behind
        with pytest.raises(_lib.MmwError):
            sb.skeletons_wait(t)
    sb.synchronize()
    assert np.array_equal(b.download(sent.shape, np.uint8), sent)
    b.free()
    sb.close()


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_nothing_else_moves():
    from mmwave_msc_amd import _lib
    sb, rows, want = _settled()
    rows_before, ev = sb.report_host()          # (the second report: no event)
    assert len(ev) == 0 and rows_before.tobytes() == rows.tobytes()
    trk_before = sb.tracks()
    plain = sb.skeletons_host()
    _same_bits(plain, want, ctx="plain")
    sb.skeletons_host(drawn=True)
    rows_after, ev = sb.report_host()
    assert len(ev) == 0 and rows_after.tobytes() == rows_before.tobytes()
    assert sb.tracks().tobytes() == trk_before.tobytes()
    # a site table moves the fade square of the report, not the skeletons
    sb.set_sites(_lib.make_sites(sb.cfg, S, m_x=np.linspace(-1.0, 1.0, S)))
    assert sb.has_sites
    rows_site, _ = sb.report_host()
    assert rows_site.tobytes() != rows_before.tobytes()
    assert sb.skeletons_host().tobytes() == plain.tobytes()
    sb.clear_sites()
    # a reset scene contributes nothing; the others keep their entries, only `row` closes up
    gone = 1
    assert (plain["scene"] == gone).any() and (plain["scene"] > gone).any()
    sb.reset_scenes(np.arange(S) == gone)
    after = sb.skeletons_host()
    keep = plain[plain["scene"] != gone].copy()
    keep["row"] = np.arange(len(keep))
    assert not (after["scene"] == gone).any()
    assert after.tobytes() == keep.tobytes()
    sb.check()
    sb.close()
