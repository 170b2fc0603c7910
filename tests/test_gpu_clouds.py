"""The live tracks' point clouds (mmw_clouds_*, include/mmw.h) on the GPU: every track's effective_data and every scene's global
ring in one call, compacted in the report's (scene, slot) order.

The rows are checked against the C oracle (oracle/c) frame by frame -- its `track_ring_frame` for the track rings, and for the
global ring the rows of each frame that its association left unassigned (Tracking.py:689-697), trimmed to the frame counts of its
`batch_ring()` -- and against the library's own per-frame getters.  The oracle's track records carry no uid; `uid` is checked
against `tracks()["uid"]` of the same state (which tests/test_gpu_dropin.py pins to the reference's ids).  The scenarios
(tests/_report_scenes.py) wrap a 3-frame ring four times, so logical and physical ring slots differ from frame 3 on, and a
writer that ignores the slot permutation fails the oracle comparison: run once with the diagnostic build
`make DIAG=cloudident DIAGFLAGS=-DMMW_MUTANT_CLOUD_IDENT_SLOTS` (selected with MMW_LIB_NAME), test 1 failed at frame 3 (the
first push into a full ring: scene 2, track 0, rows in the wrong order) and passes on the product build.  Ring slots are not
visible through the C-ABI, so the snapshot test cannot assert "identity slots" directly: it snapshots at frame 7, when the
source's slots are rotated (the mutant already fails at frame 3), restores into another layout and compares bytes."""
import functools

import numpy as np
import pytest

from tests._layouts import LAYOUTS, make_checked
from tests._report_scenes import CFG_KW, F, N, S, scenario

pytestmark = pytest.mark.gpu

DENSE_N = 256   # the truncation scenario: one dense target in frames of 256 points


@functools.lru_cache(maxsize=None)
def _dense():
    """One scene population with a single dense target (230 of 256 points): its track frames hold far more than 64 rows."""
    from mmwave_msc_amd.synth import make_scene
    n_s = 4
    pts = np.zeros((F, n_s, DENSE_N, 8), np.float32)
    cnt = np.zeros((F, n_s), np.int32)
    dts = np.zeros((F, n_s))
    for s in range(n_s):
        pts[:, s], cnt[:, s], dts[:, s] = make_scene(6400 + s, F, DENSE_N, 1)
    for a in (pts, cnt, dts):
        a.setflags(write=False)
    return pts, cnt, dts


# name -> (data, configuration, scenes used, operations applied after a frame's step: {frame: [(op, scenes, argument)]})
def _variant(name):
    half, quarter = tuple(range(0, S, 2)), tuple(range(1, S, 4))
    return {
        "base": (scenario, dict(CFG_KW), S, {}),
        "ring1": (scenario, dict(CFG_KW, fb_frames_batch=0), S, {}),
        "ring4": (scenario, dict(CFG_KW, fb_frames_batch=3), S, {}),
        "ops": (scenario, dict(CFG_KW), S, {5: [("set_batch_size", half, 2)], 7: [("pop_frame", quarter, None)]}),
        "inner": (scenario, dict(CFG_KW, seek_inner=1), 4, {}),
        "dense": (_dense, dict(tr_max_tracks=2), 4, {}),
        "dense_full": (_dense, dict(tr_max_tracks=2, ring_rows=DENSE_N), 4, {}),
    }[name]


def _inputs(name):
    data, kw, n_s, ops = _variant(name)
    pts, cnt, dts = data()
    return pts[:, :n_s], cnt[:, :n_s], dts[:, :n_s], kw, n_s, ops


@functools.lru_cache(maxsize=None)
def _oracle_trace(name):
    """Per frame, per scene: ([(ring_n[ring_len], [frame rows as the oracle stores them])] per track in effective_tracks order,
    [global ring frames, oldest first]).  Computed once per variant and shared; never modified."""
    from oracle import c_oracle as co
    pts, cnt, dts, kw, n_s, ops = _inputs(name)
    cfg = co.default_config(**kw)
    scenes = [co.OracleScene(cfg, pts.shape[2]) for _ in range(n_s)]
    mirror = [[] for _ in range(n_s)]
    out = []
    for f in range(pts.shape[0]):
        for s in range(n_s):
            c = int(cnt[f, s])
            if c == 0:
                continue   # (the frame never reaches track())
            rows = pts[f, s, : max(c, 0)].astype(np.float64)
            assoc, _ = scenes[s].track(rows, float(dts[f, s]))
            mirror[s].append(rows[np.asarray(assoc) < 0])
        for op, where, arg in ops.get(f, ()):
            for s in where:
                scenes[s].set_batch_size(arg) if op == "set_batch_size" else scenes[s].pop_frame()
        frame = []
        for s in range(n_s):
            g = scenes[s].batch_ring()
            mirror[s] = mirror[s][len(mirror[s]) - len(g):] if len(g) else []
            assert [len(m) for m in mirror[s]] == [int(v) for v in g], (name, f, s)
            trk = scenes[s].tracks()
            ents = []
            for t in range(len(trk)):
                rl = int(trk[t]["ring_len"])
                ents.append((trk[t]["ring_n"][:rl].copy(), [scenes[s].track_ring_frame(t, k) for k in range(rl)]))
            frame.append((ents, list(mirror[s])))
        out.append(frame)
    return out


def _apply_ops(sb, ops, f):
    for op, where, arg in ops.get(f, ()):
        sb.set_batch_size(arg, list(where)) if op == "set_batch_size" else sb.pop_frame(list(where))


def _step(sb, data, f):
    pts, cnt, dts = data[:3]
    sb.step_host(pts[f].astype(np.float64), cnt[f], dts[f])


def _concat(frames):
    return np.concatenate([np.zeros((0, 8))] + [np.asarray(a, np.float64).reshape(-1, 8) for a in frames])


def _check_partition(d, n_points):
    """No gap and no overlap: every entry starts where the previous one ended, the last one ends at n_points."""
    ends = np.concatenate([[0], np.cumsum(d["count"].astype(np.int64))])
    assert np.array_equal(d["first"], ends[:-1]) and int(ends[-1]) == n_points
    assert (d["count"] >= 0).all() and (d["newest"] <= d["count"]).all()


def _check_against_oracle(sb, expect, d, rows, scene_base=0, unassigned=True, ctx=""):
    ntr, trk = sb.num_tracks(), sb.tracks()
    rr = sb.ring_rows
    _check_partition(d, len(rows))
    i = 0
    for s, (ents, gframes) in enumerate(expect):
        assert int(ntr[s]) == len(ents), (ctx, s)
        for j, (rn, frames) in enumerate(ents):
            e = d[i]
            want = _concat([a[:rr] for a in frames])
            assert (int(e["scene"]), int(e["slot"]), int(e["uid"])) == (scene_base + s, j, int(trk["uid"][s, j])), (ctx, s, j)
            assert int(e["frames"]) == len(frames) and int(e["count"]) == len(want), (ctx, s, j)
            assert int(e["newest"]) == (min(int(rn[-1]), rr) if len(rn) else 0), (ctx, s, j)
            assert int(e["dropped"]) == sum(max(0, int(n) - rr) for n in rn), (ctx, s, j)
            assert rows[e["first"]: e["first"] + e["count"]].tobytes() == want.tobytes(), (ctx, s, j)
            i += 1
        if unassigned:
            e = d[i]
            want = _concat(gframes)
            assert (int(e["scene"]), int(e["slot"]), int(e["uid"]), int(e["dropped"])) == (scene_base + s, -1, -1, 0), (ctx, s)
            assert int(e["frames"]) == len(gframes) and int(e["count"]) == len(want), (ctx, s)
            assert int(e["newest"]) == (len(gframes[-1]) if gframes else 0), (ctx, s)
            assert rows[e["first"]: e["first"] + e["count"]].tobytes() == want.tobytes(), (ctx, s)
            i += 1
    assert i == len(d), ctx


def _run_against_oracle(name, sb):
    data = _inputs(name)
    trace = _oracle_trace(name)
    n_entries = 0
    for f in range(data[0].shape[0]):
        _step(sb, data, f)
        _apply_ops(sb, data[5], f)
        d, rows = sb.clouds_host(rows=True, unassigned=True, scene_base=100)
        _check_against_oracle(sb, trace[f], d, rows, scene_base=100, ctx=(name, f))
        n_entries += int((d["slot"] >= 0).sum())
    sb.check()
    return n_entries


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_rows_against_the_oracle_after_every_step(layout):
    sb = make_checked(S, N, layout, **CFG_KW)
    assert sb.ring == 3
    n = _run_against_oracle("base", sb)
    sb.close()
    assert n > 4 * S, n


# 2 ------------------------------------------------------------------------------------------------------------------------
def _batch(name, **kw):
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    data = _inputs(name)
    return SceneBatch(_lib.default_config(**{**data[3], **kw}), data[4], data[0].shape[2]), data


def test_rows_against_the_librarys_own_getters_and_the_report():
    sb, data = _batch("base")
    sb.enable_report()
    compared = 0
    for f in range(F):
        _step(sb, data, f)
        rep, _ = sb.report_host(scene_base=7)
        d, _ = sb.clouds_host(rows=True, scene_base=7)
        assert len(d) == len(rep) and (d["slot"] >= 0).all()
        for k in ("scene", "slot", "uid"):
            assert np.array_equal(d[k], rep[k]), (f, k)
        if f not in (4, 8, F - 1):
            continue
        d, rows = sb.clouds_host(rows=True, unassigned=True)
        _check_partition(d, len(rows))
        ln, _ = sb.batch_ring()
        for e in d:
            s, j = int(e["scene"]), int(e["slot"])
            if j < 0:
                want = _concat([sb.batch_ring_frame(s, k) for k in range(int(ln[s]))])
                assert int(e["frames"]) == int(ln[s])
            else:
                want = _concat([sb.track_ring_frame(s, j, k) for k in range(int(e["frames"]))])
            assert rows[e["first"]: e["first"] + e["count"]].tobytes() == want.tobytes(), (f, s, j)
            compared += 1
    sb.close()
    assert compared > 3 * S


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_points_mode_is_the_rows_rounded_once():
    from mmwave_msc_amd import _lib
    sb, data = _batch("base")
    for f in range(8):
        _step(sb, data, f)
    for unassigned in (False, True):
        d, rows = sb.clouds_host(rows=True, unassigned=unassigned)
        dp, pts = sb.clouds_host(rows=False, unassigned=unassigned)
        assert pts.dtype == _lib.CLOUD_POINT_DTYPE and len(pts) == len(rows) > 0
        assert dp.tobytes() == d.tobytes()
        xyz = rows[:, 0:3].astype(np.float32)
        for c, k in enumerate("xyz"):
            assert pts[k].tobytes() == np.ascontiguousarray(xyz[:, c]).tobytes(), k
        assert np.array_equal(pts["track"], np.repeat(np.arange(len(d), dtype=np.int32), d["count"]))
    sb.close()


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_truncated_frames_are_counted_as_dropped():
    trace = _oracle_trace("dense_full")
    long_frames = sum(1 for frame in trace for ents, _ in frame for rn, _ in ents for n in rn if n > 64)
    assert long_frames >= 8, long_frames   # (on the oracle: the run does meet frames of more than 64 rows)
    a, data = _batch("dense")
    b, _ = _batch("dense_full")
    assert (a.ring_rows, b.ring_rows) == (64, DENSE_N)
    n_dropped = 0
    for f in range(F):
        for sb in (a, b):
            _step(sb, data, f)
        da, ra = a.clouds_host(rows=True, unassigned=True)
        db, rb = b.clouds_host(rows=True, unassigned=True)
        _check_against_oracle(a, _oracle_trace("dense")[f], da, ra, ctx=("dense", f))        # the oracle's first 64 rows of each frame
        _check_against_oracle(b, trace[f], db, rb, ctx=("dense_full", f))
        assert (db["dropped"] == 0).all()
        assert np.array_equal(db["count"], da["count"] + da["dropped"]) and np.array_equal(db["frames"], da["frames"])
        n_dropped += int(da["dropped"].sum())
    a.close(); b.close()
    assert n_dropped > 8 * (230 - 64) // 2, n_dropped


# 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ring", [("ring1", 1), ("ring4", 4)])
def test_rings_of_one_and_four_frames(name, ring):
    sb, _ = _batch(name)
    assert sb.ring == ring
    assert _run_against_oracle(name, sb) > S
    sb.close()


def test_resized_and_popped_global_rings():
    sb, _ = _batch("ops")
    assert _run_against_oracle("ops", sb) > S
    sb.close()


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_seek_inner_whole_frames():
    sb, _ = _batch("inner")
    assert sb.cfg.seek_inner == 1 and sb.ring_rows >= sb.ring * N
    assert _run_against_oracle("inner", sb) > 4
    d, _ = sb.clouds_host(rows=True, unassigned=True)
    assert (d["dropped"] == 0).all()
    sb.close()


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_capacity_is_decided_on_the_device_and_nothing_is_written():
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import MmwError
    sb, data = _batch("base")
    empty_d, empty_r = sb.clouds_host(rows=True)          # no track, empty rings: nothing, and no error
    assert len(empty_d) == 0 and len(empty_r) == 0
    sb.clouds_dev(None, 0, None, 0, _lib.CLOUD_ROWS, 0)
    assert sb.clouds_wait(0) == (0, 0)
    for f in range(6):
        _step(sb, data, f)
    mode = _lib.CLOUD_ROWS | _lib.CLOUD_UNASSIGNED
    want_d, want_r = sb.clouds_host(rows=True, unassigned=True)
    _check_against_oracle(sb, _oracle_trace("base")[5], want_d, want_r)
    n_t, n_p = len(want_d), len(want_r)
    assert n_t > S and n_p > 0
    sent_d, sent_r = np.full(n_t * 32, 0xA5, np.uint8), np.full(n_p * 64, 0x5A, np.uint8)
    b_d, b_r = sb.alloc(sent_d.nbytes).upload(sent_d), sb.alloc(sent_r.nbytes).upload(sent_r)
    sb.clouds_dev(None, 0, None, 0, mode, 0)               # sizing call: no buffers at all
    with pytest.raises(MmwError) as ei:
        sb.clouds_wait(0)
    assert ei.value.code == _lib.E_CAPACITY and ei.value.needed == (n_t, n_p)
    for cap_t, cap_p in ((n_t, n_p - 1), (n_t - 1, n_p)):
        sb.clouds_dev(b_d.ptr, cap_t, b_r.ptr, cap_p, mode, 1)
        with pytest.raises(MmwError) as ei:
            sb.clouds_wait(1)
        assert ei.value.code == _lib.E_CAPACITY and ei.value.needed == (n_t, n_p)
        assert np.array_equal(b_d.download(sent_d.shape, np.uint8), sent_d)
        assert np.array_equal(b_r.download(sent_r.shape, np.uint8), sent_r)
    sb.clouds_dev(b_d.ptr, n_t, b_r.ptr, n_p, mode, 2)
    assert sb.clouds_wait(2) == (n_t, n_p)
    assert b_d.download((n_t,), _lib.CLOUD_TRACK_DTYPE).tobytes() == want_d.tobytes()
    assert b_r.download((n_p, 8), np.float64).tobytes() == want_r.tobytes()
    # refused arguments touch nothing
    for bad in (lambda: sb.clouds_dev(None, 1, b_r.ptr, 1), lambda: sb.clouds_dev(b_d.ptr, 1, None, 1), lambda: sb.clouds_dev(b_d.ptr, -1, b_r.ptr, 1),
                lambda: sb.clouds_dev(b_d.ptr, 1, b_r.ptr, -1), lambda: sb.clouds_dev(b_d.ptr, 1, b_r.ptr, 1, 4), lambda: sb.clouds_dev(b_d.ptr, 1, b_r.ptr, 1, -1),
                lambda: sb.clouds_dev(b_d.ptr, 1, b_r.ptr, 1, 0, 4), lambda: sb.clouds_dev(b_d.ptr, 1, b_r.ptr, 1, 0, -1),
                lambda: sb.clouds_dev(b_d.ptr, 1, b_r.ptr + 8, 1), lambda: sb.clouds_dev(b_d.ptr + 2, 1, b_r.ptr, 1),
                lambda: sb.clouds_wait(4), lambda: sb.clouds_wait(1)):
        with pytest.raises(MmwError) as ei:
            bad()
        assert ei.value.code == _lib.E_ARG
    b_d.free(); b_r.free()
    sb.close()


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_four_tickets_outstanding_across_four_steps():
    from mmwave_msc_amd import _lib
    a, data = _batch("base")
    b, _ = _batch("base")
    pts, cnt, dts = data[:3]
    for sb in (a, b):
        for f in range(4):
            _step(sb, data, f)
    frames = (4, 5, 6, 7)
    want = []
    for f in frames:
        want.append(b.clouds_host(rows=True, unassigned=True))
        _step(b, data, f)
    cap_t, cap_p = S * (a.track_cap + 1), S * (a.track_cap * a.ring * a.ring_rows + a.ring * N)
    d_pts = [a.alloc(pts[f].size * 8).upload(pts[f].astype(np.float64)) for f in frames]
    d_cnt = [a.alloc(S * 4).upload(cnt[f]) for f in frames]
    d_dt = [a.alloc(S * 8).upload(dts[f]) for f in frames]
    b_d = [a.alloc(cap_t * 32) for _ in frames]
    b_r = [a.alloc(cap_p * 64) for _ in frames]
    a.synchronize()
    for k in range(4):
        a.clouds_dev(b_d[k].ptr, cap_t, b_r[k].ptr, cap_p, _lib.CLOUD_ROWS | _lib.CLOUD_UNASSIGNED, k)
        a.step_dev(d_pts[k].ptr, d_cnt[k].ptr, d_dt[k].ptr)
    for k in (2, 0, 3, 1):
        n_t, n_p = a.clouds_wait(k)
        assert (n_t, n_p) == (len(want[k][0]), len(want[k][1])), k
        assert b_d[k].download((n_t,), _lib.CLOUD_TRACK_DTYPE).tobytes() == want[k][0].tobytes(), k
        assert b_r[k].download((n_p, 8), np.float64).tobytes() == want[k][1].tobytes(), k
    assert len({w[1].tobytes() for w in want}) == 4   # four different states
    a.check()
    for buf in d_pts + d_cnt + d_dt + b_d + b_r:
        buf.free()
    a.close(); b.close()


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_snapshot_round_trip_into_another_layout():
    a = make_checked(S, N, "track_wise", **CFG_KW)
    data = _inputs("base")
    for f in range(8):   # (8 pushes into 3-frame rings: the source's slots are rotated)
        _step(a, data, f)
    b = make_checked(S, N, "per_scene", **CFG_KW)
    b.restore(a.snapshot())
    for rows, unassigned in ((True, True), (False, False)):
        da, oa = a.clouds_host(rows=rows, unassigned=unassigned, scene_base=3)
        db, ob = b.clouds_host(rows=rows, unassigned=unassigned, scene_base=3)
        assert len(da) > S // 2 and da.tobytes() == db.tobytes() and oa.tobytes() == ob.tobytes()
    d, rows = b.clouds_host(rows=True, unassigned=True)
    _check_against_oracle(b, _oracle_trace("base")[7], d, rows, ctx="restored")
    a.close(); b.close()
