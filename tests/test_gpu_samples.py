"""The training samples (mmw_samples_*, include/mmw.h) on the GPU: what preprocessing.py:192-220 saves of every scene after its
track(), in one call.

Expected values come from the C oracle (oracle/c): after every frame its `tracks()` gives position 0's lifetime, centroid and
ring sizes, its `track_ring_frame` the ring's frames, and tests/_sample_ref.py (pinned to the repository's own formatters by
tests/test_sample_exports.py) turns them into the block, the CNN input and the directory entry.  The oracle's records carry no
uid; `uid` is checked against `tracks()["uid"][s, 0]` of the same state.  The scenario (tests/_report_scenes.py, three scene-frames
skipped and scene 2 kept without a cluster for three frames) has position 0 stale, absent, expiring and changing hands; its
counts are asserted on the oracle before anything is compared.  A writer that lays the frames out oldest first fails the oracle
comparison: see DESIGN.md §8g for the run of the diagnostic build `make DIAG=sampleorder DIAGFLAGS=-DMMW_MUTANT_SAMPLE_OLDEST_FIRST`."""
import functools
import os

import numpy as np
import pytest

from tests import _sample_ref as ref
from tests._golden import canon_feat
from tests._layouts import LAYOUTS, make_checked
from tests._report_scenes import CFG_KW, F, N, S, scenario

pytestmark = pytest.mark.gpu

BASE = 100   # scene_base of the comparisons


@functools.lru_cache(maxsize=None)
def _scene():
    pts, cnt, dts = scenario()
    cnt = cnt.copy()
    cnt[3, 1] = cnt[8, 1] = cnt[5, 9] = 0          # skipped frames
    for f in range(3):
        cnt[f, 2] = min(cnt[f, 2], 3)              # no cluster of 12 exists in scene 2's ring: three asked frames without a track
    cnt.setflags(write=False)
    return pts, cnt, dts


def _variant(name):
    from tests.test_gpu_clouds import _dense
    return {"base": (_scene, dict(CFG_KW), S), "ring1": (_scene, dict(CFG_KW, fb_frames_batch=0), S),
            "dense": (_dense, dict(tr_max_tracks=2), 4)}[name]


def _inputs(name):
    data, kw, n_s = _variant(name)
    pts, cnt, dts = data()
    return pts[:, :n_s], cnt[:, :n_s], dts[:, :n_s], kw, n_s


@functools.lru_cache(maxsize=None)
def _trace(name):
    """Per frame, per scene: None while the scene has no track, else position 0 as the oracle holds it after the frame --
    (lifetime, centroid[:2], ring_n[ring_len], [frames oldest first]).  Computed once per variant and shared; never modified."""
    from oracle import c_oracle as co
    pts, cnt, dts, kw, n_s = _inputs(name)
    cfg = co.default_config(**kw)
    scenes = [co.OracleScene(cfg, pts.shape[2]) for _ in range(n_s)]
    out = []
    for f in range(pts.shape[0]):
        frame = []
        for s in range(n_s):
            c = int(cnt[f, s])
            if c != 0:
                scenes[s].track(pts[f, s, :c].astype(np.float64), float(dts[f, s]))
            trk = scenes[s].tracks()
            if len(trk) == 0:
                frame.append(None)
                continue
            rl = int(trk[0]["ring_len"])
            frame.append((float(trk[0]["lifetime"]), trk[0]["centroid"][:2].copy(), trk[0]["ring_n"][:rl].copy(),
                          [scenes[s].track_ring_frame(0, k) for k in range(rl)]))
        out.append(frame)
    return out


def _gives(t):
    return t is not None and ref.is_sample(1, t[0], t[2])


def _expect(sb, trace_f, asked, absolute=False, base=BASE):
    """(dir, blocks) the export owes for one frame: the asked scenes whose position 0 is a sample, ascending."""
    from mmwave_msc_amd import _lib
    uid = sb.tracks()["uid"]
    ents, blocks = [], []
    for s, t in enumerate(trace_f):
        if not asked[s] or not _gives(t):
            continue
        ents.append(ref.entry_of(base + s, int(uid[s, 0]), t[2], t[1], _lib.SAMPLE_ENTRY_DTYPE))
        blocks.append(ref.block_of(t[3], None if absolute else t[1]))
    d = np.array(ents, _lib.SAMPLE_ENTRY_DTYPE).reshape(-1)
    return d, np.array(blocks, np.float64).reshape(-1, 192, 5)


def _step(sb, data, f):
    sb.step_host(data[0][f].astype(np.float64), data[1][f], data[2][f])


def _same(got, want, ctx):
    assert len(got[0]) == len(want[0]), (ctx, len(got[0]), len(want[0]))
    assert got[0].tobytes() == want[0].tobytes(), (ctx, got[0], want[0])
    assert got[1].shape == want[1].shape and got[1].tobytes() == want[1].tobytes(), ctx


def _batch(name, **kw):
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    data = _inputs(name)
    return SceneBatch(_lib.default_config(**{**data[3], **kw}), data[4], data[0].shape[2]), data


# 0 ------------------------------------------------------------------------------------------------------------------------
def test_the_fixture_meets_every_branch_of_the_rule_on_the_oracle():
    cnt, trace = _scene()[1], _trace("base")
    asked = cnt != 0
    samples = stale = empty = 0
    by_frames = {1: 0, 2: 0, 3: 0}
    again = 0
    for f in range(F):
        for s in range(S):
            t = trace[f][s]
            if not asked[f, s]:
                again += int(_gives(t))     # a skipped scene whose position 0 still has lifetime 0: what NULL flags report again
                continue
            if t is None:
                empty += 1
            elif _gives(t):
                samples += 1
                by_frames[len(t[3])] += 1
            else:
                assert t[0] != 0
                stale += 1
    assert (samples, stale, empty, int((~asked).sum())) == (188, 94, 3, 3)
    assert min(by_frames.values()) > 0, by_frames
    assert again >= 1, again


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_blocks_and_directory_against_the_oracle_after_every_step(layout):
    sb = make_checked(S, N, layout, **CFG_KW)
    assert sb.ring == 3 and sb.ring_rows >= 64
    data, trace = _inputs("base"), _trace("base")
    n = again = changed = 0
    prev = None
    for f in range(F):
        _step(sb, data, f)
        asked = data[1][f] != 0
        got = sb.samples_host(scenes=np.flatnonzero(asked), scene_base=BASE)
        _same(got, _expect(sb, trace[f], asked), (layout, f))
        n += len(got[0])
        # NULL flags: every scene is asked, and a skipped one whose position 0 still has lifetime 0 is reported again
        got_all = sb.samples_host(scene_base=BASE)
        _same(got_all, _expect(sb, trace[f], np.ones(S, bool)), (layout, f, "all"))
        again += len(got_all[0]) - len(got[0])
        ntr, uid0 = sb.num_tracks(), sb.tracks()["uid"][:, 0].copy()
        if prev is not None:
            changed += int(((prev[0] > 0) & (ntr > 0) & (prev[1] != uid0)).sum())
        prev = (ntr, uid0)
    sb.check()
    sb.close()
    assert n == 188 and again >= 1, (n, again)
    assert changed == 43, changed   # position 0 changed track


# 2 ------------------------------------------------------------------------------------------------------------------------
def test_frames_of_more_than_64_rows_are_cut_and_counted():
    trace = _trace("dense")
    sb, data = _batch("dense")
    assert sb.ring_rows == 64
    n = 0
    for f in range(F):
        _step(sb, data, f)
        want = _expect(sb, trace[f], np.ones(4, bool), base=0)
        got = sb.samples_host()
        _same(got, want, ("dense", f))
        for e, t in zip(got[0], [t for t in trace[f] if _gives(t)]):
            assert max(int(v) for v in t[2]) > 64 and int(e["cut"]) == sum(max(0, int(v) - 64) for v in t[2]) > 0, (f, e)
            assert int(e["rows"][0]) == int(t[2][-1])
        n += len(got[0])
    sb.close()
    assert n == 48, n


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_a_ring_of_one_frame_and_a_ring_of_four():
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import MmwError
    sb, data = _batch("ring1")
    assert sb.ring == 1
    trace = _trace("ring1")
    n = 0
    for f in range(6):
        _step(sb, data, f)
        asked = data[1][f] != 0
        got = sb.samples_host(scenes=np.flatnonzero(asked), scene_base=BASE)
        _same(got, _expect(sb, trace[f], asked), ("ring1", f))
        assert (got[0]["frames"] == 1).all() and not got[1][:, 64:].any()     # one frame and 128 zero rows
        n += len(got[0])
    sb.close()
    assert n > S
    sb, data = _batch("base", fb_frames_batch=3)
    assert sb.ring == 4
    for f in range(4):
        _step(sb, data, f)
    fill_d, fill_o = np.full(S * 48, 0xA5, np.uint8), np.full(S * 7680, 0x5A, np.uint8)
    b_d, b_o = sb.alloc(fill_d.nbytes).upload(fill_d), sb.alloc(fill_o.nbytes).upload(fill_o)
    for mode in (_lib.SAMPLE_BLOCK, _lib.SAMPLE_INPUT):
        with pytest.raises(MmwError) as ei:
            sb.samples_dev(b_d.ptr, S, b_o.ptr, mode)
        assert ei.value.code == _lib.E_ARG
    sb.synchronize()
    assert np.array_equal(b_d.download(fill_d.shape, np.uint8), fill_d) and np.array_equal(b_o.download(fill_o.shape, np.uint8), fill_o)
    b_d.free(); b_o.free()
    sb.close()


# 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sites", [False, True])
def test_the_cnn_input_is_the_stable_restatement_of_the_block(sites):
    from mmwave_msc_amd import _lib
    sb, data = _batch("base")
    mean, std = np.full(S, sb.cfg.intensity_mu), np.full(S, sb.cfg.intensity_std)
    if sites:   # half the scenes with intensity mean 0 -- their pad rows normalise to all-zero rows -- and another std
        mean[::2], std[::2] = 0.0, 3.5
        sb.set_sites(_lib.make_sites(sb.cfg, S, intensity_mu=mean, intensity_std=std))
    n = padded_zero = 0
    for f in range(F):
        _step(sb, data, f)
        if f % 3 != 2:
            continue
        for absolute in (False, True):
            d, blocks = sb.samples_host(absolute=absolute, scene_base=BASE)
            d_in, feats = sb.samples_host(inputs=True, absolute=absolute, scene_base=BASE)
            assert feats.dtype == np.float32 and feats.shape == (len(d), 8, 8, 5) and d_in.tobytes() == d.tobytes()
            for i, e in enumerate(d):
                s = int(e["scene"]) - BASE
                want = ref.input_of(blocks[i], mean[s], std[s])
                assert feats[i].tobytes() == want.tobytes(), (f, s, absolute)
                padded_zero += int((~feats[i].reshape(64, 5).any(axis=1)).any())   # an all-zero row in the input
            n += len(d)
    sb.close()
    assert n > 2 * S
    assert (padded_zero > 0) == sites


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_absolute_is_the_block_without_the_subtraction():
    sb, data = _batch("base")
    trace = _trace("base")
    for f in range(7):
        _step(sb, data, f)
    every = np.ones(S, bool)
    rel, absol = sb.samples_host(scene_base=BASE), sb.samples_host(absolute=True, scene_base=BASE)
    _same(rel, _expect(sb, trace[6], every), "relative")
    _same(absol, _expect(sb, trace[6], every, absolute=True), "absolute")
    assert len(rel[0]) > S // 2 and rel[0].tobytes() == absol[0].tobytes() and rel[1].tobytes() != absol[1].tobytes()
    sb.close()


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_capacity_is_decided_on_the_device_and_nothing_is_written():
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import MmwError
    sb, data = _batch("base")
    assert len(sb.samples_host()[0]) == 0               # no track: nothing, and no error
    sb.samples_dev(None, 0, None, _lib.SAMPLE_BLOCK)
    assert sb.samples_wait(0) == 0
    for f in range(6):
        _step(sb, data, f)
    want_d, want_b = sb.samples_host(scene_base=BASE)
    _same((want_d, want_b), _expect(sb, _trace("base")[5], np.ones(S, bool)), "capacity")
    n = len(want_d)
    assert n > 4
    fill_d, fill_o = np.full(n * 48, 0xA5, np.uint8), np.full(n * 7680, 0x5A, np.uint8)
    b_d, b_o = sb.alloc(fill_d.nbytes).upload(fill_d), sb.alloc(fill_o.nbytes).upload(fill_o)
    for mode, cap in ((_lib.SAMPLE_BLOCK, n - 1), (_lib.SAMPLE_INPUT, n - 1), (_lib.SAMPLE_BLOCK, 0)):
        sb.samples_dev(b_d.ptr if cap else None, cap, b_o.ptr if cap else None, mode, None, 1, BASE)
        with pytest.raises(MmwError) as ei:
            sb.samples_wait(1)
        assert ei.value.code == _lib.E_CAPACITY and ei.value.needed == n
        assert np.array_equal(b_d.download(fill_d.shape, np.uint8), fill_d) and np.array_equal(b_o.download(fill_o.shape, np.uint8), fill_o)
    sb.samples_dev(b_d.ptr, n, b_o.ptr, _lib.SAMPLE_BLOCK, None, 2, BASE)
    assert sb.samples_wait(2) == n
    assert b_d.download((n,), _lib.SAMPLE_ENTRY_DTYPE).tobytes() == want_d.tobytes()
    assert b_o.download((n, 192, 5), np.float64).tobytes() == want_b.tobytes()
    # refused arguments touch nothing
    for bad in (lambda: sb.samples_dev(None, 1, b_o.ptr), lambda: sb.samples_dev(b_d.ptr, 1, None), lambda: sb.samples_dev(b_d.ptr, -1, b_o.ptr),
                lambda: sb.samples_dev(b_d.ptr, 1, b_o.ptr, 4), lambda: sb.samples_dev(b_d.ptr, 1, b_o.ptr, -1),
                lambda: sb.samples_dev(b_d.ptr, 1, b_o.ptr, 0, None, 4), lambda: sb.samples_dev(b_d.ptr, 1, b_o.ptr, 0, None, -1),
                lambda: sb.samples_dev(b_d.ptr, 1, b_o.ptr + 8), lambda: sb.samples_dev(b_d.ptr + 4, 1, b_o.ptr),
                lambda: sb.samples_wait(4), lambda: sb.samples_wait(1)):
        with pytest.raises(MmwError) as ei:
            bad()
        assert ei.value.code == _lib.E_ARG
    b_d.free(); b_o.free()
    sb.close()


# 7 ------------------------------------------------------------------------------------------------------------------------
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
        want.append(b.samples_host(scene_base=BASE))
        _step(b, data, f)
    d_pts = [a.alloc(pts[f].size * 8).upload(pts[f].astype(np.float64)) for f in frames]
    d_cnt = [a.alloc(S * 4).upload(cnt[f]) for f in frames]
    d_dt = [a.alloc(S * 8).upload(dts[f]) for f in frames]
    b_d = [a.alloc(S * 48) for _ in frames]
    b_o = [a.alloc(S * 7680) for _ in frames]
    a.synchronize()
    for k in range(4):
        a.samples_dev(b_d[k].ptr, S, b_o[k].ptr, _lib.SAMPLE_BLOCK, None, k, BASE)
        a.step_dev(d_pts[k].ptr, d_cnt[k].ptr, d_dt[k].ptr)
    for k in (2, 0, 3, 1):
        n = a.samples_wait(k)
        assert n == len(want[k][0]) > 0, k
        assert b_d[k].download((n,), _lib.SAMPLE_ENTRY_DTYPE).tobytes() == want[k][0].tobytes(), k
        assert b_o[k].download((n, 192, 5), np.float64).tobytes() == want[k][1].tobytes(), k
    assert len({w[1].tobytes() for w in want}) == 4   # four different states
    a.check()
    for buf in d_pts + d_cnt + d_dt + b_d + b_o:
        buf.free()
    a.close(); b.close()


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_snapshot_round_trip_into_another_layout():
    a = make_checked(S, N, "track_wise", **CFG_KW)
    data = _inputs("base")
    for f in range(8):   # (8 pushes into 3-frame rings: the source's slots are rotated)
        _step(a, data, f)
    b = make_checked(S, N, "per_scene", **CFG_KW)
    b.restore(a.snapshot())
    for inputs in (False, True):
        da, oa = a.samples_host(inputs=inputs, scene_base=3)
        db, ob = b.samples_host(inputs=inputs, scene_base=3)
        assert len(da) > S // 2 and da.tobytes() == db.tobytes() and oa.tobytes() == ob.tobytes()
    _same(b.samples_host(scene_base=BASE), _expect(b, _trace("base")[7], np.ones(S, bool)), "restored")
    a.close(); b.close()


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_three_experiments_through_one_context(tmp_path):
    """dataset.preprocess_experiments: the golden experiment of tests/test_dataset.py twice (jobs 0 and 2) -- the reference's own
    recording, byte for byte -- around a copy that lost the lines of its first ten frame numbers (job 1), which equals
    `preprocess_experiment` run alone.  The experiments step, pop and idle in different iterations of the same loop."""
    from mmwave_msc_amd import dataset
    gold_dir = os.path.join(os.path.dirname(__file__), "golden")
    gold, off = np.load(os.path.join(gold_dir, "preprocess.npz")), np.load(os.path.join(gold_dir, "offline.npz"))
    csv1 = str(off["csv1"])
    lines = csv1.splitlines(keepends=True)
    first_ten = sorted({int(l.split(",")[0]) for l in lines})[:10]
    cut = "".join(l for l in lines if int(l.split(",")[0]) not in first_ten)
    assert 0 < len(cut) < len(csv1)
    jobs = []
    for j, shard1 in enumerate((csv1, cut, csv1)):
        root = tmp_path / f"job{j}"
        mm = root / "log" / "mmWave" / "A1"
        mm.mkdir(parents=True)
        (mm / "1.csv").write_text(shard1)
        (mm / "2.csv").write_text(str(off["csv2"]))
        kin = root / "log" / "kinect"
        kin.mkdir(parents=True)
        (kin / "A1.csv").write_text(str(gold["kinect_in"]))
        (root / "pre" / "kinect").mkdir(parents=True)
        jobs.append((str(mm), str(kin / "A1.csv"), str(root / "pre" / "mmWave" / "A1"), str(root / "pre" / "kinect" / "A1.csv"),
                     str(root / "A1_centroid.npy")))
    res = dataset.preprocess_experiments(jobs, max_pts=64, inputs=True)
    assert len(res) == 3

    def files(job):
        names = sorted(os.listdir(job[2]), key=lambda x: int(os.path.splitext(x)[0]))
        return names, [open(os.path.join(job[2], f)).read() for f in names]

    for j in (0, 2):
        pairs, invalid, cen, feats = res[j]
        assert np.array_equal(np.array(pairs, dtype=np.int64), gold["pairs"])
        names, txt = files(jobs[j])
        assert names == [str(f) for f in gold["pre_files"]] and txt == [str(t) for t in gold["pre_txt"]], j
        assert open(jobs[j][3], "rb").read().decode() == str(gold["kinect_out"])
        assert np.array_equal(cen, gold["centroids"]) and np.array_equal(np.load(jobs[j][4]), gold["centroids"])
        # the CNN inputs: the reference's, modulo the order inside groups of equal x (np.argsort leaves it open)
        want = gold["fmt_mmwave"]
        assert feats.dtype == np.float32 and feats.shape == want.shape
        # (canon_feat: both sides sorted by x, rows re-ordered inside runs of equal x only)
        assert np.array_equal(feats.reshape(-1, 64, 5)[:, :, 0], want.reshape(-1, 64, 5)[:, :, 0].astype(np.float32))
        assert np.array_equal(canon_feat(feats), canon_feat(want.astype(np.float32)))
    alone = tmp_path / "alone"
    (alone / "kinect").mkdir(parents=True)
    p1, i1, c1 = dataset.preprocess_experiment(jobs[1][0], jobs[1][1], str(alone / "mmWave"), str(alone / "kinect" / "A1.csv"),
                                               centroid_npy=str(alone / "c.npy"), max_pts=64)
    pairs, invalid, cen, feats = res[1]
    assert pairs == p1 and invalid == i1 and np.array_equal(cen, c1) and 0 < len(cen) < len(gold["centroids"])
    assert files(jobs[1]) == files((None, None, str(alone / "mmWave")))
    assert open(jobs[1][3], "rb").read() == open(alone / "kinect" / "A1.csv", "rb").read()
    assert np.array_equal(np.load(jobs[1][4]), np.load(alone / "c.npy")) and len(feats) == len(cen)
    assert res[0][1] != invalid


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_the_cnn_input_of_tied_rows_is_ordered_by_row_position():
    """MMW_SAMPLE_INPUT from the `feature_ties` scene of tests/_edge_inputs.py: the newest frame's rows share a handful of x, some
    of them the centroid's own, and tests/_sample_ref.py's rule -- (all-zero, row position) under a stable sort -- decides every
    byte.  Expected values from the oracle's ring frames and centroid; a sort that breaks ties by the larger row differs on every
    frame (asserted on the expectation)."""
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    from tests import _edge_inputs as ei
    sc = ei.equality_scenes()["feature_ties"].scene
    want_frames = ei.replay(sc)
    sb = SceneBatch(_lib.default_config(**sc.cfg), 1, sc.max_pts)
    mean, std = sb.cfg.intensity_mu, sb.cfg.intensity_std
    for f in range(len(sc.cnt)):
        sb.step_host(sc.pts[f][None], sc.cnt[f: f + 1], sc.dt[f: f + 1])
        w = want_frames[f]
        assert w.n_tracks == 1 and w.tracks["lifetime"][0] == 0
        want = ref.input_of(ref.block_of(w.rings[0], w.tracks["centroid"][0][:2]), mean, std)
        x = want.reshape(64, 5)[:, 0]
        real = want.reshape(64, 5)[:, 2] != 0
        assert real.sum() == min(64, int(sc.cnt[f])) and np.unique(x[real]).size < real.sum() // 2 and np.any(x[real] == 0)
        assert not np.array_equal(ei.ties_by_larger_row(want), want)
        d, feats = sb.samples_host(inputs=True)
        assert len(d) == 1 and feats.shape == (1, 8, 8, 5) and feats.dtype == np.float32
        assert feats[0].view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), f
    sb.close()
