"""Scene snapshots on the GPU (include/mmw.h, mmw_snapshot / mmw_restore; k_snapshot.hip).

1. continue-equivalence: a run snapshotted at frame k and restored into a fresh context of another size, another scene
   mapping and each other kernel layout continues bit for bit with the uninterrupted run and with the C oracle;
2. the double-prediction trap: scenes restored over live scenes of a track-wise context, right after those were in the last
   update lists and spawned tracks, are predicted once;
3. canonical bytes: four layouts give one snapshot, and snapshot -> restore -> snapshot gives it back;
4. refusals leave every scene as it was;
5. a drained PosturePipeline's context continues with the CNN after a restore, keypoints bit-equal;
6. the drop-in TrackBuffer / BatchedData pickle and deep-copy mid-run;
7. the new kernels spill nothing."""
import copy
import os
import pickle

import numpy as np
import pytest

from tests._fuzz import draw_case, plant_nonfinite, scene_inputs
from tests._layouts import LAYOUTS, make_checked

pytestmark = pytest.mark.gpu


def _step(sb, pts, cnt, dts, S_ctx, where):
    """One frame for the context's scenes `where` (list of slots): the other slots skip the frame."""
    N = sb.max_pts
    P = np.zeros((S_ctx, N, 8))
    n = np.zeros(S_ctx, np.int32)
    d = np.full(S_ctx, 0.1)
    for i, s in enumerate(where):
        P[s, : pts.shape[1]] = pts[i]
        n[s], d[s] = cnt[i], dts[i]
    assoc, labels, dbn = sb.step_host(P, n, d, raise_nonfinite=False, check=False)
    # (what a frame defines: the association of its rows, the labels of the DBSCAN call it made, the call's size)
    return [(assoc[s, : max(int(n[s]), 0)].tobytes(), labels[s, : max(int(dbn[s]), 0)].tobytes(), int(dbn[s])) for s in where]


def _state(sb, where):
    """Everything a scene holds, per slot in `where`, in a comparable form."""
    out = []
    err = sb.errors()
    ntr = sb.num_tracks()
    trk = sb.tracks()
    ln, rn = sb.batch_ring()
    table = sb.track_table_host(sb.track_cap)
    for s in where:
        T = int(ntr[s])
        rings = [sb.batch_ring_frame(s, k).tobytes() for k in range(int(ln[s]))]
        for j in range(T):
            rings += [sb.track_ring_frame(s, j, k).tobytes() for k in range(int(trk[s, j]["ring_len"]))]
        tb = table[s].copy()
        tb["scene"] = 0
        out.append((int(err[s]), T, trk[s, :T].tobytes(), int(ln[s]), rn[s].tobytes(), tuple(rings), tb.tobytes()))
    return out


def _frames(case, nonfinite=False):
    pts, cnt, dts = scene_inputs(case)
    if nonfinite:
        plant_nonfinite(case, pts, cnt)
    return pts.astype(np.float64), cnt, dts


# (seed, k = the frame after which the snapshot is taken, non-finite rows planted, scene 0's global ring resized): rings not yet
# full at k = 0, 1, 2; ring 1..4; seed 5 runs seek_inner_clusters; clean, unresized cases for every layout (9, 25)
CONT_CASES = [(9, 5, False, False), (25, 1, False, False), (5, 2, False, False), (3, 0, False, True), (18, 4, True, False),
              (47, 3, True, True)]


@pytest.mark.parametrize("layout_b", LAYOUTS)
@pytest.mark.parametrize("seed,k,nonfinite,resize", CONT_CASES)
def test_continue_equivalence(seed, k, nonfinite, resize, layout_b):
    from mmwave_msc_amd import _lib
    from oracle import c_oracle as co
    from tests._golden import assert_tracks_match
    case = draw_case(seed, max_pts=320, max_scenes=4, frames=9)
    kw, S, N, F = case["cfg"], case["S"], case["N"], case["F"]
    assert not (resize and (kw.get("seek_inner") or kw["fb_frames_batch"] < 1)), "a resize case needs a ring of 2 or more"
    if resize and layout_b == "one_workgroup":
        # (a restored resized ring sets var_ring: the context then runs the bulk kernels, not the one-workgroup step it was
        #  created with -- that combination would repeat another parametrisation's kernels under this one's name)
        pytest.skip("one_workgroup: a resized ring runs the bulk kernels after the restore")
    pts, cnt, dts = _frames(case, nonfinite=nonfinite)
    cnt[k, 0] = 0                                             # a skipped frame and an empty cloud right before the snapshot
    if S > 1:
        cnt[k, 1] = -1
    # A runs other kernels than B where the configuration has two layouts (seek_inner has only the per-scene one)
    A = make_checked(S, N, "per_scene" if kw.get("seek_inner") or layout_b == "track_wise" else "track_wise", **kw)
    ring = A.ring
    if resize:
        A.set_batch_size(ring - 1, [0])                       # BatchedData.change_buffer_size on scene 0
    A_out = []
    for f in range(F):
        A_out.append(_step(A, pts[f], cnt[f], dts[f], S, list(range(S))))
        if f == k:
            blob = A.snapshot()
            A_state_k = _state(A, list(range(S)))
    A_final = _state(A, list(range(S)))
    A.close()
    # B: another scene count, a permuted mapping, another layout (its other slots stay empty: they skip every frame)
    SB = S + 3
    perm = [int(v) for v in np.random.default_rng(seed).permutation(SB)[:S]]
    B = make_checked(SB, N, layout_b, **kw)
    B.restore(blob, perm)
    assert _state(B, perm) == A_state_k
    B_out = {}
    for f in range(k + 1, F):
        B_out[f] = _step(B, pts[f], cnt[f], dts[f], SB, perm)
        assert B_out[f] == A_out[f], (seed, layout_b, f)
    assert _state(B, perm) == A_final, (seed, layout_b)
    # the uninterrupted C oracle agrees with B on the restored scenes: every frame's association and DBSCAN call, and the
    # final tracks -- per scene up to the first frame on which the reference raises something other than sklearn's ValueError
    cfg = co.default_config(**kw)
    orc = [co.OracleScene(cfg, N) for _ in range(S)]
    if resize:
        orc[0].set_batch_size(ring - 1)
    live, compared = [True] * S, 0
    for f in range(F):
        for s in range(S):
            c = int(cnt[f, s])
            if c == 0 or not live[s]:
                continue
            raised = False
            try:
                oa, ol = orc[s].track(pts[f, s, : max(c, 0)], float(dts[f, s]))
            except co.OracleNonFinite:
                oa, ol, raised = orc[s].last_assoc, None, True
            except RuntimeError:
                live[s] = False
                continue
            if f > k:
                ga, gl, gn = B_out[f][s]
                assert ga == np.asarray(oa, np.int32).tobytes(), (seed, layout_b, f, s)
                if raised:
                    assert gn == _lib.DB_RAISED, (seed, layout_b, f, s, gn)
                else:
                    assert (ol is None) == (gn < 0), (seed, layout_b, f, s)
                    assert ol is None or gl == np.asarray(ol, np.int32).tobytes(), (seed, layout_b, f, s)
                compared += 1
    ntr, trk = B.num_tracks(), B.tracks()
    for s in range(S):
        if live[s]:
            assert int(ntr[perm[s]]) == orc[s].n_tracks, (seed, layout_b, s)
            assert_tracks_match(trk[perm[s], : ntr[perm[s]]], orc[s].tracks(), ctx=f"seed {seed} {layout_b} s{s}", exact=True)
    assert compared > 0, "no restored frame was compared with the oracle"
    B.close()


def _synthetic(seed, S, F, N):
    from mmwave_msc_amd.synth import make_batch
    pts, cnt, dts = make_batch(range(seed, seed + S), F, N, 3)
    return pts.astype(np.float64), cnt, dts


def test_restore_into_live_slots_predicts_once():
    """Scenes 4..7 of a track-wise context are in the last update lists and have just spawned tracks; scenes of another
    context are restored over them.  The restored scenes must continue as their uninterrupted run, the others as theirs."""
    S, N, F, k = 8, 256, 10, 3
    X_in = _synthetic(100, S, F, N)
    Y_in = _synthetic(300, 4, F, N)
    X = make_checked(S, N, "track_wise", tr_max_tracks=8)
    Xr = make_checked(S, N, "track_wise", tr_max_tracks=8)       # X uninterrupted
    Y = make_checked(4, N, "track_wise", tr_max_tracks=8)        # the restored scenes uninterrupted
    for f in range(k + 1):
        _step(X, X_in[0][f], X_in[1][f], X_in[2][f], S, list(range(S)))
        _step(Xr, X_in[0][f], X_in[1][f], X_in[2][f], S, list(range(S)))
        _step(Y, Y_in[0][f], Y_in[1][f], Y_in[2][f], 4, list(range(4)))
    assert (X.num_tracks()[4:] > 0).all() and (Y.num_tracks() > 0).all()
    X.restore(Y.snapshot(), [4, 5, 6, 7])
    for f in range(k + 1, F):
        P = np.concatenate([X_in[0][f][:4], Y_in[0][f]]); n = np.concatenate([X_in[1][f][:4], Y_in[1][f]])
        d = np.concatenate([X_in[2][f][:4], Y_in[2][f]])
        got = _step(X, P, n, d, S, list(range(S)))
        ry = _step(Y, Y_in[0][f], Y_in[1][f], Y_in[2][f], 4, list(range(4)))
        rx = _step(Xr, X_in[0][f], X_in[1][f], X_in[2][f], S, list(range(S)))
        assert got[:4] == rx[:4], f
        assert got[4:] == ry, f
        assert _state(X, [4, 5, 6, 7]) == _state(Y, [0, 1, 2, 3]), f
        assert _state(X, [0, 1, 2, 3]) == _state(Xr, [0, 1, 2, 3]), f
    for c in (X, Xr, Y):
        c.close()


# (seed, frames, non-finite rows): ring 1 (7, 26) and rings of 3 that wrap several times, with planted NaN / inf rows (9, 47): the
# physical slots of the global and the track rings have rotated, the non-finite flags sit on non-identity slots
@pytest.mark.parametrize("seed,frames,nonfinite", [(7, 7, False), (26, 7, False), (9, 11, True), (47, 11, True)])
def test_snapshots_are_canonical(seed, frames, nonfinite):
    case = draw_case(seed, max_pts=256, max_scenes=4, frames=frames)
    kw, S, N, F = case["cfg"], case["S"], case["N"], case["F"]
    kw = dict(kw, seek_inner=0)
    kw.pop("fb_frames_batch_static", None)
    pts, cnt, dts = _frames(dict(case, seek_inner=False), nonfinite=nonfinite)
    if nonfinite:
        assert kw["fb_frames_batch"] + 1 >= 3 and F > 2 * (kw["fb_frames_batch"] + 1)
        ring = kw["fb_frames_batch"] + 1
        assert any((~np.isfinite(pts[f, s, : max(int(cnt[f, s]), 0)])).any() for f in range(F - ring, F) for s in range(S))
    blobs = {}
    for layout in LAYOUTS:
        try:
            sb = make_checked(S, N, layout, **kw)
        except pytest.skip.Exception:
            continue
        for f in range(F):
            _step(sb, pts[f], cnt[f], dts[f], S, list(range(S)))
        blobs[layout] = sb.snapshot()
        # snapshot -> restore -> snapshot
        sb2 = make_checked(S, N, layout, **kw)
        sb2.restore(blobs[layout])
        assert sb2.snapshot() == blobs[layout], layout
        sb.close()
        sb2.close()
    assert len(blobs) >= 3
    if nonfinite:   # the flags of the rings' non-finite rows are in the blob, on logical frames
        from mmwave_msc_amd import snapshot
        b = next(iter(blobs.values()))
        flags = [int(np.frombuffer(b, np.int32, 16, int(o))[15]) >> 16 for o in snapshot.inspect(b)["entries"]["offset"]]
        assert any(flags), flags
    first = _layout_free(next(iter(blobs.values())))
    for layout, b in blobs.items():
        assert _layout_free(b) == first, layout


def _layout_free(blob):
    """The blob with the header's copy of the mmw_config fields that only choose kernels (the layout) zeroed: the source's
    configuration is stored verbatim, everything else must be the same bytes whatever kernels produced the state."""
    import ctypes as C
    from mmwave_msc_amd import _lib
    b = bytearray(blob)
    base = _lib.MmwSnapshotHeader.config.offset
    for name in ("kalman_dense_min_units", "chain_side_stream", "fused_step"):
        off = base + getattr(_lib.MmwConfig, name).offset
        b[off: off + 4] = bytes(4)
    return bytes(b)


def test_refused_restores_change_nothing():
    from mmwave_msc_amd import _lib
    S, N, F = 4, 128, 5
    pts, cnt, dts = _synthetic(500, S, F, N)
    src = make_checked(S, N, "per_scene", tr_max_tracks=8)
    for f in range(F):
        _step(src, pts[f], cnt[f], dts[f], S, list(range(S)))
    assert src.num_tracks().max() >= 2
    src.set_batch_frame(0, np.random.default_rng(0).uniform(-1, 1, (20, 8)))   # BatchedData(init_data): a 20-row global frame
    blob = src.snapshot()
    from mmwave_msc_amd import snapshot
    big = int(snapshot.inspect(blob)["entries"]["max_g_rows"].max())   # the largest frame the source's global rings hold
    assert big >= 20
    base = dict(tr_max_tracks=8)
    targets = [
        (dict(base, db_eps=0.31), N, [0, 1, 2, 3], "db_eps"),
        (dict(base, dim_x=6), N, [0, 1, 2, 3], "dim_x"),
        (dict(base, fb_frames_batch=1), N, [0, 1, 2, 3], "fb_frames_batch"),
        (dict(base, track_cap=1), N, [0, 1, 2, 3], "tracks"),
        (base, big - 1, [0, 1, 2, 3], "max_pts"),
        (base, N, [0, 1, 1, 3], "twice"),
    ]
    wrong = []
    for kw, npts, where, what in targets:
        T = make_checked(6, npts, "per_scene", **kw)
        for f in range(2):
            _step(T, pts[f, :, :npts], np.minimum(cnt[f], npts), dts[f], 6, [0, 1, 2, 3])
        before = T.snapshot()
        try:
            T.restore(blob, where)
            wrong.append((what, "accepted"))
        except _lib.MmwError as e:
            if e.code != _lib.E_ARG or what not in str(e):
                wrong.append((what, str(e)))
        if T.snapshot() != before:
            wrong.append((what, "state changed"))
        T.close()
    assert not wrong, wrong
    src.close()


def _posture_run(sb, pipe, d_pts, d_cnt, d_dt, frames):
    for f in frames:
        sb.step_dev(d_pts[f].data_ptr(), d_cnt[f].data_ptr(), d_dt[f].data_ptr())
        pipe.after_step()


def test_posture_pipeline_continues_after_restore():
    """A PosturePipeline (the CNN every frame, keypoints scattered one or two frames behind: tests/test_gpu_e2e.py) is drained,
    its context snapshotted and restored into another context with a pipeline of its own; both continue with the CNN.  The
    tracker state and the keypoints -- the only posture state a scene holds -- stay bit-equal."""
    import torch
    from mmwave_msc_amd.mars import MarsCNN, random_keras_weights
    from mmwave_msc_amd.posture import PosturePipeline
    from mmwave_msc_amd.synth import make_batch
    S, N, F, k = 8, 256, 12, 5
    pts, cnt, dts = make_batch(range(900, 900 + S), F, N, 3)
    model = MarsCNN.from_keras_weights(random_keras_weights(3, 3)).to("cuda:0")
    dev = torch.device("cuda", 0)
    A = make_checked(S, N, "per_scene", tr_max_tracks=4)
    pA = PosturePipeline(A, model, S * A.track_cap, overlap=True)
    with torch.cuda.stream(pA.A):
        d_pts = torch.from_numpy(pts).to(dev).double()
        d_cnt = torch.from_numpy(cnt).to(dev)
        d_dt = torch.from_numpy(dts).to(dev)
    pA.A.synchronize()
    _posture_run(A, pA, d_pts, d_cnt, d_dt, range(k + 1))
    pA.drain()                                    # (the documented order: the pipeline's scatters land before the snapshot)
    blob = A.snapshot()
    t_k = A.tracks()
    assert (A.num_tracks() > 0).all()
    assert not np.array_equal(t_k[0, 0]["keypoints"], np.asarray(A.cfg.default_posture, np.float32)), "the CNN has not run"
    B = make_checked(S, N, "track_wise", tr_max_tracks=4)
    B.restore(blob)
    pB = PosturePipeline(B, model, S * B.track_cap, overlap=True)
    assert B.tracks().tobytes() == t_k.tobytes()
    _posture_run(A, pA, d_pts, d_cnt, d_dt, range(k + 1, F))
    _posture_run(B, pB, d_pts, d_cnt, d_dt, range(k + 1, F))
    pA.close()
    pB.close()
    A.check()
    B.check()
    ta, tb = A.tracks(), B.tracks()
    assert np.array_equal(A.num_tracks(), B.num_tracks())
    assert ta.tobytes() == tb.tobytes()           # every field, the keypoints included, bit for bit
    assert not np.array_equal(ta["keypoints"], t_k["keypoints"]), "no keypoint changed after the restore"
    A.close()
    B.close()
    torch.cuda.synchronize()


def test_pickle_and_deepcopy_of_the_dropin_mid_run(tmp_path):
    from tests._golden import GOLDEN
    from mmwave_msc_amd.tracking import BatchedData, TrackBuffer
    from mmwave_msc_amd.utils import OfflineManager
    z = np.load(os.path.join(GOLDEN, "offline.npz"))
    (tmp_path / "1.csv").write_text(str(z["csv1"]))
    (tmp_path / "2.csv").write_text(str(z["csv2"]))
    frames = []
    om = OfflineManager(str(tmp_path))
    while not om.is_finished():
        ok, _, det = om.get_data()
        if ok:
            frames.append(det)
    assert len(frames) > 10
    half = len(frames) // 2

    def run(tb, batch, dets, t0):
        out = []
        for i, det in enumerate(dets):
            tb.dt = 0.1 if (t0 + i) == 0 else det["posix"][0] / 1000 - tb.t
            tb.t = det["posix"][0] / 1000
            n = tb.track_raw(det, batch)
            out.append((n, None if tb.last_assoc is None else tb.last_assoc.tobytes(), len(tb.effective_tracks),
                        tuple((t.uid, t.state.x.tobytes(), t.lifetime) for t in tb.effective_tracks)))
        return out

    tb, batch = TrackBuffer(max_pts=64), BatchedData()
    run(tb, batch, frames[:half], 0)
    tb2, batch2 = pickle.loads(pickle.dumps((tb, batch)))
    assert tb2._batch is batch2 and batch2._owner is tb2 and tb2._fused_model is None
    tb3 = copy.deepcopy(tb)
    batch3 = tb3._batch
    a = run(tb, batch, frames[half:], half)
    b = run(tb2, batch2, frames[half:], half)
    assert a == b
    # the deep copy is a tracker of its own: it did not move while the others ran, and continues as they did
    c = run(tb3, batch3, frames[half:], half)
    assert c == a
    for t in (tb, tb2, tb3):
        t.close()


def test_snapshot_kernels_compile_without_scratch():
    import re
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mmwave_msc_amd", "csrc", "k_snapshot.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    assert len([n for n in names if "k_snap_" in n]) == 6, names
    assert all(v == "0" for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)), r.stderr
    assert all(v == "0" for v in re.findall(r"VGPRs Spill: (\d+)", r.stderr)), r.stderr
