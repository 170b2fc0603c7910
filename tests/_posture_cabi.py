"""Shared by test_posture_cabi_exports.py (CPU) and test_gpu_posture_cabi.py (GPU): the scenario the batched estimate_posture of
the C-ABI is run on, and its reference -- oracle.c_oracle for the tracker and the feature tensors, oracle/mars_np.py (fp64) for
the CNN.  Nothing here touches a GPU or torch."""
import numpy as np

KW = dict(tr_max_tracks=4, tr_lifetime_dynamic=0.25, tr_lifetime_static=0.25)   # short lifetimes: tracks expire inside 12 frames
F_STEPS, N_PTS = 12, 128
MARK = 12345.0
# what oracle_run gives on scenario(48) at FB_FRAMES_BATCH = 0 (the single-frame model), pinned: eligible tracks per frame, scenes
# tracked by frame 4, scene-frames in which a track expired, surviving CNN samples
SINGLE_FRAME_48 = dict(rows=[64, 70, 71, 72, 72, 96, 96, 72, 72, 72, 72, 72], tracked_by_4=48, expired=16, samples_cnn=72)


def scenario(S, seed=5000, F=F_STEPS, N=N_PTS):
    """pts[F, S, N, 8] fp64, cnt[F, S] int32, dt[F, S]: synth scenes of one or two people; in every third scene everybody is
    10 m further along x from frame 5 on (the old tracks find no point, expire three frames later and the list is compacted
    while new tracks are spawned), in every fifth the frame counts are ragged."""
    from mmwave_msc_amd.synth import make_scene
    ps, cs, ds = [], [], []
    for s in range(S):
        p, c, d = make_scene(seed + s, F, N, 1 + s % 2, ragged=(s % 5 == 0))
        if s % 3 == 0:
            for f in range(5, F):
                p[f, : c[f], 0] += np.float32(10.0)
        ps.append(p); cs.append(c); ds.append(d)
    return np.ascontiguousarray(np.stack(ps, 1)).astype(np.float64), np.ascontiguousarray(np.stack(cs, 1)), np.ascontiguousarray(np.stack(ds, 1))


def dense2_fp64(w, hidden):
    """Dense-2 of define_CNN_3D (train.py:92) with its BatchNormalization in front, in fp64, on the hidden layer `hidden`[n][1536]
    (Dense-1's relu output): the last two lines of oracle.mars_np._forward."""
    from oracle.mars_np import _bn
    w64 = {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}
    h = _bn(np.asarray(hidden, dtype=np.float64), w64["bn2_gamma"], w64["bn2_beta"], w64["bn2_mean"], w64["bn2_var"])
    return h @ w64["dense2_w"] + w64["dense2_b"]


def hidden_fp64(w, x):
    """The hidden layer of oracle.mars_np (relu of Dense-1), fp64: mars_np._forward up to its last two lines."""
    from oracle.mars_np import _bn, _conv_same
    w64 = {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}
    h = np.asarray(x, dtype=np.float64)
    h = np.maximum(_conv_same(h, w64["conv1_w"], w64["conv1_b"]), 0.0)
    h = np.maximum(_conv_same(h, w64["conv2_w"], w64["conv2_b"]), 0.0)
    h = _bn(h, w64["bn1_gamma"], w64["bn1_beta"], w64["bn1_mean"], w64["bn1_var"])
    h = h.reshape(h.shape[0], -1)
    return np.maximum(h @ w64["dense1_w"] + w64["dense1_b"], 0.0)


def oracle_run(pts, cnt, dts, weights, cfg_kw=None):
    """The reference loop (offline_main.py:53-60) per scene on the C oracle: track -> estimate_posture every frame.  The CNN is a
    pure function of the feature tensor, so every tensor is stored, the track tagged with its index, and the fp64 CNN evaluated at
    the end for the tensor each surviving track was tagged with last (bench_e2e.oracle_reference's scheme).
    Returns finals[S] (track records), want_kp[S] ([n_tracks][57] fp64), rows[F] (eligible tracks per frame), feats[F] / owners[F]
    (the frame's tensors and (scene, track) rows), tracked_by_4 (scenes holding a track after frame 4), expired (scene-frames in
    which the track list got shorter)."""
    from oracle import c_oracle as co
    from oracle.mars_np import mars_forward_np
    F, S = cnt.shape
    cfg = co.default_config(**(cfg_kw if cfg_kw is not None else KW))
    scenes = [co.OracleScene(cfg, pts.shape[2]) for _ in range(S)]
    store, rows, feats, owners = [], [], [], []
    last_n, expired = [0] * S, 0
    tracked_by_4 = 0
    for f in range(F):
        n_f, feat_f, own_f = 0, [], []
        for s, sc in enumerate(scenes):
            c = int(cnt[f, s])
            if c > 0:
                sc.track(pts[f, s, :c], float(dts[f, s]))
            feat, owner = sc.features()
            if len(owner):
                tag = np.zeros((len(owner), 57), dtype=np.float32)
                tag[:, 0] = np.arange(len(store), len(store) + len(owner), dtype=np.float32)
                tag[:, 1] = MARK
                store.extend(feat)
                sc.set_keypoints(tag, owner)
                feat_f.append(feat)
                own_f.extend((s, int(j)) for j in owner)
            n_f += len(owner)
            expired += sc.n_tracks < last_n[s]   # the list got shorter: _maintain_tracks dropped a track this frame
            last_n[s] = sc.n_tracks
        rows.append(n_f)
        feats.append(np.concatenate(feat_f) if feat_f else np.zeros((0, 3, 8, 8, 5), np.float32))
        owners.append(np.array(own_f, dtype=np.int32).reshape(-1, 2))
        if f == 4:
            tracked_by_4 = sum(sc.n_tracks > 0 for sc in scenes)
    assert len(store) < (1 << 24)
    finals = [sc.tracks() for sc in scenes]
    need = sorted({int(r["keypoints"][0]) for fin in finals for r in fin if r["keypoints"][1] == MARK})
    kp_of = {}
    for i in range(0, len(need), 256):
        idx = need[i:i + 256]
        kp_of.update(zip(idx, mars_forward_np(weights, np.stack([store[j] for j in idx]).astype(np.float64))))
    default = np.array(list(cfg.default_posture), dtype=np.float64)
    want_kp = [np.stack([kp_of[int(r["keypoints"][0])] if r["keypoints"][1] == MARK else default for r in fin]) if len(fin) else np.zeros((0, 57))
               for fin in finals]
    return {"finals": finals, "want_kp": want_kp, "rows": rows, "feats": feats, "owners": owners, "tracked_by_4": tracked_by_4,
            "expired": expired, "samples_cnn": len(need)}


STATE_FIELDS = ("x", "P", "centroid", "spread_est", "group_disp_est", "lifetime", "point_num", "is_static", "ring_n")


def kp_err(got, want):
    """max |got - want| / max(1, |want|): the keypoint tolerance of SURVEY.md section 8c is 1e-4 of it."""
    want = np.asarray(want, dtype=np.float64)
    if want.size == 0:
        return 0.0
    return float((np.abs(np.asarray(got, dtype=np.float64) - want) / np.maximum(1.0, np.abs(want))).max())
