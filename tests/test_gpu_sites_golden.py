"""The recording of the reference under eight sites (tests/golden/sites.npz, scripts/gen_site_golden.py) replayed on the GPU: ONE
context whose scenes carry the recorded sites reproduces the reference's normalize_data bit for bit (fp64 raw rows, and fp32
raw rows where the recorded rows are exactly representable), and its track table carries the fade squares of
utils.fade_squares under each scene's constants (pinned to the recording in tests/test_sites_golden.py), equal after the one
rounding to float32 -- the equality tests/test_gpu_e2e.py uses for that output."""
import numpy as np
import pytest

from tests.test_sites_golden import GOLD, N_SITES, same_bits, site_kw

pytestmark = pytest.mark.gpu


def _ctx(N):
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    g = np.load(GOLD)
    kws = [site_kw(r) for r in g["sites"]]
    sb = SceneBatch(_lib.default_config(tr_max_tracks=4), N_SITES, N)
    sb.set_sites(_lib.make_sites(sb.cfg, N_SITES, **{k: [kw[k] for kw in kws] for k in kws[0]}))
    return g, kws, sb


def test_normalize_under_recorded_sites_fp64_and_fp32():
    g, kws, sb = _ctx(256)
    S, N = N_SITES, 256
    for key_raw, key_norm, f32 in (("raw", "norm", False), ("raw32", "norm32", True)):
        raw = np.zeros((S, N, 5))
        n = np.zeros(S, np.int32)
        for i in range(S):
            r = g[f"{key_raw}_{i}"]
            raw[i, : len(r)], n[i] = r, len(r)
        if not f32:
            pts, n_out = sb.normalize_host(raw, n)
        else:
            r32 = raw.astype(np.float32)
            b_raw = sb.buf("g_raw", r32.nbytes).upload(r32)
            b_n = sb.buf("g_n", S * 4).upload(n)
            b_out, b_no = sb.buf("g_out", S * N * 64), sb.buf("g_no", S * 4)
            sb.normalize_dev(b_raw.ptr, b_n.ptr, b_out.ptr, b_no.ptr, f32=True)
            n_out, pts = b_no.download((S,), np.int32), b_out.download((S, N, 8), np.float64)
        for i in range(S):
            want = g[f"{key_norm}_{i}"]
            assert 0 < len(want) < n[i]                      # the site keeps a row and drops a row
            assert n_out[i] == len(want) and same_bits(pts[i, : n_out[i]], want), (key_raw, i, int(n_out[i]), len(want))
    sb.close()


def test_track_table_fade_squares_under_recorded_sites(monkeypatch):
    from mmwave_msc_amd import constants as const
    from mmwave_msc_amd import utils
    from mmwave_msc_amd.synth import make_batch
    g, kws, sb = _ctx(256)
    S, N, F = N_SITES, 256, 8
    pts, cnt, dts = make_batch(range(60, 60 + S), F, N, 2)
    for f in range(F):
        sb.step_host(pts[f].astype(np.float64), cnt[f], dts[f])
    feat, owner = sb.features_host()
    assert len(owner) >= S
    kp = np.random.default_rng(5).normal(0, 0.5, size=(len(owner), 57)).astype(np.float32)
    sb.set_keypoints_host(kp, owner)
    trk, ntr = sb.tracks(), sb.num_tracks()
    tab = sb.track_table_host(sb.track_cap)
    checked = 0
    for s in range(S):
        for name, key in (("M_X", "m_x"), ("M_Y", "m_y"), ("M_Z", "m_z"), ("V_SCREEN_FADE_SIZE_MAX", "v_screen_fade_size_max"),
                          ("V_SCREEN_FADE_SIZE_MIN", "v_screen_fade_size_min"), ("V_SCREEN_FADE_WEIGHT", "v_screen_fade_weight")):
            monkeypatch.setattr(const, name, kws[s][key])
        assert ntr[s] >= 1
        for j in range(int(ntr[s])):
            px, pz, size = utils.fade_squares(trk[s, j]["x"], trk[s, j]["keypoints"])
            row = tab[s, j]
            assert row["alive"] == 1
            assert row["fade_x"] == np.float32(px) and row["fade_z"] == np.float32(pz) and row["fade_size"] == np.float32(size), (s, j)
            checked += 1
    assert checked >= S
    sb.close()


def test_feature_maps_under_recorded_sites_meet_the_pinned_restatement():
    """mmw_features of one context whose scenes carry the recorded sites: every feature tensor equals, after the one rounding to
    float32, format_single_frame_np -- pinned to the reference's recorded format_single_frame under each site's intensity scale in
    tests/test_sites_golden.py -- of that track's own ring frames, taken relative to its centroid (relative_coordinates,
    Utils.py:455-463), under the SCENE's intensity scale; and not under the context's, where the two differ."""
    from mmwave_msc_amd.synth import make_batch
    from tests._golden import assert_feat_identical
    from tests.test_sites_golden import format_single_frame_np
    g, kws, sb = _ctx(256)
    S, N, F = N_SITES, 256, 8
    pts, cnt, dts = make_batch(range(160, 160 + S), F, N, 2)
    pts = pts.astype(np.float64)
    pts[..., 7] = np.random.default_rng(9).integers(0, 300, size=pts.shape[:-1])   # intensities over 0 .. 300
    for f in range(F):
        sb.step_host(pts[f], cnt[f], dts[f])
    feat, owner = sb.features_host()
    trk = sb.tracks()
    assert set(owner[:, 0].tolist()) == set(range(S)), "every recorded site must own a feature tensor"
    other = 0
    for row, (s, j) in enumerate(owner):
        rec = trk[s, j]
        frames = []
        for k in range(int(rec["ring_len"])):
            fr = sb.track_ring_frame(int(s), int(j), k)
            fr[:, 0] -= rec["centroid"][0]
            fr[:, 1] -= rec["centroid"][1]
            frames.append(fr)
        want = format_single_frame_np(frames, kws[s]["intensity_mu"], kws[s]["intensity_std"]).astype(np.float32)
        assert_feat_identical(feat[row], want, ctx=f"scene {s} track {j}")   # (both sides order ties by row position)
        ctx_scale = format_single_frame_np(frames, sb.cfg.intensity_mu, sb.cfg.intensity_std).astype(np.float32)
        if (kws[s]["intensity_mu"], kws[s]["intensity_std"]) != (sb.cfg.intensity_mu, sb.cfg.intensity_std):
            assert not np.array_equal(ctx_scale, want)
            other += 1
    assert other >= 1
    sb.close()


def test_tied_feature_maps_under_a_scene_intensity_scale():
    """k_features_site on the `feature_ties` scene of tests/_edge_inputs.py (rows of equal x, rows on the centroid's x): two scenes
    fed the same frames, scene 0 under the context's intensity scale and scene 1 under its own.  After every frame each feature
    tensor equals, bit for bit, format_frames_ref of the ORACLE's ring frames and centroid under the scene's scale; scene 0's is
    the oracle's own tensor, and scene 1's differs from it in the intensity column alone -- the same tied order."""
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    from tests import _edge_inputs as ei
    from tests._golden import assert_feat_identical
    from tests._sort_inputs import MU, STD, format_frames_ref
    sc = ei.equality_scenes()["feature_ties"].scene
    want_frames = ei.replay(sc)
    S = 2
    sb = SceneBatch(_lib.default_config(**sc.cfg), S, sc.max_pts)
    mu, std = [sb.cfg.intensity_mu, MU], [sb.cfg.intensity_std, STD]
    assert (mu[0], std[0]) != (mu[1], std[1])
    sb.set_sites(_lib.make_sites(sb.cfg, S, intensity_mu=mu, intensity_std=std))
    assert sb.has_sites
    ring, seen = sb.ring, 0
    for f in range(len(sc.cnt)):
        sb.step_host(np.stack([sc.pts[f]] * S), np.full(S, sc.cnt[f], np.int32), np.full(S, sc.dt[f]))
        feat, owner = sb.features_host()
        w = want_frames[f]
        assert owner.tolist() == [[s, 0] for s in range(S) for _ in w.owner], f
        if len(owner) == 0:
            continue
        frames, counts = np.zeros((1, ring, 64, 8)), np.full((1, ring), -1, np.int32)
        for k, rows in enumerate(w.rings[0]):
            m = min(64, len(rows))
            frames[0, k, :m], counts[0, k] = rows[:m], w.tracks["ring_n"][0][k]
        for s in range(S):
            want = format_frames_ref(frames, counts, w.tracks["centroid"][0][:2], mu[s], std[s], ring)
            assert_feat_identical(feat[s].reshape(ring, 64, 5), want[0], ctx=f"frame {f} scene {s}")
        assert_feat_identical(feat[0], w.feat[0], ctx=f"frame {f}: the context's scale is the oracle's")
        assert np.array_equal(feat[1][..., :4], feat[0][..., :4]) and not np.array_equal(feat[1][..., 4], feat[0][..., 4])
        assert not np.array_equal(ei.ties_by_larger_row(w.feat[0]), w.feat[0])
        seen += 1
    assert seen == 3
    sb.close()
