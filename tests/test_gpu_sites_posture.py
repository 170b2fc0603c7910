"""Per-scene sites through the posture entries: the on-device chain of an attached model (mmw_frame_posture_host: its own
k_features launch inside the frame) and PosturePipeline (mmw_features_async).  The feature maps carry the scene's intensity
scale, so the keypoints the CNN writes into the tracks -- and the track-table rows that show them -- must be those of a context
created with the site as its configuration, bit for bit, and must differ from those of the context's own configuration."""
import numpy as np
import pytest

from tests.test_gpu_sites import KW, SITES, _inputs, _model, _site_rows, _tracks_bytes

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k", [1, 4, 5])   # the sites whose intensity scale is not the default
def test_attached_model_chain_uses_the_scenes_site(k):
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    N, F = 256, 12
    raw, cnt, dts, which = _inputs(6, N, F, seed=2100)
    assert which[k] == k
    raw, cnt, dts = raw[:, k: k + 1], cnt[:, k: k + 1], dts[:, k: k + 1]   # one scene: a radar mounted as SITES[k]
    model = _model()
    site = SITES[k]
    mount = {key: site[key] for key in ("s_height", "s_tilt")}
    ctxs = {"site": SceneBatch(_lib.default_config(**KW), 1, N), "twin": SceneBatch(_lib.default_config(**KW, **site), 1, N),
            "mount_only": SceneBatch(_lib.default_config(**KW, **mount), 1, N)}   # (the same mounting, the default intensity scale)
    ctxs["site"].set_sites(_site_rows(ctxs["site"].cfg, [site]))
    got = {}
    for name, sb in ctxs.items():
        sb.attach_posture(model)
        rows = []
        for f in range(F):
            o = sb.frame_host(cnt[f], dts[f], raw=raw[f], posture=True)
            rows.append((o["posture_rows"], o["n_out"].tobytes(), o["assoc"][0, : o["n_out"][0]].tobytes(), o["n_tracks"].tobytes()))
        got[name] = (rows, _tracks_bytes(sb, [0]), sb.track_table_host(sb.track_cap).tobytes(), sb.tracks()[0, : int(sb.num_tracks()[0])]["keypoints"].copy())
        sb.close()
    assert sum(r[0] for r in got["site"][0]) >= F // 2, "the chain must have estimated postures"
    assert got["site"][:3] == got["twin"][:3]
    # not vacuous: with the context's own intensity scale the keypoints are others (the tracker's integers are the same)
    assert got["mount_only"][0] == got["site"][0]
    assert got["mount_only"][3].shape == got["site"][3].shape and not np.array_equal(got["mount_only"][3], got["site"][3])


def test_posture_pipeline_over_a_mixed_context_equals_uniform_contexts():
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    from mmwave_msc_amd.posture import PosturePipeline
    S, N, F = 12, 256, 10
    raw, cnt, dts, which = _inputs(S, N, F, seed=2300)
    model = _model()

    def run(sb):
        pipe = PosturePipeline(sb, model, S * sb.track_cap, overlap=False)
        b_pts, b_no = sb.buf("p_pts", S * N * 64), sb.buf("p_no", S * 4)
        for f in range(F):
            b_raw = sb.buf("p_raw", raw[f].nbytes).upload(raw[f])
            b_n = sb.buf("p_n", S * 4).upload(cnt[f])
            b_dt = sb.buf("p_dt", S * 8).upload(dts[f])
            sb.normalize_dev(b_raw.ptr, b_n.ptr, b_pts.ptr, b_no.ptr)
            sb.step_dev(b_pts.ptr, b_no.ptr, b_dt.ptr)
            pipe.after_step()
            sb.synchronize()   # (the input buffers are rewritten by the next frame's uploads)
        pipe.close()
        sb.check()
        table = sb.track_table_host(sb.track_cap)
        out = (_tracks_bytes(sb, range(S)), [table[s].tobytes() for s in range(S)], pipe.rows_total)
        sb.close()
        return out

    mixed = SceneBatch(_lib.default_config(**KW), S, N)
    mixed.set_sites(_site_rows(mixed.cfg, [SITES[w] for w in which]))
    m_trk, m_tab, m_rows = run(mixed)
    assert m_rows >= S
    differs = 0
    for k, site in enumerate(SITES):
        u_trk, u_tab, _ = run(SceneBatch(_lib.default_config(**KW, **site), S, N))
        for s in range(S):
            if which[s] == k:
                assert len(m_trk[s]) > 0 and m_trk[s] == u_trk[s] and m_tab[s] == u_tab[s], (k, s)
            else:
                differs += m_tab[s] != u_tab[s]
    assert differs >= S   # scenes under another site's configuration come out differently
