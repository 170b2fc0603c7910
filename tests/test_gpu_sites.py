"""Per-scene site parameters on the GPU (include/mmw.h: mmw_set_sites; csrc/k_misc.hip: the k_*_site kernels).

A context whose scenes carry different sites -- sensor mounting, intensity scale, window / monitoring point -- must give every
scene exactly what a context created with that site as its mmw_config gives it (today's path), and what the C oracle gives for
that configuration.  Every comparison here is bit for bit: the site kernels run the same arithmetic as the kernels of a context
without sites, on the scene's values instead of the context's."""
import ctypes as C

import numpy as np
import pytest

from tests._layouts import LAYOUTS, make_checked

pytestmark = pytest.mark.gpu

# six installations; neighbouring scenes of the mixed context differ in every group of fields
SITES = [
    dict(s_height=1.8, s_tilt=-5.0),                                                        # the default mounting
    dict(s_height=0.6, s_tilt=12.5, intensity_mu=40.0, intensity_std=55.5),
    dict(s_height=2.9, s_tilt=-35.0, m_x=-0.5, m_y=-1.25, m_z=0.9),
    dict(s_height=1.25, s_tilt=-5.0000001, v_screen_fade_size_max=0.5, v_screen_fade_size_min=0.1, v_screen_fade_weight=0.02),
    dict(s_height=2.2, s_tilt=-20.0, intensity_mu=0.0, intensity_std=1.0, m_x=1.0, m_y=-0.3, m_z=2.0),
    dict(s_height=1.5, s_tilt=3.0, intensity_mu=120.0, intensity_std=300.0, v_screen_fade_weight=0.2),
]
KW = dict(tr_max_tracks=4)


def _orc_cfg(site):
    """The C oracle's configuration for a site: it knows the mounting and the intensity scale (the window is not part of it)."""
    from oracle import c_oracle as co
    return co.default_config(**{k: v for k, v in site.items() if k in ("s_height", "s_tilt", "intensity_mu", "intensity_std")}, **KW)


def _site_rows(cfg, kws):
    """SITE_DTYPE rows for a list of site dicts (each over `cfg`)."""
    from mmwave_msc_amd import _lib
    return np.concatenate([_lib.make_sites(cfg, 1, **kw) for kw in kws])


def _raw_for(pts, site):
    """Room-frame rows [.., 8] -> the raw sensor rows [.., 5] of a radar mounted as `site`: the inverse of normalize_data's
    transform (subtract the height, rotate by +tilt).  It need not invert to the bit: every context is fed the same raw rows."""
    a = np.radians(site["s_tilt"])
    c, s = np.cos(a), np.sin(a)
    y, z = pts[..., 1].astype(np.float64), pts[..., 2].astype(np.float64) - site["s_height"]
    raw = np.zeros(pts.shape[:-1] + (5,))
    raw[..., 0] = pts[..., 0]
    raw[..., 1] = c * y + s * z
    raw[..., 2] = -s * y + c * z
    raw[..., 3] = pts[..., 6]
    return raw


def _inputs(S, N, F, seed=900):
    """raw[F, S, N, 5], cnt[F, S], dt[F, S], site index per scene (interleaved: scene s has site s % 6)."""
    from mmwave_msc_amd.synth import make_batch
    which = np.arange(S) % len(SITES)
    raw = np.zeros((F, S, N, 5))
    cnt = np.zeros((F, S), np.int32)
    dts = np.zeros((F, S))
    rng = np.random.default_rng(seed)
    for s in range(S):
        p, c, d = make_batch([seed + s], F, N, 1 + s % 3, ragged=(s % 4 == 0))
        raw[:, s] = _raw_for(p[:, 0], SITES[which[s]])
        raw[:, s, :, 4] = rng.uniform(0.0, 300.0, size=(F, N))   # intensities over 0 .. 300
        cnt[:, s], dts[:, s] = c[:, 0], d[:, 0]
        for f in range(F):
            raw[f, s, cnt[f, s]:] = 0.0
    return raw, cnt, dts, which


def _model():
    from mmwave_msc_amd.mars import MarsCNN, random_keras_weights
    return MarsCNN.from_keras_weights(random_keras_weights(seed=4, frames=3)).to("cuda:0")


def _frame(sb, model, raw, cnt, dt, path):
    """One frame through `path`; returns per-scene outputs (rows, n_out, assoc, labels, db_n) as arrays [S, ...]."""
    import torch
    S, N = sb.S, sb.max_pts
    if path == "frame_host":
        out = sb.frame_host(cnt, dt, raw=raw, want_rows=True)
        rows, n_out, assoc, labels, dbn = out["rows"].copy(), out["n_out"].copy(), out["assoc"].copy(), out["labels"].copy(), out["db_n"].copy()
    else:   # the separate calls: normalize_dev -> step_dev -> features -> CNN -> set_keypoints
        b_raw = sb.buf("t_raw", raw.nbytes).upload(raw)
        b_n = sb.buf("t_n", S * 4).upload(np.ascontiguousarray(cnt, np.int32))
        b_dt = sb.buf("t_dt", S * 8).upload(np.ascontiguousarray(dt, np.float64))
        b_pts, b_no = sb.buf("t_pts", S * N * 64), sb.buf("t_no", S * 4)
        b_as, b_lab, b_dbn = sb.buf("t_as", S * N * 4), sb.buf("t_lab", S * sb.UM * 4), sb.buf("t_dbn", S * 4)
        sb.normalize_dev(b_raw.ptr, b_n.ptr, b_pts.ptr, b_no.ptr)
        sb.step_dev(b_pts.ptr, b_no.ptr, b_dt.ptr, b_as.ptr, b_lab.ptr, b_dbn.ptr)
        sb.check()
        n_out = b_no.download((S,), np.int32)
        rows = b_pts.download((S, N, 8), np.float64)
        assoc, labels, dbn = b_as.download((S, N), np.int32), b_lab.download((S, sb.UM), np.int32), b_dbn.download((S,), np.int32)
    # estimate_posture behind the step (a context of many scenes: features -> CNN -> keypoints, as PosturePipeline does)
    feat, owner = sb.features_host()
    keep = n_out[owner[:, 0]] > 0 if len(owner) else np.zeros(0, bool)   # (a skipped frame is not estimated, offline_main.py:56-60)
    if keep.any():
        with torch.no_grad():
            kp = model(torch.from_numpy(feat[keep]).to("cuda:0")).float().cpu().numpy()
        sb.set_keypoints_host(kp, owner[keep])
    for s in range(S):
        rows[s, max(int(n_out[s]), 0):] = 0.0
        assoc[s, max(int(n_out[s]), 0):] = -1
        labels[s, max(int(dbn[s]), 0):] = -1
    return rows, n_out, assoc, labels, dbn


def _state(sb):
    """Everything a scene holds and shows, per scene, in a comparable form."""
    ntr, trk = sb.num_tracks(), sb.tracks()
    ln, rn = sb.batch_ring()
    table = sb.track_table_host(sb.track_cap)
    feat, owner = sb.features_host()
    out = []
    for s in range(sb.S):
        T = int(ntr[s])
        rings = [sb.batch_ring_frame(s, k).tobytes() for k in range(int(ln[s]))]
        for j in range(T):
            rings += [sb.track_ring_frame(s, j, k).tobytes() for k in range(int(trk[s, j]["ring_len"]))]
        mine = owner[:, 0] == s if len(owner) else np.zeros(0, bool)
        out.append(dict(n_tracks=T, tracks=trk[s, :T].tobytes(), ring=(int(ln[s]), rn[s].tobytes()), rings=tuple(rings),
                        feat=feat[mine].tobytes(), feat_owner=owner[mine, 1].tobytes() if len(owner) else b"",
                        table=table[s].tobytes(), keypoints=trk[s, :T]["keypoints"].tobytes()))
    return out


def _run(sb, model, raw, cnt, dts, path):
    frames = [_frame(sb, model, raw[f], cnt[f], dts[f], path) for f in range(raw.shape[0])]
    return frames, _state(sb)


@pytest.mark.parametrize("path", ["frame_host", "separate_calls"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_mixed_context_equals_uniform_contexts_and_oracle(layout, path):
    """64 scenes over 6 interleaved sites, 12 frames, the posture CNN behind every step: every scene of the mixed context equals, bit for
    bit, the same scene of a context created with that site as its configuration (normalised rows and counts, association,
    labels, db_n, track records, ring frames, feature tensors, keypoints, track-table rows) and, in its integers and its
    normalised rows, the C oracle built with that scene's configuration."""
    from mmwave_msc_amd import _lib
    from oracle import c_oracle as co
    S, N, F = 64, 256, 12
    raw, cnt, dts, which = _inputs(S, N, F)
    model = _model()
    mixed = make_checked(S, N, layout, **KW)
    mixed.set_sites(_site_rows(mixed.cfg, [SITES[w] for w in which]))
    assert mixed.has_sites
    m_frames, m_state = _run(mixed, model, raw, cnt, dts, path)
    mixed.close()
    # not vacuous: every scene keeps rows in every frame and holds a track at the end
    for f in range(F):
        assert (m_frames[f][1] > 0).all(), (f, m_frames[f][1])
    assert all(st["n_tracks"] >= 1 for st in m_state), [st["n_tracks"] for st in m_state]
    assert any(len(st["feat"]) for st in m_state)
    # ... and the mounting matters: the same raw rows normalised under two mountings differ
    a = co.normalize(_orc_cfg(SITES[0]), raw[0, 0, : cnt[0, 0]])
    b = co.normalize(_orc_cfg(SITES[1]), raw[0, 0, : cnt[0, 0]])
    assert a.shape != b.shape or not np.array_equal(a, b)
    for k, site in enumerate(SITES):
        uni = make_checked(S, N, layout, **KW, **site)
        assert not uni.has_sites
        u_frames, u_state = _run(uni, model, raw, cnt, dts, path)
        uni.close()
        for s in np.flatnonzero(which == k):
            for f in range(F):
                for name, m, u in zip(("rows", "n_out", "assoc", "labels", "db_n"), m_frames[f], u_frames[f]):
                    assert m[s].tobytes() == u[s].tobytes(), (layout, path, "site", k, "scene", int(s), "frame", f, name)
            for key in m_state[s]:
                assert m_state[s][key] == u_state[s][key], (layout, path, "site", k, "scene", int(s), key)
    # the oracle, one OracleScene per scene with that scene's configuration
    for s in range(S):
        cfg = _orc_cfg(SITES[which[s]])
        orc = co.OracleScene(cfg, N)
        for f in range(F):
            rows, n_out, assoc, labels, dbn = (v[s] for v in m_frames[f])
            want = co.normalize(cfg, raw[f, s, : cnt[f, s]])
            assert n_out == len(want) and rows[:n_out].tobytes() == want.tobytes(), (s, f, "normalised rows vs oracle")
            oa, ol = orc.track(want, dts[f, s])
            assert np.array_equal(assoc[:n_out], oa), (s, f)
            assert (ol is None) == (dbn < 0), (s, f)
            if ol is not None:
                assert np.array_equal(labels[:dbn], ol), (s, f)
        assert orc.n_tracks == m_state[s]["n_tracks"], s


KEYS = ("rows", "n_out", "assoc", "labels", "db_n", "n_tracks")


def _defined(o):
    """frame_host's arrays with everything a frame does not define blanked: rows and association entries past n_out, labels past
    db_n (the device buffers keep what earlier frames left there)."""
    out = {k: o[k].copy() for k in KEYS}
    for s in range(len(out["n_out"])):
        m = max(int(out["n_out"][s]), 0)
        out["rows"][s, m:] = 0.0
        out["assoc"][s, m:] = -1
        out["labels"][s, max(int(out["db_n"][s]), 0):] = -1
    return out


def _tracks_bytes(sb, scenes):
    """The live track records of `scenes`, scene by scene (plain slices: a fancy-indexed copy of an aligned structured array does
    not carry its padding bytes)."""
    trk, ntr = sb.tracks(), sb.num_tracks()
    return [trk[s, : int(ntr[s])].tobytes() for s in scenes]


def _one_frame_outputs(sb, raw, cnt, dts, frames=4):
    outs = []
    for f in range(frames):
        o = _defined(sb.frame_host(cnt[f], dts[f], raw=raw[f], want_rows=True))
        outs.append(tuple(o[k].tobytes() for k in KEYS))
    feat, owner = sb.features_host()
    return outs, feat.tobytes(), owner.tobytes(), _tracks_bytes(sb, range(sb.S)), sb.track_table_host(sb.track_cap).tobytes()


def test_sites_equal_to_the_config_change_nothing_and_clear_sites_goes_back():
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    S, N, F = 12, 256, 4
    raw, cnt, dts, _ = _inputs(S, N, F, seed=300)
    cfg_kw = dict(SITES[4], **KW)
    plain = SceneBatch(_lib.default_config(**cfg_kw), S, N)
    want = _one_frame_outputs(plain, raw, cnt, dts)
    snap_plain = plain.snapshot()
    sb = SceneBatch(_lib.default_config(**cfg_kw), S, N)
    assert not sb.has_sites and sb.sites().tobytes() == _lib.make_sites(sb.cfg, S).tobytes()
    sb.set_sites(_lib.make_sites(sb.cfg, S))
    assert sb.has_sites
    assert _one_frame_outputs(sb, raw, cnt, dts) == want
    # a snapshot does not carry sites: same size, and for sites equal to the config the same bytes
    assert sb.snapshot_size() == plain.snapshot_size() and sb.snapshot() == snap_plain
    sb.set_sites(_site_rows(sb.cfg, [SITES[1]]), [5])
    sb.clear_sites()
    assert not sb.has_sites and sb.sites().tobytes() == _lib.make_sites(sb.cfg, S).tobytes()
    sb.reset()
    assert _one_frame_outputs(sb, raw, cnt, dts) == want
    plain.close()
    sb.close()


def test_partial_and_repeated_sets_and_a_change_between_frames():
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    from oracle import c_oracle as co
    S, N, F = 20, 256, 8
    raw, cnt, dts, _ = _inputs(S, N, F, seed=500)
    raw[:, :] = raw[:, :1]   # (every scene sees scene 0's rows: a default-mounted radar's)
    cnt[:, :], dts[:, :] = cnt[:, :1], dts[:, :1]
    ref = SceneBatch(_lib.default_config(**KW), S, N)
    sb = SceneBatch(_lib.default_config(**KW), S, N)
    base = _lib.make_sites(sb.cfg, S)
    sb.set_sites(_site_rows(sb.cfg, [SITES[2], SITES[3]]), [3, 17])
    want = base.copy()
    want[[3, 17]] = _site_rows(sb.cfg, [SITES[2], SITES[3]])
    assert sb.sites().tobytes() == want.tobytes()
    sb.set_sites(_site_rows(sb.cfg, [SITES[4]]), [17])            # a second call overrides the first
    want[17] = _site_rows(sb.cfg, [SITES[4]])[0]
    assert sb.sites().tobytes() == want.tobytes()
    sb.set_sites(_site_rows(sb.cfg, [SITES[0]]), [17])            # ... back to the default mounting for scene 17
    k = 4
    for f in range(F):
        if f == k + 1:   # a change between frame k and k + 1: scene 17 moves to another mounting, its tracks carry over
            before = sb.tracks()[17:18].copy()[0]
            n_before = int(sb.num_tracks()[17])
            assert n_before >= 1
            sb.set_sites(_site_rows(sb.cfg, [SITES[5]]), [17])
        o = _defined(sb.frame_host(cnt[f], dts[f], raw=raw[f], want_rows=True))
        r = _defined(ref.frame_host(cnt[f], dts[f], raw=raw[f], want_rows=True))
        others = [s for s in range(S) if s not in (3, 17)]
        for key in ("rows", "n_out", "assoc", "labels", "db_n", "n_tracks"):
            assert o[key][others].tobytes() == r[key][others].tobytes(), (f, key)
        if f <= k:
            for key in ("rows", "n_out", "assoc", "labels", "db_n", "n_tracks"):
                assert o[key][17].tobytes() == r[key][17].tobytes(), (f, key)
        assert o["n_out"][3] != r["n_out"][3] or o["rows"][3].tobytes() != r["rows"][3].tobytes()
        if f == k + 1:
            new = co.normalize(_orc_cfg(SITES[5]), raw[f, 17, : cnt[f, 17]])
            assert o["n_out"][17] == len(new) and o["rows"][17, : len(new)].tobytes() == new.tobytes()
            assert o["rows"][17].tobytes() != r["rows"][17].tobytes()
            # the tracks continue from their state of frame k: same identities, one frame older
            after = sb.tracks()[17]
            uids = set(before["uid"][:n_before].tolist())
            assert uids & set(after["uid"][: int(sb.num_tracks()[17])].tolist()), "the tracks of frame k must carry over"
    assert _tracks_bytes(ref, others) == _tracks_bytes(sb, others)
    ref.close()
    sb.close()


def test_refusals_are_atomic():
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    S, N = 9, 64
    sb = SceneBatch(_lib.default_config(**KW), S, N)
    L, h = sb.L, sb.h
    good = _site_rows(sb.cfg, [SITES[k % 6] for k in range(S)])

    def refused(scenes, n, sites, names):
        before = sb.sites().tobytes()
        had = sb.has_sites
        idx = np.ascontiguousarray(scenes, np.int32) if scenes is not None else None
        rc = L.mmw_set_sites(h, idx.ctypes.data if idx is not None else None, n, sites.ctypes.data if sites is not None else None)
        assert rc == _lib.E_ARG, (rc, names)
        msg = (L.mmw_last_error(h) or b"").decode()
        assert names in msg, (names, msg)
        assert sb.sites().tobytes() == before and sb.has_sites == had

    for armed in (False, True):   # before any table exists, and with one in use
        if armed:
            sb.set_sites(good[:4], [8, 2, 4, 6])
        refused([0, 1, S], 3, good[:3], "entry 2")                       # out of range, last of several good ones
        refused([0, -1], 2, good[:2], "entry 1")
        refused([3, 5, 3], 3, good[:3], "entry 2")                       # a duplicate
        refused(None, -1, good, "n = -1")
        refused(None, S + 1, np.concatenate([good, good[:1]]), f"n = {S + 1}")
        refused(None, 2, None, "NULL")
        bad = good.copy()
        bad["reserved_"][S - 1] = 1.0
        refused(None, S, bad, f"entry {S - 1}")                            # non-zero reserved_, the last of many good ones
        bad = good.copy()
        bad["reserved_"][0] = -0.0
        refused(None, S, bad, "entry 0")
    with pytest.raises(_lib.MmwError):
        sb.set_sites(good[:2], [1, 1])
    # the values themselves are not judged: a site may hold anything a config may
    odd = good[:1].copy()
    odd["intensity_std"], odd["s_height"] = 0.0, np.nan
    sb.set_sites(odd, [0])
    assert sb.sites()[:1].tobytes() == odd.tobytes()
    sb.set_sites(good[:0])   # n = 0: nothing changes
    sb.close()


def test_reset_keeps_sites_and_restore_leaves_the_destination_sites_alone():
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    S, N, F, k = 12, 256, 9, 5
    raw, cnt, dts, which = _inputs(S, N, F, seed=700)
    kws = [SITES[w] for w in which]
    A = SceneBatch(_lib.default_config(**KW), S, N)
    A.set_sites(_site_rows(A.cfg, kws))
    sites_a = A.sites().tobytes()
    plain_size = None
    outs = []
    for f in range(F):
        outs.append(_defined(A.frame_host(cnt[f], dts[f], raw=raw[f], want_rows=True)))
        if f == k:
            pick = [1, 4, 8]
            blob = A.snapshot(pick)
            plain_size = A.snapshot_size(pick)
            tr_k = _tracks_bytes(A, pick)
    final = _tracks_bytes(A, pick)
    assert len(blob) == plain_size
    # B: the picked scenes go to other slots that were given the same sites: they continue bit for bit
    SB, dst = 7, [5, 0, 3]
    B = SceneBatch(_lib.default_config(**KW), SB, N)
    B.set_sites(_site_rows(B.cfg, [kws[s] for s in pick]), dst)
    sites_b = B.sites().tobytes()
    B.restore(blob, dst)
    assert B.sites().tobytes() == sites_b and _tracks_bytes(B, dst) == tr_k
    for f in range(k + 1, F):
        R = np.zeros((SB, N, 5)); n = np.zeros(SB, np.int32); d = np.full(SB, 0.1)
        for i, s in enumerate(pick):
            R[dst[i]], n[dst[i]], d[dst[i]] = raw[f, s], cnt[f, s], dts[f, s]
        o = _defined(B.frame_host(n, d, raw=R, want_rows=True))
        for i, s in enumerate(pick):
            for key in ("rows", "n_out", "assoc", "labels", "db_n", "n_tracks"):
                assert o[key][dst[i]].tobytes() == outs[f][key][s].tobytes(), (f, s, key)
    assert _tracks_bytes(B, dst) == final
    # C: restored into slots with OTHER sites: the tracks arrive intact, the next frame is normalised with the destination's site
    from oracle import c_oracle as co
    Cx = SceneBatch(_lib.default_config(**KW), SB, N)
    other = [SITES[(which[s] + 1) % 6] for s in pick]
    Cx.set_sites(_site_rows(Cx.cfg, other), dst)
    Cx.restore(blob, dst)
    assert _tracks_bytes(Cx, dst) == tr_k
    f = k + 1
    R = np.zeros((SB, N, 5)); n = np.zeros(SB, np.int32); d = np.full(SB, 0.1)
    for i, s in enumerate(pick):
        R[dst[i]], n[dst[i]], d[dst[i]] = raw[f, s], cnt[f, s], dts[f, s]
    o = Cx.frame_host(n, d, raw=R, want_rows=True)
    for i, s in enumerate(pick):
        want = co.normalize(_orc_cfg(other[i]), raw[f, s, : cnt[f, s]])
        assert o["n_out"][dst[i]] == len(want) and o["rows"][dst[i], : len(want)].tobytes() == want.tobytes()
    # reset_scenes and reset keep the sites
    mask = np.zeros(S, bool); mask[[0, 4]] = True
    A.reset_scenes(mask)
    assert A.sites().tobytes() == sites_a and A.has_sites
    A.reset()
    assert A.sites().tobytes() == sites_a and A.has_sites
    o = _defined(A.frame_host(cnt[0], dts[0], raw=raw[0], want_rows=True))
    assert o["rows"].tobytes() == outs[0]["rows"].tobytes() and o["assoc"].tobytes() == outs[0]["assoc"].tobytes()
    for x in (A, B, Cx):
        x.close()


def test_non_finite_rows_under_a_site_flag_as_the_uniform_twin_does():
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    S, N, F = 6, 256, 6
    raw, cnt, dts, _ = _inputs(S, N, F, seed=1100)
    site = SITES[4]
    raw[:, :] = _inputs(S, N, F, seed=1100)[0][:, 4:5]   # every scene sees the rows of a scene mounted as SITES[4]
    cnt[:, :], dts[:, :] = cnt[:, 4:5], dts[:, 4:5]
    raw[2, 1, 3, 3] = np.nan      # a NaN doppler: the row is kept, its velocities are NaN -> sklearn's ValueError in apply_DBscan
    raw[3, 2, 5, 3] = np.inf
    raw[1, 3, 7, 0] = np.nan      # a NaN coordinate: the row is dropped
    twin = SceneBatch(_lib.default_config(**KW, **site), S, N)
    sb = SceneBatch(_lib.default_config(**KW), S, N)
    sb.set_sites(_site_rows(sb.cfg, [site] * S))
    for f in range(F):
        res = []
        for x in (sb, twin):
            try:
                o = _defined(x.frame_host(cnt[f], dts[f], raw=raw[f], want_rows=True))
                res.append(("ok",) + tuple(o[k].tobytes() for k in KEYS))
            except ValueError as e:
                res.append(("raised", e.code, str(e).split(":", 1)[-1]))
            res.append(x.errors().tobytes())
            x.clear_errors(_lib.ERRBIT_NONFINITE_NAN | _lib.ERRBIT_NONFINITE_INF)
        assert res[0] == res[2] and res[1] == res[3], (f, res[0][0], res[2][0])
    assert _tracks_bytes(sb, range(S)) == _tracks_bytes(twin, range(S))
    assert np.frombuffer(sb.errors().tobytes(), np.int32).sum() == 0
    sb.close()
    twin.close()


def test_tlv_path_under_mixed_sites_equals_host_decode_and_normalize_host():
    """mmw_normalize_tlv under mixed sites = radar.decode_tlv_bodies_numpy + normalize_host under the same sites, on the
    decoded packets of the recorded UART streams."""
    from mmwave_msc_amd import _lib, radar
    from mmwave_msc_amd.batch import SceneBatch
    from tests._uart_recording import load
    N = 256
    groups = {}
    for s in load():
        if not float(s.cfg["numDopplerBins"]).is_integer():
            continue
        key = tuple(sorted(s.cfg.items()))
        groups.setdefault(key, []).extend(r.body for r in s.reads if r.ok and 0 < r.num_obj <= N)
    key, bodies = max(groups.items(), key=lambda kv: len(kv[1]))
    cfg0 = dict(key)
    bodies = bodies[:48]
    S = len(bodies)
    assert S >= 6, S
    sb = SceneBatch(_lib.default_config(**KW), S, N)
    sb.set_sites(_site_rows(sb.cfg, [SITES[s % 6] for s in range(S)]))
    stride = max(len(b) for b in bodies)
    stride += stride & 1
    packed = np.zeros((S, stride), np.uint8)
    for s, b in enumerate(bodies):
        packed[s, : len(b)] = np.frombuffer(b, np.uint8)
    raw, cnt = radar.decode_tlv_bodies_numpy(packed, cfg0)
    buf = np.zeros((S, N, 5))
    m = min(N, raw.shape[1])
    buf[:, :m] = raw[:, :m]
    with np.errstate(all="ignore"):
        want_pts, want_n = sb.normalize_host(buf, cnt.astype(np.int32))
    offs = (np.arange(S, dtype=np.int64) * stride)
    b_pk = sb.buf("tlv_pk", packed.nbytes).upload(packed)
    b_off = sb.buf("tlv_off", offs.nbytes).upload(offs)
    b_pts, b_no = sb.buf("tlv_pts", S * N * 64), sb.buf("tlv_no", S * 4)
    ucfg = radar.uart_cfg(cfg0)
    sb.normalize_tlv_dev(b_pk.ptr, packed.nbytes, b_off.ptr, ucfg, b_pts.ptr, b_no.ptr)
    n_out = b_no.download((S,), np.int32)
    pts = b_pts.download((S, N, 8), np.float64)
    assert np.array_equal(n_out, want_n)
    for s in range(S):
        assert pts[s, : n_out[s]].tobytes() == want_pts[s, : n_out[s]].tobytes(), s
    sb.close()


def test_local_sharded_tracker_applies_each_shards_slice():
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    from mmwave_msc_amd.dist import LocalShardedTracker
    S, N, F = 10, 256, 6
    raw, cnt, dts, which = _inputs(S, N, F, seed=1300)
    one = SceneBatch(_lib.default_config(**KW), S, N)
    sites = _site_rows(one.cfg, [SITES[w] for w in which])
    one.set_sites(sites)
    lst = LocalShardedTracker(lambda: _lib.default_config(**KW), S, N, devices=[0, 0])
    lst.set_sites(sites)
    for sh in lst.shards:
        assert sh["sb"].sites().tobytes() == sites[sh["lo"]: sh["hi"]].tobytes()
    for f in range(F):
        one.frame_host(cnt[f], dts[f], raw=raw[f])
        lst.run(lambda g, sh: sh["sb"].frame_host(cnt[f, sh["lo"]: sh["hi"]], dts[f, sh["lo"]: sh["hi"]], raw=raw[f, sh["lo"]: sh["hi"]]))
    assert one.num_tracks().sum() >= S
    assert lst.gather_table(4).tobytes() == one.track_table_host(4).tobytes()
    with pytest.raises(ValueError):
        lst.set_sites(sites[:-1])
    lst.close()
    one.close()


def test_site_struct_is_96_bytes_everywhere():
    import os
    import re
    from mmwave_msc_amd import _lib
    assert _lib.SITE_DTYPE.itemsize == 96 and _lib.ABI_STRUCTS["mmw_scene_site"] is _lib.SITE_DTYPE
    assert list(_lib.SITE_DTYPE.names) == list(_lib.SITE_FIELDS) + ["reserved_"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "mmw.h")).read()
    body = re.search(r"typedef struct mmw_scene_site \{(.*?)\} mmw_scene_site;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in re.findall(r"double ([^;]+);", body) for n in decl.split(",")]
    assert names == list(_lib.SITE_DTYPE.names) and len(names) * 8 == 96
