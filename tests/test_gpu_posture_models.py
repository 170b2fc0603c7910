"""GPU tests of the per-scene posture models (include/mmw.h: mmw_posture_attach_models, mmw_posture_set_scene_models,
mmw_posture_group_rows, mmw_posture_owners; csrc/k_feat_models.hip).  A context whose scenes are served by several
models must give every scene the keypoints of a context that holds that scene's model alone -- bit for bit: the rows of a model
form one band that starts on a multiple of 256, and the CNN kernels give a row the same bits wherever it stands (test 1 measures
that premise).  The fp64 oracle (oracle/mars_np.py) bounds the keypoints with the project's KP_TOL; tracker state is bit-equal to
the C oracle."""
import ctypes as C

import numpy as np
import pytest

from tests import _posture_cabi as pc
from tests._layouts import make_checked
from tests._posture_gpu import CANARY, KP_TOL, KW, N, CModel, _dev, _live, _step, _stream, _weights
from tests._posture_models import NONE, grouped_owners

pytestmark = pytest.mark.gpu


def _attach_models(sb, models, frames, scene_model, cap_rows):
    """The status of mmw_posture_attach_models for CModels (or bare structs) and a map (None: NULL)."""
    from mmwave_msc_amd import _lib
    structs = [getattr(m, "struct", m) for m in models]
    arr = (_lib.MmwPostureModel * max(len(structs), 1))(*structs)
    smap = np.ascontiguousarray(scene_model, dtype=np.int32) if scene_model is not None else None
    return sb.L.mmw_posture_attach_models(sb.h, arr, len(structs), frames, smap.ctypes.data if smap is not None else None, cap_rows)


def _set_models(sb, model_of, scenes=None):
    a = np.ascontiguousarray(model_of, dtype=np.int32)
    idx = np.ascontiguousarray(scenes, dtype=np.int32) if scenes is not None else None
    return sb.L.mmw_posture_set_scene_models(sb.h, idx.ctypes.data if idx is not None else None, len(a), a.ctypes.data if len(a) else None)


def _get_models(sb):
    out = np.full(sb.S + 4, 4242, dtype=np.int32)   # (four canary words behind the map)
    assert sb.L.mmw_posture_get_scene_models(sb.h, out.ctypes.data) == 0
    assert (out[sb.S:] == 4242).all()
    return out[: sb.S].copy()


def _group_rows(sb, n_models):
    rows, n = np.full(n_models + 4, 4242, dtype=np.int32), C.c_int32(-1)
    assert sb.L.mmw_posture_group_rows(sb.h, rows.ctypes.data, C.byref(n)) == 0
    assert n.value == n_models and (rows[n_models:] == 4242).all()
    return rows[:n_models].tolist()


def _owners(sb, cap):
    out, n = np.full((cap + 4, 2), 4242, dtype=np.int32), C.c_int32(-1)
    assert sb.L.mmw_posture_owners(sb.h, out.ctypes.data, cap, C.byref(n)) == 0, sb.L.mmw_last_error(sb.h)
    assert 0 <= n.value <= cap and (out[n.value:] == 4242).all()
    return out[: n.value].copy()


def _estimate(sb):
    rows = C.c_int32(-1)
    assert sb.L.mmw_estimate_posture(sb.h, C.byref(rows)) == 0, sb.L.mmw_last_error(sb.h)
    return rows.value


def _kp_bytes(ntr, trk, s):
    return trk[s, : ntr[s]]["keypoints"].tobytes()


def _uniform(S, layout, frames, w, pts, cnt, dts, F=None):
    """The frames on a context that holds `w` alone, through mmw_posture_attach_frames: (n_tracks, tracks) at the end."""
    sb = make_checked(S, N, layout, **KW[frames])
    model = CModel(sb, w)
    assert sb.L.mmw_posture_attach_frames(sb.h, C.byref(model.struct), frames, S * sb.track_cap) == 0, sb.L.mmw_last_error(sb.h)
    for f in range(F if F is not None else cnt.shape[0]):
        _step(sb, pts[f], cnt[f], dts[f])
        _estimate(sb)
    out = _live(sb)
    model.free()
    sb.close()
    return out


# ---- 1. the premise: a row's result does not depend on where it stands in the batch ---------------------------------------------
@pytest.mark.parametrize("K,n", [(2048, 512), (6144, 1536)])
def test_a_rows_result_does_not_depend_on_its_place_in_the_batch(K, n):
    """300 rows as rows 0 .. 299 of a 300-row batch (rows_padded 512) and as rows 700 .. 999 of a 1000-row batch (rows_padded 1024)
    of other data, through the stateless entries: hidden layer and keypoints equal in every bit.  K = 2048, n = 512 crosses the
    256 x 128 tiles, K = 6144, n = 1536 the 256 x 192 ones, both with their 128 x 128 tails."""
    import torch
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.marsweights import FOLDED_KEYS, fold_keras_weights, model_dims
    L = _lib.load()
    frames = K // 2048
    dims = model_dims(frames)
    assert (dims.flat, dims.hidden) == (K, n)
    f = fold_keras_weights(_weights(3, frames))
    d = {k: _dev(f[k]) for k in FOLDED_KEYS}
    rng = np.random.default_rng(K)
    mine = rng.normal(0, 0.5, size=(300,) + dims.input).astype(np.float32)
    big = rng.normal(0, 0.7, size=(1000,) + dims.input).astype(np.float32)
    big[700:] = mine
    ld = 2 * K + 256
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    w16 = torch.empty((n, 2 * K), dtype=torch.float16, device="cuda")
    assert L.mmw_mars_split_weights(_stream(), d["dense1_w"].data_ptr(), K, w16.data_ptr(), 2 * K, n, K, word.data_ptr()) == 0, L.mmw_last_error(None)

    def chain(x):
        rows = len(x)
        padded = (rows + 255) // 256 * 256
        xt = _dev(x)
        act16 = torch.zeros((padded, ld), dtype=torch.float16, device="cuda")
        flags = torch.zeros(2 + 64, dtype=torch.int32, device="cuda")
        hidden = torch.full((padded, n), CANARY, dtype=torch.float32, device="cuda")
        kp = torch.full((rows, 57), CANARY, dtype=torch.float32, device="cuda")
        assert L.mmw_mars_conv_split(_stream(), frames, xt.data_ptr(), d["conv1_w"].data_ptr(), d["conv1_b"].data_ptr(), d["conv2_w"].data_ptr(),
                                     d["conv2_b"].data_ptr(), act16.data_ptr(), ld, rows, word.data_ptr(), flags.data_ptr()) == 0, L.mmw_last_error(None)
        assert L.mmw_mars_dense1_split(_stream(), act16.data_ptr(), ld, w16.data_ptr(), 2 * K, d["dense1_b"].data_ptr(), hidden.data_ptr(), padded, K, n) == 0, L.mmw_last_error(None)
        assert L.mmw_mars_dense2(_stream(), hidden.data_ptr(), n, d["dense2_w"].data_ptr(), d["dense2_b"].data_ptr(), kp.data_ptr(), rows, n) == 0, L.mmw_last_error(None)
        torch.cuda.synchronize()
        return hidden[:rows], kp

    h_a, kp_a = chain(mine)
    h_b, kp_b = chain(big)
    assert int(word.item()) == 0, "the inputs are in range: no sample was flagged"
    assert bool((h_a > 0).any()) and bool((kp_a != CANARY).all())
    dh = int((h_a.view(torch.int32) != h_b[700:].view(torch.int32)).sum())
    dk = int((kp_a.view(torch.int32) != kp_b[700:].view(torch.int32)).sum())
    print(f"K={K} n={n}: {dh} hidden words and {dk} keypoint words of 300 rows differ between the two places")
    assert dh == 0 and dk == 0, (dh, dk)
    assert not torch.equal(kp_b[:300], kp_a), "the other rows of the large batch are other data"


# ---- 2. a mixed context against the oracle and against uniform contexts -----------------------------------------------------
_ORACLE = {}


def _oracle(frames, seed, S=48):
    """scenario(S) and its oracle run with random_keras_weights(seed, frames): computed once, never changed."""
    if (frames, seed, S) not in _ORACLE:
        pts, cnt, dts = pc.scenario(S)
        w = _weights(seed, frames)
        _ORACLE[frames, seed, S] = dict(pts=pts, cnt=cnt, dts=dts, w=w, ref=pc.oracle_run(pts, cnt, dts, w, cfg_kw=KW[frames]))
    return _ORACLE[frames, seed, S]


@pytest.mark.parametrize("frames,n_models,layout", [(1, 3, "one_workgroup"), (1, 3, "per_scene"), (3, 2, "per_scene")],
                         ids=["single_frame-3-one_workgroup", "single_frame-3-per_scene", "3_frame-2-per_scene"])
def test_mixed_context_against_the_oracle_and_uniform_contexts(frames, n_models, layout):
    S = 48
    runs = [_oracle(frames, seed) for seed in range(n_models)]
    pts, cnt, dts = runs[0]["pts"], runs[0]["cnt"], runs[0]["dts"]
    ref = runs[0]["ref"]
    F = cnt.shape[0]
    model_of = np.arange(S) % (n_models + 1) - 1   # (three models: s % 4 - 1, a quarter of the scenes on MMW_POSTURE_NONE)
    want = [grouped_owners(ref["owners"][f], model_of, n_models) for f in range(F)]
    for f in range(4, F):
        assert (want[f][1] >= 1).all(), (f, want[f][1])
    assert any(len(ref["finals"][s]) for s in np.flatnonzero(model_of == NONE)), "an excluded scene must hold a live track at the end"
    sb = make_checked(S, N, layout, **KW[frames])
    L = sb.L
    models = [CModel(sb, r["w"]) for r in runs]
    assert _attach_models(sb, models, frames, model_of, S * sb.track_cap) == 0, L.mmw_last_error(sb.h)
    assert np.array_equal(_get_models(sb), model_of)
    for f in range(F):
        _step(sb, pts[f], cnt[f], dts[f])
        rows = _estimate(sb)
        assert rows == len(want[f][0]), (f, rows, len(want[f][0]))
        assert _group_rows(sb, n_models) == want[f][1].tolist(), f
        assert np.array_equal(_owners(sb, S * sb.track_cap), want[f][0]), f
    ntr, trk = _live(sb)
    word = C.c_int32(-1)
    assert L.mmw_posture_range(sb.h, C.byref(word)) == 0 and word.value == 0
    default = np.array(list(sb.cfg.default_posture), dtype=np.float32)
    uniform = [_uniform(S, layout, frames, r["w"], pts, cnt, dts) for r in runs]
    worst, differs, mapped = 0.0, 0, 0
    for s in range(S):
        got = trk[s, : ntr[s]]
        assert len(ref["finals"][s]) == int(ntr[s]), s
        for name in pc.STATE_FIELDS:
            assert np.array_equal(got[name], ref["finals"][s][name]), (s, name)
        m = int(model_of[s])
        if m == NONE:
            assert (got["keypoints"] == default).all(), s
            continue
        worst = max(worst, pc.kp_err(got["keypoints"], runs[m]["ref"]["want_kp"][s]))
        assert np.array_equal(ntr, uniform[m][0])
        assert _kp_bytes(ntr, trk, s) == _kp_bytes(*uniform[m], s), (s, "differs from the uniform context of its model", m)
        if ntr[s]:
            mapped += 1
            differs += all(_kp_bytes(ntr, trk, s) != _kp_bytes(*uniform[o], s) for o in range(n_models) if o != m)
    print(f"{n_models} models of {frames} frame(s), {layout}: keypoint error {worst:.3e} over {mapped} mapped scenes with tracks, "
          f"{differs} of them differ from every other model's uniform context")
    assert worst <= KP_TOL, worst
    assert mapped >= S // 3 and 2 * differs >= mapped, (mapped, differs)
    for m in models:
        m.free()
    sb.close()


# ---- 3. band edges and the scan's chunking --------------------------------------------------------------------------------------
def test_band_edges_at_256_and_257_rows_over_2050_scenes():
    """S = 2050: every thread of the scan takes three scenes and the last threads none.  The map is chosen from the eligible counts
    of a uniform twin so that model 0 gets exactly 256 rows, model 1 exactly 257, model 2 only scenes without a row, model 3 no
    scene; everybody else is excluded.  One call: exactly those 513 tracks get keypoints."""
    S, F = 2050, 6
    pts, cnt, dts = pc.scenario(S, F=F)
    cnt[:, [7, 1000, 1777, S - 1]] = 0   # (every scene of scenario(2050) holds an eligible track at frame 6: these four see no point at all)
    sb, twin = make_checked(S, N, "per_scene", **KW[1]), make_checked(S, N, "per_scene", **KW[1])
    L = sb.L
    models = [CModel(sb, _weights(seed, 1)) for seed in range(4)]
    assert _attach_models(sb, models, 1, None, S * sb.track_cap) == 0, L.mmw_last_error(sb.h)
    assert (_get_models(sb) == 0).all()
    for f in range(F):
        _step(sb, pts[f], cnt[f], dts[f])
        _step(twin, pts[f], cnt[f], dts[f])
    _, owners = twin.features_host()
    counts = np.bincount(owners[:, 0], minlength=S)
    ones, twos, none = np.flatnonzero(counts == 1), np.flatnonzero(counts == 2), np.flatnonzero(counts == 0)
    assert len(ones) >= 256 + 255 and len(twos) >= 1 and len(none) >= 3, (len(ones), len(twos), len(none))
    model_of = np.full(S, NONE, dtype=np.int32)
    model_of[ones[:256]] = 0
    model_of[ones[256: 256 + 255]] = 1   # 255 one-row scenes and a two-row scene: 257 rows
    model_of[twos[-1]] = 1
    model_of[none[[0, len(none) // 2, -1]]] = 2
    assert _set_models(sb, model_of) == 0, L.mmw_last_error(sb.h)
    assert np.array_equal(_get_models(sb), model_of)
    ntr, before = _live(sb)
    rows = _estimate(sb)
    assert _group_rows(sb, 4) == [256, 257, 0, 0] and rows == 513
    want, per = grouped_owners(owners, model_of, 4)
    assert per.tolist() == [256, 257, 0, 0]
    got = _owners(sb, 513)
    assert np.array_equal(got, want)
    ntr2, after = _live(sb)
    assert np.array_equal(ntr, ntr2)
    changed = (before["keypoints"] != after["keypoints"]).any(axis=-1)        # [S, cap]
    expect = np.zeros_like(changed)
    expect[want[:, 0], want[:, 1]] = True
    assert changed.sum() == 513 and np.array_equal(changed, expect), (int(changed.sum()), int((changed != expect).sum()))
    for name in pc.STATE_FIELDS:
        assert before[name].tobytes() == after[name].tobytes(), name
    word = C.c_int32(-1)
    assert L.mmw_posture_range(sb.h, C.byref(word)) == 0 and word.value == 0
    for m in models:
        m.free()
    sb.close(); twin.close()


# ---- 4. moving scenes between models ----------------------------------------------------------------------------------------
def test_moving_scenes_between_models_and_to_none():
    S, MOVE = 48, 6
    a, b = _oracle(1, 0), _oracle(1, 1)
    pts, cnt, dts = a["pts"].copy(), a["cnt"], a["dts"]
    F = cnt.shape[0]
    # (scenario(48) spawns no track in a scene of s % 3 == 2 after frame 6: in half of them everybody is 10 m further along x from
    #  frame 8 on, so that the old tracks expire and new ones are born after the move)
    for s in range(2, S, 6):
        for f in range(8, F):
            pts[f, s, : cnt[f, s], 0] += 10.0
    owners_f = pc.oracle_run(pts, cnt, dts, a["w"], cfg_kw=KW[1])["owners"]
    sb = make_checked(S, N, "per_scene", **KW[1])
    L = sb.L
    models = [CModel(sb, a["w"]), CModel(sb, b["w"])]
    assert _attach_models(sb, models, 1, None, S * sb.track_cap) == 0, L.mmw_last_error(sb.h)
    model_of = np.zeros(S, dtype=np.int32)
    for f in range(F):
        if f == MOVE:
            ntr_m, trk_m = _live(sb)
            model_of[np.arange(S) % 3 == 1] = 1
            model_of[np.arange(S) % 3 == 2] = NONE
            moved = np.flatnonzero(model_of != 0)
            assert _set_models(sb, model_of[moved], moved) == 0, L.mmw_last_error(sb.h)
            assert np.array_equal(_get_models(sb), model_of)
        _step(sb, pts[f], cnt[f], dts[f])
        rows = _estimate(sb)
        want, per = grouped_owners(owners_f[f], model_of, 2)
        assert rows == len(want) and _group_rows(sb, 2) == per.tolist(), f
    last = {(int(s), int(j)) for s, j in _owners(sb, S * sb.track_cap)}
    ntr, trk = _live(sb)
    ua, ub = (_uniform(S, "per_scene", 1, r["w"], pts, cnt, dts) for r in (a, b))
    assert np.array_equal(ntr, ua[0]) and np.array_equal(ntr, ub[0])
    default = np.array(list(sb.cfg.default_posture), dtype=np.float32)
    seen = dict(on_a=0, b_last=0, b_other=0, kept=0, born=0)
    for s in range(S):
        for j in range(int(ntr[s])):
            kp, kp_a, kp_b = (t[s, j]["keypoints"].tobytes() for t in (trk, ua[1], ub[1]))
            if s % 3 == 0:
                assert kp == kp_a, (s, j)
                seen["on_a"] += 1
            elif s % 3 == 1:
                if (s, j) in last:
                    assert kp == kp_b, (s, j)
                    seen["b_last"] += 1
                else:
                    assert kp in (kp_a, kp_b), (s, j)
                    seen["b_other"] += 1
            else:
                then = [i for i in range(int(ntr_m[s])) if trk_m[s, i]["uid"] == trk[s, j]["uid"]]
                if then:   # the track existed at the move: it keeps the keypoints it had then
                    assert kp == trk_m[s, then[0]]["keypoints"].tobytes(), (s, j)
                    seen["kept"] += 1
                else:
                    assert kp == default.tobytes(), (s, j)
                    seen["born"] += 1
    print("tracks checked:", seen)
    assert seen["on_a"] >= 8 and seen["b_last"] >= 8 and seen["kept"] >= 1 and seen["born"] >= 1, seen
    mask = np.zeros(S, bool)
    mask[[1, 2, 7]] = True
    sb.reset_scenes(mask)
    assert np.array_equal(_get_models(sb), model_of)
    sb.reset()
    assert np.array_equal(_get_models(sb), model_of)
    for m in models:
        m.free()
    sb.close()


# ---- 5. sites together with models ----------------------------------------------------------------------------------------------
def test_sites_and_models_give_each_scene_its_uniform_context():
    """The set-up of test_mixed_sites_give_each_scene_the_keypoints_of_its_uniform_context with two of its sites and two models:
    every scene carries one of the four (site, model) pairs and equals, bit for bit, the context created with that site as its
    configuration and attached with that model alone.  Through the Python face."""
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    from tests.test_gpu_sites import KW as SKW, SITES, _inputs, _site_rows
    S, F = 12, 10
    raw, cnt, dts, _ = _inputs(S, 256, F, seed=2500)
    sites, ws = [SITES[1], SITES[5]], [_weights(4, 3), _weights(5, 3)]
    site_of, model_of = np.arange(S) % 2, (np.arange(S) // 2) % 2

    def run(sb, attach):
        attach(sb)
        b_pts, b_no = sb.buf("p_pts", S * 256 * 64), sb.buf("p_no", S * 4)
        total = 0
        for f in range(F):
            b_raw = sb.buf("p_raw", raw[f].nbytes).upload(raw[f])
            b_n = sb.buf("p_n", S * 4).upload(cnt[f])
            b_dt = sb.buf("p_dt", S * 8).upload(dts[f])
            sb.normalize_dev(b_raw.ptr, b_n.ptr, b_pts.ptr, b_no.ptr)
            sb.step_dev(b_pts.ptr, b_no.ptr, b_dt.ptr)
            total += sb.estimate_posture()
            if attach is attach_mixed:
                per, own = sb.posture_group_rows(), sb.posture_owners()
                assert len(per) == 2 and per.sum() == len(own)
                assert (model_of[own[: per[0], 0]] == 0).all() and (model_of[own[per[0]:, 0]] == 1).all()
            sb.synchronize()
        sb.check()
        ntr, trk = sb.num_tracks(), sb.tracks()
        out = [trk[s, : ntr[s]]["keypoints"].tobytes() for s in range(S)]
        sb.attach_posture_batch(None)
        sb.close()
        return out, total

    def attach_mixed(sb):
        sb.set_sites(_site_rows(sb.cfg, [sites[k] for k in site_of]))
        sb.attach_posture_models(ws, model_of)
        assert np.array_equal(sb.scene_models(), model_of)

    m_kp, m_rows = run(SceneBatch(_lib.default_config(**SKW), S, 256), attach_mixed)
    assert m_rows >= S
    differs = 0
    for k, site in enumerate(sites):
        for m, w in enumerate(ws):
            u_kp, _ = run(SceneBatch(_lib.default_config(**SKW, **site), S, 256), lambda sb: sb.attach_posture_batch(w, S * sb.track_cap))
            for s in range(S):
                if site_of[s] == k and model_of[s] == m:
                    assert len(m_kp[s]) > 0 and m_kp[s] == u_kp[s], (k, m, s)
                else:
                    differs += m_kp[s] != u_kp[s]
    assert differs >= 2 * S   # (of 3 S comparisons) under another site or another model a scene comes out differently


# ---- 6. capacity, refusals, detach ----------------------------------------------------------------------------------------------
def test_capacity_refusals_and_detach():
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.marsweights import fold_keras_weights
    S = 16
    pts, cnt, dts = pc.scenario(S, seed=6300)
    ws = [_weights(seed, 1) for seed in range(3)]
    model_of = (np.arange(S) % 3).astype(np.int32)
    sb, clean = make_checked(S, N, "per_scene", **KW[1]), make_checked(S, N, "per_scene", **KW[1])
    L = sb.L
    models, cmodels = [CModel(sb, w) for w in ws], [CModel(clean, w) for w in ws]
    for f in range(6):
        _step(sb, pts[f], cnt[f], dts[f])
        _step(clean, pts[f], cnt[f], dts[f])
    # capacity: exactly the frame's total over three non-empty bands, then one row less
    _, owners = sb.features_host()
    want, per = grouped_owners(owners, model_of, 3)
    eligible = len(owners)
    assert (per >= 1).all() and eligible >= 8
    assert _attach_models(sb, models, 1, model_of, eligible) == 0, L.mmw_last_error(sb.h)
    assert _estimate(sb) == eligible and _group_rows(sb, 3) == per.tolist()
    assert np.array_equal(_owners(sb, eligible), want)
    assert _attach_models(clean, cmodels, 1, model_of, eligible) == 0 and _estimate(clean) == eligible   # (the twin: the same successful calls)
    n = C.c_int32(-5)
    few = np.full((eligible, 2), 4242, dtype=np.int32)
    assert L.mmw_posture_owners(sb.h, few.ctypes.data, eligible - 1, C.byref(n)) == _lib.E_CAPACITY and n.value == -5 and (few == 4242).all()
    _step(sb, pts[6], cnt[6], dts[6])
    _step(clean, pts[6], cnt[6], dts[6])
    eligible = len(sb.features_host()[1])
    _, stepped = _live(sb)
    assert _attach_models(sb, models, 1, model_of, eligible - 1) == 0
    rows = C.c_int32(5)
    assert L.mmw_estimate_posture(sb.h, C.byref(rows)) == _lib.E_CAPACITY and rows.value == 0
    assert b"cap_rows" in L.mmw_last_error(sb.h)
    assert sb.tracks(cap=stepped.shape[1]).tobytes() == stepped.tobytes(), "a keypoint changed in a refused call"
    assert _group_rows(sb, 3) == [0, 0, 0] and len(_owners(sb, 8)) == 0
    # attach refusals: MMW_E_ARG, the message names the offending model, the earlier attachment stays and gives the bytes of a
    # context that never saw the refusal
    cap = S * sb.track_cap
    assert _attach_models(sb, models[:2], 1, model_of % 2, cap) == 0 and _attach_models(clean, cmodels[:2], 1, model_of % 2, cap) == 0
    null = _lib.MmwPostureModel.from_buffer_copy(models[1].struct)
    null.conv2_w = None
    d1 = fold_keras_weights(ws[2])["dense1_w"].copy()
    d1[100, 7] = np.float32(7e4)
    hot = CModel(sb, ws[2], dense1_w=d1)
    three = make_checked(4, N, "per_scene", **KW[3])
    m3 = CModel(three, _weights(0, 3))
    assert _attach_models(three, [m3], 1, None, 64) == _lib.E_ARG and b"FB_FRAMES_BATCH" in L.mmw_last_error(three.h)
    assert L.mmw_estimate_posture(three.h, None) == _lib.E_ARG
    m3.free(); three.close()
    bad_map, low_map = model_of.copy(), model_of.copy()
    bad_map[S - 1], low_map[3] = 3, -2
    refusals = [
        (dict(models=[], scene_model=None), b"n_models = 0"),
        (dict(models=models * 3, scene_model=None), b"n_models = 9"),
        (dict(models=models, scene_model=bad_map), b"scene %d is given model 3" % (S - 1)),
        (dict(models=models, scene_model=low_map), b"scene 3 is given model -2"),
        (dict(models=models, scene_model=None, frames=3), b"FB_FRAMES_BATCH"),
        (dict(models=[models[0], null, models[2]], scene_model=None), b"model 1:"),
        (dict(models=[models[0], models[1], hot], scene_model=None), b"model 2:"),
    ]
    for kw, text in refusals:
        assert _attach_models(sb, kw["models"], kw.get("frames", 1), kw["scene_model"], cap) == _lib.E_ARG, text
        assert text in L.mmw_last_error(sb.h), (text, L.mmw_last_error(sb.h))
        assert np.array_equal(_get_models(sb), model_of % 2)
        assert _estimate(sb) == _estimate(clean) == eligible
        assert _group_rows(sb, 2) == _group_rows(clean, 2)
        (na, ta), (nb, tb) = _live(sb), _live(clean)
        assert np.array_equal(na, nb) and all(ta[s, : na[s]].tobytes() == tb[s, : nb[s]].tobytes() for s in range(S)), text
    hot.free()
    # mmw_posture_set_scene_models: refused on the host, the map stays
    for scenes, ids, text in (([3, 5, 3], [0, 1, 0], b"entry 2"), ([0, S], [1, 1], b"entry 1"), ([0, -1], [1, 1], b"entry 1"),
                              ([4, 6], [0, 2], b"entry 1"), ([4, 6], [-2, 0], b"entry 0"), (None, [0] * (S + 1), b"n = %d" % (S + 1))):
        assert _set_models(sb, ids, scenes) == _lib.E_ARG, text
        assert text in L.mmw_last_error(sb.h), (text, L.mmw_last_error(sb.h))
        assert np.array_equal(_get_models(sb), model_of % 2)
    assert _set_models(sb, [NONE, 1], [4, 6]) == 0 and _get_models(sb)[4] == NONE and _get_models(sb)[6] == 1
    assert _set_models(sb, []) == 0                                             # n = 0: nothing changes
    # a one-model attachment takes MMW_POSTURE_NONE as well; the legacy entry attaches the map "every scene on model 0"
    assert L.mmw_posture_attach_frames(sb.h, C.byref(models[0].struct), 1, cap) == 0 and (_get_models(sb) == 0).all()
    assert _estimate(sb) == eligible and _group_rows(sb, 1) == [eligible]
    assert _set_models(sb, [NONE] * S) == 0 and _estimate(sb) == 0 and _group_rows(sb, 1) == [0]   # every scene excluded: an empty call
    # detach through the old entry: MMW_E_ARG afterwards, and a second detach is fine
    assert _attach_models(sb, models, 1, model_of, cap) == 0
    assert L.mmw_posture_attach(sb.h, None, 0) == 0
    assert L.mmw_estimate_posture(sb.h, C.byref(rows)) == _lib.E_ARG
    assert L.mmw_posture_get_scene_models(sb.h, few.ctypes.data) == _lib.E_ARG and _set_models(sb, [0]) == _lib.E_ARG
    assert L.mmw_posture_group_rows(sb.h, few.ctypes.data, C.byref(n)) == _lib.E_ARG and n.value == -5
    assert L.mmw_posture_attach(sb.h, None, 0) == 0
    for m in models + cmodels:
        m.free()
    sb.close(); clean.close()
