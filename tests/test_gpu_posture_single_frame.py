"""GPU tests of the single-frame posture model (define_CNN, train.py:33-68) behind the C-ABI: the fp32 Conv2D pair
(mmw_mars_conv2d; csrc/k_mars2d.hip), Dense-2 at k = 512, the range repair (mmw_mars_range_fixup_frames), the `frames` argument of
mmw_posture_attach_frames and the one-scene chain (mmw_attach_posture_frames / mmw_frame_posture_host) on contexts with
FB_FRAMES_BATCH = 0.  The batched chain itself (mmw_posture_attach_frames / mmw_estimate_posture / mmw_posture_range) is tested
for both models in test_gpu_posture_cabi.py.

Tolerances are the project's: conv activations within 1e-4 of the fp64 _conv_same (test_hip_convs_match_torch_and_oracle),
keypoints within 1e-4 * max(1, |want|) of oracle/mars_np.py (tests/_posture_cabi.kp_err), the range repair within 1e-4 of the
sample's largest output (test_split_arithmetic_knows_fp16s_range), Dense-2 within 2 x torch.addmm's error + 5e-7
(test_dense2_against_fp64_and_addmm), tracker state bit for bit."""
import ctypes as C

import numpy as np
import pytest

from tests import _posture_cabi as pc
from tests._layouts import make_checked
from tests._posture_gpu import CANARY, KP_TOL, KW, N, CModel, _dev, _live, _step, _stream, _weights

pytestmark = pytest.mark.gpu
KW1 = KW[1]


# ---- 1. k_mars_conv2d ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 7, 65, 600])
def test_conv2d_against_fp64_and_torch(batch):
    import torch
    from mmwave_msc_amd import _lib
    from oracle.mars_np import _conv_same
    L = _lib.load()
    w = _weights(11, 1)
    rng = np.random.default_rng(batch)
    x = rng.normal(0, 0.5, size=(batch, 8, 8, 5)).astype(np.float32)
    x[:, 6:, :, :] = 0.0   # zero-padded rows as real feature maps have
    wd = {k: _dev(w[k].reshape(-1)) for k in ("conv1_w", "conv1_b", "conv2_w", "conv2_b")}
    pad = 3   # canary samples behind the batch

    def run(xs):
        n = xs.shape[0]
        xt = _dev(xs)
        out = torch.full((n + pad, 64, 32), CANARY, dtype=torch.float32, device="cuda")
        rc = L.mmw_mars_conv2d(_stream(), xt.data_ptr(), wd["conv1_w"].data_ptr(), wd["conv1_b"].data_ptr(), wd["conv2_w"].data_ptr(),
                               wd["conv2_b"].data_ptr(), out.data_ptr(), n)
        assert rc == 0, L.mmw_last_error(None)
        torch.cuda.synchronize()
        return out

    out = run(x)
    assert bool((out[batch:] == CANARY).all()), "rows past n were written"
    got = out[:batch].cpu().numpy().reshape(batch, 8, 8, 32)
    f64 = {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}
    h = np.maximum(_conv_same(x.astype(np.float64), f64["conv1_w"], f64["conv1_b"]), 0)
    ref = np.maximum(_conv_same(h, f64["conv2_w"], f64["conv2_b"]), 0)
    # torch's convolutions, run because this test asks for them: (kh,kw,in,out) -> (out,in,kh,kw), channels-first and back
    F = torch.nn.functional
    w1t, w2t = _dev(w["conv1_w"].transpose(3, 2, 0, 1)), _dev(w["conv2_w"].transpose(3, 2, 0, 1))
    ht = torch.relu(F.conv2d(_dev(x).permute(0, 3, 1, 2), w1t, wd["conv1_b"], padding=1))
    ref_t = torch.relu(F.conv2d(ht, w2t, wd["conv2_b"], padding=1)).permute(0, 2, 3, 1).cpu().numpy()
    e64, et = float(np.abs(got - ref).max()), float(np.abs(got - ref_t).max())
    print(f"conv2d batch={batch}: error {e64:.3e} against fp64, {et:.3e} against torch.conv2d; largest activation {np.abs(ref).max():.3f}")
    assert e64 <= 1e-4 and et <= 1e-4, (e64, et)
    assert (ref > 0).mean() > 0.2 and (ref == 0).mean() > 0.2   # (both sides of the ReLU are exercised)
    assert torch.equal(run(x).view(torch.int32), out.view(torch.int32)), "two runs differ"
    # a sample's result does not depend on the batch around it ...
    if batch >= 57:
        sub = run(x[40:57])
        assert torch.equal(sub[:17].view(torch.int32), out[40:57].view(torch.int32))
    # ... and a NaN sample stays in its own rows (NaN through the ReLUs, as Keras')
    bad = x.copy()
    r = batch // 2
    bad[r, 3, 4, 2] = np.nan
    outn = run(bad)
    assert bool(torch.isnan(outn[r]).any())
    keep = torch.ones(batch + pad, dtype=torch.bool, device="cuda")
    keep[r] = False
    assert torch.equal(outn[keep].view(torch.int32), out[keep].view(torch.int32))


# ---- 2. k_mars_dense2 at k = 512 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 57, 256, 1000])
def test_dense2_at_k_512_against_fp64_and_addmm(n):
    import torch
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.marsweights import fold_keras_weights
    L = _lib.load()
    f = fold_keras_weights(_weights(5, 1))
    assert f["dense2_w"].shape == (57, 512)
    dev = torch.device("cuda", 0)
    w2, b2 = torch.from_numpy(f["dense2_w"]).to(dev), torch.from_numpy(f["dense2_b"]).to(dev)
    g = torch.Generator(device="cpu").manual_seed(100 + n)
    hidden = torch.relu(torch.randn((n, 512), generator=g) * 1.5 + 0.3).to(dev)   # what Dense-1's relu leaves: about 40 % zeros
    pad = 300   # canary rows behind the batch: a 128-row tile and more

    def run(h, k=512):
        kp = torch.full((h.shape[0] + pad, 57), CANARY, dtype=torch.float32, device=dev)
        rc = L.mmw_mars_dense2(_stream(), h.data_ptr(), h.stride(0), w2.data_ptr(), b2.data_ptr(), kp.data_ptr(), h.shape[0], k)
        assert rc == 0, L.mmw_last_error(None)
        torch.cuda.synchronize()
        return kp

    kp = run(hidden)
    assert bool((kp[n:] == CANARY).all()), "rows past n were written"
    want = b2.double() + hidden.double() @ w2.double().t()
    ref = torch.addmm(b2, hidden, w2.t())
    scale = want.abs().clamp(min=1.0)
    ek, eg = float(((kp[:n].double() - want).abs() / scale).max()), float(((ref.double() - want).abs() / scale).max())
    print(f"dense2 k=512 n={n}: error {ek:.3e}, torch.addmm {eg:.3e}")
    assert ek <= KP_TOL, (ek, eg)
    assert ek <= 2.0 * eg + 5e-7, (ek, eg)
    assert torch.equal(run(hidden).view(torch.int32), kp.view(torch.int32)), "two runs differ"
    if n >= 57:   # a row's result does not depend on the batch around it
        sub = run(hidden[40:57].contiguous())
        assert torch.equal(sub[:17].view(torch.int32), kp[40:57].view(torch.int32))
    bad = hidden.clone()   # a NaN row stays in its own output row
    r = n // 2
    bad[r, 7] = float("nan")
    kpn = run(bad)
    assert bool(torch.isnan(kpn[r]).all())
    keep = torch.ones(n + pad, dtype=torch.bool, device=dev)
    keep[r] = False
    assert torch.equal(kpn[keep].view(torch.int32), kp[keep].view(torch.int32))
    wide = torch.zeros((n, 512 + 64), dtype=torch.float32, device=dev)   # a padded leading dimension reads the same values
    wide[:, :512] = hidden
    wide[:, 512:] = float("nan")
    assert torch.equal(run(wide).view(torch.int32), kp.view(torch.int32))


# ---- 3. mmw_mars_range_fixup_frames(frames = 1) on its own ------------------------------------------------------------------------
@pytest.mark.parametrize("hot", [(3, 77, 199), tuple(range(5, 75))], ids=["3_hot", "70_hot"])
def test_range_fixup_single_frame_rewrites_exactly_the_flagged_rows(hot):
    """The list mmw_mars_conv_split(frames = 1) builds, repaired by mmw_mars_range_fixup_frames(frames = 1): the flagged rows of a
    canary-filled kp are rewritten in fp32 (within 1e-4 of the oracle, scaled by the sample's largest output), every other row
    keeps the canary, the list is emptied; 70 flagged samples raise bit 1 and exactly 64 of them are rewritten."""
    import torch
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.marsweights import FOLDED_KEYS, fold_keras_weights
    from oracle.mars_np import mars_forward_np
    L = _lib.load()
    n = 200
    w = _weights(3, 1)
    f = fold_keras_weights(w)
    rng = np.random.default_rng(17)
    feat = rng.normal(0, 0.5, size=(n, 8, 8, 5)).astype(np.float32)
    feat[list(hot)] *= np.float32(1e5)
    want = mars_forward_np(w, feat[list(hot)].astype(np.float64))
    d = {k: _dev(f[k]) for k in FOLDED_KEYS}
    x = _dev(feat)
    ld = 2 * 2048 + 256
    act16 = torch.zeros((256, ld), dtype=torch.float16, device="cuda")
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    flags = torch.zeros(2 + 64, dtype=torch.int32, device="cuda")
    rc = L.mmw_mars_conv_split(_stream(), 1, x.data_ptr(), d["conv1_w"].data_ptr(), d["conv1_b"].data_ptr(), d["conv2_w"].data_ptr(),
                               d["conv2_b"].data_ptr(), act16.data_ptr(), ld, n, word.data_ptr(), flags.data_ptr())
    assert rc == 0, L.mmw_last_error(None)
    torch.cuda.synchronize()
    listed = flags.cpu().numpy()
    assert listed[0] == len(hot) and int(word.item()) == 1
    assert set(listed[2:2 + min(len(hot), 64)]) <= set(hot) and len(set(listed[2:2 + min(len(hot), 64)])) == min(len(hot), 64)
    word.zero_()
    kp = torch.full((n, 57), CANARY, dtype=torch.float32, device="cuda")
    scratch = torch.zeros(_lib.RANGE_FIXUP_SCRATCH, dtype=torch.uint8, device="cuda")
    rc = L.mmw_mars_range_fixup_frames(_stream(), 1, x.data_ptr(), flags.data_ptr(), n, d["conv1_w"].data_ptr(), d["conv1_b"].data_ptr(),
                                       d["conv2_w"].data_ptr(), d["conv2_b"].data_ptr(), d["dense1_w"].data_ptr(), 2048, d["dense1_b"].data_ptr(),
                                       d["dense2_w"].data_ptr(), d["dense2_b"].data_ptr(), scratch.data_ptr(), kp.data_ptr(), word.data_ptr())
    assert rc == 0, L.mmw_last_error(None)
    torch.cuda.synchronize()
    got = kp.cpu().numpy()
    after = flags.cpu().numpy()
    rewritten = sorted(int(i) for i in np.nonzero((got != CANARY).any(axis=1))[0])
    assert after[0] == 0, "the list is emptied for the next call"
    if len(hot) <= 64:
        assert rewritten == sorted(hot) and after[1] == len(hot)
        assert int(word.item()) & 2 == 0, "bit 1 stays clear"
    else:
        assert len(rewritten) == 64 and after[1] == 64 and rewritten == sorted(int(i) for i in listed[2:66])
        assert int(word.item()) & 2 == 2, "more flagged samples than the fix-up holds"
    rows = [list(hot).index(i) for i in rewritten]
    assert (got[rewritten] != CANARY).all()
    err = float((np.abs(got[rewritten] - want[rows]) / np.maximum(1.0, np.abs(want[rows]).max(axis=1, keepdims=True))).max())
    print(f"range fix-up, {len(hot)} hot samples: {len(rewritten)} rows rewritten, error {err:.3e}; largest keypoint {np.abs(want).max():.3e}")
    assert err <= 1e-4 and float(np.abs(want).max()) > 1e3, err


# ---- 4. - 6. the batched chain: end to end, the range repair, refusals / capacity / detach are test_gpu_posture_cabi.py's tests,
#      parametrised over the model; here is what only the `frames` argument brings -------------------------------------------------
def test_frames_argument_and_the_model_are_held_to_the_contexts_ring():
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    S = 16
    w1, w3 = _weights(1, 1), _weights(1, 3)
    sb = make_checked(S, N, "per_scene", **KW1)
    L = sb.L
    model = CModel(sb, w1)
    # frames against the ring, both ways; rings nobody has a model for
    three = SceneBatch(_lib.default_config(**pc.KW), 4, N)
    m3 = CModel(three, w3)
    for ctx, mod, bad in ((three, m3, 1), (sb, model, 3), (sb, model, 2), (three, m3, 0)):
        assert L.mmw_posture_attach_frames(ctx.h, C.byref(mod.struct), bad, 64) == _lib.E_ARG, bad
        assert b"FB_FRAMES_BATCH" in L.mmw_last_error(ctx.h)
        assert L.mmw_estimate_posture(ctx.h, None) == _lib.E_ARG   # ... nothing was attached
    single = SceneBatch(_lib.default_config(fb_frames_batch=0, **pc.KW), 4, N)
    sm = CModel(single, w3)
    assert single.L.mmw_posture_attach(single.h, C.byref(sm.struct), 64) == _lib.E_ARG         # the legacy entry: FB_FRAMES_BATCH = 2 only
    assert b"FB_FRAMES_BATCH" in single.L.mmw_last_error(single.h)
    sm.free(); single.close()
    with pytest.raises(ValueError, match="3-frame.*FB_FRAMES_BATCH = 0"):
        sb.attach_posture_batch(w3)
    with pytest.raises(ValueError, match="1-frame.*FB_FRAMES_BATCH = 2"):
        three.attach_posture_batch(w1)
    one3 = SceneBatch(_lib.default_config(**pc.KW), 1, N)
    assert L.mmw_attach_posture_frames(one3.h, C.byref(m3.struct), 1) == _lib.E_ARG and b"FB_FRAMES_BATCH" in L.mmw_last_error(one3.h)
    one3.close()
    assert L.mmw_attach_posture_frames(sb.h, C.byref(model.struct), 1) == _lib.E_ARG and b"one-scene" in L.mmw_last_error(sb.h)
    model.free(); m3.free()
    three.close(); sb.close()


def test_frames_3_is_the_legacy_entry():
    """frames = 3 IS mmw_posture_attach: twin 16-scene contexts, byte-equal keypoints."""
    S = 16
    pts, cnt, dts = pc.scenario(S, seed=6300)
    w3 = _weights(1, 3)
    rows = C.c_int32(5)
    kps = []
    for entry in ("mmw_posture_attach", "mmw_posture_attach_frames"):
        ctx = make_checked(S, N, "per_scene", **pc.KW)
        L = ctx.L
        mod = CModel(ctx, w3)
        args = (ctx.h, C.byref(mod.struct), S * ctx.track_cap) if entry == "mmw_posture_attach" else (ctx.h, C.byref(mod.struct), 3, S * ctx.track_cap)
        assert getattr(L, entry)(*args) == 0, L.mmw_last_error(ctx.h)
        total = 0
        for f in range(8):
            _step(ctx, pts[f], cnt[f], dts[f])
            assert L.mmw_estimate_posture(ctx.h, C.byref(rows)) == 0
            total += rows.value
        ntr, trk = _live(ctx)
        kps.append((total, ntr.tobytes(), trk["keypoints"].tobytes()))
        mod.free()
        ctx.close()
    assert kps[0] == kps[1] and kps[0][0] >= S


# ---- 7. the one-scene chain ----------------------------------------------------------------------------------------------------
def test_one_scene_chain_runs_the_single_frame_model_behind_the_step():
    """mmw_attach_posture_frames(frames = 1) + mmw_frame_posture_host on a one-scene context with FB_FRAMES_BATCH = 0: rows and
    tracker state as the oracle's, keypoints within tolerance -- and BIT-equal to features -> mmw_mars_conv2d ->
    mmw_mars_head_small called one by one on a twin context (the same kernels, so the same bits)."""
    import torch
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    from mmwave_msc_amd.mars import MarsCNN
    from mmwave_msc_amd.synth import make_scene
    L = _lib.load()
    F = 12
    p, c, d = make_scene(4242, F, N, 2)
    pts, cnt, dts = p.astype(np.float64)[:, None], c[:, None], d[:, None]
    w = _weights(7, 1)
    ref = pc.oracle_run(pts, cnt, dts, w, cfg_kw=KW1)
    assert max(ref["rows"]) >= 2 and sum(ref["rows"]) >= 12, ref["rows"]
    model = MarsCNN.from_keras_weights(w).to("cuda:0")
    assert model.frames == 1 and not model.has_small_path()
    sb = SceneBatch(_lib.default_config(**KW1), 1, N)
    twin = SceneBatch(_lib.default_config(**KW1), 1, N)
    with pytest.raises(_lib.MmwError):
        sb.frame_host(cnt[0], dts[0], pts=pts[0], posture=True)   # no model attached yet: refused before anything is queued
    sb.attach_posture(model)
    w1 = model.dense1_dhwc.weight
    for f in range(F):
        r = sb.frame_host(cnt[f], dts[f], pts=pts[f], posture=True)
        assert r["posture_rows"] == ref["rows"][f], (f, r["posture_rows"], ref["rows"][f])
        twin.frame_host(cnt[f], dts[f], pts=pts[f])
        feat, owner = twin.features_host()
        assert len(owner) == ref["rows"][f] and feat.shape[1:] == (8, 8, 5)
        if len(owner):
            n = len(owner)
            x = _dev(feat)
            act = torch.empty((n, 2048), dtype=torch.float32, device="cuda")
            hidden = torch.empty((n, 512), dtype=torch.float32, device="cuda")
            kp = torch.empty((n, 57), dtype=torch.float32, device="cuda")
            assert L.mmw_mars_conv2d(_stream(), x.data_ptr(), model.k_w1.data_ptr(), model.k_b1.data_ptr(), model.k_w2.data_ptr(), model.k_b2.data_ptr(),
                                     act.data_ptr(), n) == 0, L.mmw_last_error(None)
            assert L.mmw_mars_head_small(_stream(), act.data_ptr(), 2048, w1.data_ptr(), w1.stride(0), model.dense1_dhwc.bias.data_ptr(),
                                         model.dense2.weight.data_ptr(), model.dense2.bias.data_ptr(), hidden.data_ptr(), kp.data_ptr(), n, 2048, 512) == 0
            torch.cuda.synchronize()
            twin.set_keypoints_host(kp.cpu().numpy(), owner)
        (na, ta), (nb, tb) = _live(sb), _live(twin)
        assert np.array_equal(na, nb)
        for name in ta.dtype.names:   # tracker state AND keypoints, bit for bit
            assert ta[name].tobytes() == tb[name].tobytes(), (f, name)
    ntr, trk = _live(sb)
    want, got = ref["finals"][0], trk[0, : ntr[0]]
    assert len(want) == int(ntr[0]) >= 2
    for name in pc.STATE_FIELDS:
        assert np.array_equal(got[name], want[name]), name
    err = pc.kp_err(got["keypoints"], ref["want_kp"][0])
    print(f"one-scene chain, single-frame model: {len(want)} tracks, keypoint error {err:.3e}")
    assert err <= KP_TOL, err
    sb.attach_posture(None)
    with pytest.raises(_lib.MmwError):
        sb.frame_host(cnt[0], dts[0], pts=pts[0], posture=True)
    sb.close(); twin.close()


def test_trackbuffer_attaches_a_single_frame_model_under_fb_frames_batch_0(monkeypatch):
    """TrackBuffer.attach_posture_model takes the single-frame MarsCNN when FB_FRAMES_BATCH = 0 (offline_main's one round trip per
    frame) and the attached loop equals the unattached one: tracker state bit for bit, keypoints within the CNN tolerance (the
    unattached loop runs the split-fp16 tiles, the attached one Keras' fp32).  What it refused before it still refuses."""
    import bench_ingest
    from mmwave_msc_amd import constants as const
    from mmwave_msc_amd.mars import MarsCNN
    from mmwave_msc_amd.synth import make_scene
    from mmwave_msc_amd.tracking import BatchedData, TrackBuffer
    w = _weights(9, 1)
    model = MarsCNN.from_keras_weights(w).to("cuda:0")
    model3 = MarsCNN.from_keras_weights(_weights(9, 3)).to("cuda:0")
    ring3 = TrackBuffer(max_pts=256)
    assert ring3.attach_posture_model(model) is False and ring3.attach_posture_model(model3) is True   # (FB_FRAMES_BATCH = 2: as before)
    ring3.close()
    monkeypatch.setattr(const, "FB_FRAMES_BATCH", 0)
    monkeypatch.setattr(const, "FB_FRAMES_BATCH_STATIC", 0)
    p, c, d = make_scene(91, 14, 220, 3, ragged=True)
    ang = np.radians(const.S_TILT)
    raw = bench_ingest.raw_rows_from_normalised(p, float(np.cos(ang)), float(np.sin(ang)), float(const.S_HEIGHT)).astype(np.float64)
    att, ab = TrackBuffer(max_pts=256), BatchedData()
    dev, db = TrackBuffer(max_pts=256), BatchedData()

    class KerasLike:
        def predict(self, x, verbose=0):
            return np.zeros((len(x), 57), np.float32)

    assert att.attach_posture_model(model3) is False and att.attach_posture_model(KerasLike()) is False and att._fused_model is None
    assert att.attach_posture_model(model) is True and att._fused_model is model
    estimated = 0
    for f in range(14):
        n = int(c[f])
        det = {k: list(raw[f, :n, i]) for i, k in enumerate(("x", "y", "z", "doppler", "peakVal"))}
        for tb, bb in ((att, ab), (dev, db)):
            tb.dt = float(d[f])
            kept = tb.track_raw(det, bb)
            if kept:
                assert tb._posture_done == (tb is att)
                tb.estimate_posture(model)
                assert not tb._posture_done
        ta, td = att.effective_tracks, dev.effective_tracks
        assert len(ta) == len(td), f
        for x, y in zip(ta, td):
            assert np.array_equal(x.state.x, y.state.x) and np.array_equal(x.state.P, y.state.P) and x.uid == y.uid, f
            assert pc.kp_err(x.keypoints, y.keypoints) <= KP_TOL, f
            estimated += int(not np.array_equal(x.keypoints, np.asarray(const.MODEL_DEFAULT_POSTURE, dtype=np.float32)))
    assert len(att.effective_tracks) >= 2 and estimated >= 10
    assert att.attach_posture_model(None) is False and att._fused_model is None
    att.close(); dev.close()
