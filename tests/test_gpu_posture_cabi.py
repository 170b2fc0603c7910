"""GPU tests of the batched estimate_posture behind the C-ABI (include/mmw.h: mmw_posture_attach / mmw_posture_attach_frames,
mmw_estimate_posture, mmw_posture_range) for both models -- the 3-frame define_CNN_3D and the single-frame define_CNN, one test body
per assertion, parametrised over `frames` -- and of its two kernels (mmw_mars_dense2, mmw_mars_split_weights; csrc/k_dense2.hip).
What exists for the single-frame model only is in test_gpu_posture_single_frame.py.

Tolerances are the project's: keypoints within 1e-4 * max(1, |want|) of the fp64 oracle, tracker state bit
for bit.  Dense-2 is additionally held against the kernel it stands in for (torch.addmm, MarsCNN's call) in the form the Dense-1
test uses: error <= 2 x addmm's error + 5e-7, both measured here against fp64 on the same fp32 operands."""
import ctypes as C

import numpy as np
import pytest

from tests import _posture_cabi as pc
from tests._layouts import make_checked
from tests._posture_gpu import CANARY, KP_TOL, KW, N, CModel, _live, _step, _stream, _weights, attach_batch

pytestmark = pytest.mark.gpu


# ---- 1. k_split_weights ------------------------------------------------------------------------------------------------------
def _split_on_device(w32):
    """(w16 as a CPU int16 tensor, flag) of mmw_mars_split_weights on the fp32 CPU tensor w32[n][k]."""
    import torch
    from mmwave_msc_amd import _lib
    L = _lib.load()
    n, k = w32.shape
    d_w = w32.cuda().contiguous()
    d_out = torch.full((n, 2 * k), -1, dtype=torch.int16, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = L.mmw_mars_split_weights(_stream(), d_w.data_ptr(), k, d_out.data_ptr(), 2 * k, n, k, flag.data_ptr())
    assert rc == 0, L.mmw_last_error(None)
    torch.cuda.synchronize()
    return d_out.cpu(), int(flag.item())


def test_split_weights_equals_interleave_split_bit_for_bit():
    import torch
    from mmwave_msc_amd.mars import interleave_split
    from mmwave_msc_amd.marsweights import fold_keras_weights
    w32 = torch.from_numpy(fold_keras_weights(_weights(3, 3))["dense1_w"])
    assert tuple(w32.shape) == (1536, 6144)
    got, flag = _split_on_device(w32)
    assert flag == 0
    assert torch.equal(got, interleave_split(w32).view(torch.int16))
    # subnormals of fp32 and of fp16, both zeros, values next to fp16's largest -- and then one entry outside its range
    rng = np.random.default_rng(8)
    m = rng.normal(0.0, 1.0, size=(64, 96)).astype(np.float32)
    m[0, :8] = [0.0, -0.0, 1e-40, -1e-40, 3e-6, -5.9e-8, 65503.0, -65000.0]
    m[5, 40:44] = [2.0 ** -24, 2.0 ** -25, 6.1e-5, -6.0e-5]
    t = torch.from_numpy(m.copy())
    got, flag = _split_on_device(t)
    assert flag == 0, "nothing here is outside fp16's range"
    assert torch.equal(got, interleave_split(t).view(torch.int16))
    m[63, 95] = 7e4
    t = torch.from_numpy(m.copy())
    got, flag = _split_on_device(t)
    assert flag == 1
    assert torch.equal(got, interleave_split(t).view(torch.int16))


# ---- 2. k_mars_dense2 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 57, 256, 8500, 31744])
def test_dense2_against_fp64_and_addmm(n):
    import torch
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.marsweights import fold_keras_weights
    L = _lib.load()
    f = fold_keras_weights(_weights(5, 3))
    dev = torch.device("cuda", 0)
    w2, b2 = torch.from_numpy(f["dense2_w"]).to(dev), torch.from_numpy(f["dense2_b"]).to(dev)
    g = torch.Generator(device="cpu").manual_seed(100 + n)
    hidden = torch.relu(torch.randn((n, 1536), generator=g) * 1.5 + 0.3).to(dev)   # what Dense-1's relu leaves: about 40 % zeros
    pad = 300   # canary rows behind the batch: a 128-row tile and more

    def run(h):
        kp = torch.full((h.shape[0] + pad, 57), CANARY, dtype=torch.float32, device=dev)
        rc = L.mmw_mars_dense2(_stream(), h.data_ptr(), h.stride(0), w2.data_ptr(), b2.data_ptr(), kp.data_ptr(), h.shape[0], 1536)
        assert rc == 0, L.mmw_last_error(None)
        torch.cuda.synchronize()
        return kp

    kp = run(hidden)
    assert bool((kp[n:] == CANARY).all()), "rows past n were written"
    want = b2.double() + hidden.double() @ w2.double().t()
    ref = torch.addmm(b2, hidden, w2.t())
    scale = want.abs().clamp(min=1.0)
    ek, eg = float(((kp[:n].double() - want).abs() / scale).max()), float(((ref.double() - want).abs() / scale).max())
    print(f"dense2 n={n}: error {ek:.3e}, torch.addmm {eg:.3e}")
    assert ek <= KP_TOL, (ek, eg)
    assert ek <= 2.0 * eg + 5e-7, (ek, eg)
    assert torch.equal(run(hidden).view(torch.int32), kp.view(torch.int32)), "two runs differ"
    # a row's result does not depend on the batch around it (the same summation order for every row and batch size) ...
    if n >= 57:
        sub = run(hidden[40:57].contiguous())
        assert torch.equal(sub[:17].view(torch.int32), kp[40:57].view(torch.int32))
    # ... and a NaN row stays in its own output row
    bad = hidden.clone()
    r = n // 2
    bad[r, 7] = float("nan")
    kpn = run(bad)
    assert bool(torch.isnan(kpn[r]).all())
    keep = torch.ones(n + pad, dtype=torch.bool, device=dev)
    keep[r] = False
    assert torch.equal(kpn[keep].view(torch.int32), kp[keep].view(torch.int32))
    # a padded leading dimension reads the same values
    if n <= 8500:
        wide = torch.zeros((n, 1536 + 64), dtype=torch.float32, device=dev)
        wide[:, :1536] = hidden
        wide[:, 1536:] = float("nan")
        kpw = torch.full((n + pad, 57), CANARY, dtype=torch.float32, device=dev)
        assert L.mmw_mars_dense2(_stream(), wide.data_ptr(), wide.stride(0), w2.data_ptr(), b2.data_ptr(), kpw.data_ptr(), n, 1536) == 0
        torch.cuda.synchronize()
        assert torch.equal(kpw.view(torch.int32), kp.view(torch.int32))


# ---- 3. + 4. end to end through the C entries, against the oracle and against PosturePipeline ----------------------------------
PINNED = {(1, 48): pc.SINGLE_FRAME_48}   # (frames, S) -> what the oracle run is known to give
_REF = {}


def _ref(frames, S):
    """scenario(S) and its oracle run for the model of `frames` frames, computed once for the cases that follow one another and
    never changed (one slot: the 640-scene run is not kept)."""
    if (frames, S) not in _REF:
        _REF.clear()
        pts, cnt, dts = pc.scenario(S)
        w = _weights(0, frames)
        _REF[frames, S] = dict(pts=pts, cnt=cnt, dts=dts, w=w, ref=pc.oracle_run(pts, cnt, dts, w, cfg_kw=KW[frames]))
    return _REF[frames, S]


@pytest.mark.parametrize("frames,S,layout", [(3, 48, "one_workgroup"), (3, 640, "track_wise"), (1, 48, "one_workgroup"), (1, 48, "per_scene")],
                         ids=["48-one_workgroup", "640-track_wise", "single_frame-48-one_workgroup", "single_frame-48-per_scene"])
def test_estimate_posture_through_the_c_entries_vs_oracle_and_pipeline(frames, S, layout):
    from mmwave_msc_amd.marsweights import model_dims
    r = _ref(frames, S)
    pts, cnt, dts, w, ref = r["pts"], r["cnt"], r["dts"], r["w"], r["ref"]
    F = cnt.shape[0]
    assert 3 * ref["tracked_by_4"] >= S and ref["expired"] >= 1
    for name, value in PINNED.get((frames, S), {}).items():
        assert ref[name] == value, name
    # -- the C entries only: ctypes, mmw_dev_alloc / mmw_memcpy_*, no torch tensor on the path
    sb = make_checked(S, N, layout, **KW[frames])
    assert sb.ring == frames and (sb.step_kind() == 1) == (layout == "one_workgroup") and (sb.step_kind() == 4 or layout != "track_wise")
    L = sb.L
    model = CModel(sb, w)
    assert attach_batch(sb, frames, model.struct, S * sb.track_cap) == 0, L.mmw_last_error(sb.h)
    for f in range(F):
        _step(sb, pts[f], cnt[f], dts[f])
        rows = C.c_int32(-1)
        assert L.mmw_estimate_posture(sb.h, C.byref(rows)) == 0, L.mmw_last_error(sb.h)
        assert rows.value == ref["rows"][f], (f, rows.value, ref["rows"][f])
    ntr, trk = _live(sb)
    word = C.c_int32(-1)
    assert L.mmw_posture_range(sb.h, C.byref(word)) == 0 and word.value == 0
    checked, worst = 0, 0.0
    for s in range(S):   # every live track of every scene
        want, got = ref["finals"][s], trk[s, : ntr[s]]
        assert len(want) == int(ntr[s]), s
        for name in pc.STATE_FIELDS:
            assert np.array_equal(got[name], want[name]), (s, name)
        worst = max(worst, pc.kp_err(got["keypoints"], ref["want_kp"][s]))
        checked += len(want)
    print(f"C entries, {frames}-frame model, {S} scenes, {layout}: {checked} tracks, keypoint error {worst:.3e}")
    assert checked == ref["samples_cnn"] >= S // 3
    assert worst <= KP_TOL, worst
    feat_c, owner_c = sb.features_host()
    # -- the same frames through PosturePipeline(overlap=False) + MarsCNN on a twin context
    import torch
    from mmwave_msc_amd.mars import MarsCNN
    from mmwave_msc_amd.posture import PosturePipeline
    twin = make_checked(S, N, layout, **KW[frames])
    cnn = MarsCNN.from_keras_weights(w).to("cuda:0")
    assert cnn.frames == frames
    pipe = PosturePipeline(twin, cnn, S * twin.track_cap, overlap=False)
    for f in range(F):
        _step(twin, pts[f], cnt[f], dts[f])
        pipe.after_step()
        twin.synchronize()   # (the input buffers are rewritten by the next frame's uploads)
    pipe.close()
    ntr2, trk2 = _live(twin)
    assert np.array_equal(ntr, ntr2)
    between = 0.0
    for s in range(S):
        a, b = trk[s, : ntr[s]], trk2[s, : ntr2[s]]
        for name in pc.STATE_FIELDS + ("uid", "min_vals", "max_vals", "n_est", "ring_len"):
            assert np.array_equal(a[name], b[name]), (s, name)
        between = max(between, pc.kp_err(a["keypoints"], b["keypoints"].astype(np.float64)))
    print(f"C entries against PosturePipeline: keypoints differ by {between:.3e}")
    assert between <= KP_TOL, between
    feat_p, owner_p = twin.features_host()
    assert np.array_equal(owner_c, owner_p) and np.array_equal(owner_c, ref["owners"][F - 1])
    assert feat_c.shape == (ref["rows"][F - 1],) + model_dims(frames).input and feat_c.tobytes() == feat_p.tobytes()
    assert attach_batch(sb, frames, None, 0) == 0
    model.free()
    twin.close()
    sb.close()
    torch.cuda.synchronize()


# ---- 5. range ----------------------------------------------------------------------------------------------------------------
def _outside_fp16(w):
    """Two sets of folded-tensor replacements for CModel that the batched chain must refuse: a BatchNorm-folded Dense-1 row of
    3e6, and a conv bias that is not finite."""
    from mmwave_msc_amd.marsweights import fold_keras_weights
    f32 = fold_keras_weights(w)
    d1 = f32["dense1_w"].copy()
    d1[100] *= np.float32(3e6 / np.abs(d1[100]).max())
    cb = f32["conv2_b"].copy()
    cb[3] = np.float32("inf")
    return dict(dense1_w=d1), dict(conv2_b=cb)


# (the largest keypoint the oracle gives the repaired sample: both far outside fp16's range; the single-frame model's is pinned)
@pytest.mark.parametrize("frames,hot_kp", [(3, (1e3, np.inf)), (1, (1.3e5, 1.5e5))], ids=["3", "1"])
def test_out_of_range_sample_is_repaired_and_bad_weights_are_refused(frames, hot_kp):
    """The intensities of the last frame of a one-person scene scaled by 1e5 push ONE feature tensor of the last call out of fp16's
    range: the device-side fp32 repair (k_mars_conv / k_mars_conv2d) recomputes that sample (bit 0 of the range word, read once),
    its keypoints -- and everybody else's -- stay within 1e-4 of the fp64 oracle.  A model with a BatchNorm-folded Dense-1 row of
    3e6, or a conv bias that is not finite, is refused with MMW_E_ARG and the context goes on stepping."""
    from mmwave_msc_amd import _lib
    S, HOT = 16, 2
    pts, cnt, dts = pc.scenario(S, seed=6100)
    F = cnt.shape[0]
    pts[F - 1, HOT, :, 7] *= 1e5   # peakVal: (1e5 * 30 - mu) / std leaves 65 504 far behind; the tracker does not read the column
    w = _weights(2, frames)
    ref = pc.oracle_run(pts, cnt, dts, w, cfg_kw=KW[frames])
    hot = [int((np.abs(f.reshape(len(f), -1)).max(axis=1) >= 65504.0).sum()) if len(f) else 0 for f in ref["feats"]]
    assert hot == [0] * (F - 1) + [1], hot
    largest = float(np.abs(ref["want_kp"][HOT]).max()) if len(ref["want_kp"][HOT]) else 0.0
    assert hot_kp[0] < largest < hot_kp[1], largest
    sb = make_checked(S, N, "per_scene", **KW[frames])
    sb.attach_posture_batch(w, S * sb.track_cap)
    for f in range(F):
        if f == F - 1:
            assert sb.posture_range() == 0, "nothing left fp16's range before the last frame"
        _step(sb, pts[f], cnt[f], dts[f])
        assert sb.estimate_posture() == ref["rows"][f]
    ntr, trk = _live(sb)
    assert sb.posture_range() == 1, "bit 0: a sample was repaired; bit 1 (surplus) must be clear"
    assert sb.posture_range() == 0, "the word is cleared by the read"
    worst, worst_hot = 0.0, 0.0
    for s in range(S):
        assert len(ref["finals"][s]) == int(ntr[s])
        e = pc.kp_err(trk[s, : ntr[s]]["keypoints"], ref["want_kp"][s])
        worst, worst_hot = max(worst, e), (e if s == HOT else worst_hot)
    print(f"range, {frames}-frame model: keypoint error {worst:.3e} over all tracks, {worst_hot:.3e} for the repaired sample")
    assert int(ntr[HOT]) >= 1 and worst <= KP_TOL, (worst, worst_hot)
    # weights outside fp16's range: refused, loudly, and nothing changes
    before = trk.tobytes()
    bad, bad2 = (CModel(sb, w, **rep) for rep in _outside_fp16(w))
    assert attach_batch(sb, frames, bad.struct, 64) == _lib.E_ARG
    assert b"fp16" in sb.L.mmw_last_error(sb.h)
    assert attach_batch(sb, frames, bad2.struct, 64) == _lib.E_ARG
    assert _live(sb)[1].tobytes() == before
    _step(sb, pts[F - 1], cnt[F - 1], dts[F - 1])          # the context still steps, and the earlier model is still attached
    assert sb.estimate_posture() >= 1
    sb.check()
    bad.free(); bad2.free()
    sb.close()


# ---- 6. refusals, capacity, detach, sites ------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames,null_field,short_ld", [(3, "dense2_b", 6142), (1, "conv2_w", 2044)], ids=["3", "1"])
def test_refusals_capacity_and_detach(frames, null_field, short_ld):
    from mmwave_msc_amd import _lib
    S = 16
    pts, cnt, dts = pc.scenario(S, seed=6300)
    w = _weights(1, frames)
    sb = make_checked(S, N, "per_scene", **KW[frames])
    L = sb.L
    rows, word = C.c_int32(5), C.c_int32(5)
    assert L.mmw_estimate_posture(sb.h, C.byref(rows)) == _lib.E_ARG and rows.value == 0      # no model
    assert L.mmw_posture_range(sb.h, C.byref(word)) == _lib.E_ARG
    model = CModel(sb, w)
    assert attach_batch(sb, frames, model.struct, 0) == _lib.E_ARG                             # cap_rows < 1
    null = _lib.MmwPostureModel.from_buffer_copy(model.struct)
    setattr(null, null_field, None)
    assert attach_batch(sb, frames, null, 64) == _lib.E_ARG                                    # a null pointer
    off = _lib.MmwPostureModel.from_buffer_copy(model.struct)
    off.dense1_ld = short_ld
    assert attach_batch(sb, frames, off, 64) == _lib.E_ARG                                     # dense1_ld
    for rep in _outside_fp16(w):                                                               # weights outside fp16's range
        bad = CModel(sb, w, **rep)
        assert attach_batch(sb, frames, bad.struct, 64) == _lib.E_ARG and b"fp16" in L.mmw_last_error(sb.h)
        bad.free()
    assert L.mmw_estimate_posture(sb.h, None) == _lib.E_ARG                                    # ... none of them attached anything
    # capacity: one row short of the eligible tracks
    for f in range(6):                                                                         # (and the context still steps)
        _step(sb, pts[f], cnt[f], dts[f])
    sb.check()
    feat, owner = sb.features_host()
    eligible = len(owner)
    assert eligible >= 8
    assert attach_batch(sb, frames, model.struct, eligible) == 0, L.mmw_last_error(sb.h)
    assert L.mmw_estimate_posture(sb.h, C.byref(rows)) == 0 and rows.value == eligible
    _, before = _live(sb)
    _step(sb, pts[6], cnt[6], dts[6])
    eligible = len(sb.features_host()[1])
    _, stepped = _live(sb)
    assert attach_batch(sb, frames, model.struct, eligible - 1) == 0
    assert L.mmw_estimate_posture(sb.h, C.byref(rows)) == _lib.E_CAPACITY and rows.value == 0
    assert b"cap_rows" in L.mmw_last_error(sb.h)
    assert sb.tracks(cap=stepped.shape[1]).tobytes() == stepped.tobytes(), "a keypoint changed in a refused call"
    assert stepped["keypoints"].tobytes() != np.zeros_like(stepped["keypoints"]).tobytes() and before.shape[0] == S
    # detach, then MMW_E_ARG again
    assert attach_batch(sb, frames, None, 0) == 0
    assert L.mmw_estimate_posture(sb.h, C.byref(rows)) == _lib.E_ARG
    assert attach_batch(sb, frames, None, 0) == 0   # (detaching twice is fine)
    model.free()
    sb.close()


def test_mixed_sites_give_each_scene_the_keypoints_of_its_uniform_context():
    """As test_gpu_sites.py does for the features: a context whose scenes carry different sites (intensity scales) gives every
    scene the keypoints of a context created with that site as its configuration, bit for bit."""
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    from tests.test_gpu_sites import KW, SITES, _inputs, _site_rows
    S, F = 12, 10
    raw, cnt, dts, which = _inputs(S, 256, F, seed=2500)
    w = _weights(4, 3)

    def run(sb):
        sb.attach_posture_batch(w, S * sb.track_cap)
        b_pts, b_no = sb.buf("p_pts", S * 256 * 64), sb.buf("p_no", S * 4)
        total = 0
        for f in range(F):
            b_raw = sb.buf("p_raw", raw[f].nbytes).upload(raw[f])
            b_n = sb.buf("p_n", S * 4).upload(cnt[f])
            b_dt = sb.buf("p_dt", S * 8).upload(dts[f])
            sb.normalize_dev(b_raw.ptr, b_n.ptr, b_pts.ptr, b_no.ptr)
            sb.step_dev(b_pts.ptr, b_no.ptr, b_dt.ptr)
            total += sb.estimate_posture()
            sb.synchronize()
        sb.check()
        ntr = sb.num_tracks()
        trk = sb.tracks()
        out = [trk[s, : ntr[s]]["keypoints"].tobytes() for s in range(S)]
        sb.close()
        return out, total

    mixed = SceneBatch(_lib.default_config(**KW), S, 256)
    mixed.set_sites(_site_rows(mixed.cfg, [SITES[k] for k in which]))
    m_kp, m_rows = run(mixed)
    assert m_rows >= S
    differs = 0
    for k, site in enumerate(SITES):
        u_kp, _ = run(SceneBatch(_lib.default_config(**KW, **site), S, 256))
        for s in range(S):
            if which[s] == k:
                assert len(m_kp[s]) > 0 and m_kp[s] == u_kp[s], (k, s)
            else:
                differs += m_kp[s] != u_kp[s]
    assert differs >= S // 2   # scenes under another site's intensity scale come out differently
