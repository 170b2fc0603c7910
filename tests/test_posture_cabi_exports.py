"""The batched estimate_posture of the C-ABI (include/mmw.h: mmw_posture_attach, mmw_estimate_posture, mmw_posture_range) and its
two kernels (mmw_mars_dense2, mmw_mars_split_weights), as far as a machine without a GPU can check them: the symbols, the refusals
that never reach a device, the torch-free BatchNorm fold against MarsCNN's tensors, the fp64 statement of Dense-2 the GPU test
compares with, the scenario of the GPU test (oracle only) and the compiler's report on the new kernels."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from mmwave_msc_amd import _lib
from tests import _posture_cabi as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mmw_posture_attach", "mmw_estimate_posture", "mmw_posture_range", "mmw_mars_dense2", "mmw_mars_split_weights")


def test_new_symbols_are_exported_and_bound():
    L = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _lib.EXPORTS, name
        assert hasattr(raw, name), f"{name} not exported by libmmw_hip.so"
        assert getattr(L, name).argtypes is not None, f"{name} has no prototype in _lib.load()"


def test_null_context_is_refused():
    L = _lib.load()
    rows, word = C.c_int32(7), C.c_int32(7)
    m = _lib.MmwPostureModel()
    assert L.mmw_estimate_posture(None, C.byref(rows)) == _lib.E_ARG
    assert L.mmw_estimate_posture(None, None) == _lib.E_ARG
    assert L.mmw_posture_attach(None, C.byref(m), 16) == _lib.E_ARG
    assert L.mmw_posture_attach(None, None, 0) == _lib.E_ARG
    assert L.mmw_posture_range(None, C.byref(word)) == _lib.E_ARG
    assert b"null" in (L.mmw_last_error(None) or b"")


def test_kernel_entries_refuse_bad_arguments_without_a_device():
    """Negative counts, null operands, misaligned or short leading dimensions: MMW_E_ARG before any HIP call (where there is
    no GPU a launch would fail with MMW_E_HIP instead)."""
    L = _lib.load()
    p = 0x10000   # a 16-byte aligned non-null value; never dereferenced
    assert L.mmw_mars_dense2(None, p, 1536, p, p, p, -1, 1536) == _lib.E_ARG
    assert L.mmw_mars_dense2(None, None, 1536, p, p, p, 4, 1536) == _lib.E_ARG
    assert L.mmw_mars_dense2(None, p, 1536, None, p, p, 4, 1536) == _lib.E_ARG
    assert L.mmw_mars_dense2(None, p, 1536, p, None, p, 4, 1536) == _lib.E_ARG
    assert L.mmw_mars_dense2(None, p, 1536, p, p, None, 4, 1536) == _lib.E_ARG
    assert L.mmw_mars_dense2(None, p, 1536, p, p, p, 4, 1534) == _lib.E_ARG      # k not a multiple of 4
    assert L.mmw_mars_dense2(None, p, 1532, p, p, p, 4, 1536) == _lib.E_ARG      # ldh < k
    assert L.mmw_mars_dense2(None, p + 4, 1536, p, p, p, 4, 1536) == _lib.E_ARG  # hidden not 16-byte aligned
    assert L.mmw_mars_dense2(None, p, 1536, p, p, p, 0, 1536) == _lib.MMW_OK     # nothing to do
    assert L.mmw_mars_split_weights(None, p, 6144, p, 12288, -1, 6144, None) == _lib.E_ARG
    assert L.mmw_mars_split_weights(None, None, 6144, p, 12288, 8, 6144, None) == _lib.E_ARG
    assert L.mmw_mars_split_weights(None, p, 6144, None, 12288, 8, 6144, None) == _lib.E_ARG
    assert L.mmw_mars_split_weights(None, p, 6144, p, 12288, 8, 6100, None) == _lib.E_ARG   # k not a multiple of 32
    assert L.mmw_mars_split_weights(None, p, 6144, p, 12280, 8, 6144, None) == _lib.E_ARG   # ld16 < 2 k
    assert L.mmw_mars_split_weights(None, p, 6144, p, 12288, 0, 6144, None) == _lib.MMW_OK
    assert b"mmw_mars_split_weights" in (L.mmw_last_error(None) or b"")


@pytest.mark.parametrize("frames", [3, 1])
def test_numpy_fold_equals_marscnn_bit_for_bit(frames):
    import torch
    from mmwave_msc_amd.mars import MarsCNN
    from mmwave_msc_amd.marsweights import fold_keras_weights, random_keras_weights
    w = random_keras_weights(seed=11 + frames, frames=frames)
    m = MarsCNN.from_keras_weights(w)
    f = fold_keras_weights(w)
    assert f["frames"] == frames
    pairs = {"conv1_w": m.k_w1, "conv1_b": m.k_b1, "conv2_w": m.k_w2, "conv2_b": m.k_b2, "dense1_w": m.dense1_dhwc.weight,
             "dense1_b": m.dense1_dhwc.bias, "dense2_w": m.dense2.weight, "dense2_b": m.dense2.bias}
    for k, t in pairs.items():
        t = t.detach().cpu().contiguous()
        assert f[k].dtype == np.float32 and f[k].flags.c_contiguous and f[k].shape == tuple(t.shape), (k, f[k].shape, tuple(t.shape))
        assert torch.equal(torch.from_numpy(f[k]).view(torch.int32), t.view(torch.int32)), k   # the bits, not the values (-0, NaN)


def test_batch_module_and_fold_helper_import_without_torch():
    code = ("import sys; sys.modules['torch'] = None\n"
            "import mmwave_msc_amd.batch as b, mmwave_msc_amd.marsweights as mw\n"
            "f = mw.fold_keras_weights(mw.random_keras_weights(1, 3))\n"
            "assert f['dense1_w'].shape == (1536, 6144) and f['dense2_w'].shape == (57, 1536)\n"
            "assert hasattr(b.SceneBatch, 'attach_posture_batch') and hasattr(b.SceneBatch, 'estimate_posture') and hasattr(b.SceneBatch, 'posture_range')\n"
            "assert 'torch' not in [k for k, v in sys.modules.items() if v is not None]\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]


def test_fp64_dense2_statement_is_the_oracles_last_layer():
    """What test_gpu_posture_cabi.py compares mmw_mars_dense2 with: BatchNormalization + Dense-2 in fp64 on the hidden layer of
    oracle.mars_np.  Here: that statement on the oracle's hidden layer IS the oracle's output, and the folded fp32 weights of the
    kernel (fold_keras_weights) state the same layer to fp32 rounding."""
    from mmwave_msc_amd.marsweights import fold_keras_weights, random_keras_weights
    from oracle.mars_np import mars_forward_np
    w = random_keras_weights(seed=5, frames=3)
    x = np.random.default_rng(3).normal(0.0, 1.0, size=(6, 3, 8, 8, 5))
    hidden = pc.hidden_fp64(w, x)
    assert hidden.shape == (6, 1536) and (hidden > 0).any()
    want = mars_forward_np(w, x)
    got = pc.dense2_fp64(w, hidden)
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    f = fold_keras_weights(w)
    folded = hidden @ f["dense2_w"].astype(np.float64).T + f["dense2_b"].astype(np.float64)
    assert pc.kp_err(folded, want) <= 1e-5   # (fp32 rounding of 1536 weights per output: far inside the 1e-4 of the keypoints)


@pytest.mark.parametrize("frames", [3, 1])
def test_folded_dense1_is_the_oracles_hidden_layer(frames):
    """The Dense-1 counterpart: BatchNormalization + Dense-1 + relu of oracle.mars_np (pc.hidden_fp64) against the folded fp32
    Dense-1 of fold_keras_weights on the same fp64 conv activations.  The bound is what rounding each folded weight and bias to
    fp32 allows: half an ulp, 2^-24, of every term's magnitude, with a factor 2 for stating it on the rounded values."""
    from mmwave_msc_amd.marsweights import fold_keras_weights, model_dims, random_keras_weights
    from oracle.mars_np import _conv_same
    d = model_dims(frames)
    w = random_keras_weights(seed=5, frames=frames)
    w64 = {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}
    x = np.random.default_rng(3).normal(0.0, 1.0, size=(6,) + d.input)
    a = np.maximum(_conv_same(x, w64["conv1_w"], w64["conv1_b"]), 0.0)
    a_flat = np.maximum(_conv_same(a, w64["conv2_w"], w64["conv2_b"]), 0.0).reshape(6, -1)
    f = fold_keras_weights(w)
    w1, b1 = f["dense1_w"].astype(np.float64), f["dense1_b"].astype(np.float64)
    assert a_flat.shape == (6, d.flat) and w1.shape == (d.hidden, d.flat)
    got = np.maximum(a_flat @ w1.T + b1, 0.0)
    want = pc.hidden_fp64(w, x)
    bound = 2.0 ** -23 * (np.abs(a_flat) @ np.abs(w1).T + np.abs(b1))
    print(f"folded Dense-1, frames={frames}: largest error / bound = {(np.abs(got - want) / bound).max():.3f}")
    assert (want > 0).any() and (np.abs(got - want) <= bound).all()


@pytest.mark.parametrize("frames", [3, 1])
def test_model_dims_are_the_librarys_through_its_own_refusals(frames):
    """marsweights.model_dims against cnn_dims() of csrc/mmw_ctx.hpp, without a device: the entries that take the model's flat size
    as a leading dimension accept exactly it and refuse anything shorter (their argument checks come before any HIP call and
    allow null buffers at n = 0)."""
    from mmwave_msc_amd.marsweights import model_dims
    L = _lib.load()
    flat = model_dims(frames).flat

    def fixup(ldw):
        return L.mmw_mars_range_fixup_frames(None, frames, None, None, 0, None, None, None, None, None, ldw, None, None, None, None, None, None)

    def conv_split(ld_out):
        return L.mmw_mars_conv_split(None, frames, None, None, None, None, None, None, ld_out, 0, None, None)

    assert fixup(flat) == _lib.MMW_OK and fixup(flat - 4) == _lib.E_ARG
    # (accepted = past the argument check: with nothing to launch the entry still asks HIP for its last error, MMW_E_HIP without a GPU)
    assert conv_split(2 * flat) in (_lib.MMW_OK, _lib.E_HIP) and conv_split(2 * flat - 8) == _lib.E_ARG


@pytest.mark.parametrize("S", [48, 640])
def test_gpu_scenario_moves_its_track_lists(S):
    """The inputs of the end-to-end GPU test, with the oracle alone: at least a third of the scenes hold tracks by frame 4, at least
    one track expires before frame 12, and the eligible-track count changes from frame to frame."""
    from mmwave_msc_amd.marsweights import random_keras_weights
    pts, cnt, dts = pc.scenario(S)
    assert pts.shape == (pc.F_STEPS, S, pc.N_PTS, 8) and (cnt > 0).all()
    ref = pc.oracle_run(pts, cnt, dts, random_keras_weights(0, 3))
    assert 3 * ref["tracked_by_4"] >= S, ref["tracked_by_4"]
    assert ref["expired"] >= 1
    assert len(set(ref["rows"])) >= 3 and max(ref["rows"]) > ref["rows"][-1] >= S // 3, ref["rows"]
    assert sum(len(f) for f in ref["finals"]) == ref["samples_cnn"] >= S // 3


def test_new_kernels_compile_without_scratch():
    """k_mars_dense2 and k_split_weights (csrc/k_dense2.hip), from the compiler's own resource report: no scratch, no spilled
    register; Dense-2 (eight 32x32 accumulators = 128 registers per lane, one workgroup per CU by design) stays inside the file."""
    from tests._isa import _device_isa, _kernel_report, assert_clean, kernel_body
    rep, asm = _device_isa(("k_dense2",))["k_dense2"]
    rows = {k[0]: k for k in _kernel_report(rep)}
    for short in ("k_mars_dense2", "k_split_weights"):
        hit = [v for k, v in rows.items() if short in k]
        assert len(hit) == 1, (short, list(rows))
        name, scratch, vspill, vgprs, occ, sspill = hit[0]
        assert_clean(hit)
        body = kernel_body(asm, name)
        assert "scratch_" not in body
        if short == "k_mars_dense2":
            assert vgprs <= 256 and occ >= 1, hit[0]
            assert body.count("v_mfma_f32_32x32x2_f32") >= 32 and "global_load_dwordx4" in body and "ds_read_b128" in body
