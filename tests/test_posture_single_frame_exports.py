"""The single-frame posture model (define_CNN, train.py:33-68) behind the C-ABI -- mmw_mars_conv2d, mmw_mars_range_fixup_frames,
mmw_posture_attach_frames, mmw_attach_posture_frames (include/mmw.h) -- as far as a machine without a GPU can check it: the
symbols, the refusals that never reach a device, the scenario of the GPU test on the oracle alone, and the compiler's report on
k_mars_conv2d (csrc/k_mars2d.hip)."""
import ctypes as C
import os
import re

import numpy as np

from mmwave_msc_amd import _lib
from tests import _posture_cabi as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mmw_mars_conv2d", "mmw_mars_range_fixup_frames", "mmw_posture_attach_frames", "mmw_attach_posture_frames")


def test_new_entries_are_declared_bound_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmw.h")).read(), flags=re.S)
    L = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), f"{name} not declared in include/mmw.h"
        assert name in _lib.EXPORTS, name
        assert hasattr(raw, name), f"{name} not exported by libmmw_hip.so"
        assert getattr(L, name).argtypes is not None, f"{name} has no prototype in _lib.load()"


def test_refusals_that_never_reach_a_device():
    """Null context, frames = 2, negative n, null operands: MMW_E_ARG before any HIP call (where there is no GPU a launch would
    fail with MMW_E_HIP instead)."""
    L = _lib.load()
    p = 0x10000   # a 16-byte aligned non-null value; never dereferenced
    m = _lib.MmwPostureModel()
    for frames in (1, 3):
        assert L.mmw_posture_attach_frames(None, C.byref(m), frames, 16) == _lib.E_ARG
        assert L.mmw_posture_attach_frames(None, None, frames, 0) == _lib.E_ARG
        assert L.mmw_attach_posture_frames(None, C.byref(m), frames) == _lib.E_ARG
        assert L.mmw_attach_posture_frames(None, None, frames) == _lib.E_ARG
    assert b"null" in (L.mmw_last_error(None) or b"")
    assert L.mmw_mars_conv2d(None, p, p, p, p, p, p, -1) == _lib.E_ARG
    for hole in range(6):   # each operand null in turn
        args = [p] * 6
        args[hole] = None
        assert L.mmw_mars_conv2d(None, *args, 4) == _lib.E_ARG, hole
    assert b"mmw_mars_conv2d" in (L.mmw_last_error(None) or b"")
    assert L.mmw_mars_conv2d(None, p, p, p, p, p, p, 0) == _lib.MMW_OK   # nothing to do

    def fixup(frames, n=4, ldw=2048, **null):
        a = dict(feat=p, flags=p, cw1=p, cb1=p, cw2=p, cb2=p, w1=p, b1=p, w2=p, b2=p, scratch=p, kp=p)
        a.update({k: None for k in null})
        return L.mmw_mars_range_fixup_frames(None, frames, a["feat"], a["flags"], n, a["cw1"], a["cb1"], a["cw2"], a["cb2"], a["w1"], ldw, a["b1"],
                                             a["w2"], a["b2"], a["scratch"], a["kp"], None)

    for frames in (2, 0, 4, -1):
        assert fixup(frames) == _lib.E_ARG, frames
        assert b"FB_FRAMES_BATCH" in (L.mmw_last_error(None) or b""), frames
    assert fixup(1, n=-1) == _lib.E_ARG
    assert fixup(1, ldw=2044) == _lib.E_ARG       # shorter than define_CNN's Dense-1 rows
    assert fixup(3, ldw=2048) == _lib.E_ARG       # ... and 2048 is shorter than define_CNN_3D's
    assert fixup(1, ldw=2050) == _lib.E_ARG       # not a multiple of 4
    for k in ("feat", "flags", "cw1", "cb1", "cw2", "cb2", "w1", "b1", "w2", "b2", "scratch", "kp"):
        assert fixup(1, **{k: True}) == _lib.E_ARG, k
    assert fixup(1, n=0) == _lib.MMW_OK and fixup(3, n=0, ldw=6144) == _lib.MMW_OK


def test_gpu_scenario_at_one_frame_per_track():
    """The inputs of the end-to-end GPU test with the oracle alone, at FB_FRAMES_BATCH = 0: the eligible tracks per frame, every
    scene tracked by frame 4, sixteen scene-frames in which a track expires, 72 surviving CNN samples -- and single-frame tensors."""
    from mmwave_msc_amd.marsweights import random_keras_weights
    pts, cnt, dts = pc.scenario(48)
    ref = pc.oracle_run(pts, cnt, dts, random_keras_weights(0, 1), cfg_kw=dict(pc.KW, fb_frames_batch=0))
    for name, value in pc.SINGLE_FRAME_48.items():
        assert ref[name] == value, (name, ref[name])
    assert all(f.shape[1:] == (8, 8, 5) for f in ref["feats"])


def test_conv2d_kernel_compiles_without_scratch():
    """k_mars_conv2d from the compiler's own resource report: no scratch, no spilled register, both fp32 matrix instructions in the
    body, conv2's 72 weights resident beside a 32x32 accumulator, the padded planes and conv1's weights in under 12 KB of LDS."""
    from tests._isa import _device_isa, _kernel_report, assert_clean, kernel_body
    rep, asm = _device_isa(("k_mars2d",))["k_mars2d"]
    rows = _kernel_report(rep)
    assert len(rows) == 1 and "k_mars_conv2d" in rows[0][0], rows
    name, scratch, vspill, vgprs, occ, sspill = rows[0]
    lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", rep).group(1))
    print(f"k_mars_conv2d: {vgprs} VGPRs, {lds} bytes of LDS per workgroup, {occ} waves per SIMD")
    assert_clean(rows)
    body = kernel_body(asm, name)
    assert "scratch_" not in body
    assert body.count("v_mfma_f32_32x32x2_f32") == 72 and body.count("v_mfma_f32_16x16x4_f32") == 24
    assert 72 + 16 <= vgprs <= 256 and occ >= 1
    assert lds == (5 * 100 + 16 * 100 + 48 * 16 + 48) * 4
