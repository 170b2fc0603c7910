"""Shared by the GPU tests of the two posture models (test_gpu_posture_cabi.py, test_gpu_posture_single_frame.py): weights, device
arrays, a model uploaded into a context's device memory, and stepping a context on the scenario of tests/_posture_cabi.py.  This
module uses torch and the GPU; _posture_cabi.py stays free of both."""
import ctypes as C

import numpy as np

from tests import _posture_cabi as pc

N = pc.N_PTS
KP_TOL = 1e-4
CANARY = -777.25
KW = {3: pc.KW, 1: dict(pc.KW, fb_frames_batch=0)}   # the configuration of a context that holds the model of `frames` frames


def _weights(seed, frames):
    from mmwave_msc_amd.marsweights import random_keras_weights
    return random_keras_weights(seed, frames)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream or None


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class CModel:
    """The weights of struct mmw_posture_model in device memory of a context, uploaded through mmw_dev_alloc / mmw_memcpy_h2d."""

    def __init__(self, sb, weights, **replace):
        from mmwave_msc_amd import _lib
        from mmwave_msc_amd.batch import DevBuf
        from mmwave_msc_amd.marsweights import FOLDED_KEYS, fold_keras_weights
        f = dict(fold_keras_weights(weights), **replace)
        self.frames = f["frames"]
        self.bufs = {k: DevBuf(sb, f[k].nbytes).upload(f[k]) for k in FOLDED_KEYS}
        self.struct = _lib.MmwPostureModel.of(*(self.bufs[k].ptr for k in FOLDED_KEYS), dense1_ld=f["dense1_w"].shape[1])

    def free(self):
        for b in self.bufs.values():
            b.free()


def attach_batch(sb, frames, struct, cap_rows):
    """The status of the batched chain's attach entry as a C caller spells it for this model: mmw_posture_attach -- the legacy
    entry, called as such -- for the 3-frame model, mmw_posture_attach_frames for the single-frame one; struct = None detaches."""
    m = C.byref(struct) if struct is not None else None
    return sb.L.mmw_posture_attach(sb.h, m, cap_rows) if frames == 3 else sb.L.mmw_posture_attach_frames(sb.h, m, frames, cap_rows)


def _step(sb, pts_f, cnt_f, dt_f):
    S = sb.S
    b_p = sb.buf("pc_pts", S * N * 64).upload(pts_f)
    b_n = sb.buf("pc_n", S * 4).upload(cnt_f)
    b_d = sb.buf("pc_dt", S * 8).upload(dt_f)
    sb.step_dev(b_p.ptr, b_n.ptr, b_d.ptr)


def _live(sb):
    sb.check()
    ntr = sb.num_tracks()
    return ntr, sb.tracks(cap=max(int(ntr.max()), 1))
