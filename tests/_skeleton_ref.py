"""What mmw_skeletons_* must return, restated in numpy from the semantics in include/mmw.h ("live-track skeletons"): the five numpy
lines of Visualizer.update_posture (Visualizer.py:274-283) as read -- the reshape(3, 19) view, the norm of column 1 minus column 2
against 0.5, the mirror of row 0 and the two in-place `+=` of fp64 shape-(1,) arrays on float32 rows, which numpy computes in fp64
and casts back.  No live run of the reference's Visualizer pins this (it imports Qt, pyqtgraph and matplotlib): the pin is those
lines as read.  Works on state read back through entries older than the skeletons (`tracks()`, `report_host()`) and never goes
through the skeleton entries themselves."""
import numpy as np

from mmwave_msc_amd import _lib


def skeleton_of(kp, x0, x1):
    """(skipped, gap float32, joint float32[19, 3]) of one track: kp float32[57], x0 / x1 the fp64 state's first two entries."""
    m = np.asarray(kp, np.float32).reshape(3, 19)
    x0, x1 = np.float64(x0), np.float64(x1)
    with np.errstate(all="ignore"):
        g = m[:, 1] - m[:, 2]                                   # float32 - float32: one fp32 subtraction each
        g = g.astype(np.float64)
        s = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]          # fp64; the products of fp32 values are exact
        skipped = bool(s > 0.25)                                # (False for a NaN)
        gap = np.float32(np.sqrt(s))
        joint = np.empty((19, 3), np.float32)
        joint[:, 0] = (-(m[0].astype(np.float64)) + x0).astype(np.float32)   # mirrored, shifted: ONE rounding, from fp64
        joint[:, 1] = (m[2].astype(np.float64) + x1).astype(np.float32)      # depth
        joint[:, 2] = m[1]                                                   # height, untouched
    return skipped, gap, joint


def fp32_arithmetic_joint_x(kp0, x0):
    """What joint x would be if the shift were done in float32 (`-kp + fp32(x)`): NOT what the reference computes."""
    return np.float32(-np.float32(kp0)) + np.float32(np.float64(x0))


def expected(rows, tracks, scene_base=0):
    """SKELETON_DTYPE[len(rows)] in MMW_SKEL_ALL: entry i for `report_host(scene_base)` row i, the track itself taken from
    `tracks()` [S, cap] of the same state by the row's scene and slot."""
    out = np.zeros(len(rows), _lib.SKELETON_DTYPE)
    for i, r in enumerate(rows):
        t = tracks[int(r["scene"]) - scene_base, int(r["slot"])]
        skipped, gap, joint = skeleton_of(t["keypoints"], t["x"][0], t["x"][1])
        out[i]["scene"], out[i]["slot"], out[i]["uid"], out[i]["row"] = r["scene"], r["slot"], t["uid"], i
        out[i]["flags"], out[i]["gap"], out[i]["joint"] = (_lib.SKEL_SKIPPED if skipped else 0), gap, joint
    return out


def drawn(entries):
    """MMW_SKEL_DRAWN from MMW_SKEL_ALL: the entries whose flag bit 0 is clear, order and `row` kept."""
    return entries[(entries["flags"] & _lib.SKEL_SKIPPED) == 0]
