"""Planting a scene of chosen tracks through an edited snapshot blob (tests/test_gpu_stance.py, tests/test_gpu_kp_scatter.py): the one
place that knows where a version-1 section keeps what it edits.  A section is a 64-byte scene header (int32 words: [0] n_tracks,
[1] g_len, [2:6] g_n, [13] next_uid, [15] skipped) and SNAP_TRACK_BYTES per track: x[k] at 8 k, ring_len at 1224, uid at 1228,
ring_n[4] at 1232, the keypoints at 1264."""
import ctypes as C

import numpy as np

from mmwave_msc_amd import _lib

REC_X, REC_RING_LEN, REC_UID, REC_RING_N, REC_KP = 0, 1224, 1228, 1232, 1264


def plant_tracks(sb, scene, uids, x0_step=0.25):
    """Scene `scene` of `sb`, which holds at least one track, becomes len(uids) live tracks: its first record repeated, list position
    k under uid uids[k] with x[0] = x0_step * k and a ring of one frame of no rows; the global ring empty, next_uid past every uid."""
    n = len(uids)
    blob = sb.snapshot(scenes=[scene])
    hb = C.sizeof(_lib.MmwSnapshotHeader)
    hdr = _lib.MmwSnapshotHeader.from_buffer_copy(blob[:hb])
    ent = _lib.MmwSnapshotEntry.from_buffer_copy(blob[hdr.header_bytes: hdr.header_bytes + hdr.entry_bytes])
    off = ent.offset
    shdr = np.frombuffer(blob[off: off + _lib.SNAP_SCENE_HDR_BYTES], np.int32).copy()
    rec0 = bytearray(blob[off + _lib.SNAP_SCENE_HDR_BYTES: off + _lib.SNAP_SCENE_HDR_BYTES + _lib.SNAP_TRACK_BYTES])
    shdr[0], shdr[1], shdr[2:6], shdr[13] = n, 0, 0, max(int(u) for u in uids) + 1     # n_tracks, g_len, g_n, next_uid
    shdr[15] &= 0xFF00                                       # (no frame of the global ring is left to hold a NaN)
    rec0[REC_RING_LEN:REC_RING_LEN + 4] = np.int32(1).tobytes()   # ring_len 1 ...
    rec0[REC_RING_N:REC_RING_N + 16] = bytes(16)                  # ... of no rows
    recs = []
    for k in range(n):
        r = bytearray(rec0)
        r[REC_X:REC_X + 8] = np.float64(x0_step * k).tobytes()   # x[0]
        r[REC_UID:REC_UID + 4] = np.int32(uids[k]).tobytes()
        recs.append(bytes(r))
    sec = shdr.tobytes() + b"".join(recs)
    ent.bytes, ent.n_tracks, ent.g_len, ent.max_g_rows, ent.max_trk_rows = len(sec), n, 0, 0, 0
    hdr.total_bytes = off + len(sec)
    new = bytes(memoryview(hdr)) + bytes(memoryview(ent)) + bytes(off - hb - C.sizeof(ent)) + sec
    sb.restore(new, scenes=[scene])
