"""Planting chosen track positions through an edited snapshot blob, for tests/test_gpu_heat.py and scripts/bench_heat.py: the one
place beside tests/_snap_plant.py (whose offsets it takes) that builds version-1 sections by hand.
  plant_xy       one scene becomes tracks at chosen (x[0], x[1])
  context_blob   a blob of EVERY scene of a context, all holding the same planted tracks (the benchmark's full map)
  plant_state    a track's nine state words with zero covariance and lifetime 0, in a blob the caller restores; with `dts` an empty
                 frame then moves the track by its velocity times the chosen multiplier"""
import ctypes as C

import numpy as np

from mmwave_msc_amd import _lib
from tests._snap_plant import REC_RING_LEN, REC_RING_N, REC_UID, REC_X

FAR = 100.0   # an x no track of the scenarios comes near


def _section(sb, scene, uids, xy):
    """(header, entry of `scene` alone, section bytes): the scene's first record repeated, list position k under uid uids[k] at x[0],
    x[1] = xy[k], a ring of one frame of no rows; the global ring empty, next_uid past every uid."""
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
    rec0[REC_RING_LEN:REC_RING_LEN + 4] = np.int32(1).tobytes()
    rec0[REC_RING_N:REC_RING_N + 16] = bytes(16)
    recs = []
    for k in range(n):
        r = bytearray(rec0)
        r[REC_X:REC_X + 16] = np.array(xy[k], np.float64).tobytes()      # x[0], x[1]
        r[REC_UID:REC_UID + 4] = np.int32(uids[k]).tobytes()
        recs.append(bytes(r))
    sec = shdr.tobytes() + b"".join(recs)
    ent.bytes, ent.n_tracks, ent.g_len, ent.max_g_rows, ent.max_trk_rows = len(sec), n, 0, 0, 0
    return hdr, ent, sec


def plant_xy(sb, scene, uids, xy):
    """Scene `scene` of `sb`, which holds at least one track, becomes len(uids) live tracks at the positions xy (one restore)."""
    hdr, ent, sec = _section(sb, scene, uids, xy)
    hb, off = C.sizeof(_lib.MmwSnapshotHeader), ent.offset
    hdr.total_bytes = off + len(sec)
    sb.restore(bytes(memoryview(hdr)) + bytes(memoryview(ent)) + bytes(off - hb - C.sizeof(ent)) + sec, scenes=[scene])


def context_blob(sb, uids, xy):
    """A blob of all sb.S scenes, each scene 0's first record repeated at the positions xy: sections back to back behind the
    directory, which starts on 16 bytes as the library lays it out."""
    hdr, ent, sec = _section(sb, 0, uids, xy)
    S, hb = sb.S, C.sizeof(_lib.MmwSnapshotHeader)
    assert len(sec) % 16 == 0
    base = (hb + S * hdr.entry_bytes + 15) // 16 * 16
    hdr.n_scenes, hdr.total_bytes = S, base + S * len(sec)
    ents = (_lib.MmwSnapshotEntry * S)()
    for i in range(S):
        C.memmove(C.byref(ents[i]), C.byref(ent), C.sizeof(ent))
        ents[i].offset = base + i * len(sec)
    return bytes(memoryview(hdr)) + bytes(memoryview(ents)) + bytes(base - hb - S * hdr.entry_bytes) + sec * S


def plant_state(blob, offset, x):
    """In the bytearray `blob`, the first track of the section at `offset` gets x = [px, py, pz, vx, vy, vz] (the other three state
    words 0), zero covariance and lifetime 0."""
    at = offset + _lib.SNAP_SCENE_HDR_BYTES
    blob[at: at + 72] = np.array(list(x) + [0.0, 0.0, 0.0], np.float64).tobytes()
    blob[at + 72: at + 72 + 648] = bytes(648)
    blob[at + 8 * 151: at + 8 * 152] = np.float64(0.0).tobytes()


def dts(multipliers):
    """dt[k][scene] from the per-scene predict multipliers L_k of consecutive empty frames (all non-zero: a lifetime of 0 marks a
    track as just updated): a frame moves a track by its velocity times L_k."""
    L = np.array(multipliers, np.float64)          # [scene][k]
    assert (L != 0).all()
    return np.diff(np.concatenate([np.zeros((len(L), 1)), L], axis=1), axis=1).T
