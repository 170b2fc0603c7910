"""Planting chosen tracks through an edited snapshot blob, for the GPU suites and scripts/bench_heat.py: the one place that knows
where a version-1 section keeps what it edits, and the one that builds sections by hand.  A section is a 64-byte scene header
(int32 words: [0] n_tracks, [1] g_len, [2:6] g_n, [13] next_uid, [15] skipped) and SNAP_TRACK_BYTES per track, in which the REC_*
below are byte offsets.  tests/test_feature_harness.py checks all of it on a blob built without a GPU.
  directory, record_at   where a blob keeps a scene's track records, from the library's own reading of the directory
  plant_state            a track's nine state words with zero covariance and lifetime 0, in a blob the caller restores; with `dts` an
                         empty frame then moves the track by its velocity times the chosen multiplier
  plant_word             one fp64 word of a record
  plant_tracks, plant_xy one scene becomes tracks under chosen uids at chosen x[0] / (x[0], x[1])
  context_blob           a blob of EVERY scene of a context, all holding the same planted tracks (the benchmark's full map)"""
import struct

import numpy as np

from mmwave_msc_amd import _lib, snapshot

# x[9] and P[9][9] are fp64; x, P, lifetime and ring_len sit where the public TRACK_DTYPE has them.  uid and ring_n[4] are in the
# snapshot's own order -- the public record has them the other way round -- and its keypoints start 16 bytes later than the public ones.
REC_X, REC_P, REC_LIFETIME, REC_RING_LEN, REC_UID, REC_RING_N, REC_KP = 0, 72, 1208, 1224, 1228, 1232, 1264
P_BYTES = 8 * 9 * 9

FAR = 100.0   # an x no track of the scenarios comes near


def directory(blob):
    """The blob's directory (snapshot.ENTRY_DTYPE, one entry per scene) after the library's own checks."""
    return snapshot.inspect(blob)["entries"]


def record_at(entries, scene, track=0):
    """The byte offset of track `track` of the `scene`-th section."""
    return int(entries["offset"][scene]) + _lib.SNAP_SCENE_HDR_BYTES + _lib.SNAP_TRACK_BYTES * track


def plant_word(blob, at, value):
    blob[at: at + 8] = np.float64(value).tobytes()


def plant_state(blob, at, x6):
    """In the bytearray `blob`, the track record at `at` gets x = [px, py, pz, vx, vy, vz] (the other three state words 0), zero
    covariance and lifetime 0."""
    blob[at + REC_X: at + REC_P] = np.array(list(x6) + [0.0, 0.0, 0.0], np.float64).tobytes()
    blob[at + REC_P: at + REC_P + P_BYTES] = bytes(P_BYTES)
    plant_word(blob, at + REC_LIFETIME, 0.0)


def dts(multipliers):
    """dt[k][scene] from the per-scene predict multipliers L_k of consecutive empty frames (all non-zero: a lifetime of 0 marks a
    track as just updated): a frame moves a track by its velocity times L_k."""
    L = np.array(multipliers, np.float64)          # [scene][k]
    assert (L != 0).all()
    return np.diff(np.concatenate([np.zeros((len(L), 1)), L], axis=1), axis=1).T


def _section(sb, scene, uids, xy):
    """(the header's bytes, the entry of `scene` alone, section bytes): the scene's first record repeated, list position k under uid
    uids[k] at x[0], x[1] = xy[k] (None: the record's own), a ring of one frame of no rows; the global ring empty, next_uid past
    every uid."""
    n = len(uids)
    blob = sb.snapshot(scenes=[scene])
    ent = directory(blob)[0]
    off = int(ent["offset"])
    shdr = np.frombuffer(blob[off: off + _lib.SNAP_SCENE_HDR_BYTES], np.int32).copy()
    rec0 = bytearray(blob[off + _lib.SNAP_SCENE_HDR_BYTES: off + _lib.SNAP_SCENE_HDR_BYTES + _lib.SNAP_TRACK_BYTES])
    shdr[0], shdr[1], shdr[2:6], shdr[13] = n, 0, 0, max(int(u) for u in uids) + 1     # n_tracks, g_len, g_n, next_uid
    shdr[15] &= 0xFF00                                       # (no frame of the global ring is left to hold a NaN)
    rec0[REC_RING_LEN:REC_RING_LEN + 4] = np.int32(1).tobytes()   # ring_len 1 ...
    rec0[REC_RING_N:REC_RING_N + 16] = bytes(16)                  # ... of no rows
    recs = []
    for k in range(n):
        r = bytearray(rec0)
        for i, v in enumerate(xy[k]):                        # x[0], x[1]
            if v is not None:
                plant_word(r, REC_X + 8 * i, v)
        r[REC_UID:REC_UID + 4] = np.int32(uids[k]).tobytes()
        recs.append(bytes(r))
    sec = shdr.tobytes() + b"".join(recs)
    ent["bytes"], ent["n_tracks"], ent["g_len"], ent["max_g_rows"], ent["max_trk_rows"] = len(sec), n, 0, 0, 0
    return blob[:snapshot.HEADER_BYTES], ent, sec


def _blob(head, ent, sec, n):
    """A blob of n scenes that all hold the section `sec`: sections back to back behind the directory, which ends on 16 bytes as
    the library lays it out."""
    assert len(sec) % 16 == 0
    H, hb, eb = _lib.MmwSnapshotHeader, snapshot.HEADER_BYTES, snapshot.ENTRY_BYTES
    base = (hb + n * eb + 15) // 16 * 16
    head = bytearray(head)
    struct.pack_into("<Q", head, H.total_bytes.offset, base + n * len(sec))
    struct.pack_into("<i", head, H.n_scenes.offset, n)
    ents = np.repeat(ent, n)
    ents["offset"] = base + len(sec) * np.arange(n)
    return bytes(head) + ents.tobytes() + bytes(base - hb - n * eb) + sec * n


def plant_xy(sb, scene, uids, xy):
    """Scene `scene` of `sb`, which holds at least one track, becomes len(uids) live tracks at the positions xy (one restore)."""
    sb.restore(_blob(*_section(sb, scene, uids, xy), 1), scenes=[scene])


def plant_tracks(sb, scene, uids, x0_step=0.25):
    """... at x[0] = x0_step * k for list position k, x[1] the first record's own."""
    plant_xy(sb, scene, uids, [(x0_step * k, None) for k in range(len(uids))])


def context_blob(sb, uids, xy):
    """A blob of all sb.S scenes, each scene 0's first record repeated at the positions xy."""
    return _blob(*_section(sb, 0, uids, xy), sb.S)
