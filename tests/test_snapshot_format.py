"""The scene-snapshot format (include/mmw.h, version 1) on the host, without a GPU: the ctypes mirror of its structs, a blob
built by hand from the documented layout, and every refusal of mmw_snapshot_inspect."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

from mmwave_msc_amd import _lib, snapshot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_text():
    return open(os.path.join(ROOT, "include", "mmw.h")).read()


def test_struct_sizes_and_offsets_match_the_header():
    H, E = _lib.MmwSnapshotHeader, _lib.MmwSnapshotEntry
    # header: magic[8], version, header_bytes, total_bytes (u64), 8 int32, then the verbatim mmw_config
    assert H.magic.offset == 0 and H.version.offset == 8 and H.header_bytes.offset == 12 and H.total_bytes.offset == 16
    assert H.n_scenes.offset == 24 and H.track_cap.offset == 48 and H.config.offset == 56
    assert C.sizeof(H) == 56 + C.sizeof(_lib.MmwConfig) == 600
    assert E.offset.offset == 0 and E.bytes.offset == 8 and E.n_tracks.offset == 16 and E.ring_size.offset == 36
    assert C.sizeof(E) == 48 == snapshot.ENTRY_DTYPE.itemsize
    txt = _header_text()
    assert re.search(r'#define MMW_SNAP_MAGIC "MMWSNAP"', txt)
    assert re.search(r"#define MMW_SNAP_VERSION 1\b", txt)
    assert re.search(r"#define MMW_SNAP_TRACK_BYTES 1504\b", txt) and re.search(r"#define MMW_SNAP_SCENE_HDR_BYTES 64\b", txt)
    # a track record of the blob = the 1496-byte record (TRACK_DTYPE's fields are a subset of it) + 8 bytes of zeros, 16-aligned
    assert _lib.SNAP_TRACK_BYTES % 16 == 0 and _lib.SNAP_TRACK_BYTES == 187 * 8 + 8


def _section(n_tracks, g_rows, trk_rows):
    """One scene section as the format describes it: canonical header, records, track-ring rows, global-ring rows."""
    hdr = np.zeros(16, np.int32)
    hdr[0], hdr[1] = n_tracks, len(g_rows)
    hdr[2:2 + len(g_rows)] = g_rows
    hdr[6:10] = np.arange(4)        # g_slot: the identity
    recs = np.zeros((n_tracks, _lib.SNAP_TRACK_BYTES), np.uint8)
    rows = (sum(g_rows) + sum(trk_rows)) * 64
    return hdr.tobytes() + recs.tobytes() + np.arange(rows // 8, dtype=np.float64).tobytes()


def build_blob(scenes, n_scenes=None, version=1, magic=b"MMWSNAP\0", total=None, offsets=None):
    cfg = _lib.default_config()
    secs = [_section(*sc) for sc in scenes]
    n = len(secs)
    base = (600 + n * 48 + 15) // 16 * 16
    offs, at = [], base
    for s in secs:
        offs.append(at)
        at += len(s)
    if offsets is not None:
        offs = offsets
    tot = at if total is None else total
    head = bytearray(base)
    struct.pack_into("<8sIIQ8i", head, 0, magic, version, 600, tot, n if n_scenes is None else n_scenes, 48, 512, 3, 64, 9, 8, 0)
    head[56:600] = bytes(memoryview(cfg))
    for i, (sc, s) in enumerate(zip(scenes, secs)):
        ntr, g_rows, trk_rows = sc
        struct.pack_into("<QQ8i", head, 600 + 48 * i, offs[i], len(s), ntr, len(g_rows), max(g_rows, default=0),
                         max(trk_rows, default=0), 0, 0, 0, 0)
    return bytes(head) + b"".join(secs)


SCENES = [(2, [100, 37, 5], [20, 64, 3]), (0, [7], []), (1, [], [])]


def test_inspect_accepts_a_blob_built_from_the_documented_layout():
    blob = build_blob(SCENES)
    info = snapshot.inspect(blob)
    h, e = info["header"], info["entries"]
    assert h["magic"] == b"MMWSNAP" and h["version"] == 1 and h["total_bytes"] == len(blob) and h["n_scenes"] == 3
    assert (h["max_pts"], h["ring"], h["ring_rows"], h["dim_x"], h["track_cap"]) == (512, 3, 64, 9, 8)
    assert h["config"]["db_eps"] == 0.3 and h["config"]["fb_frames_batch"] == 2
    assert list(e["n_tracks"]) == [2, 0, 1] and list(e["g_len"]) == [3, 1, 0]
    assert int(e["offset"][0]) == 752 and all(int(o) % 16 == 0 for o in e["offset"])
    assert int(e["offset"][-1] + e["bytes"][-1]) == len(blob)
    assert int(e["bytes"][0]) == 64 + 2 * 1504 + (142 + 87) * 64
    assert snapshot.inspect(build_blob([]))["header"]["n_scenes"] == 0


def _refused(blob, what):
    with pytest.raises(_lib.MmwError) as ei:
        snapshot.inspect(blob)
    assert ei.value.code == _lib.E_ARG
    whats = (what,) if isinstance(what, str) else what
    assert any(w in str(ei.value) for w in whats), str(ei.value)


def test_inspect_refuses_bad_magic_and_unknown_version():
    _refused(build_blob(SCENES, magic=b"MMWSNAQ\0"), "magic")
    _refused(build_blob(SCENES, version=2), "version")


def test_inspect_refuses_a_truncated_directory_or_header():
    blob = build_blob(SCENES)
    _refused(blob[:300], "header")
    # the header announces 3 entries, the blob ends inside the directory (total_bytes says so too)
    short = bytearray(blob[:650])
    struct.pack_into("<Q", short, 16, 650)
    _refused(bytes(short), "truncated")


def test_inspect_refuses_offsets_out_of_order_or_past_the_end():
    good = build_blob(SCENES)
    e = snapshot.inspect(good)["entries"]
    o = [int(v) for v in e["offset"]]
    _refused(build_blob(SCENES, offsets=[o[1], o[0], o[2]]), "out of order")
    _refused(build_blob(SCENES, offsets=[o[0] + 16, o[1], o[2]]), "out of order")
    # the last section runs past the end of the blob
    blob = bytearray(good)
    struct.pack_into("<Q", blob, 600 + 48 * 2 + 8, int(e["bytes"][2]) + 1024)
    _refused(bytes(blob), "bytes at offset")


def test_inspect_refuses_a_scene_count_that_disagrees_with_the_sizes():
    # two entries announced, three sections present: the directory no longer lines up with the sections or the total
    _refused(build_blob(SCENES, n_scenes=2), ("account for", "out of order"))
    _refused(build_blob(SCENES, n_scenes=4), ("truncated", "out of order", "out of range", "bytes at offset"))
    _refused(build_blob(SCENES, total=len(build_blob(SCENES)) + 16), "total_bytes")


def test_snapshot_symbols_are_exported():
    L = C.CDLL(_lib.LIB_PATH)
    for name in ("mmw_snapshot_size", "mmw_snapshot", "mmw_restore", "mmw_snapshot_inspect"):
        assert hasattr(L, name) and name in _lib.EXPORTS
