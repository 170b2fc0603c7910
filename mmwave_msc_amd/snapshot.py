"""Scene snapshots (include/mmw.h, format version 1): describe a blob on the host, without a GPU.

`SceneBatch.snapshot` / `snapshot_dev` / `restore` move the state itself; `inspect` reads what a blob holds and refuses a
malformed one exactly as `mmw_restore` would before it looks at a target context.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

HEADER_BYTES = C.sizeof(_lib.MmwSnapshotHeader)
ENTRY_BYTES = C.sizeof(_lib.MmwSnapshotEntry)
ENTRY_DTYPE = np.dtype([("offset", "<u8"), ("bytes", "<u8"), ("n_tracks", "<i4"), ("g_len", "<i4"), ("max_g_rows", "<i4"),
                        ("max_trk_rows", "<i4"), ("err", "<i4"), ("ring_size", "<i4"), ("reserved_", "<i4", (2,))])
assert ENTRY_DTYPE.itemsize == ENTRY_BYTES


def _host_bytes(blob) -> bytes:
    if isinstance(blob, (bytes, bytearray, memoryview)):
        return bytes(blob)
    if isinstance(blob, np.ndarray):
        return np.ascontiguousarray(blob).tobytes()
    raise TypeError(f"a snapshot blob on the host (bytes / bytearray / numpy array), not {type(blob).__name__}")


def inspect(blob) -> dict:
    """mmw_snapshot_inspect: {'header': dict of the header's fields (config as a dict), 'entries': structured numpy array of
    the directory (ENTRY_DTYPE)}.  Raises MmwError (E_ARG) on a malformed blob."""
    b = _host_bytes(blob)
    L = _lib.load()
    info = _lib.MmwSnapshotInfo()
    buf = C.create_string_buffer(b, len(b))
    _lib.check(L.mmw_snapshot_inspect(buf, len(b), C.byref(info)))
    h = info.header
    head = {name: getattr(h, name) for name, _ in _lib.MmwSnapshotHeader._fields_ if name != "config"}
    cfg = {}
    for name, _ in _lib.MmwConfig._fields_:
        v = getattr(h.config, name)
        cfg[name] = list(v) if not isinstance(v, (int, float)) else v
    head["config"] = cfg
    n = int(h.n_scenes)
    entries = np.frombuffer(b, dtype=ENTRY_DTYPE, count=n, offset=HEADER_BYTES).copy()
    return {"header": head, "entries": entries}
