"""SceneBatch: S independent scenes (S reference `TrackBuffer`s + their global
`BatchedData`) resident on one MI355X, stepped together through the C-ABI.

This is the batched face of the hot path; `tracking.TrackBuffer` is the
single-scene, reference-shaped face built on top of it.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from . import _lib
from ._lib import MmwError, RING_MAX, NKP, SUMMARY_DTYPE, TRACK_DTYPE, error_for


class DevBuf:
    """A device allocation owned by a context (hipMalloc through the C-ABI)."""

    def __init__(self, batch: "SceneBatch", nbytes: int):
        self.batch, self.nbytes = batch, int(nbytes)
        p = C.c_void_p()
        batch._chk(batch.L.mmw_dev_alloc(batch.h, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def upload(self, arr: np.ndarray):
        a = np.ascontiguousarray(arr)
        assert a.nbytes <= self.nbytes, (a.nbytes, self.nbytes)
        self.batch._chk(self.batch.L.mmw_memcpy_h2d(self.batch.h, self.ptr, a.ctypes.data, a.nbytes))
        return self

    def download(self, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes, (out.nbytes, self.nbytes)
        self.batch._chk(self.batch.L.mmw_memcpy_d2h(self.batch.h, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr and self.batch.h:
            self.batch.L.mmw_dev_free(self.batch.h, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class RadarRead(NamedTuple):
    """What `SceneBatch.read_radars` leaves on the device: pts[S][max_pts][8] fp64, n[S] int32, dt[S] fp64 -- `step_dev`'s input --,
    status[S] int32 (`_lib.UART_*`, bit 8 = `_lib.UART_CHUNK_DROPPED`) and frame_number[S] uint32."""
    pts: DevBuf
    n: DevBuf
    dt: DevBuf
    status: DevBuf
    frame_number: DevBuf


class SceneBatch:
    def __init__(self, cfg: "_lib.MmwConfig | None" = None, n_scenes: int = 1, max_pts: int = 512, device: int = 0):
        self.L = _lib.load()
        self.cfg = cfg if cfg is not None else _lib.default_config()
        self.h = None
        h = C.c_void_p()
        rc = self.L.mmw_create(C.byref(self.cfg), int(n_scenes), int(max_pts), int(device), C.byref(h))
        _lib.check(rc)
        self.h = h
        self.S, self.max_pts, self.device = int(n_scenes), int(max_pts), int(device)
        dims = [C.c_int32() for _ in range(5)]
        self._chk(self.L.mmw_get_dims(self.h, *[C.byref(d) for d in dims]))
        self.track_cap, self.ring, self.ring_rows = dims[2].value, dims[3].value, dims[4].value
        self.UM = self.ring * self.max_pts
        self._bufs = {}
        self._frame_out = None      # frame_host(reuse_out=True): the result arrays of the last call
        self._posture_model = None
        self._posture_batch = None   # attach_posture_batch: the weights' device buffers
        # entries / rows / points the `*_host` exports' device buffers hold; they grow to what the device says it needs
        self._export_caps = {"report": (64, 64), "clouds": (64, 4096), "skeletons": (64,), "radar_log": (64, 4096)}

    # -- plumbing -------------------------------------------------------------
    def _chk(self, rc):
        _lib.check(rc, self.h)

    def close(self):
        if self.h:
            for b in list(self._bufs.values()):
                b.free()
            self._bufs.clear()
            self._free_posture_batch()
            self.L.mmw_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def buf(self, name: str, nbytes: int) -> DevBuf:
        b = self._bufs.get(name)
        if b is None or b.nbytes < nbytes:
            if b is not None:
                b.free()
            b = DevBuf(self, nbytes)
            self._bufs[name] = b
        return b

    def alloc(self, nbytes: int) -> DevBuf:
        return DevBuf(self, nbytes)

    def set_stream(self, stream_ptr):
        """Raw hipStream_t (0 / None = the context's own non-blocking stream; 1 = HIP's legacy default stream)."""
        self._chk(self.L.mmw_set_stream(self.h, stream_ptr))

    def follow_torch_stream(self, stream=None):
        """Run this context's kernels on a torch stream (default: torch's current one), so that torch ops and the
        `*_dev` calls that share device tensors with them are ordered without host synchronisation.  torch reports
        the legacy default stream as pointer 0, which `mmw_set_stream` reads as "the context's own stream" -- the
        legacy handle (include/mmw.h: MMW_STREAM_LEGACY) is passed for it."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        ptr = int(s.cuda_stream)
        self.set_stream(ptr if ptr else 1)

    def stream_wait(self, stream=None):
        """mmw_stream_wait: work queued on `stream` (a torch stream; default torch's current one on this device) after this call
        starts only when everything queued on the context's stream so far has finished -- no host wait.  For consumers of device
        buffers the context wrote (the all-gather of the track table, a torch op on feature rows) that run on another stream."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        self._chk(self.L.mmw_stream_wait(self.h, int(s.cuda_stream)))

    def wait_stream(self, stream=None):
        """mmw_wait_stream, the other direction: what this context queues from now on starts only when everything queued on
        `stream` (default torch's current one) so far has finished -- before the context REWRITES a device buffer a consumer on
        that stream may still be reading (the track table of the previous all-gather)."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        self._chk(self.L.mmw_wait_stream(self.h, int(s.cuda_stream)))

    def set_chain_side_stream(self, on: bool):
        """Small-cloud DBSCAN workers beside the association kernel (second stream) on / off, from the next step on."""
        self._chk(self.L.mmw_set_chain_side_stream(self.h, 1 if on else 0))

    def side_workers(self) -> int:
        """mmw_side_workers: 0 = the DBSCAN chain workers are not in use (not configured, or their streams share a hardware
        queue with the context's stream), 1 = in use, 2 = configured but no step has checked the streams yet."""
        return int(self.L.mmw_side_workers(self.h))

    def diag_queue(self) -> np.ndarray:
        """mmw_diag_queue: the 32 words of the DBSCAN work queues ([4] = bounded waits given up, also reported by check())."""
        out = np.zeros(32, dtype=np.int32)
        self._chk(self.L.mmw_diag_queue(self.h, out.ctypes.data))
        return out

    def streams_concurrent(self, stream_a: int, stream_b: int) -> bool:
        """mmw_streams_concurrent: do kernels on HIP stream b (raw handles) run beside a running kernel of stream a?"""
        rc = int(self.L.mmw_streams_concurrent(self.h, stream_a, stream_b))
        if rc < 0:
            self._chk(rc)
        return rc == 1

    def step_kind(self) -> int:
        """mmw_step_kind: 1 = the one-workgroup step (k_scene), 2 = two launches, 4 = the bulk kernels."""
        return int(self.L.mmw_step_kind(self.h))

    def kalman_layout(self) -> int:
        """mmw_kalman_layout: 1 = the batched Kalman kernels are laid out over the tracks of the context, 0 = per scene."""
        return int(self.L.mmw_kalman_layout(self.h))

    def synchronize(self):
        self._chk(self.L.mmw_synchronize(self.h))

    def _scene_flags(self, scenes, upload_to: str = None):
        """The scene mask the C-ABI takes: None for scenes=None (every scene), else int32[S] with 1 at `scenes` -- or, with
        `upload_to`, the device pointer of the buffer of that name, holding it."""
        if scenes is None:
            return None
        flags = np.zeros(self.S, dtype=np.int32)
        flags[np.asarray(scenes, dtype=np.int64)] = 1
        return self.buf(upload_to, self.S * 4).upload(flags).ptr if upload_to else flags

    @staticmethod
    def _host_ptr(a):
        return None if a is None else a.ctypes.data

    def pop_frame(self, scenes=None):
        """BatchedData.pop_frame() on the global ring of the given scenes (default: all)."""
        self._chk(self.L.mmw_pop_frame(self.h, self._host_ptr(self._scene_flags(scenes))))

    def set_batch_size(self, new_size: int, scenes=None):
        """BatchedData.change_buffer_size(new_size) on the global ring of the given scenes (default: all)."""
        self._chk(self.L.mmw_set_batch_size(self.h, self._host_ptr(self._scene_flags(scenes)), int(new_size)))

    def set_batch_frame(self, scene: int, rows: np.ndarray):
        """BatchedData(init_data): the scene's global ring becomes one frame holding `rows` (n, 8)."""
        rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 8)
        self._chk(self.L.mmw_set_batch_frame(self.h, int(scene), rows.ctypes.data, len(rows)))

    # -- per-scene sites ------------------------------------------------------
    def set_sites(self, sites, scenes=None):
        """mmw_set_sites: give `scenes` (default: scenes 0 .. len(sites)-1) their own site -- sensor mounting, intensity scale,
        window / monitoring point -- as a `_lib.SITE_DTYPE` array (`_lib.make_sites`).  From the next call on, normalisation,
        feature maps and the track table use each scene's site; the tracker itself keeps reading the context's config.  Scenes
        never listed keep the config's values.  Refused (MmwError, E_ARG) with no site changed for an index out of range or
        listed twice, more sites than scenes, or a non-zero `reserved_`."""
        a = np.ascontiguousarray(np.asarray(sites, dtype=_lib.SITE_DTYPE).reshape(-1))
        idx = None
        if scenes is not None:
            idx = np.ascontiguousarray(np.asarray(scenes, dtype=np.int32).reshape(-1))
            if len(idx) != len(a):
                raise ValueError(f"set_sites: {len(a)} sites for {len(idx)} scenes")
        self._chk(self.L.mmw_set_sites(self.h, idx.ctypes.data if idx is not None else None, len(a), a.ctypes.data if len(a) else None))

    def sites(self) -> np.ndarray:
        """mmw_get_sites: the effective site of every scene, SITE_DTYPE[S] (the config's values where none was set)."""
        out = np.zeros(self.S, dtype=_lib.SITE_DTYPE)
        self._chk(self.L.mmw_get_sites(self.h, out.ctypes.data))
        return out

    def clear_sites(self):
        """mmw_clear_sites: every scene back to the context's config, and to the kernels of a context without sites."""
        self._chk(self.L.mmw_clear_sites(self.h))

    @property
    def has_sites(self) -> bool:
        rc = int(self.L.mmw_has_sites(self.h))
        if rc < 0:
            self._chk(rc)
        return rc == 1

    def reset(self):
        self._chk(self.L.mmw_reset(self.h))

    def reset_scenes(self, mask):
        """Fresh TrackBuffer / BatchedData for the scenes where `mask` is true (mmw_reset_scenes); the others keep their state."""
        m = np.ascontiguousarray(np.asarray(mask).astype(np.int32).reshape(self.S))
        self._chk(self.L.mmw_reset_scenes(self.h, m.ctypes.data))

    def errors(self) -> np.ndarray:
        """Sticky error bits per scene (mmw_get_errors): 1 singular, 2 division by zero, 4 capacity, 8 bad point count,
        16 / 32 apply_DBscan reached with a NaN / an infinite value in the ring (sklearn's ValueError, Utils.py:272-278)."""
        out = np.zeros(self.S, dtype=np.int32)
        self._chk(self.L.mmw_get_errors(self.h, out.ctypes.data))
        return out

    def clear_errors(self, bits: int, scenes=None):
        """mmw_clear_errors: clears the given sticky bits (of the given scenes; default all) and nothing else -- for a caller that
        catches the reference's ValueError (non-finite rows: the scene's state is what the reference's is) and carries on."""
        self._chk(self.L.mmw_clear_errors(self.h, self._host_ptr(self._scene_flags(scenes)), int(bits)))

    def check(self):
        self._chk(self.L.mmw_check(self.h))

    # -- hot path -------------------------------------------------------------
    def step_dev(self, pts_ptr, n_ptr, dt_ptr, assoc_ptr=None, labels_ptr=None, dbn_ptr=None):
        """TrackBuffer.track for all scenes; every argument is a device pointer (int) or a `DevBuf` (what `read_radars` returns)."""
        self._chk(self.L.mmw_step(self.h, *[getattr(a, "ptr", a) for a in (pts_ptr, n_ptr, dt_ptr, assoc_ptr, labels_ptr, dbn_ptr)]))

    def step_dev_f32(self, pts_ptr, n_ptr, dt_ptr, assoc_ptr=None, labels_ptr=None, dbn_ptr=None):
        """mmw_step_f32: the same with the frame's rows as fp32 ([S][max_pts][8] float, device pointer), promoted exactly."""
        self._chk(self.L.mmw_step_f32(self.h, pts_ptr, n_ptr, dt_ptr, assoc_ptr, labels_ptr, dbn_ptr))

    def normalize_dev(self, raw_ptr, n_raw_ptr, pts_ptr, n_out_ptr, f32: bool = False):
        """Utils.normalize_data on device buffers: raw[S][max_pts][5] (fp64, or fp32 with f32=True) -> pts[S][max_pts][8] fp64."""
        fn = self.L.mmw_normalize_f32 if f32 else self.L.mmw_normalize
        self._chk(fn(self.h, raw_ptr, n_raw_ptr, pts_ptr, n_out_ptr))

    def normalize_tlv_dev(self, packets_ptr, packets_bytes, tlv_offset_ptr, uart_cfg, pts_ptr, n_out_ptr):
        """mmw_normalize_tlv: the radar's own wire format (detected-points TLV bodies, 12 B per object) decoded as ReadIWR14xx.read
        does (ReadDataIWR1443.py:153-171) and normalised (Utils.normalize_data) in one kernel: packets (device bytes),
        tlv_offset[S] (device int64: byte offset of each scene's TLV body, < 0 = none), uart_cfg (`_lib.MmwUartCfg`, host)
        -> pts[S][max_pts][8] fp64, n_out[S] (device).  Nothing outside packets[0 .. packets_bytes) is read; a body that does not
        fit, or announces more than max_pts objects, gives n_out = _lib.BAD_FRAME (the next step raises the scene's bad count)."""
        self._chk(self.L.mmw_normalize_tlv(self.h, packets_ptr, int(packets_bytes), tlv_offset_ptr, C.byref(uart_cfg), pts_ptr, n_out_ptr))

    # -- device-resident radar readers ------------------------------------------
    def open_radars(self, config_parameters, t0: float = None):
        """mmw_uart_open: one `ReadIWR14xx` per scene on the device -- a zeroed 2^15-byte byteBuffer, byteBufferLength 0 -- from the
        reference's `configParameters` dict (one for every scene, or a list of S), with main.py's `t` = t0 (default: now)."""
        import time
        from .radar import uart_cfg
        lst = [config_parameters] if isinstance(config_parameters, dict) else list(config_parameters)
        if len(lst) not in (1, self.S):
            raise ValueError(f"open_radars: {len(lst)} configParameters for {self.S} scenes (one, or one per scene)")
        arr = (_lib.MmwUartCfg * len(lst))(*[uart_cfg(p) for p in lst])
        self._chk(self.L.mmw_uart_open(self.h, arr, len(lst), float(time.time() if t0 is None else t0)))

    def close_radars(self):
        self._chk(self.L.mmw_uart_close(self.h))

    def read_radars_dev(self, chunks_ptr, chunk_off_ptr, chunks_bytes, now, pts_ptr, n_out_ptr, dt_ptr, status_ptr, frame_ptr, flags_ptr=None):
        """mmw_uart_read, the pointer form: ReadIWR14xx.read + Utils.normalize_data for every flagged scene in one kernel.  chunks
        (device bytes, 4-byte aligned), chunk_off[S + 1] (device int64), flags[S] (device int32 or None = every scene) ->
        pts[S][max_pts][8] fp64, n_out[S], dt[S] fp64, status[S] (`_lib.UART_*`), frame_number[S] uint32, all on the device and
        ready for `step_dev`.  Asynchronous; nothing is read back."""
        self._chk(self.L.mmw_uart_read(self.h, chunks_ptr, chunk_off_ptr, int(chunks_bytes), flags_ptr, float(now), pts_ptr, n_out_ptr, dt_ptr,
                                       status_ptr, frame_ptr))

    def _radar_staging(self, nbytes: int) -> np.ndarray:
        """A host block of at least nbytes for read_radars' one upload: pinned when torch can provide it, pageable otherwise."""
        st = getattr(self, "_radar_host", None)
        if st is None or st.nbytes < nbytes:
            size = max(2 * nbytes, 1 << 16)
            try:
                import torch
                self._radar_pin = torch.empty(size, dtype=torch.uint8, pin_memory=True)
                st = self._radar_pin.numpy()
            except Exception:
                st = np.empty(size, dtype=np.uint8)
            self._radar_host = st
        return st

    def read_radars(self, chunks, now: float, scenes=None):
        """One `read()` per scene with `chunks[s]` (bytes-like; b"" is still a read) as what its port delivered at time `now`:
        offsets, flags and bytes are packed into one host block and uploaded with ONE copy, then `read_radars_dev`.  `scenes`:
        the scenes that read (default all; `chunks` still has S entries).  Returns `RadarRead(pts, n, dt, status, frame_number)`
        of `DevBuf`s owned by this object and rewritten by the next call; `step_dev(r.pts, r.n, r.dt)` takes them as they are, and
        nobody has to download `status` / `frame_number`."""
        S = self.S
        if len(chunks) != S:
            raise ValueError(f"read_radars: {len(chunks)} chunks for {S} scenes")
        views = [np.frombuffer(c, dtype=np.uint8) for c in chunks]
        off = np.zeros(S + 1, dtype=np.int64)
        np.cumsum([len(v) for v in views], out=off[1:])
        total = int(off[S])
        head = ((S + 1) * 8 + S * 4 + 15) // 16 * 16          # [S + 1] int64 offsets | [S] int32 flags | pad | the bytes
        nbytes = head + (total + 15) // 16 * 16 + 16
        host = self._radar_staging(nbytes)
        host[: (S + 1) * 8].view(np.int64)[:] = off
        flags = host[(S + 1) * 8: (S + 1) * 8 + S * 4].view(np.int32)
        flags[:] = 1 if scenes is None else self._scene_flags(scenes)
        for s, v in enumerate(views):
            host[head + off[s]: head + off[s + 1]] = v
        b_in = self.buf("radar_in", nbytes)
        self._chk(self.L.mmw_memcpy_h2d(self.h, b_in.ptr, host.ctypes.data, head + total))
        r = RadarRead(self.buf("radar_pts", S * self.max_pts * 64), self.buf("radar_n", S * 4), self.buf("radar_dt", S * 8),
                      self.buf("radar_status", S * 4), self.buf("radar_frame", S * 4))
        self.read_radars_dev(b_in.ptr + head, b_in.ptr, total, now, r.pts.ptr, r.n.ptr, r.dt.ptr, r.status.ptr, r.frame_number.ptr,
                             b_in.ptr + (S + 1) * 8)
        return r

    def radar_state(self, scene: int):
        """mmw_uart_get_state: (byteBuffer -- all 2^15 bytes, stale ones included --, byteBufferLength, t_last) of one scene."""
        buf = np.zeros(_lib.UART_BUFFER, dtype=np.uint8)
        n, t = C.c_int32(0), C.c_double(0.0)
        self._chk(self.L.mmw_uart_get_state(self.h, int(scene), buf.ctypes.data, C.byref(n), C.byref(t)))
        return buf, int(n.value), float(t.value)

    def set_radar_state(self, scene: int, buf, length: int, t_last: float):
        """mmw_uart_set_state: the other direction (a scene moved in from another context; tests)."""
        a = np.ascontiguousarray(np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf, dtype=np.uint8)
        if a.shape != (_lib.UART_BUFFER,):
            raise ValueError(f"set_radar_state: the buffer has {_lib.UART_BUFFER} bytes, not {a.shape}")
        self._chk(self.L.mmw_uart_set_state(self.h, int(scene), a.ctypes.data, int(length), float(t_last)))

    def set_radar_time(self, t: float, scenes=None):
        """mmw_uart_set_time: main.py's `t` restarts at `t` for the given scenes (default all), e.g. after `reset_scenes`."""
        self._chk(self.L.mmw_uart_set_time(self.h, self._host_ptr(self._scene_flags(scenes)), float(t)))

    # -- radar log ----------------------------------------------------------------
    def enable_radar_log(self, on: bool = True):
        """mmw_uart_log_enable (after `open_radars`): from now on every `read_radars` also keeps each scene's decoded frame as it
        came off the wire -- the recorder's `dataOk, frameNumber, detObj` (DataLogging.py:36) -- for `radar_log_*`; on=False frees
        it.  Until enabled, the log calls are refused (E_ARG) and the context launches nothing of them."""
        self._chk(self.L.mmw_uart_log_enable(self.h, 1 if on else 0))

    def radar_log_dev(self, dir_ptr, cap_frames: int, rows_ptr, cap_rows: int, frame_select: int = 1, flags_ptr=None, ticket: int = 0,
                      scene_base: int = 0):
        """mmw_uart_log_async: the frame each asked scene decoded at the last `read_radars` into device buffers -- a
        `_lib.UART_FRAME_DTYPE` directory entry per scene whose frame number is a multiple of `frame_select`, scenes ascending,
        and their objects back to back (`_lib.UART_OBJECT_DTYPE`: the reference's detObj bit for bit).  `flags_ptr`: device
        int32[S], the scenes asked (None = all).  A frame is handed out once; call after every read.  Queued on the context's
        stream -- no host wait.  Tickets 0 .. 3 (`radar_log_host` uses 3).  `rows_ptr` 16-byte aligned."""
        self._chk(self.L.mmw_uart_log_async(self.h, dir_ptr, int(cap_frames), rows_ptr, int(cap_rows), flags_ptr, int(frame_select),
                                            int(scene_base), int(ticket)))

    def radar_log_wait(self, ticket: int = 0):
        """(n_frames, n_rows) of the `radar_log_dev` call with this ticket: waits for its counts only, not for the stream.  Buffers
        too small: MmwError with code E_CAPACITY and the counts needed in `.needed` -- nothing was written, no frame consumed."""
        return self._export_wait(self.L.mmw_uart_log_wait, ticket)

    def radar_log_host(self, frame_select: int = 1, scenes=None, scene_base: int = 0):
        """(dir[n_frames] UART_FRAME_DTYPE, rows[n_rows] UART_OBJECT_DTYPE): entry i owns rows[first : first + count].  `scenes`:
        the scenes asked (default all); the others keep their frame for a later call.  The device buffers are kept and grow to
        what the device says it needs (one retry; a refused export loses nothing)."""
        flags_ptr = self._scene_flags(scenes, "radar_log_flags")
        return self._export_host("radar_log", lambda *a: self.radar_log_dev(*a[:4], frame_select, flags_ptr, a[4], scene_base),
                                 self.L.mmw_uart_log_wait, ("radar_log_dir", _lib.UART_FRAME_DTYPE), ("radar_log_rows", _lib.UART_OBJECT_DTYPE))

    def step_host(self, pts: np.ndarray, n: np.ndarray, dt: np.ndarray, raise_nonfinite: bool = True, check: bool = True):
        """Host convenience (H2D + step + D2H).  Returns (assoc[S,NP], labels[S,UM], db_n[S]).  raise_nonfinite=False: a scene
        whose apply_DBscan call raised sklearn's ValueError (a NaN / infinite row in its ring) does not raise here -- its db_n is
        DB_RAISED (-2), its sticky bit stays set (`errors()`, `clear_errors()`), every other scene's results are as always.
        check=False: no scene error raises (the caller reads `errors()`); failures of the call itself still do."""
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        n = np.ascontiguousarray(n, dtype=np.int32)
        dt = np.ascontiguousarray(dt, dtype=np.float64)
        assert pts.shape == (self.S, self.max_pts, 8) and n.shape == (self.S,) and dt.shape == (self.S,)
        assoc = np.full((self.S, self.max_pts), -1, dtype=np.int32)
        labels = np.full((self.S, self.UM), -1, dtype=np.int32)
        dbn = np.full(self.S, -1, dtype=np.int32)
        rc = self.L.mmw_step_host(self.h, pts.ctypes.data, n.ctypes.data, dt.ctypes.data,
                                  assoc.ctypes.data, labels.ctypes.data, dbn.ctypes.data)
        scene_error = rc in (_lib.E_NONFINITE, _lib.E_SINGULAR, _lib.E_DIVZERO, _lib.E_CAPACITY)   # (the results are complete: the check is the last thing)
        if not ((rc == _lib.E_NONFINITE and not raise_nonfinite) or (scene_error and not check)):
            self._chk(rc)
        return assoc, labels, dbn

    def attach_posture(self, model=None):
        """mmw_attach_posture_frames (with frames = 3: mmw_attach_posture): hands the context a `mars.MarsCNN` (on this GPU; the
        3-frame model, or the single-frame one on a context with FB_FRAMES_BATCH = 0) so that `frame_host(posture=True)` runs
        TrackBuffer.estimate_posture behind the step in the same round trip; None detaches.  Only the model's tensors are read
        (k_w1 .. k_b2, dense1_dhwc, dense2).  The context keeps the weights' device pointers: the model must stay where it is
        (in-place updates are fine) until detached."""
        if model is None:
            self._chk(self.L.mmw_attach_posture_frames(self.h, None, self.ring))
            self._posture_model = None
            return
        d1, d2 = model.dense1_dhwc, model.dense2
        m = _lib.MmwPostureModel.of(*(t.data_ptr() for t in (model.k_w1, model.k_b1, model.k_w2, model.k_b2, d1.weight, d1.bias, d2.weight, d2.bias)),
                                    dense1_ld=d1.weight.stride(0))
        self._chk(self.L.mmw_attach_posture_frames(self.h, C.byref(m), model.frames))
        self._posture_model = model   # (keeps the tensors alive)

    def attach_posture_batch(self, weights=None, cap_rows: int = None):
        """mmw_posture_attach_frames (with frames = 3: mmw_posture_attach): the batched `TrackBuffer.estimate_posture` for every
        scene of this context, no torch on the path.
        `weights`: Keras-convention tensors of the context's model -- define_CNN_3D when FB_FRAMES_BATCH = 2, the single-frame
        define_CNN when FB_FRAMES_BATCH = 0 -- as a dict, an `.npz` or a Keras `.h5` path (what
        `MarsCNN.from_keras_weights` / `MarsCNN.load` take); both BatchNorms are folded on the host in fp64
        (`marsweights.fold_keras_weights`), the fp32 tensors uploaded and kept by this object, the split-fp16 Dense-1 operand built
        on the device.  `cap_rows` (default: S * track_cap) = the most tracks one call can estimate.  None detaches and frees.
        Refused: a model whose frame count is not the context's FB_FRAMES_BATCH + 1 (ValueError); with MmwError, E_ARG:
        FB_FRAMES_BATCH + 1 not 3 or 1, cap_rows < 1, a weight outside fp16's range."""
        if weights is None:
            self._chk(self.L.mmw_posture_attach_frames(self.h, None, self.ring, 0))
            self._free_posture_batch()
            return
        from .marsweights import FOLDED_KEYS, fold_keras_weights, load_keras_weights
        f = fold_keras_weights(load_keras_weights(weights))
        if f["frames"] != self.ring:
            raise ValueError(f"attach_posture_batch: these weights are the {f['frames']}-frame model's, this context holds {self.ring} "
                             f"frame(s) per track (FB_FRAMES_BATCH = {self.ring - 1})")
        cap = int(cap_rows if cap_rows is not None else self.S * self.track_cap)
        bufs = {k: DevBuf(self, f[k].nbytes).upload(f[k]) for k in FOLDED_KEYS}
        m = _lib.MmwPostureModel.of(*(bufs[k].ptr for k in FOLDED_KEYS), dense1_ld=f["dense1_w"].shape[1])
        rc = self.L.mmw_posture_attach_frames(self.h, C.byref(m), self.ring, cap)
        if rc != 0:   # (refused atomically: an earlier model stays attached, with its own buffers)
            for b in bufs.values():
                b.free()
            self._chk(rc)
        self._free_posture_batch()
        self._posture_batch = bufs

    def _free_posture_batch(self):
        if self._posture_batch:
            for b in self._posture_batch.values():
                b.free()
        self._posture_batch = None

    # -- per-scene posture models ----------------------------------------------
    def attach_posture_models(self, weights_list, scene_model=None, cap_rows: int = None):
        """mmw_posture_attach_models: several models behind one `estimate_posture`.  `weights_list`: 1 .. 8 entries, each whatever
        `attach_posture_batch` takes (folded by `marsweights.fold_keras_weights`, uploaded and kept by this object); `scene_model`:
        the model index of every scene, int[S] with `_lib.POSTURE_NONE` (-1) for a scene no model estimates (default: every scene
        on model 0); `cap_rows` (default: S * track_cap) = the most tracks one call can estimate, over all models.  Replaces an
        earlier attachment of either kind; `attach_posture_batch(None)` detaches.  Refused with nothing changed: a model whose
        frame count is not the context's FB_FRAMES_BATCH + 1, a map of another length (ValueError); with MmwError, E_ARG: a count
        outside 1 .. 8, a map entry outside [-1, n_models), cap_rows < 1, a weight outside fp16's range (the message names the
        model)."""
        from .marsweights import FOLDED_KEYS, fold_keras_weights, load_keras_weights
        folded = [fold_keras_weights(load_keras_weights(w)) for w in weights_list]
        for i, f in enumerate(folded):
            if f["frames"] != self.ring:
                raise ValueError(f"attach_posture_models: model {i} is the {f['frames']}-frame model, this context holds {self.ring} "
                                 f"frame(s) per track (FB_FRAMES_BATCH = {self.ring - 1})")
        smap = None
        if scene_model is not None:
            smap = np.ascontiguousarray(np.asarray(scene_model, dtype=np.int32).reshape(-1))
            if len(smap) != self.S:
                raise ValueError(f"attach_posture_models: a map of {len(smap)} entries for {self.S} scenes")
        cap = int(cap_rows if cap_rows is not None else self.S * self.track_cap)
        bufs = {}
        try:
            for i, f in enumerate(folded):
                for k in FOLDED_KEYS:
                    bufs[i, k] = DevBuf(self, f[k].nbytes).upload(f[k])
            structs = (_lib.MmwPostureModel * max(len(folded), 1))(*(
                _lib.MmwPostureModel.of(*(bufs[i, k].ptr for k in FOLDED_KEYS), dense1_ld=f["dense1_w"].shape[1]) for i, f in enumerate(folded)))
            rc = self.L.mmw_posture_attach_models(self.h, structs, len(folded), self.ring, smap.ctypes.data if smap is not None else None, cap)
        except BaseException:
            for b in bufs.values():
                b.free()
            raise
        if rc != 0:   # (refused atomically: an earlier attachment stays, with its own buffers)
            for b in bufs.values():
                b.free()
            self._chk(rc)
        self._free_posture_batch()
        self._posture_batch = bufs

    def set_scene_models(self, model_of, scenes=None):
        """mmw_posture_set_scene_models: move `scenes` (default: scenes 0 .. len(model_of)-1) to the models `model_of` (indices into
        the attached list, `_lib.POSTURE_NONE` = no model), from the next `estimate_posture` on.  The tracks keep the keypoints
        they have.  Refused (MmwError, E_ARG) with the map unchanged for an index out of range or listed twice, more entries than
        scenes, an id outside [-1, n_models), or no attachment."""
        a = np.ascontiguousarray(np.asarray(model_of, dtype=np.int32).reshape(-1))
        idx = None
        if scenes is not None:
            idx = np.ascontiguousarray(np.asarray(scenes, dtype=np.int32).reshape(-1))
            if len(idx) != len(a):
                raise ValueError(f"set_scene_models: {len(a)} models for {len(idx)} scenes")
        self._chk(self.L.mmw_posture_set_scene_models(self.h, idx.ctypes.data if idx is not None else None, len(a), a.ctypes.data if len(a) else None))

    def scene_models(self) -> np.ndarray:
        """mmw_posture_get_scene_models: the model index of every scene, int32[S] (`_lib.POSTURE_NONE` = no model)."""
        out = np.zeros(self.S, dtype=np.int32)
        self._chk(self.L.mmw_posture_get_scene_models(self.h, out.ctypes.data))
        return out

    def posture_group_rows(self) -> np.ndarray:
        """mmw_posture_group_rows: the rows every model estimated in the last `estimate_posture`, int32[n_models]."""
        rows, n = np.zeros(_lib.POSTURE_MODELS_MAX, dtype=np.int32), C.c_int32(0)
        self._chk(self.L.mmw_posture_group_rows(self.h, rows.ctypes.data, C.byref(n)))
        return rows[: n.value].copy()

    def posture_owners(self) -> np.ndarray:
        """mmw_posture_owners: (scene, track list position) of every row the last `estimate_posture` estimated, int32[n, 2], model
        by model and within a model by ascending scene.  Synchronises."""
        cap = int(self.posture_group_rows().sum())
        out, n = np.zeros((max(cap, 1), 2), dtype=np.int32), C.c_int32(0)
        self._chk(self.L.mmw_posture_owners(self.h, out.ctypes.data, cap, C.byref(n)))
        return out[: n.value].copy()

    def estimate_posture(self) -> int:
        """mmw_estimate_posture: features -> CNN -> `track.keypoints` for every eligible track of every scene, queued behind the
        last step on the context's stream (the host waits for the row count only).  Returns the tracks estimated."""
        rows = C.c_int32(0)
        self._chk(self.L.mmw_estimate_posture(self.h, C.byref(rows)))
        return int(rows.value)

    def posture_range(self) -> int:
        """mmw_posture_range: reads and clears the sticky range word of `estimate_posture` -- bit 0: a sample left fp16's range and
        was recomputed in fp32 (valid), bit 1: more than 64 such samples in one call, the surplus is meaningless.  Synchronises."""
        word = C.c_int32(0)
        self._chk(self.L.mmw_posture_range(self.h, C.byref(word)))
        return int(word.value)

    def frame_host(self, n: np.ndarray, dt: np.ndarray, raw: np.ndarray = None, pts: np.ndarray = None, want_rows: bool = False,
                   want_labels: bool = True, posture: bool = False, reuse_out: bool = False):
        """mmw_frame_host: one frame of every scene from host memory in ONE round trip.  `raw`[S,NP,5] radar rows (normalised
        on the device, Utils.normalize_data) or `pts`[S,NP,8] normalised rows; n[S], dt[S].  Returns a dict: assoc[S,NP],
        db_n[S], n_out[S] (rows that reached track()), n_tracks[S], labels[S,UM] (want_labels), rows[S,NP,8] (want_rows, raw form)."""
        assert (raw is None) != (pts is None)
        src = np.ascontiguousarray(raw if raw is not None else pts, dtype=np.float64)
        assert src.shape == (self.S, self.max_pts, 5 if raw is not None else 8), src.shape
        n = np.ascontiguousarray(n, dtype=np.int32)
        dt = np.ascontiguousarray(dt, dtype=np.float64)
        if reuse_out and self._frame_out is not None:
            out = self._frame_out   # (the caller copies what it keeps before the next call: TrackBuffer)
            out.pop("posture_rows", None)
        else:
            out = {"assoc": np.full((self.S, self.max_pts), -1, dtype=np.int32), "db_n": np.full(self.S, -1, dtype=np.int32),
                   "n_out": np.zeros(self.S, dtype=np.int32), "n_tracks": np.zeros(self.S, dtype=np.int32),
                   "labels": np.full((self.S, self.UM), -1, dtype=np.int32)}
            if reuse_out:
                self._frame_out = out
        if not want_labels and not reuse_out:
            out.pop("labels")
        if want_rows and raw is not None:
            out["rows"] = np.zeros((self.S, self.max_pts, 8))
        elif "rows" in out:
            out.pop("rows")
        args = (self.h, src.ctypes.data if raw is not None else None, src.ctypes.data if raw is None else None,
                n.ctypes.data, dt.ctypes.data, out["rows"].ctypes.data if "rows" in out else None,
                out["n_out"].ctypes.data, out["assoc"].ctypes.data,
                out["labels"].ctypes.data if want_labels else None, out["db_n"].ctypes.data, out["n_tracks"].ctypes.data)
        if posture:   # ... and estimate_posture with the attached model behind the step (mmw_frame_posture_host)
            rows = C.c_int32(0)
            rc = self.L.mmw_frame_posture_host(*args, C.byref(rows))
            out["posture_rows"] = int(rows.value)   # (written before the first scene error is reported: a caller that catches the
            self._chk(rc)                           #  reference's ValueError must still see that estimate_posture ran on the device)
        else:
            self._chk(self.L.mmw_frame_host(*args))
        return out

    def normalize_host(self, raw: np.ndarray, n_raw: np.ndarray):
        """Utils.normalize_data for all scenes: raw[S,NP,5] -> (pts[S,NP,8], n_out[S])."""
        raw = np.ascontiguousarray(raw, dtype=np.float64)
        n_raw = np.ascontiguousarray(n_raw, dtype=np.int32)
        assert raw.shape == (self.S, self.max_pts, 5)
        b_raw = self.buf("norm_raw", raw.nbytes).upload(raw)
        b_n = self.buf("norm_n", n_raw.nbytes).upload(n_raw)
        b_out = self.buf("norm_out", self.S * self.max_pts * 64)
        b_no = self.buf("norm_no", self.S * 4)
        self._chk(self.L.mmw_normalize(self.h, b_raw.ptr, b_n.ptr, b_out.ptr, b_no.ptr))
        n_out = b_no.download((self.S,), np.int32)
        pts = b_out.download((self.S, self.max_pts, 8), np.float64)
        for s in range(self.S):
            pts[s, n_out[s]:] = 0.0
        return pts, n_out

    def dbscan_host(self, pts: np.ndarray, n: np.ndarray, eps=None, min_samples=None, raise_nonfinite: bool = True):
        """Utils.apply_DBscan labels for S clouds: pts[S,max_n,8] -> (labels[S,max_n], n_clusters[S]).  A cloud with a NaN / an
        infinite value raises ValueError as sklearn's input validation does (Utils.py:272-278); with raise_nonfinite=False such
        clouds come back with n_clusters = -16 (NaN) / -32 (infinity) and labels -1."""
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        n = np.ascontiguousarray(n, dtype=np.int32)
        max_n = pts.shape[1]
        assert pts.shape == (self.S, max_n, 8)
        b_p = self.buf("db_pts", pts.nbytes).upload(pts)
        b_n = self.buf("db_n", n.nbytes).upload(n)
        b_l = self.buf("db_lab", self.S * max_n * 4)
        b_c = self.buf("db_ncl", self.S * 4)
        self._chk(self.L.mmw_dbscan(self.h, b_p.ptr, b_n.ptr, max_n,
                                    self.cfg.db_eps if eps is None else float(eps),
                                    self.cfg.db_min_samples if min_samples is None else int(min_samples),
                                    b_l.ptr, b_c.ptr))
        labels = b_l.download((self.S, max_n), np.int32)
        ncl = b_c.download((self.S,), np.int32)
        for s in range(self.S):
            labels[s, n[s]:] = -1
            if ncl[s] < 0:   # sklearn's input validation refused the cloud (a NaN / an infinite value): no labels
                labels[s] = -1
        if raise_nonfinite and (ncl < 0).any():
            s = int(np.flatnonzero(ncl < 0)[0])
            raise _lib.MmwNonFinite(_lib.E_NONFINITE, f"cloud {s}: " + ("Input X contains NaN." if ncl[s] == -_lib.ERRBIT_NONFINITE_NAN
                                                                       else "Input X contains infinity or a value too large for dtype('float64')."))
        return labels, ncl

    def features_dev(self, feat_ptr, owner_ptr, cap_rows: int) -> int:
        nrows = C.c_int32(0)
        self._chk(self.L.mmw_features(self.h, feat_ptr, owner_ptr, int(cap_rows), C.byref(nrows)))
        return nrows.value

    def features_async(self, feat_ptr, owner_ptr, uid_ptr, cap_rows: int, ticket: int = 0):
        """mmw_features without the host wait (pipelined callers): rows behind the last step on the context's stream."""
        self._chk(self.L.mmw_features_async(self.h, feat_ptr, owner_ptr, uid_ptr, int(cap_rows), int(ticket)))

    def features_wait(self, ticket: int = 0) -> int:
        """Rows of the `features_async` call with this ticket (waits for its total only, not for the stream)."""
        nrows = C.c_int32(0)
        self._chk(self.L.mmw_features_wait(self.h, int(ticket), C.byref(nrows)))
        return nrows.value

    def set_keypoints_uid_dev(self, kp_ptr, owner_ptr, uid_ptr, n_rows: int):
        """Keypoint scatter matched by track creation ordinal (rows taken one or more frames ago)."""
        self._chk(self.L.mmw_set_keypoints_uid(self.h, kp_ptr, owner_ptr, uid_ptr, int(n_rows)))

    def set_keypoints_ticket_dev(self, kp_ptr, owner_ptr, uid_ptr, n_rows: int, ticket: int):
        """The same for the rows `features_async(ticket=ticket)` wrote: rows of a scene that `reset`, `reset_scenes` or `restore`
        touched since then are dropped -- its uids start over, and a uid of before must not alias one of after."""
        self._chk(self.L.mmw_set_keypoints_ticket(self.h, kp_ptr, owner_ptr, uid_ptr, int(n_rows), int(ticket)))

    def features_host(self, cap_rows=None):
        """Returns (feat[B,ring,8,8,5] float32 (or [B,8,8,5] when ring == 1), owner[B,2])."""
        cap = int(cap_rows if cap_rows is not None else self.S * self.track_cap)
        per = self.ring * 64 * 5
        b_f = self.buf("feat", max(cap, 1) * per * 4)
        b_o = self.buf("owner", max(cap, 1) * 8)
        nrows = self.features_dev(b_f.ptr, b_o.ptr, cap)
        shape = (nrows, self.ring, 8, 8, 5) if self.ring > 1 else (nrows, 8, 8, 5)
        if nrows == 0:
            return np.zeros(shape, np.float32), np.zeros((0, 2), np.int32)
        feat = b_f.download((nrows, per), np.float32).reshape(shape)
        owner = b_o.download((nrows, 2), np.int32)
        return feat, owner

    def set_keypoints_dev(self, kp_ptr, owner_ptr, n_rows: int):
        self._chk(self.L.mmw_set_keypoints(self.h, kp_ptr, owner_ptr, int(n_rows)))

    def set_keypoints_host(self, kp: np.ndarray, owner: np.ndarray):
        kp = np.ascontiguousarray(kp, dtype=np.float32).reshape(-1, NKP)
        owner = np.ascontiguousarray(owner, dtype=np.int32).reshape(-1, 2)
        if len(owner) == 0:
            return
        b_k = self.buf("kp", kp.nbytes).upload(kp)
        b_o = self.buf("kp_owner", owner.nbytes).upload(owner)
        self.set_keypoints_dev(b_k.ptr, b_o.ptr, len(owner))

    # -- read-back ------------------------------------------------------------
    def num_tracks(self) -> np.ndarray:
        out = np.zeros(self.S, dtype=np.int32)
        self._chk(self.L.mmw_get_num_tracks(self.h, out.ctypes.data))
        return out

    def tracks(self, cap=None) -> np.ndarray:
        """effective_tracks of every scene as a structured array [S, cap] (zero past n_tracks)."""
        cap = int(cap if cap is not None else self.track_cap)
        out = np.zeros((self.S, cap), dtype=TRACK_DTYPE)
        self._chk(self.L.mmw_get_tracks(self.h, out.ctypes.data, cap))
        return out

    def batch_ring(self):
        ln = np.zeros(self.S, dtype=np.int32)
        rn = np.zeros((self.S, RING_MAX), dtype=np.int32)
        self._chk(self.L.mmw_get_batch_ring(self.h, ln.ctypes.data, rn.ctypes.data))
        return ln, rn

    def track_ring_frame(self, scene: int, track: int, k: int) -> np.ndarray:
        out = np.zeros((self.ring_rows, 8))
        n = C.c_int32(0)
        self._chk(self.L.mmw_get_track_ring_frame(self.h, scene, track, k, out.ctypes.data, C.byref(n)))
        return out[: n.value].copy()

    def batch_ring_frame(self, scene: int, k: int) -> np.ndarray:
        out = np.zeros((self.max_pts, 8))
        n = C.c_int32(0)
        self._chk(self.L.mmw_get_batch_ring_frame(self.h, scene, k, out.ctypes.data, C.byref(n)))
        return out[: n.value].copy()

    def inner_calls(self, cap_labels=None):
        """seek_inner_clusters calls of the last step (contexts with seek_inner = 1): per scene a list of label arrays,
        one per call, in track-list order (mmw_get_inner)."""
        cap = int(cap_labels if cap_labels is not None else 2 * self.ring * self.ring_rows)
        n = np.zeros(self.S, dtype=np.int32)
        rows = np.zeros((self.S, 16), dtype=np.int32)
        lab = np.full((self.S, cap), -2, dtype=np.int32)
        self._chk(self.L.mmw_get_inner(self.h, n.ctypes.data, rows.ctypes.data, lab.ctypes.data, cap))
        out = []
        for s in range(self.S):
            calls, off = [], 0
            for k in range(min(int(n[s]), 16)):
                calls.append(lab[s, off: off + rows[s, k]].copy())
                off += int(rows[s, k])
            out.append(calls)
        return out

    def track_table_dev(self, table_ptr, slots: int, scene_base: int = 0):
        self._chk(self.L.mmw_track_table(self.h, table_ptr, int(slots), int(scene_base)))

    def track_table_host(self, slots: int, scene_base: int = 0) -> np.ndarray:
        b = self.buf("table", self.S * slots * SUMMARY_DTYPE.itemsize)
        self.track_table_dev(b.ptr, slots, scene_base)
        return b.download((self.S, slots), SUMMARY_DTYPE)

    def _export_wait(self, wait, ticket: int, counts: int = 2):
        """The counts of an export's `*_wait` entry -- a pair, or with counts=1 one int; E_CAPACITY becomes an MmwError that
        carries them in `.needed`."""
        n = [C.c_int32(0) for _ in range(counts)]
        rc = wait(self.h, int(ticket), *[C.byref(v) for v in n])
        got = tuple(int(v.value) for v in n) if counts > 1 else int(n[0].value)
        if rc == _lib.E_CAPACITY:
            err = error_for(rc, _lib.last_error(self.h))
            err.needed = got
            raise err
        self._chk(rc)
        return got

    def _export_host(self, name: str, issue, wait, *outs):
        """What the `*_host` exports share: issue under the last ticket, wait for the counts, on E_CAPACITY grow to what the
        device says it needs and ask once more, download.  `outs`: a (buffer name, dtype) per output array, sized by
        `_export_caps[name]`; `issue(ptr, cap, [ptr, cap,] ticket)` queues the export; `wait` is its `*_wait` entry.  One retry is
        enough: a refused export writes and consumes nothing, and nothing else runs on the context's stream in between, so the
        counts it reported are the counts the second call finds.  Returns one array per output."""
        ticket = _lib.EXPORT_TICKETS - 1
        for attempt in (0, 1):
            caps = self._export_caps[name]
            bufs = [self.buf(bn, cap * np.dtype(dt).itemsize) for (bn, dt), cap in zip(outs, caps)]
            issue(*[v for b, cap in zip(bufs, caps) for v in (b.ptr, cap)], ticket)
            try:
                counts = self._export_wait(wait, ticket)
                break
            except MmwError as e:
                if e.code != _lib.E_CAPACITY or attempt:
                    raise
                if max(e.needed) >= 2 ** 31 - 1:   # (saturated: more than an int32 counts -- no buffer can be offered)
                    raise MmwError(_lib.E_CAPACITY, f"{name}_host: what this context holds exceeds INT32_MAX entries, rows or points; "
                                                    "ask for fewer scenes per context") from e
                self._export_caps[name] = tuple(max(cap, need) for cap, need in zip(caps, e.needed))
        return tuple(b.download((n,), dt) if n else np.zeros(0, dt) for b, (_, dt), n in zip(bufs, outs, counts))

    # -- live-track report ----------------------------------------------------
    def enable_report(self, on: bool = True):
        """mmw_report_enable: the tracks live now become the baseline of the next report (they produce no event); on=False
        frees it.  Until enabled, the report calls are refused (E_ARG) and the context launches nothing of them."""
        self._chk(self.L.mmw_report_enable(self.h, 1 if on else 0))

    def report_async(self, rows_ptr, cap_rows: int, events_ptr, cap_events: int, scene_base: int = 0, ticket: int = 0):
        """mmw_report_async: one `_lib.TRACK_REPORT_DTYPE` row per live track in (scene, slot) order and the
        `_lib.TRACK_EVENT_DTYPE` events since the previous report into device buffers, queued behind the last step on the
        context's stream -- no host wait.  Tickets 0 .. 3 (`report_host` uses 3)."""
        self._chk(self.L.mmw_report_async(self.h, rows_ptr, int(cap_rows), events_ptr, int(cap_events), int(scene_base), int(ticket)))

    def report_wait(self, ticket: int = 0):
        """(n_rows, n_events) of the `report_async` call with this ticket: waits for its counts only, not for the stream.
        Buffers too small: MmwError with code E_CAPACITY and the counts needed in `.needed` -- nothing was written and the
        baseline is unchanged, so the same report can be asked for again with room."""
        return self._export_wait(self.L.mmw_report_wait, ticket)

    def report_host(self, scene_base: int = 0):
        """The report as two structured arrays: (rows[n_rows] TRACK_REPORT_DTYPE, events[n_events] TRACK_EVENT_DTYPE).  A
        difference of states, not a log: a track born and gone between two reports appears in neither.  The buffers grow to
        what the device says it needs (a refused report loses nothing)."""
        return self._export_host("report", lambda *a: self.report_async(*a[:4], scene_base, a[4]), self.L.mmw_report_wait,
                                 ("report_rows", _lib.TRACK_REPORT_DTYPE), ("report_events", _lib.TRACK_EVENT_DTYPE))

    # -- live-track point clouds ----------------------------------------------
    def clouds_dev(self, dir_ptr, cap_tracks: int, out_ptr, cap_points: int, mode: int = 0, ticket: int = 0, scene_base: int = 0):
        """mmw_clouds_async: every live track's `effective_data` into device buffers -- a `_lib.CLOUD_TRACK_DTYPE` directory entry
        per track in the report's (scene, slot) order and, back to back, their points (`_lib.CLOUD_POINT_DTYPE`, mode
        `_lib.CLOUD_POINTS`) or ring rows (float64[8], `_lib.CLOUD_ROWS`); `| _lib.CLOUD_UNASSIGNED` adds each scene's global ring as
        an entry with slot -1.  Queued behind the last step on the context's stream -- no host wait.  Tickets 0 .. 3
        (`clouds_host` uses 3).  `out_ptr` 16-byte aligned."""
        self._chk(self.L.mmw_clouds_async(self.h, dir_ptr, int(cap_tracks), out_ptr, int(cap_points), int(mode), int(scene_base), int(ticket)))

    def clouds_wait(self, ticket: int = 0):
        """(n_tracks, n_points) of the `clouds_dev` call with this ticket: waits for its counts only, not for the stream.  Buffers
        too small: MmwError with code E_CAPACITY and the counts needed in `.needed` -- nothing was written."""
        return self._export_wait(self.L.mmw_clouds_wait, ticket)

    def clouds_host(self, rows: bool = False, unassigned: bool = False, scene_base: int = 0):
        """(dir[n_tracks] CLOUD_TRACK_DTYPE, points[n_points] CLOUD_POINT_DTYPE) -- or, with rows=True, the ring rows
        float64[n_points, 8]: entry i owns out[first : first + count], frames oldest first (`track.batch.effective_data`), and
        without `unassigned` entry i is the track of `report_host` row i.  The device buffers are kept and grow to what the
        device says it needs (one retry)."""
        mode = (_lib.CLOUD_ROWS if rows else _lib.CLOUD_POINTS) | (_lib.CLOUD_UNASSIGNED if unassigned else 0)
        odt = np.dtype((np.float64, (8,))) if rows else _lib.CLOUD_POINT_DTYPE
        return self._export_host("clouds", lambda *a: self.clouds_dev(*a[:4], mode, a[4], scene_base), self.L.mmw_clouds_wait,
                                 ("cloud_dir", _lib.CLOUD_TRACK_DTYPE), ("cloud_out", odt))

    # -- training samples -----------------------------------------------------
    def samples_dev(self, dir_ptr, cap_samples: int, out_ptr, mode: int = 0, flags_ptr=None, ticket: int = 0, scene_base: int = 0):
        """mmw_samples_async: what preprocessing.py:192-220 saves of every asked scene whose `effective_tracks[0]` was updated by
        the last step (lifetime 0) -- a `_lib.SAMPLE_ENTRY_DTYPE` directory entry per sample, scenes ascending, and per entry the
        (192, 5) float64 block of `relative_coordinates` + `format_batched_frames` (`_lib.SAMPLE_BLOCK`) or the (8, 8, 5) float32
        CNN input `format_mmwave_to_npy` makes of it (`_lib.SAMPLE_INPUT`); `| _lib.SAMPLE_ABSOLUTE` leaves the centroid in.
        `flags_ptr`: device int32[S], the scenes that ran track() this frame (None = all).  Queued behind the last step on the
        context's stream -- no host wait.  Tickets 0 .. 3 (`samples_host` uses 3).  `out_ptr` 16-byte aligned."""
        self._chk(self.L.mmw_samples_async(self.h, dir_ptr, int(cap_samples), out_ptr, int(mode), flags_ptr, int(scene_base), int(ticket)))

    def samples_wait(self, ticket: int = 0) -> int:
        """Samples of the `samples_dev` call with this ticket: waits for its count only, not for the stream.  Buffers too small:
        MmwError with code E_CAPACITY and the count needed in `.needed` -- nothing was written."""
        return self._export_wait(self.L.mmw_samples_wait, ticket, counts=1)

    def samples_host(self, inputs: bool = False, absolute: bool = False, scenes=None, scene_base: int = 0):
        """(dir[n] SAMPLE_ENTRY_DTYPE, blocks): blocks float64[n, 192, 5], or with inputs=True float32[n, 8, 8, 5].  `scenes`:
        the scenes that ran track() this frame (default all).  At most one sample per scene, so the buffers are sized by the
        context's scene count and never grow."""
        mode = (_lib.SAMPLE_INPUT if inputs else _lib.SAMPLE_BLOCK) | (_lib.SAMPLE_ABSOLUTE if absolute else 0)
        edt = _lib.SAMPLE_ENTRY_DTYPE
        shape, dt = (_lib.SAMPLE_INPUT_SHAPE, np.float32) if inputs else (_lib.SAMPLE_BLOCK_SHAPE, np.float64)
        item = int(np.prod(shape)) * np.dtype(dt).itemsize
        flags_ptr = self._scene_flags(scenes, "sample_flags")
        b_d, b_o = self.buf("sample_dir", self.S * edt.itemsize), self.buf("sample_out", self.S * item)
        self.samples_dev(b_d.ptr, self.S, b_o.ptr, mode, flags_ptr, _lib.EXPORT_TICKETS - 1, scene_base)
        n = self.samples_wait(_lib.EXPORT_TICKETS - 1)
        d = b_d.download((n,), edt) if n else np.zeros(0, edt)
        out = b_o.download((n,) + shape, dt) if n else np.zeros((0,) + shape, dt)
        return d, out

    # -- live-track skeletons -------------------------------------------------
    def skeletons_dev(self, out_ptr, cap: int, mode: int = 0, ticket: int = 0, scene_base: int = 0):
        """mmw_skeletons_async: every live track's room-frame skeleton (`_lib.SKELETON_DTYPE`: the keypoints mirrored and shifted
        to the track's position as Visualizer.update_posture does, with its plausibility check in `flags` / `gap`) into a device
        buffer, in the report's (scene, slot) order.  `_lib.SKEL_ALL`: one entry per live track, entry i is `report_host` row i;
        `_lib.SKEL_DRAWN`: only the entries the reference draws, `row` keeping the report index.  Queued behind the last step on
        the context's stream -- no host wait.  Tickets 0 .. 3 (`skeletons_host` uses 3).  `out_ptr` 16-byte aligned.  Called
        between the step and `estimate_posture` it gives what main.py:56 displays (last frame's keypoints around this frame's
        position), called after `estimate_posture` this frame's keypoints."""
        self._chk(self.L.mmw_skeletons_async(self.h, out_ptr, int(cap), int(mode), int(scene_base), int(ticket)))

    def skeletons_wait(self, ticket: int = 0):
        """(n_out, n_live) of the `skeletons_dev` call with this ticket: waits for its counts only, not for the stream.  Buffer
        too small: MmwError with code E_CAPACITY and both counts in `.needed` -- nothing was written."""
        return self._export_wait(self.L.mmw_skeletons_wait, ticket)

    def skeletons_host(self, drawn: bool = False, scene_base: int = 0) -> np.ndarray:
        """The skeletons as a `_lib.SKELETON_DTYPE` array: one per live track (entry i is `report_host` row i), or with
        drawn=True only those the reference's check lets through.  The device buffer is kept and grows to what the device says
        it needs (one retry)."""
        mode = _lib.SKEL_DRAWN if drawn else _lib.SKEL_ALL
        return self._export_host("skeletons", lambda ptr, cap, ticket: self.skeletons_dev(ptr, cap, mode, ticket, scene_base),
                                 self.L.mmw_skeletons_wait, ("skeletons", _lib.SKELETON_DTYPE))[0]

    # -- per-scene tables and by-uid samplers (zones, trails, tripwires) --------
    def _set_scene_table(self, name, noun, setter, make, dtype, per_scene, table, scenes):
        """One mmw_set_* call of a per-scene table: `table` is what `make` takes or its result, the pair (counts, dtype[n, per_scene])."""
        if isinstance(table, tuple) and len(table) == 2 and isinstance(table[1], np.ndarray) and table[1].dtype == dtype:
            cnt, tab = table
        else:
            cnt, tab = make(table)
        cnt = np.ascontiguousarray(np.asarray(cnt, dtype=np.int32).reshape(-1))
        tab = np.ascontiguousarray(tab.reshape(-1, per_scene))
        if len(cnt) != len(tab):
            raise ValueError(f"{name}: {len(cnt)} counts for {len(tab)} scenes' {noun}")
        idx = None
        if scenes is not None:
            idx = np.ascontiguousarray(np.asarray(scenes, dtype=np.int32).reshape(-1))
            if len(idx) != len(cnt):
                raise ValueError(f"{name}: {len(cnt)} entries for {len(idx)} scenes")
        self._chk(setter(self.h, idx.ctypes.data if idx is not None else None, len(cnt), cnt.ctypes.data if len(cnt) else None,
                         tab.ctypes.data if len(cnt) else None))

    def _get_scene_table(self, getter, dtype, per_scene):
        """One mmw_get_* call: (counts int32[S], table dtype[S, per_scene]) from the host mirror."""
        cnt = np.zeros(self.S, dtype=np.int32)
        tab = np.zeros((self.S, per_scene), dtype=dtype)
        self._chk(getter(self.h, cnt.ctypes.data, tab.ctypes.data))
        return cnt, tab

    def _sample(self, sample_dev, prefix, t, scenes):
        """A sample call from host arrays: `t` and the scene flags go up through the kept buffers `<prefix>_t` and `<prefix>_flags`."""
        t_ptr = None
        if t is not None:
            t_ptr = self.buf(prefix + "_t", self.S * 8).upload(np.ascontiguousarray(np.broadcast_to(np.asarray(t, dtype=np.float64), (self.S,)))).ptr
        sample_dev(self._scene_flags(scenes, prefix + "_flags"), t_ptr)

    # -- zone occupancy -------------------------------------------------------
    def set_zones(self, zones, scenes=None):
        """mmw_set_zones: give `scenes` (default: scenes 0 .. len(zones)-1) their zones -- `zones` is what `_lib.make_zones` takes (a
        list per scene of dicts or tuples) or its result, the pair (n_zones, ZONE_DTYPE[n, 16]).  Scenes never listed keep what they
        have; the listed scenes' memberships are void (their next export starts with a ZEV_REBASED).  Refused (MmwError, E_ARG) with
        nothing changed for an index out of range or listed twice, more entries than scenes, a NaN bound, x0 > x1 or y0 > y1, a
        margin that is negative or not finite, or a non-zero `reserved_`."""
        self._set_scene_table("set_zones", "zones", self.L.mmw_set_zones, _lib.make_zones, _lib.ZONE_DTYPE, _lib.ZONES_MAX, zones, scenes)

    def zones(self):
        """mmw_get_zones: (n_zones int32[S], zones ZONE_DTYPE[S, 16]) of every scene, from the host mirror; zero past a scene's zones."""
        return self._get_scene_table(self.L.mmw_get_zones, _lib.ZONE_DTYPE, _lib.ZONES_MAX)

    def clear_zones(self):
        """mmw_clear_zones: waits for the stream and frees table and baseline; the context launches what one without zones does."""
        self._chk(self.L.mmw_clear_zones(self.h))

    @property
    def has_zones(self) -> bool:
        rc = int(self.L.mmw_has_zones(self.h))
        if rc < 0:
            self._chk(rc)
        return rc == 1

    def zones_async(self, rows_ptr, cap_rows: int, events_ptr, cap_events: int, scene_base: int = 0, ticket: int = 0):
        """mmw_zones_async: one `_lib.ZONE_ROW_DTYPE` row per defined zone in (scene, zone) order and the `_lib.ZONE_EVENT_DTYPE`
        membership changes since the previous export into device buffers, queued behind the last step on the context's stream --
        no host wait.  Tickets 0 .. 3 (`zones_host` uses 3)."""
        self._chk(self.L.mmw_zones_async(self.h, rows_ptr, int(cap_rows), events_ptr, int(cap_events), int(scene_base), int(ticket)))

    def zones_wait(self, ticket: int = 0):
        """(n_rows, n_events) of the `zones_async` call with this ticket: waits for its counts only, not for the stream.  Buffers
        too small: MmwError with code E_CAPACITY and the counts needed in `.needed` -- nothing was written and the baseline is
        unchanged, so the same export can be asked for again with room."""
        return self._export_wait(self.L.mmw_zones_wait, ticket)

    def zones_host(self, scene_base: int = 0):
        """The zone export as two structured arrays: (rows[n_rows] ZONE_ROW_DTYPE, events[n_events] ZONE_EVENT_DTYPE); fold the events
        with `zones.Roster`.  The buffers grow to what the device says it needs (a refused export loses nothing)."""
        self._export_caps.setdefault("zones", (64, 64))   # (its entry exists from the first call on: a context without zones keeps the four it had)
        return self._export_host("zones", lambda *a: self.zones_async(*a[:4], scene_base, a[4]), self.L.mmw_zones_wait,
                                 ("zone_rows", _lib.ZONE_ROW_DTYPE), ("zone_events", _lib.ZONE_EVENT_DTYPE))

    # -- track trails ---------------------------------------------------------
    def enable_trails(self, depth: int):
        """mmw_trails_enable: per live uid a ring of its last `depth` (1 .. `_lib.TRAIL_DEPTH_MAX`) sampled positions, with the time
        of its first sample and the distance it walked; every trail starts empty, also when trails were enabled before.  depth=0
        frees them.  Until enabled, the trail calls are refused (E_ARG) and the context launches nothing of them."""
        self._chk(self.L.mmw_trails_enable(self.h, int(depth)))

    def sample_trails_dev(self, flags_ptr=None, t_ptr=None):
        """mmw_trails_sample: one sample of every live track of the asked scenes, queued behind the last step on the context's
        stream -- no host wait.  `flags_ptr`: device int32[S], non-zero = asked (the step's n_pts array serves; None = every
        scene); `t_ptr`: device float64[S], the samples' time (None = each scene's count of earlier sample calls)."""
        self._chk(self.L.mmw_trails_sample(self.h, flags_ptr, t_ptr))

    def sample_trails(self, t=None, scenes=None):
        """`sample_trails_dev` from host arrays: `t` float64[S] or a scalar for every scene (None = the call ordinals), `scenes` the
        scenes to sample (default all)."""
        self._sample(self.sample_trails_dev, "trail", t, scenes)

    def trails_dev(self, dir_ptr, cap_tracks: int, points_ptr, cap_points: int, last: int = 0, ticket: int = 0, scene_base: int = 0):
        """mmw_trails_async: every live track's trail into device buffers -- a `_lib.TRAIL_TRACK_DTYPE` directory entry per track in
        the report's (scene, slot) order and, back to back, their points (`_lib.TRAIL_POINT_DTYPE`), oldest first; `last` > 0 cuts
        every trail to its newest `last` points.  Queued on the context's stream -- no host wait.  Tickets 0 .. 3 (`trails_host`
        uses 3).  Both pointers 8-byte aligned."""
        self._chk(self.L.mmw_trails_async(self.h, dir_ptr, int(cap_tracks), points_ptr, int(cap_points), int(last), int(scene_base), int(ticket)))

    def trails_wait(self, ticket: int = 0):
        """(n_tracks, n_points) of the `trails_dev` call with this ticket: waits for its counts only, not for the stream.  Buffers
        too small: MmwError with code E_CAPACITY and the counts needed in `.needed` -- nothing was written."""
        return self._export_wait(self.L.mmw_trails_wait, ticket)

    def trails_host(self, last: int = 0, scene_base: int = 0):
        """(dir[n_tracks] TRAIL_TRACK_DTYPE, points[n_points] TRAIL_POINT_DTYPE): entry i owns points[first : first + count], oldest
        first, and is the track of `report_host` row i; `trails.split` gives the views.  The device buffers are kept and grow to
        what the device says it needs (one retry; the export consumes nothing)."""
        self._export_caps.setdefault("trails", (64, 4096))   # (its entry exists from the first call on, as the zones')
        return self._export_host("trails", lambda *a: self.trails_dev(*a[:4], last, a[4], scene_base), self.L.mmw_trails_wait,
                                 ("trail_dir", _lib.TRAIL_TRACK_DTYPE), ("trail_points", _lib.TRAIL_POINT_DTYPE))

    # -- tripwires ------------------------------------------------------------
    def enable_tripwires(self, log_depth: int = 256):
        """mmw_tripwires_enable: per scene a wire table (0 wires to begin with), per-uid sides, per-wire crossing counters and a log
        of `log_depth` (1 .. `_lib.TRIPWIRE_LOG_MAX`) events; everything starts over, also when tripwires were enabled before.
        log_depth=0 frees them.  Until enabled, the tripwire calls are refused (E_ARG) -- `tripwires()` reports 0 wires -- and the
        context launches nothing of them."""
        self._chk(self.L.mmw_tripwires_enable(self.h, int(log_depth)))

    def set_tripwires(self, wires, scenes=None):
        """mmw_set_tripwires: give `scenes` (default: scenes 0 .. len(wires)-1) their wires -- `wires` is what
        `_lib.make_tripwires` takes (a list per scene of dicts or tuples) or its result, the pair (n_wires, TRIPWIRE_DTYPE[n, 16]).
        Scenes never listed keep what they have; the listed scenes' counters restart at 0 and their sides are void (their next
        sample logs a TW_REBASED).  Refused (MmwError, E_ARG) with nothing changed for an index out of range or listed twice, more
        entries than scenes, a coordinate that is not finite, A == B, a margin that is negative or not finite, a squared length or
        band that is zero or not finite, or a non-zero `reserved_`."""
        self._set_scene_table("set_tripwires", "wires", self.L.mmw_set_tripwires, _lib.make_tripwires, _lib.TRIPWIRE_DTYPE, _lib.TRIPWIRES_MAX, wires, scenes)

    def tripwires(self):
        """mmw_get_tripwires: (n_wires int32[S], wires TRIPWIRE_DTYPE[S, 16]) of every scene, from the host mirror; zero past a
        scene's wires."""
        return self._get_scene_table(self.L.mmw_get_tripwires, _lib.TRIPWIRE_DTYPE, _lib.TRIPWIRES_MAX)

    def sample_tripwires_dev(self, flags_ptr=None, t_ptr=None):
        """mmw_tripwires_sample: every live track's side of every wire of the asked scenes, crossings counted and logged, queued
        behind the last step on the context's stream -- no host wait.  `flags_ptr`: device int32[S], non-zero = asked (the step's
        n_pts array serves; None = every scene); `t_ptr`: device float64[S], the events' time (None = each scene's count of earlier
        sample calls)."""
        self._chk(self.L.mmw_tripwires_sample(self.h, flags_ptr, t_ptr))

    def sample_tripwires(self, t=None, scenes=None):
        """`sample_tripwires_dev` from host arrays: `t` float64[S] or a scalar for every scene (None = the call ordinals), `scenes`
        the scenes to sample (default all)."""
        self._sample(self.sample_tripwires_dev, "tripwire", t, scenes)

    def tripwires_async(self, rows_ptr, cap_rows: int, events_ptr, cap_events: int, scene_base: int = 0, ticket: int = 0):
        """mmw_tripwires_async: one `_lib.TRIPWIRE_ROW_DTYPE` row per defined wire in (scene, wire) order and the
        `_lib.TRIPWIRE_EVENT_DTYPE` events logged since the previous successful export into device buffers, queued on the context's
        stream -- no host wait.  Tickets 0 .. 3 (`tripwires_host` uses 3).  Both pointers 8-byte aligned."""
        self._chk(self.L.mmw_tripwires_async(self.h, rows_ptr, int(cap_rows), events_ptr, int(cap_events), int(scene_base), int(ticket)))

    def tripwires_wait(self, ticket: int = 0):
        """(n_rows, n_events) of the `tripwires_async` call with this ticket: waits for its counts only, not for the stream.  Buffers
        too small: MmwError with code E_CAPACITY and the counts needed in `.needed` -- nothing was written and nothing was taken, so
        the same export can be asked for again with room."""
        return self._export_wait(self.L.mmw_tripwires_wait, ticket)

    def tripwires_host(self, scene_base: int = 0):
        """The tripwire export as two structured arrays: (rows[n_rows] TRIPWIRE_ROW_DTYPE, events[n_events] TRIPWIRE_EVENT_DTYPE);
        fold the events with `tripwires.Tally`.  The buffers grow to what the device says it needs (a refused export loses
        nothing)."""
        self._export_caps.setdefault("tripwires", (64, 256))   # (its entry exists from the first call on, as the zones')
        return self._export_host("tripwires", lambda *a: self.tripwires_async(*a[:4], scene_base, a[4]), self.L.mmw_tripwires_wait,
                                 ("tripwire_rows", _lib.TRIPWIRE_ROW_DTYPE), ("tripwire_events", _lib.TRIPWIRE_EVENT_DTYPE))

    # -- stance watch ---------------------------------------------------------
    def enable_stance(self, log_depth: int = 256):
        """mmw_stance_enable: per scene a rule table (no rule to begin with), per-uid stance classes, the fall and long-lie counters
        and a log of `log_depth` (1 .. `_lib.STANCE_LOG_MAX`) events; everything starts over, also when stance was enabled before.
        log_depth=0 frees it.  Until enabled, the stance calls are refused (E_ARG) -- `stance_rules()` reports 0 rules -- and the
        context launches nothing of them."""
        self._chk(self.L.mmw_stance_enable(self.h, int(log_depth)))

    def set_stance_rules(self, rules, scenes=None):
        """mmw_set_stance_rules: give `scenes` (default: scenes 0 .. len(rules)-1) their rule -- `rules` is what
        `_lib.make_stance_rules` takes (a list per scene of zero or one dict or tuple) or its result, the pair (n_rules,
        STANCE_RULE_DTYPE[n, 1]).  Scenes never listed keep what they have; the listed scenes' counters restart at 0 and their
        classes are void (their next sample logs a SEV_REBASED).  Refused (MmwError, E_ARG) with nothing changed for an index out of
        range or listed twice, more entries than scenes, a height, margin, window or gap that is not finite, a negative margin,
        window or long_lie, max_gap <= 0, h_lie + margin not below h_stand - margin, or a non-zero `reserved_`."""
        self._set_scene_table("set_stance_rules", "rules", self.L.mmw_set_stance_rules, _lib.make_stance_rules, _lib.STANCE_RULE_DTYPE,
                              _lib.STANCE_RULES_MAX, rules, scenes)

    def stance_rules(self):
        """mmw_get_stance_rules: (n_rules int32[S], rules STANCE_RULE_DTYPE[S, 1]) of every scene, from the host mirror; zero where a
        scene has no rule."""
        return self._get_scene_table(self.L.mmw_get_stance_rules, _lib.STANCE_RULE_DTYPE, _lib.STANCE_RULES_MAX)

    def sample_stance_dev(self, flags_ptr=None, t_ptr=None):
        """mmw_stance_sample: every live track's stance class of the asked scenes from the keypoints its record holds now, changes,
        falls and long lies counted and logged, queued behind `estimate_posture` / `set_keypoints*` on the context's stream -- no
        host wait.  `flags_ptr`: device int32[S], non-zero = asked (None = every scene); `t_ptr`: device float64[S], the events' time
        (None = each scene's count of earlier sample calls)."""
        self._chk(self.L.mmw_stance_sample(self.h, flags_ptr, t_ptr))

    def sample_stance(self, t=None, scenes=None):
        """`sample_stance_dev` from host arrays: `t` float64[S] or a scalar for every scene (None = the call ordinals), `scenes` the
        scenes to sample (default all)."""
        self._sample(self.sample_stance_dev, "stance", t, scenes)

    def stance_async(self, rows_ptr, cap_rows: int, events_ptr, cap_events: int, scene_base: int = 0, ticket: int = 0):
        """mmw_stance_async: one `_lib.STANCE_ROW_DTYPE` row per scene with a rule and the `_lib.STANCE_EVENT_DTYPE` events logged
        since the previous successful export into device buffers, queued on the context's stream -- no host wait.  Tickets 0 .. 3
        (`stance_host` uses 3).  Both pointers 8-byte aligned."""
        self._chk(self.L.mmw_stance_async(self.h, rows_ptr, int(cap_rows), events_ptr, int(cap_events), int(scene_base), int(ticket)))

    def stance_wait(self, ticket: int = 0):
        """(n_rows, n_events) of the `stance_async` call with this ticket: waits for its counts only, not for the stream.  Buffers
        too small: MmwError with code E_CAPACITY and the counts needed in `.needed` -- nothing was written and nothing was taken, so
        the same export can be asked for again with room."""
        return self._export_wait(self.L.mmw_stance_wait, ticket)

    def stance_host(self, scene_base: int = 0):
        """The stance export as two structured arrays: (rows[n_rows] STANCE_ROW_DTYPE, events[n_events] STANCE_EVENT_DTYPE); fold the
        events with `stance.Watch`.  The buffers grow to what the device says it needs (a refused export loses nothing)."""
        self._export_caps.setdefault("stance", (64, 256))   # (its entry exists from the first call on, as the zones')
        return self._export_host("stance", lambda *a: self.stance_async(*a[:4], scene_base, a[4]), self.L.mmw_stance_wait,
                                 ("stance_rows", _lib.STANCE_ROW_DTYPE), ("stance_events", _lib.STANCE_EVENT_DTYPE))

    # -- dwell heat maps ------------------------------------------------------
    def enable_heat(self, cells: int):
        """mmw_heat_enable: per scene a grid table (no grid to begin with), `cells` (1 .. `_lib.HEAT_CELLS_MAX`) cells of dwell time,
        samples and visits, and per live uid its last cell and time; everything starts over, also when heat was enabled before.
        16 bytes a cell and scene: 4096 scenes x 1024 cells are 67 MB.  Until enabled, the heat calls are refused (E_ARG) --
        `get_heat_grids()` reports 0 grids -- and the context launches nothing of them."""
        if int(cells) == 0:
            raise ValueError("enable_heat: cells must be positive (disable_heat() frees the maps)")
        self._chk(self.L.mmw_heat_enable(self.h, int(cells)))

    def disable_heat(self):
        """mmw_heat_enable(0): waits for the stream and frees the maps; the context launches what one without heat does."""
        self._chk(self.L.mmw_heat_enable(self.h, 0))

    def set_heat_grids(self, grids, scenes=None):
        """mmw_set_heat_grids: give `scenes` (default: scenes 0 .. len(grids)-1) their grid -- `grids` is what `_lib.make_heat_grids`
        takes (a list per scene of zero or one dict or tuple) or its result, the pair (n_grids, HEAT_GRID_DTYPE[n, 1]).  Scenes never
        listed keep what they have; the listed scenes' cells and counters restart at 0 and no interval is credited across the call.
        Refused (MmwError, E_ARG) with nothing changed for an index out of range or listed twice, more entries than scenes, an x0, y0
        or cell that is not finite, cell <= 0, a max_gap that is NaN or <= 0, nx or ny < 1, more cells than were enabled, or a
        non-zero `reserved_`."""
        self._set_scene_table("set_heat_grids", "grids", self.L.mmw_set_heat_grids, _lib.make_heat_grids, _lib.HEAT_GRID_DTYPE,
                              _lib.HEAT_GRIDS_MAX, grids, scenes)

    def get_heat_grids(self):
        """mmw_get_heat_grids: (n_grids int32[S], grids HEAT_GRID_DTYPE[S, 1]) of every scene, from the host mirror; zero where a
        scene has no grid or heat is off."""
        return self._get_scene_table(self.L.mmw_get_heat_grids, _lib.HEAT_GRID_DTYPE, _lib.HEAT_GRIDS_MAX)

    def sample_heat_dev(self, flags_ptr=None, t_ptr=None):
        """mmw_heat_sample: every live track of the asked scenes with a grid adds a sample, maybe a visit, and the time since its
        previous sample to the cell it is in, queued behind the last step on the context's stream -- no host wait.  `flags_ptr`:
        device int32[S] (None = every scene), `t_ptr`: device float64[S] (None = the scenes' call ordinals)."""
        self._chk(self.L.mmw_heat_sample(self.h, flags_ptr, t_ptr))

    def sample_heat(self, t=None, scenes=None):
        """`sample_heat_dev` from host arrays: `t` float64[S] or a scalar for every scene (None = the call ordinals), `scenes` the
        scenes to sample (default all)."""
        self._sample(self.sample_heat_dev, "heat", t, scenes)

    def heat_dev(self, rows_ptr, cap_rows: int, cells_ptr, cap_cells: int, clear: bool = False, flags_ptr=None, scene_base: int = 0, ticket: int = 0):
        """mmw_heat_async: one `_lib.HEAT_ROW_DTYPE` row per scene with a grid (with `flags_ptr`, device int32[S]: of the flagged
        scenes) and one `_lib.HEAT_CELL_DTYPE` entry per cell of theirs with samples > 0, in (scene, cell) order, into device buffers;
        row i owns cells[first : first + count].  clear=True restarts what was exported at 0 -- when everything fitted.  Queued on
        the context's stream -- no host wait.  Tickets 0 .. 3 (`heat_host` uses 3).  Both buffers 8-byte aligned."""
        self._chk(self.L.mmw_heat_async(self.h, rows_ptr, int(cap_rows), cells_ptr, int(cap_cells), flags_ptr,
                                        _lib.HEAT_CLEAR if clear else _lib.HEAT_KEEP, int(scene_base), int(ticket)))

    def heat_wait(self, ticket: int = 0):
        """(n_rows, n_cells) of the `heat_dev` call with this ticket: waits for its counts only, not for the stream.  Buffers too
        small: MmwError with code E_CAPACITY and the counts needed in `.needed` -- nothing was written and nothing was cleared."""
        return self._export_wait(self.L.mmw_heat_wait, ticket)

    def heat_host(self, clear: bool = False, scenes=None, scene_base: int = 0):
        """The heat export as two structured arrays: (rows[n_rows] HEAT_ROW_DTYPE, cells[n_cells] HEAT_CELL_DTYPE); `heat.dense`
        makes an (ny, nx) map of a scene, `heat.Accumulator` folds clear=True windows.  The buffers grow to what the device says it
        needs (a refused export clears nothing)."""
        self._export_caps.setdefault("heat", (64, 4096))   # (its entry exists from the first call on, as the zones')
        flags_ptr = self._scene_flags(scenes, "heat_export_flags")
        return self._export_host("heat", lambda *a: self.heat_dev(*a[:4], clear, flags_ptr, scene_base, a[4]), self.L.mmw_heat_wait,
                                 ("heat_rows", _lib.HEAT_ROW_DTYPE), ("heat_cells", _lib.HEAT_CELL_DTYPE))

    # -- snapshot / restore ---------------------------------------------------
    def _scene_list(self, scenes):
        if scenes is None:
            return None, 0
        a = np.ascontiguousarray(np.asarray(scenes, dtype=np.int32).reshape(-1))
        return a, len(a)

    def snapshot_size(self, scenes=None) -> int:
        """mmw_snapshot_size: bytes of the snapshot of `scenes` (default: all, in order); nothing is written."""
        a, n = self._scene_list(scenes)
        out = C.c_size_t(0)
        self._chk(self.L.mmw_snapshot_size(self.h, a.ctypes.data if a is not None else None, n, C.byref(out)))
        return int(out.value)

    def _snapshot_into(self, scenes, out):
        """One mmw_snapshot call into `out` (a DevBuf or None): (nbytes, written).  Too small a buffer writes nothing and
        reports the size the blob needs."""
        a, n = self._scene_list(scenes)
        got = C.c_size_t(0)
        cap = out.nbytes if out is not None else 0
        rc = self.L.mmw_snapshot(self.h, a.ctypes.data if a is not None else None, n, out.ptr if out is not None else None, cap, C.byref(got))
        if rc == _lib.E_ARG and got.value > cap:
            return int(got.value), False
        self._chk(rc)
        return int(got.value), True

    def snapshot_dev(self, scenes=None, out: DevBuf = None):
        """mmw_snapshot into device memory: (DevBuf, nbytes) -- for device-to-device moves (`restore((buf, nbytes))` on
        another context of the same device).  Pass the DevBuf of an earlier call as `out` to reuse it: a buffer large enough
        costs one call (one drain, one size pass and its read-back, the pack); a missing or small one a sizing call first.
        Waits for everything queued on the context, the side stream included."""
        nbytes, done = self._snapshot_into(scenes, out)
        if not done:
            out = DevBuf(self, nbytes)
            nbytes, done = self._snapshot_into(scenes, out)
            assert done, nbytes
        return out, nbytes

    def snapshot(self, scenes=None) -> bytes:
        """The state of `scenes` (default: all, in order) as a versioned, layout-independent blob (include/mmw.h)."""
        nbytes, done = self._snapshot_into(scenes, self._bufs.get("snapshot"))
        if not done:
            nbytes, done = self._snapshot_into(scenes, self.buf("snapshot", nbytes))
            assert done, nbytes
        return self._bufs["snapshot"].download((nbytes,), np.uint8).tobytes()

    def restore(self, blob, scenes=None):
        """mmw_restore: blob scene i -> scene scenes[i] (default: scene i).  `blob`: bytes (host) or (DevBuf, nbytes) on the
        device (what `snapshot_dev` returns).  Refused (MmwError, E_ARG) with no scene changed when the blob or the
        configuration does not fit."""
        a, n = self._scene_list(scenes)
        tmp = None
        if isinstance(blob, tuple):
            buf, nbytes = blob
            if not isinstance(buf, DevBuf) or int(nbytes) > buf.nbytes:
                raise TypeError("restore((DevBuf, nbytes)): a device blob and its size")
            ptr = buf.ptr
        else:
            b = np.frombuffer(bytes(blob), dtype=np.uint8)
            tmp = DevBuf(self, max(len(b), 16)).upload(b)
            ptr, nbytes = tmp.ptr, len(b)
        try:
            self._chk(self.L.mmw_restore(self.h, ptr, int(nbytes), a.ctypes.data if a is not None else None, n))
        finally:
            if tmp is not None:
                tmp.free()

    # -- profiling ------------------------------------------------------------
    def stats(self) -> np.ndarray:
        out = np.zeros(8, dtype=np.uint64)
        self._chk(self.L.mmw_stats_get(self.h, out.ctypes.data))
        return out

    def stats_ext(self) -> np.ndarray:
        """[0..7] as `stats`; [30] k_features algorithmic bytes, [31] feature tensors written (include/mmw.h)."""
        out = np.zeros(32, dtype=np.uint64)
        self._chk(self.L.mmw_stats_get_ext(self.h, out.ctypes.data))
        return out

    def stats_reset(self):
        self._chk(self.L.mmw_stats_reset(self.h))

    def profile(self, on, kernels=None):
        """HIP-event timing of the kernels: all of them (on=True), none (on=False), or the ids in `kernels`."""
        mask = 0
        if kernels is not None:
            for k in kernels:
                mask |= 2 << int(k)
        elif on:
            mask = 1
        self._chk(self.L.mmw_profile_enable(self.h, mask))

    def profile_reset(self):
        self._chk(self.L.mmw_profile_reset(self.h))

    def profile_get(self, kid: int):
        ms, cnt = C.c_double(0), C.c_int64(0)
        self._chk(self.L.mmw_profile_get(self.h, kid, C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value
