"""Online input step: the IWR1443 UART stream into `normalize_data`'s input (reference src/ReadDataIWR1443.py).

`parse_config_file` restates `ReadIWR14xx.__parseConfigFile` (ReadDataIWR1443.py:203-262: radar .cfg ->
range / doppler scales); `UartFrameParser` is `ReadIWR14xx.read` (27-201) without the serial port: the caller
feeds whatever bytes arrived, the parser keeps the reference's byte buffer discipline (append if it fits, cut to
the LAST magic word, parse one packet, drop it) and returns the same `(dataOK, frameNumber, detObj)` triple.
The packet itself is decoded by the C-ABI's host function `mmw_parse_uart_cap` (include/mmw.h).  Opening and
configuring the serial ports (pyserial, `__serialConfig`) stays with the application.

Parity: pinned by a recording of the reference's own read() under numpy 1.26 (tests/golden/uart_decode.npz,
oracle/gen_uart_golden.py) -- short and odd totalPacketLen values, objects read from the stale bytes of the 2^15-byte
buffer, the int64 wrap of `2 ** xyzQFormat` included.  One declared difference: more than `max_obj` objects raise
`_lib.MmwError` (MMW_E_ARG) where the reference decodes them.

Many radars in one context: `SceneBatch.open_radars / read_radars` keep this same buffer discipline per scene on the device
(mmw_uart_read, csrc/k_uart.hip) -- there a packet over `max_pts` objects is dropped as the reference drops a decoded one.

Recording: `ExperimentLogger` is DataLogging.py's `write_thread` (50-89) per scene, fed by `SceneBatch.radar_log_host` -- the
frames the device readers decoded, so the log is what the tracker saw.
"""
from __future__ import annotations

import ctypes as C
import os
import time

import numpy as np

from . import _lib

MAX_BUFFER = 2 ** 15          # ReadDataIWR1443.py:24
NUM_TX_ANT = 3                # hard-coded there (214-215)


def parse_config_file(path: str) -> dict:
    """numDopplerBins, numRangeBins, rangeResolutionMeters, rangeIdxToMeters, dopplerResolutionMps, maxRange,
    maxVelocity (+ framePeriodicity) from the `profileCfg` and `frameCfg` lines of a radar .cfg."""
    start_freq = idle = ramp_end = slope = n_adc = rate = None
    chirp0 = chirp1 = loops = period = None
    with open(path) as fh:
        for line in fh:
            w = line.rstrip("\r\n").split(" ")
            if "profileCfg" in w[0]:
                start_freq, idle, ramp_end = int(float(w[2])), int(w[3]), float(w[5])
                slope, n_adc, rate = float(w[8]), int(w[10]), int(w[11])
            elif "frameCfg" in w[0]:
                chirp0, chirp1, loops, period = int(w[1]), int(w[2]), int(w[3]), float(w[5])
    pow2 = 1
    while n_adc > pow2:
        pow2 *= 2
    p = {}
    chirps = (chirp1 - chirp0 + 1) * loops
    p["numDopplerBins"] = chirps / NUM_TX_ANT
    p["numRangeBins"] = pow2
    p["rangeResolutionMeters"] = (3e8 * rate * 1e3) / (2 * slope * 1e12 * n_adc)
    p["rangeIdxToMeters"] = (3e8 * rate * 1e3) / (2 * slope * 1e12 * p["numRangeBins"])
    p["dopplerResolutionMps"] = 3e8 / (2 * start_freq * 1e9 * (idle + ramp_end) * 1e-6 * p["numDopplerBins"] * NUM_TX_ANT)
    p["maxRange"] = (300 * 0.9 * rate) / (2 * slope * 1e3)
    p["maxVelocity"] = 3e8 / (4 * start_freq * 1e9 * (idle + ramp_end) * 1e-6 * NUM_TX_ANT)
    p["framePeriodicity"] = period
    return p


_UartCfg = _lib.MmwUartCfg


def uart_cfg(config_parameters: dict) -> "_lib.MmwUartCfg":
    """struct mmw_uart_cfg from the reference's configParameters dict (rangeIdxToMeters, dopplerResolutionMps, numDopplerBins)."""
    return _lib.MmwUartCfg(float(config_parameters["rangeIdxToMeters"]), float(config_parameters["dopplerResolutionMps"]),
                           int(config_parameters["numDopplerBins"]), 0)


def find_tlv(buf) -> tuple:
    """mmw_find_tlv on a bytes-like object: (found, body_offset, n_obj, frame_number, packet_start, packet_len) -- the packet
    part of ReadIWR14xx.read (ReadDataIWR1443.py:47-113) without decoding an object: what the host does per packet when the
    GPU decodes the detected-points TLV itself (SceneBatch.normalize_tlv_dev).  found only for a body that lies, with every
    object it announces, inside `buf`: a packet the reference would complete from stale bytes of its buffer is refused."""
    a = np.frombuffer(buf, dtype=np.uint8)
    off, n = C.c_int64(-1), C.c_int32(0)
    frame = C.c_uint32(0)
    start, plen = C.c_size_t(0), C.c_size_t(0)
    rc = _lib.load().mmw_find_tlv(a.ctypes.data, len(a), C.byref(off), C.byref(n), C.byref(frame), C.byref(start), C.byref(plen))
    if rc < 0:
        raise _lib.MmwError(rc, "mmw_find_tlv: bad arguments")
    return rc == 1, int(off.value), int(n.value), int(frame.value), int(start.value), int(plen.value)


def encode_tlv_bodies(raw: np.ndarray, counts: np.ndarray, qfmt: int, doppler_resolution_mps: float, stride: int = 0) -> np.ndarray:
    """A synthetic sensor: the detected-points TLV BODIES an IWR1443 would have sent for raw rows (x, y, z, doppler, peakVal) --
    u16 numObj, u16 xyzQFormat, then per object int16 rangeIdx (0), dopplerIdx = round(doppler / resolution), peakVal, and
    x, y, z = round(coordinate * 2^Q) (ReadDataIWR1443.py:107-150) -- one body per scene at a fixed stride (default: the smallest
    multiple of 16 that holds max_pts objects).  raw[..., N, 5], counts[...] -> uint8 [..., stride].  Used by the tests and by
    bench_ingest.py's `tlv` leg; decoding them (mmw_parse_uart / mmw_normalize_tlv) gives the QUANTISED rows, not `raw`."""
    raw = np.asarray(raw)
    lead, N = raw.shape[:-2], raw.shape[-2]
    if stride <= 0:
        stride = (4 + 12 * N + 15) // 16 * 16
    assert stride >= 4 + 12 * N and stride % 2 == 0
    out = np.zeros(lead + (stride,), dtype=np.uint8)
    words = out.view(np.uint16).reshape(lead + (stride // 2,))
    cnt = np.clip(np.asarray(counts), 0, N).astype(np.uint16)
    words[..., 0] = cnt
    words[..., 1] = qfmt
    obj = np.zeros(lead + (N, 6), dtype=np.int16)
    obj[..., 1] = np.clip(np.rint(raw[..., 3].astype(np.float64) / doppler_resolution_mps), -32768, 32767).astype(np.int16)
    obj[..., 2] = np.clip(np.rint(raw[..., 4].astype(np.float64)), -32768, 32767).astype(np.int16)
    obj[..., 3:6] = np.clip(np.rint(raw[..., 0:3].astype(np.float64) * float(2 ** qfmt)), -32768, 32767).astype(np.int16)
    valid = np.arange(N).reshape((1,) * len(lead) + (N,)) < cnt[..., None]
    obj[~valid] = 0
    words[..., 2: 2 + 6 * N] = obj.view(np.uint16).reshape(lead + (6 * N,))
    return out


def xyz_q_divisor(qfmt) -> np.ndarray:
    """What the reference divides x, y, z by: `2 ** xyzQFormat` with the u16 Q format as a numpy int64 (ReadDataIWR1443.py:118),
    which wraps -- 2^q for q <= 62, -2^63 for q = 63, 0 for q >= 64 (x / 0 = +-inf, 0 / 0 = NaN).  fp64, the shape of qfmt."""
    q = np.asarray(qfmt, dtype=np.int64)
    pow2 = np.left_shift(np.int64(1), np.minimum(q, 62)).astype(np.float64)
    return np.where(q <= 62, pow2, np.where(q == 63, -(2.0 ** 63), 0.0))


def decode_tlv_bodies_numpy(bodies: np.ndarray, cfg: dict):
    """The reference's decode (ReadDataIWR1443.py:153-171 under its numpy 1.26: int16 wrap, the int64 `2 ** Q` of
    `xyz_q_divisor`) of `encode_tlv_bodies`-shaped bodies, in numpy: (raw[..., N, 5] float64, counts[...]).  The checker's
    restatement -- the product decodes on the device; tests/test_uart_decode.py pins it to the reference's recorded read()."""
    lead, stride = bodies.shape[:-1], bodies.shape[-1]
    words = np.ascontiguousarray(bodies).view(np.uint16).reshape(lead + (stride // 2,))
    cnt = words[..., 0].astype(np.int32)
    q = xyz_q_divisor(words[..., 1])
    N = (stride - 4) // 12
    obj = words[..., 2: 2 + 6 * N].reshape(lead + (N, 6)).view(np.int16)
    dop = obj[..., 1].copy()
    hi = dop > (cfg["numDopplerBins"] / 2 - 1)
    dop[hi] = (dop[hi].astype(np.int32) - 65535).astype(np.int16)
    raw = np.zeros(lead + (N, 5))
    with np.errstate(divide="ignore", invalid="ignore"):
        raw[..., 0:3] = obj[..., 3:6] / q[..., None, None]
    raw[..., 3] = dop * cfg["dopplerResolutionMps"]
    raw[..., 4] = obj[..., 2]
    return raw, cnt


class UartFrameParser:
    def __init__(self, config_parameters: dict, max_obj: int = 1024):
        self.configParameters = dict(config_parameters)
        self.byteBuffer = np.zeros(MAX_BUFFER, dtype=np.uint8)
        self.byteBufferLength = 0
        self.max_obj = int(max_obj)
        self._cfg = _UartCfg(float(config_parameters["rangeIdxToMeters"]), float(config_parameters["dopplerResolutionMps"]),
                             int(config_parameters["numDopplerBins"]), 0)
        self._raw = np.zeros((self.max_obj, 5))
        self._rng = np.zeros(self.max_obj)
        self._n, self._frame = C.c_int32(0), C.c_uint32(0)
        self._start, self._plen = C.c_size_t(0), C.c_size_t(0)

    def feed(self, data: bytes):
        """One call of `read()` with `data` as what the port delivered: (dataOK, frameNumber, detObj).  Raises ValueError where
        the reference does (a packet that announces objects past the end of the 2^15-byte buffer) and _lib.MmwError (MMW_E_ARG)
        for more than max_obj objects, which the reference decodes."""
        vec = np.frombuffer(data, dtype=np.uint8)
        if self.byteBufferLength + len(vec) < MAX_BUFFER:       # (a chunk that does not fit is dropped, as there)
            self.byteBuffer[self.byteBufferLength: self.byteBufferLength + len(vec)] = vec
            self.byteBufferLength += len(vec)
        if self.byteBufferLength <= 16:
            return 0, 0, {}
        rc, start = self._parse()
        if start > 0:                                           # cut to the last magic word, then decode there: words past
            rest = self.byteBufferLength - start                # byteBufferLength are the stale bytes of the CUT buffer
            self.byteBuffer[:rest] = self.byteBuffer[start: self.byteBufferLength].copy()
            self.byteBufferLength = rest
            rc, _ = self._parse()
        if rc == _lib.E_CAPACITY:
            raise ValueError("mmw_parse_uart_cap: the packet's words reach past the end of the 2^15-byte buffer")
        if rc < 0:
            raise _lib.MmwError(rc, "mmw_parse_uart_cap: more objects than max_obj or bad arguments")
        if rc == _lib.UART_NONE:                                # no magic word, or the packet is not complete yet
            return 0, 0, {}
        det, ok, idx = {}, 0, 36
        if rc == _lib.UART_POINTS:
            k = self._n.value
            r = self._raw[:k]
            det = {"numObj": k, "range": self._rng[:k].copy(), "doppler": r[:, 3].copy(), "peakVal": r[:, 4].astype(np.int16),
                   "x": r[:, 0].copy(), "y": r[:, 1].copy(), "z": r[:, 2].copy(), "timestamp": round(time.time() * 1000)}
            ok, idx = 1, 48 + 12 * k
        elif self._num_detected() > 0:
            idx = 44                                            # TLV type and length were read: another TLV first
        if self.byteBufferLength > idx:                         # "remove already processed data" (188-195), totalPacketLen
            total = self._plen.value                            # bytes, whatever it is (0 drops nothing)
            rest = self.byteBufferLength - total
            self.byteBuffer[:rest] = self.byteBuffer[total: self.byteBufferLength].copy()
            self.byteBufferLength = rest
        return ok, int(self._frame.value), det

    def _parse(self):
        rc = _lib.load().mmw_parse_uart_cap(self.byteBuffer.ctypes.data, self.byteBufferLength, MAX_BUFFER, C.byref(self._cfg),
                                            self._raw.ctypes.data, self._rng.ctypes.data, self.max_obj, C.byref(self._n),
                                            C.byref(self._frame), C.byref(self._start), C.byref(self._plen))
        return rc, int(self._start.value)

    def _num_detected(self) -> int:
        b = self.byteBuffer
        return int(b[28]) | int(b[29]) << 8 | int(b[30]) << 16 | int(b[31]) << 24


class ExperimentLogger:
    """DataLogging.py's `write_thread` (50-89) for many scenes: `paths` maps a scene id (as `radar_log_host` reports it, scene_base
    included) to the directory of its experiment, which must exist; frames of other scenes are ignored.  Per scene a pandas buffer
    of `Frame, X, Y, Z, Doppler, Intensity, Timestamp` rows is appended to `<dir>/<k>.csv` (k = 1, 2, ...; no header, no index)
    whenever it holds FB_WRITE_BUFFER_SIZE rows or the shard has FB_EXPERIMENT_FILE_SIZE frames, which starts the next shard --
    the files `utils.OfflineManager`, `dataset.preprocess_experiment` and `train` start from.  A frame with zero objects adds no
    row but counts as a frame, as there.  Declared difference: `close()` writes what is still buffered; the reference loses its
    unflushed rows at KeyboardInterrupt."""

    COLUMNS = ("Frame", "X", "Y", "Z", "Doppler", "Intensity", "Timestamp")

    def __init__(self, paths: dict):
        import pandas as pd
        self._pd = pd
        self.paths = {int(s): str(p) for s, p in paths.items()}
        # per scene: [data_buffer, cur_file_index, frames_in_cur_file]
        self._state = {s: [pd.DataFrame(), 1, 0] for s in self.paths}
        self.frames_written = {s: 0 for s in self.paths}

    def _flush(self, scene: int):
        st = self._state[scene]
        st[0].to_csv(os.path.join(self.paths[scene], f"{st[1]}.csv"), mode="a", index=False, header=False)
        st[0].drop(st[0].index, inplace=True)

    def write(self, dir, rows):
        """One export of `SceneBatch.radar_log_host`: every directory entry of a scene in `paths` is one `queue.get()` of the
        reference's writer."""
        from . import constants as const
        pd = self._pd
        for e in dir:
            scene = int(e["scene"])
            st = self._state.get(scene)
            if st is None:
                continue
            r = rows[int(e["first"]): int(e["first"]) + int(e["count"])]
            data = {"Frame": int(e["frame_number"]), "X": r["x"], "Y": r["y"], "Z": r["z"], "Doppler": r["doppler"],
                    "Intensity": r["peak_val"].astype(np.int16), "Timestamp": round(float(e["t"]) * 1000)}
            st[0] = pd.concat([st[0], pd.DataFrame(data)], ignore_index=True)
            st[2] += 1
            self.frames_written[scene] += 1
            if len(st[0]) >= const.FB_WRITE_BUFFER_SIZE or st[2] >= const.FB_EXPERIMENT_FILE_SIZE:
                self._flush(scene)
                if st[2] >= const.FB_EXPERIMENT_FILE_SIZE:
                    st[2] = 0
                    st[1] += 1

    def close(self):
        for scene, st in self._state.items():
            if len(st[0]):
                self._flush(scene)
