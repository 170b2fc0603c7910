"""A plain numpy restatement of the reference's ReadIWR14xx.read (src/ReadDataIWR1443.py:27-201) with main.py:44-47 on top, for
the checks of the device-resident radar readers (csrc/k_uart.hip): no ctypes and no library.  It keeps byteBuffer[2^15],
byteBufferLength and main.py's `t`; read(chunk, now) answers in the kernel's terms.  The objects are decoded by the already
pinned radar.decode_tlv_bodies_numpy from the buffer's own bytes, the stale ones past byteBufferLength included.  Pinned to the
reference's recorded read() in tests/test_uart_buffer.py."""
import numpy as np

from mmwave_msc_amd import radar

CAP = 2 ** 15                                   # maxBufferSize
MAGIC = np.array([2, 1, 4, 3, 6, 5, 8, 7], np.uint8)
NONE, POINTS, PACKET, OVERFLOW, RAISED = 0, 1, 2, 3, 4   # MMW_UART_*: the low byte of mmw_uart_read's status
CHUNK_DROPPED = 256                             # MMW_UART_CHUNK_DROPPED
BAD_FRAME = -3                                  # MMW_BAD_FRAME: n of an OVERFLOW read
MAX_OBJ = (CAP - 48) // 12                      # 2726: one object more reaches past the buffer, and the reference raises


class UartReadRef:
    def __init__(self, config_parameters: dict, max_pts: int = MAX_OBJ, t0: float = 0.0):
        self.cfg = dict(config_parameters)
        self.max_pts = int(max_pts)
        self.byteBuffer = np.zeros(CAP, dtype=np.uint8)
        self.byteBufferLength = 0
        self.t_last = float(t0)
        self.range = np.zeros(0)                # rangeIdx * rangeIdxToMeters of the last POINTS read (the log's sixth column)
        self.moves = []                         # ("cut" | "drop", first byte moved, bytes moved) of every move to the front so far

    def set_state(self, buf, length: int, t_last: float):
        self.byteBuffer = np.array(buf, dtype=np.uint8).reshape(CAP).copy()
        self.byteBufferLength, self.t_last = int(length), float(t_last)

    def _u32(self, at: int) -> int:
        return int(self.byteBuffer[at: at + 4].astype(np.int64) @ np.array([1, 2 ** 8, 2 ** 16, 2 ** 24], np.int64))

    def read(self, chunk, now: float):
        """(status, frame_number, n, raw[n, 5], dt) of one read() that finds `chunk` waiting at the port at time `now`: raw holds
        x, y, z, doppler, peakVal.  RAISED is the reference's ValueError (frame_number 0, as a caller who caught it has none);
        OVERFLOW a packet it decodes with more than max_pts objects (n = BAD_FRAME, no rows); dt moves on POINTS only."""
        B = self.byteBuffer
        vec = np.frombuffer(chunk, dtype=np.uint8)
        dropped = 0
        if self.byteBufferLength + len(vec) < CAP:                                   # 42-46
            B[self.byteBufferLength: self.byteBufferLength + len(vec)] = vec
            self.byteBufferLength += len(vec)
        else:
            dropped = CHUNK_DROPPED
        magic_ok, total = False, 0
        if self.byteBufferLength > 16:                                               # 49-80
            start = None
            for loc in np.where(B[0: self.byteBufferLength - 8] == MAGIC[0])[0][::-1]:
                if np.all(B[loc: loc + 8] == MAGIC):
                    start = int(loc)
                    break
            if start is not None:
                B[: self.byteBufferLength - start] = B[start: self.byteBufferLength].copy()
                self.moves.append(("cut", start, self.byteBufferLength - start))
                self.byteBufferLength -= start
                if self.byteBufferLength > 16:
                    total = self._u32(12)
                    magic_ok = self.byteBufferLength >= total
        none = np.zeros((0, 5))
        if not magic_ok:
            return NONE | dropped, 0, 0, none, 0.0
        status, frame, idx, n, raw, dt = PACKET, self._u32(20), 36, 0, none, 0.0     # 85-150
        if self._u32(28) > 0:
            idx = 44
            if self._u32(36) == 1:
                num = int(B[44]) | int(B[45]) << 8
                if 48 + 12 * num > CAP:      # the matmul of an empty slice at the buffer's end raises; nothing is dropped
                    return RAISED | dropped, 0, 0, none, 0.0
                idx = 48 + 12 * num
                body = np.zeros((1, 4 + 12 * max(num, 1)), np.uint8)
                body[0, : 4 + 12 * num] = B[44: idx]
                dec, cnt = radar.decode_tlv_bodies_numpy(body, self.cfg)
                assert int(cnt[0]) == num
                if num > self.max_pts:
                    status, n = OVERFLOW, BAD_FRAME
                else:
                    status, n, raw = POINTS, num, dec[0, :num].copy()
                    self.range = B[48: idx].view("<i2")[0::6] * self.cfg["rangeIdxToMeters"]
                    dt = now - self.t_last                                           # main.py:44-47
                    self.t_last = now
        if self.byteBufferLength > idx:                                              # 188-195
            B[: self.byteBufferLength - total] = B[total: self.byteBufferLength].copy()
            self.moves.append(("drop", total, self.byteBufferLength - total))
            self.byteBufferLength -= total
        return status | dropped, frame, n, raw, dt
