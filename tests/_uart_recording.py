"""Reader for tests/golden/uart_decode.npz: the reference's ReadIWR14xx.read (src/ReadDataIWR1443.py:27-201) recorded under
the numpy it pins (1.26) by oracle/gen_uart_golden.py -- every read() of every stream with its chunk, dataOK, frameNumber,
byteBufferLength, the buffer after it, whether it raised ValueError and, when it decoded, the TLV body it read and its detObj."""
import json
import os
from dataclasses import dataclass

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "uart_decode.npz")
DET_KEYS = ("x", "y", "z", "doppler", "peakVal", "range")


@dataclass
class Read:
    index: int            # within its stream
    chunk: bytes
    ok: int
    frame: int
    raised: bool
    buflen: int
    buf: bytes            # byteBuffer[:byteBufferLength] after the call
    num_obj: int          # -1 unless ok
    body: bytes           # the TLV body the reference read (u16 numObj, u16 Q, 12 bytes per object), b"" unless ok
    det: np.ndarray       # [num_obj, 6] fp64: x, y, z, doppler, peakVal, range
    idx: np.ndarray       # [num_obj, 2] int16: rangeIdx, dopplerIdx


@dataclass
class Stream:
    name: str
    cfg: dict             # configParameters (numDopplerBins as the reference had it: a float)
    reads: list


def load(path=GOLD):
    g = np.load(path)
    sl = lambda key, off, i: g[key][g[off][i]: g[off][i + 1]]
    out = []
    sr = g["stream_reads"]
    for s, name in enumerate(g["names"]):
        c = g["cfg"][s]
        cfg = {"rangeIdxToMeters": float(c[0]), "dopplerResolutionMps": float(c[1]), "numDopplerBins": float(c[2])}
        reads = []
        for k, r in enumerate(range(int(sr[s]), int(sr[s + 1]))):
            reads.append(Read(k, sl("chunk", "chunk_off", r).tobytes(), int(g["ok"][r]), int(g["frame"][r]), bool(g["raised"][r]),
                              int(g["buflen"][r]), sl("buf", "buf_off", r).tobytes(), int(g["num_obj"][r]), sl("body", "body_off", r).tobytes(),
                              sl("det", "det_off", r), sl("idx", "det_off", r)))
        out.append(Stream(str(name), cfg, reads))
    return out


GOLD_BUFFER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "uart_buffer.npz")


@dataclass
class BufferRead:
    """A read of tests/golden/uart_buffer.npz (oracle/gen_uart_golden.py --buffer): the same reference under the same numpy, with
    packets of up to 1024 objects and buffers filled to the 2^15-byte rule; of the buffer it keeps the SHA-256 of all 2^15 bytes."""
    index: int
    chunk: bytes
    ok: int
    frame: int
    raised: bool
    buflen: int
    digest: bytes         # hashlib.sha256(byteBuffer.tobytes()).digest() after the call
    num_obj: int          # -1 unless ok
    det: np.ndarray       # [num_obj, 6] fp64: x, y, z, doppler, peakVal, range


def load_buffer(path=GOLD_BUFFER):
    g = np.load(path)
    sl = lambda key, off, i: g[key][g[off][i]: g[off][i + 1]]
    out = []
    sr = g["stream_reads"]
    for s, name in enumerate(g["names"]):
        c = g["cfg"][s]
        cfg = {"rangeIdxToMeters": float(c[0]), "dopplerResolutionMps": float(c[1]), "numDopplerBins": float(c[2])}
        reads = [BufferRead(k, sl("chunk", "chunk_off", r).tobytes(), int(g["ok"][r]), int(g["frame"][r]), bool(g["raised"][r]),
                            int(g["buflen"][r]), g["digest"][r].tobytes(), int(g["num_obj"][r]), sl("det", "det_off", r))
                 for k, r in enumerate(range(int(sr[s]), int(sr[s + 1])))]
        out.append(Stream(str(name), cfg, reads))
    return out


def meta(path=GOLD):
    return json.loads(str(np.load(path)["meta"]))


def same_bits(a, b) -> bool:
    """fp64 arrays equal bit for bit (signed zeros and the sign of inf included), NaN matching NaN whatever its payload."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (a.view(np.int64) == b.view(np.int64))))
