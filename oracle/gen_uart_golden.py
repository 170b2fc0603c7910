#!/usr/bin/env python3
"""Records the reference's UART reader, ReadIWR14xx.read (src/ReadDataIWR1443.py:27-201), under the numpy it pins (1.26) into
tests/golden/uart_decode.npz -- TEST INFRASTRUCTURE, run by hand with a numpy-1.26 interpreter (this image:
/opt/conda/bin/python3.9 oracle/gen_uart_golden.py [out.npz]).  Under numpy >= 2 that read() raises OverflowError in its decode
branch (`dopplerIdx[...] - 65535`), so oracle/gen_golden.py's `uart` recording holds no decoded packet; under 1.26 it decodes.

The reference module is imported at run time with the pyserial stand-in (oracle/serial_shim), __init__ (which opens ports) is
bypassed and a fake Dataport delivers the chunks, as gen_golden.py's gen_uart does.  Every read() of every stream is recorded:
the chunk fed, dataOK, frameNumber, byteBufferLength, byteBuffer[:byteBufferLength] after the call, whether it raised
ValueError, and for a decoded packet numObj, the TLV body as the reference read it (u16 numObj, u16 xyzQFormat, 12 bytes per
object -- stale bytes of its 2^15-byte buffer included), x, y, z, doppler, peakVal, range (fp64) and rangeIdx, dopplerIdx.

Data only: the arrays are concatenations, `*_off` are offsets into them (one per read, one past the end).

`--buffer [out.npz]` writes the second recording instead, tests/golden/uart_buffer.npz: the same read() at the full size of its
2^15-byte buffer (see `buffer_streams` below).  The first recording does not change by it.
"""
import json
import os
import struct
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden", "uart_decode.npz")
MAGIC = bytes([2, 1, 4, 3, 6, 5, 8, 7])
CAP = 2 ** 15
SEEDS = {"random_full_range": 101, "doppler_edges": 102, "q_format": 103, "random_mix": 104, "splits": 105}
CFG_A = {"rangeIdxToMeters": 0.0436, "dopplerResolutionMps": 0.1252, "numDopplerBins": 16.0}


def packet(frame, objs, q=9, tlv_type=1, num_det=None, num_obj=None, total=None):
    """One TI mmWave demo UART packet: header (36 B) + one TLV whose body is u16 numObj, u16 Q, then objs as six u16 words
    (rangeIdx, dopplerIdx, peakVal, x, y, z; any int, taken mod 2^16).  num_det / num_obj / total override what the header
    and the body announce."""
    o = (np.asarray(objs, dtype=np.int64).reshape(-1, 6) & 0xFFFF).astype("<u2")
    body = struct.pack("<HH", len(o) if num_obj is None else num_obj, q) + o.tobytes()
    tlv = struct.pack("<II", tlv_type, len(body)) + body
    tot = 36 + len(tlv) if total is None else total
    return MAGIC + struct.pack("<IIIIIII", 0x01020304, tot, 0xA1443, frame, 123456, len(o) if num_det is None else num_det, 1) + tlv


def objs_random(rng, n, full=True):
    if full:
        return rng.integers(0, 65536, size=(n, 6))
    o = np.zeros((n, 6), np.int64)
    o[:, 0] = rng.integers(0, 256, n)
    o[:, 1] = rng.integers(-40, 41, n)
    o[:, 2] = rng.integers(0, 4000, n)
    o[:, 3:6] = rng.integers(-3000, 3000, size=(n, 3))
    return o


def stream_random_full_range():
    """Valid packets, all six u16 fields over their full range (int16 wrap in every field), random Q 0..20, one per read."""
    rng = np.random.default_rng(SEEDS["random_full_range"])
    return CFG_A, [packet(1000 + i, objs_random(rng, int(rng.integers(0, 13))), q=int(rng.integers(0, 21))) for i in range(40)]


def stream_doppler_edges(nbins, seed_off):
    """Doppler indices numDopplerBins/2 - 2 .. numDopplerBins/2 + 1 (and the int16 extremes) for one configParameters."""
    rng = np.random.default_rng(SEEDS["doppler_edges"] + seed_off)
    cfg = {"rangeIdxToMeters": 0.0436, "dopplerResolutionMps": 0.1252, "numDopplerBins": nbins}
    h = nbins / 2
    dops = list(range(int(np.floor(h)) - 3, int(np.ceil(h)) + 3)) + [-32768, -32767, -2, -1, 0, 1, 32766, 32767]
    chunks = []
    for i in range(0, len(dops), 4):
        d = dops[i: i + 4]
        o = objs_random(rng, len(d), full=False)
        o[:, 1] = d
        chunks.append(packet(2000 + i, o))
    return cfg, chunks


def stream_q_format():
    """xyzQFormat 0 .. 70 and a few up to 65535, coordinates 0, +-1, the int16 extremes and random ones."""
    rng = np.random.default_rng(SEEDS["q_format"])
    qs = list(range(71)) + [100, 127, 128, 255, 256, 1000, 4096, 32767, 32768, 65534, 65535]
    chunks = []
    for i, q in enumerate(qs):
        o = objs_random(rng, 5, full=False)
        o[0, 3:6] = (0, 1, -1)
        o[1, 3:6] = (32767, -32768, 0)
        o[2, 3:6] = (-1, 0, 1)
        o[3, 3:6] = (0, 0, 0)
        chunks.append(packet(3000 + i, o, q=q))
    return CFG_A, chunks


def stream_header_edges():
    """numObj = 0 with objects announced; no objects announced; a first TLV that is not detected points; totalPacketLen
    0, 20, 35, 36, 44, 47, 48 with the bytes present (each fed alone, then a few non-magic bytes: the drop rule both ways)."""
    rng = np.random.default_rng(7)
    o = lambda n: objs_random(rng, n, full=False)
    ch = [packet(10, o(0), num_det=3), b"\x00" * 5, packet(11, o(2), num_det=0), b"\x00" * 3,
          packet(12, o(3), tlv_type=2), b"\x11" * 4, packet(13, o(3), tlv_type=6), packet(14, o(3), tlv_type=0), b"\x00" * 2]
    for k, tot in enumerate((0, 20, 35, 36, 44, 47, 48)):
        ch += [packet(20 + k, o(2), total=tot), b"\x05" * 7]
    ch += [packet(30, o(4), total=48, num_det=0) + b"\x09" * 9, packet(31, o(4), total=44, tlv_type=3) + b"\x09" * 9]
    return CFG_A, ch


def stream_objects_past_packet():
    """totalPacketLen shorter than the objects the body announces, the objects still within the received bytes (the
    reference decodes them from whatever follows, then drops only totalPacketLen bytes)."""
    rng = np.random.default_rng(8)
    ch = []
    for k, (n, short) in enumerate(((4, 1), (6, 3), (3, 3), (5, 5))):
        p = packet(40 + k, objs_random(rng, n, full=False))
        p = p[:12] + struct.pack("<I", len(p) - 12 * short) + p[16:]
        ch += [p + bytes(rng.integers(0, 256, 12, dtype=np.uint8)).replace(b"\x02", b"\x03"), b"\x00" * 4]
    return CFG_A, ch


def stream_stale_bytes():
    """Objects (and header words) past the received bytes: the reference reads them from the stale content of its 2^15-byte
    buffer -- what earlier, longer packets left there --, and raises ValueError for objects past the buffer's end."""
    rng = np.random.default_rng(9)
    big = objs_random(rng, 60, full=True)
    big[40:] = 0x0707
    ch = [packet(50, big) + b"\x00" * 8]                          # decoded, dropped: leaves 776 stale bytes behind
    ch += [packet(51, objs_random(rng, 3, full=False), num_obj=45)]      # 3 objects sent, 45 announced
    ch += [packet(52, objs_random(rng, 2, full=False), num_obj=6) + b"\x00" * 4]
    ch += [packet(53, objs_random(rng, 2, full=False), num_obj=6, total=60)]   # announced objects past the packet AND the bytes
    p = packet(54, objs_random(rng, 1, full=False))[:20]           # 20 bytes sent, the header says 17: frame number,
    ch += [p[:12] + struct.pack("<I", 17) + p[16:], b"\x00"]       # numDetectedObj, the TLV come from stale bytes
    ch += [packet(55, objs_random(rng, 2, full=False), num_obj=2730) + b"\x00" * 2]   # objects past 2^15: ValueError
    ch += [b"\x00" * 3, packet(56, objs_random(rng, 2, full=False)) + b"\x00" * 2]
    return CFG_A, ch


def stream_over_max_obj():
    """1100 objects (the reference decodes them; the product's UartFrameParser(max_obj=1024) refuses them: MmwError)."""
    rng = np.random.default_rng(10)
    o = objs_random(rng, 1100, full=False)
    o[8:] = 0
    return CFG_A, [packet(60, objs_random(rng, 2, full=False)), packet(61, o) + b"\x00" * 2, packet(62, objs_random(rng, 2, full=False))]


def stream_splits():
    """A short packet split at every byte: the head, then the rest, frame by frame."""
    rng = np.random.default_rng(SEEDS["splits"])
    ch = []
    for k in range(1, 72):
        p = packet(100 + k, objs_random(rng, 2, full=True))
        assert len(p) == 72
        ch += [p[:k], p[k:]]
    return CFG_A, ch


def stream_multi_and_garbage():
    """Several packets per chunk (the LAST magic word wins), garbage before and between, a partial magic word, and a chunk
    dropped by the maxBufferSize rule while a long packet is pending."""
    rng = np.random.default_rng(12)
    o = lambda n: objs_random(rng, n, full=False)
    p = [packet(200 + i, o(i % 5)) for i in range(8)]
    ch = [b"\x00\x11\x02\x01garbage" + p[0], p[1] + b"\x02\x01\x04" + p[2], p[3][:30], p[3][30:] + b"junk" + p[4] + b"\x07" * 3,
          b"\x02\x01\x04", p[5][:20], p[5][20:] + p[6][:10], p[6][10:], p[7] + b"\x02\x01\x04\x03\x06\x05\x08"]
    pend = packet(210, o(2), total=30000)                          # announces 30000 bytes
    ch += [pend, bytes(20000), bytes(13000), bytes(2000)]          # the 13000-byte chunk does not fit: dropped
    ch += [packet(211, o(3)) + b"\x00" * 2, packet(212, o(1))]
    return CFG_A, ch


def stream_random_mix():
    """A seeded mix of all of the above, cut into random chunks."""
    rng = np.random.default_rng(SEEDS["random_mix"])
    data = b""
    for i in range(160):
        kind = int(rng.integers(0, 12))
        n = int(rng.integers(0, 9))
        ob = objs_random(rng, n, full=bool(rng.integers(0, 2)))
        q = int(rng.choice([0, 7, 8, 9, 9, 15, 62, 63, 64, 65535]))
        if kind == 0:
            pk = packet(500 + i, ob, q=q, num_det=0)
        elif kind == 1:
            pk = packet(500 + i, ob, q=q, tlv_type=int(rng.integers(2, 8)))
        elif kind == 2:
            pk = packet(500 + i, ob, q=q, total=int(rng.choice([0, 20, 36, 44, 48])))
        elif kind == 3:
            pk = packet(500 + i, ob, q=q, num_obj=n + int(rng.integers(1, 6)))
        elif kind == 4:
            pk = packet(500 + i, ob, q=q, num_obj=0, num_det=int(rng.integers(1, 4)))
        else:
            pk = packet(500 + i, ob, q=q)
        if rng.integers(0, 4) == 0:
            pk = bytes(rng.integers(0, 256, int(rng.integers(1, 12)), dtype=np.uint8)) + pk
        data += pk
    cuts = np.sort(rng.choice(np.arange(1, len(data)), size=len(data) // 60, replace=False))
    return CFG_A, [data[a:b] for a, b in zip([0] + list(cuts), list(cuts) + [len(data)])]


def streams():
    out = [("random_full_range",) + stream_random_full_range()]
    for k, nb in enumerate((16.0, 32.0, 64.0, 64 / 3, 1.0, 2.0, 3.0, 12.5)):
        out.append((f"doppler_edges_{k}",) + stream_doppler_edges(nb, k))
    out += [("q_format",) + stream_q_format(), ("header_edges",) + stream_header_edges(),
            ("objects_past_packet",) + stream_objects_past_packet(), ("stale_bytes",) + stream_stale_bytes(),
            ("over_max_obj",) + stream_over_max_obj(), ("splits",) + stream_splits(),
            ("multi_and_garbage",) + stream_multi_and_garbage(), ("random_mix",) + stream_random_mix()]
    return out


class _Port:
    def __init__(self):
        self.q = b""

    @property
    def in_waiting(self):
        return len(self.q)

    def read(self, n):
        d, self.q = self.q[:n], self.q[n:]
        return d

    def write(self, *_):
        pass

    def close(self):
        pass


def _reader(mod, cfgp):
    rd = object.__new__(mod.ReadIWR14xx)
    rd.MMWDEMO_UART_MSG_DETECTED_POINTS = 1
    rd.maxBufferSize = CAP
    rd.magicWord = [2, 1, 4, 3, 6, 5, 8, 7]
    rd.byteBuffer = np.zeros(CAP, dtype="uint8")
    rd.byteBufferLength = 0
    rd.configParameters = dict(cfgp)
    rd.Dataport = _Port()
    rd.CLIport = _Port()
    return rd


def _packet_view(buf, length, chunk):
    """The reader's buffer as its decode sees it: `chunk` appended if it fits, then cut to the last magic word in
    buf[0 .. length-8) (what read() does before it reads the header) -- used to take the TLV body the reference read."""
    b = buf.copy()
    if length + len(chunk) < CAP:
        b[length: length + len(chunk)] = np.frombuffer(chunk, dtype=np.uint8)
        length += len(chunk)
    for s in np.nonzero(b[: max(length - 8, 0)] == MAGIC[0])[0][::-1]:
        if bytes(b[s: s + 8]) == MAGIC:
            b[: length - s] = b[s: length].copy()
            break
    return b


def record(mod, name, cfgp, chunks, acc):
    rd = _reader(mod, cfgp)
    for ch in chunks:
        view = _packet_view(rd.byteBuffer, int(rd.byteBufferLength), ch)
        rd.Dataport.q = ch
        raised = 0
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")   # the overflow of `2 ** Q` and x / 0 warn; the values are the recording
            try:
                ok, fn, det = rd.read()
            except ValueError:
                ok, fn, det, raised = 0, 0, {}, 1
        acc["chunk"].append(np.frombuffer(ch, dtype=np.uint8))
        acc["ok"].append(int(ok))
        acc["frame"].append(int(fn))
        acc["raised"].append(raised)
        L = int(rd.byteBufferLength)
        acc["buflen"].append(L)
        acc["buf"].append(rd.byteBuffer[:L].copy())
        if ok:
            n = int(det["numObj"])
            body = view[44: 48 + 12 * n].copy()
            w = body.view("<u2")
            assert int(w[0]) == n and np.array_equal(w[2:].view("<i2")[0::6], det["rangeIdx"]), name   # the body it read
            assert np.array_equal(w[2:].view("<i2")[2::6], det["peakVal"]), name
            acc["num_obj"].append(n)
            acc["body"].append(body)
            acc["det"].append(np.stack([np.asarray(det[k], dtype=np.float64).reshape(n) for k in ("x", "y", "z", "doppler", "peakVal", "range")], axis=1))
            acc["idx"].append(np.stack([np.asarray(det["rangeIdx"]), np.asarray(det["dopplerIdx"])], axis=1).astype(np.int16).reshape(n, 2))
        else:
            acc["num_obj"].append(-1)
            acc["body"].append(np.zeros(0, np.uint8))
            acc["det"].append(np.zeros((0, 6)))
            acc["idx"].append(np.zeros((0, 2), np.int16))


def _offsets(parts):
    return np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)


def generate(path):
    from oracle.ref_import import REFERENCE_SRC
    sys.dont_write_bytecode = True
    for p in (os.path.join(HERE, "serial_shim"), REFERENCE_SRC):
        if p not in sys.path:
            sys.path.insert(0, p)
    import importlib
    mod = importlib.import_module("ReadDataIWR1443")
    acc = {k: [] for k in ("chunk", "ok", "frame", "raised", "buflen", "buf", "num_obj", "body", "det", "idx")}
    names, cfgs, s_reads = [], [], [0]
    for name, cfgp, chunks in streams():
        record(mod, name, cfgp, chunks, acc)
        names.append(name)
        cfgs.append([cfgp["rangeIdxToMeters"], cfgp["dopplerResolutionMps"], cfgp["numDopplerBins"]])
        s_reads.append(len(acc["ok"]))
    meta = {"numpy": np.__version__, "python": sys.version.split()[0], "seeds": SEEDS,
            "reference": "src/ReadDataIWR1443.py ReadIWR14xx.read (the reference pins numpy 1.26.3)"}
    out = {
        "meta": np.array(json.dumps(meta, sort_keys=True)), "names": np.array(names), "cfg": np.array(cfgs, np.float64),
        "stream_reads": np.array(s_reads, np.int64),
        "chunk": np.concatenate(acc["chunk"]), "chunk_off": _offsets(acc["chunk"]),
        "ok": np.array(acc["ok"], np.int8), "frame": np.array(acc["frame"], np.int64), "raised": np.array(acc["raised"], np.int8),
        "buflen": np.array(acc["buflen"], np.int64), "buf": np.concatenate(acc["buf"]), "buf_off": _offsets(acc["buf"]),
        "num_obj": np.array(acc["num_obj"], np.int64), "body": np.concatenate(acc["body"]), "body_off": _offsets(acc["body"]),
        "det": np.concatenate(acc["det"]), "idx": np.concatenate(acc["idx"]), "det_off": _offsets(acc["det"]),
    }
    np.savez_compressed(path, **out)
    return out


# ---- the second recording: the buffer mechanics at full size (tests/golden/uart_buffer.npz; `--buffer [out.npz]`) ----------
# Packets of up to 1024 objects, several per buffer, split across chunks, with totalPacketLen on either side of the bytes
# received, and the 2^15-byte rule at its edge.  Every byte that is not a header is FILLER: position-distinguishing (a move by a
# wrong shift, pass or mask lands on other values), never 2 (no filler forms a magic word), with a period of 247 = 13 * 19 that
# is coprime to the 16-byte pieces and the 4096-byte passes of the device's byte mover, and compressible.  Per read the file
# keeps the chunk, dataOK, frameNumber, raised, byteBufferLength, the SHA-256 of all 2^15 buffer bytes after the call and, when
# it decoded, numObj and the detObj columns.
OUT_BUFFER = os.path.join(ROOT, "tests", "golden", "uart_buffer.npz")
CFG_B = {"rangeIdxToMeters": 0.0872, "dopplerResolutionMps": 0.0626, "numDopplerBins": 32.0}
SEED_BUFFER = 2015


def filler(n, phase):
    return (9 + (131 * (np.arange(n, dtype=np.int64) + phase)) % 247).astype(np.uint8).tobytes()


def big_packet(frame, n, phase, q=15, num_obj=None, total=None, pad=True):
    """A packet whose n objects are filler bytes (Q 15: x, y, z within +-1 m, so that about half the rows pass normalize_data); padded with filler to a multiple of 32 bytes as the sensor sends it
    (totalPacketLen counts the padding) unless `total` says otherwise or pad is off."""
    p = packet(frame, np.frombuffer(filler(12 * n, phase), "<u2").reshape(-1, 6), q=q, num_obj=num_obj, total=total)
    if total is None and pad:
        tot = (len(p) + 31) // 32 * 32
        p = p[:12] + struct.pack("<I", tot) + p[16:] + filler(tot - len(p), phase + 7)
    return p


def bstream_several_per_buffer():
    """Several packets in one chunk behind a little garbage: the LAST magic word wins, at a position past 4096, 8192, 16384
    with more than 4096 bytes behind it -- the cut moves them by 1, 2, 3 and 0 modulo 4."""
    P = big_packet
    return CFG_A, [filler(37, 1) + P(1, 1024, 11) + P(2, 600, 12) + P(3, 342, 13),
                   filler(2, 2) + P(4, 600, 14, q=7) + P(5, 1024, 15, q=7),
                   filler(3, 3) + P(6, 341, 16) + P(7, 337, 17) + P(8, 1024, 18, q=12),
                   P(9, 338, 19) + P(10, 600, 20),
                   filler(4099, 4) + P(11, 341, 21, q=0) + filler(5, 5),
                   P(12, 337, 22) + filler(3, 6), P(13, 338, 23), filler(1, 7) + P(14, 342, 24) + filler(11, 8)]


def bstream_split_across_chunks():
    """Packets that arrive in pieces behind garbage: appends of 1 to 4097 bytes and more onto every length, the head of the next
    packet behind a decoded one (the drop moves it to the front)."""
    a, b, c = big_packet(21, 1024, 31), big_packet(22, 600, 32, q=10), big_packet(23, 341, 33)
    d = big_packet(24, 342, 34, q=8)
    return CFG_B, [filler(1001, 9) + a[:1], a[1:4096], a[4096:8193], a[8193:] + b[:8], b[8:5000], b[5000:] + filler(13, 10),
                   filler(4097, 11), c[:3], c[3:19], c[19:4115], c[4115:] + d[:7], d[7:8], d[8:4104], d[4104:], filler(9, 12)]


def bstream_total_packet_len():
    """totalPacketLen shorter than the bytes received (decoded, and only that many bytes dropped: moves to the front of more than
    4096 bytes by 1, 3, 2 and 0 modulo 4, and by a large odd length) and longer (pending until the bytes are there)."""
    P = big_packet
    return CFG_A, [P(31, 1024, 41, total=4097) + filler(6000, 13), P(32, 600, 42, total=7251) + filler(5000, 14),
                   P(33, 342, 43, total=4098) + filler(4500, 15), P(34, 600, 44, total=20000), filler(9000, 16), filler(3760, 17),
                   P(35, 1024, 45, total=12001, q=11) + filler(9000, 18), P(36, 341, 46) + filler(2, 19),
                   P(37, 600, 47, total=2000) + filler(100, 41)]


def bstream_fill_to_the_rule():
    """byteBufferLength + byteCount = 32 767 (kept) and 32 768 (dropped), with chunks of 1, 2, 12 000 and 12 001 bytes and with a
    pending packet that announces 32 767 bytes: the fill-up that completes it is dropped at one byte more, kept at the byte, and the
    whole buffer is then dropped by that odd totalPacketLen."""
    return CFG_A, [big_packet(41, 600, 51, total=32767), filler(13519, 20), filler(12001, 21), filler(12000, 22),
                   filler(20000, 23), filler(12766, 24), filler(2, 25), filler(1, 26), filler(1, 27), b"", filler(12000, 28)]


def bstream_fill_from_empty():
    """An empty buffer and one chunk of 32 768 bytes (dropped), then of 32 767 (kept; nothing can follow it)."""
    return CFG_B, [filler(CAP, 29), filler(CAP - 1, 30), filler(1, 31)]


def bstream_announced_bounds():
    """A buffer full of stale filler, then 3 objects sent with 2726 announced (the last object ends at byte 32 760: decoded from
    the stale bytes) and with 2727 (it ends at 32 772: ValueError), then an honest packet."""
    P = big_packet
    return CFG_A, [filler(32000, 32), P(51, 3, 61, num_obj=2726, pad=False) + filler(9, 33), P(52, 3, 62, num_obj=2727, pad=False) + filler(9, 34),
                   P(53, 2, 63) + filler(4, 35)]


def bstream_stale_after_long():
    """A 1024-object packet decoded and dropped leaves its bytes behind; then 3 objects sent and 900, 300 and 257 announced."""
    P = big_packet
    return CFG_B, [P(61, 1024, 71) + filler(8, 36), P(62, 3, 72, num_obj=900, pad=False) + filler(5, 37),
                   P(63, 3, 73, num_obj=300, q=6, pad=False) + filler(5, 38), P(64, 3, 74, num_obj=257, pad=False) + filler(5, 39),
                   P(65, 2, 75) + filler(3, 40)]


def bstream_random_big():
    """A seeded run of 1024-, 600-, 342-, 341-, 338- and 337-object packets with garbage between, cut into random chunks."""
    rng = np.random.default_rng(SEED_BUFFER)
    data = b""
    for i, n in enumerate((1024, 341, 600, 342, 1024, 337, 600, 338, 1024, 600)):
        data += filler(int(rng.integers(0, 40)), 100 + i) + big_packet(80 + i, n, 80 + i, q=int(rng.integers(0, 16)))
    cuts, at = [0], 0
    while at < len(data):
        at = min(at + int(rng.choice([1, 3, 17, 500, 4095, 4097, 6000, 9000])), len(data))
        cuts.append(at)
    return CFG_A, [data[a:b] for a, b in zip(cuts, cuts[1:])]


def buffer_streams():
    return [("several_per_buffer",) + bstream_several_per_buffer(), ("split_across_chunks",) + bstream_split_across_chunks(),
            ("total_packet_len",) + bstream_total_packet_len(), ("fill_to_the_rule",) + bstream_fill_to_the_rule(),
            ("fill_from_empty",) + bstream_fill_from_empty(), ("announced_bounds",) + bstream_announced_bounds(),
            ("stale_after_long",) + bstream_stale_after_long(), ("random_big",) + bstream_random_big()]


def generate_buffer(path):
    import hashlib
    import importlib
    from oracle.ref_import import REFERENCE_SRC
    sys.dont_write_bytecode = True
    for p in (os.path.join(HERE, "serial_shim"), REFERENCE_SRC):
        if p not in sys.path:
            sys.path.insert(0, p)
    mod = importlib.import_module("ReadDataIWR1443")
    acc = {k: [] for k in ("chunk", "ok", "frame", "raised", "buflen", "digest", "num_obj", "det")}
    names, cfgs, s_reads = [], [], [0]
    for name, cfgp, chunks in buffer_streams():
        rd = _reader(mod, cfgp)
        for ch in chunks:
            rd.Dataport.q = ch
            raised = 0
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                try:
                    ok, fn, det = rd.read()
                except ValueError:
                    ok, fn, det, raised = 0, 0, {}, 1
            acc["chunk"].append(np.frombuffer(ch, dtype=np.uint8))
            acc["ok"].append(int(ok))
            acc["frame"].append(int(fn))
            acc["raised"].append(raised)
            acc["buflen"].append(int(rd.byteBufferLength))
            assert rd.byteBuffer.shape == (CAP,) and rd.byteBuffer.dtype == np.uint8
            acc["digest"].append(np.frombuffer(hashlib.sha256(rd.byteBuffer.tobytes()).digest(), dtype=np.uint8))
            n = int(det["numObj"]) if ok else -1
            acc["num_obj"].append(n)
            acc["det"].append(np.stack([np.asarray(det[k], dtype=np.float64).reshape(n) for k in ("x", "y", "z", "doppler", "peakVal", "range")], axis=1)
                              if ok else np.zeros((0, 6)))
        names.append(name)
        cfgs.append([cfgp["rangeIdxToMeters"], cfgp["dopplerResolutionMps"], cfgp["numDopplerBins"]])
        s_reads.append(len(acc["ok"]))
    meta = {"numpy": np.__version__, "python": sys.version.split()[0], "seed": SEED_BUFFER, "filler": "9 + (131 * (i + phase)) % 247",
            "reference": "src/ReadDataIWR1443.py ReadIWR14xx.read (the reference pins numpy 1.26.3)"}
    out = {
        "meta": np.array(json.dumps(meta, sort_keys=True)), "names": np.array(names), "cfg": np.array(cfgs, np.float64),
        "stream_reads": np.array(s_reads, np.int64),
        "chunk": np.concatenate(acc["chunk"]), "chunk_off": _offsets(acc["chunk"]),
        "ok": np.array(acc["ok"], np.int8), "frame": np.array(acc["frame"], np.int64), "raised": np.array(acc["raised"], np.int8),
        "buflen": np.array(acc["buflen"], np.int64), "digest": np.stack(acc["digest"]),
        "num_obj": np.array(acc["num_obj"], np.int64), "det": np.concatenate(acc["det"]), "det_off": _offsets(acc["det"]),
    }
    np.savez_compressed(path, **out)
    return out


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if len(sys.argv) > 1 and sys.argv[1] == "--buffer":
        path = sys.argv[2] if len(sys.argv) > 2 else OUT_BUFFER
        o = generate_buffer(path)
        print(f"{path}: {len(o['names'])} streams, {len(o['ok'])} reads, {int(o['ok'].sum())} decoded, {int(o['raised'].sum())} raised, "
              f"{len(o['det'])} objects, largest {int(o['num_obj'].max())}, numpy {np.__version__}, {os.path.getsize(path)} bytes")
        sys.exit(0)
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    o = generate(path)
    print(f"{path}: {len(o['names'])} streams, {len(o['ok'])} reads, {int(o['ok'].sum())} decoded, {int(o['raised'].sum())} raised, "
          f"{len(o['det'])} objects, numpy {np.__version__}, {os.path.getsize(path)} bytes")
