"""The device-resident radar readers (mmw_uart_open / mmw_uart_read, csrc/k_uart.hip): ReadIWR14xx.read (reference
src/ReadDataIWR1443.py:27-201) + Utils.normalize_data for every scene of a context in one kernel, against the reference's own
recorded read() (tests/golden/uart_decode.npz), against radar.UartFrameParser, and through the tracker."""
import struct

import numpy as np
import pytest

from tests._layouts import make_checked
from tests._uart_recording import load as load_recording, same_bits

pytestmark = pytest.mark.gpu
MAGIC = bytes([2, 1, 4, 3, 6, 5, 8, 7])
CFGP = {"rangeIdxToMeters": 0.0436, "dopplerResolutionMps": 0.1252, "numDopplerBins": 32.0}


def _wrap(frame, body, n_obj, pad_to=32):
    """A UART packet around a detected-points TLV body (u16 numObj, u16 Q, objects): magic word, the eight header words, the TLV
    head, and padding to a multiple of `pad_to` bytes as the sensor sends it (totalPacketLen counts the padding)."""
    tlv = struct.pack("<II", 1, len(body)) + body
    total = (36 + len(tlv) + pad_to - 1) // pad_to * pad_to
    pkt = MAGIC + struct.pack("<IIIIIII", 0x01020304, total, 0xA1443, frame, 1, n_obj, 1) + tlv
    return pkt + b"\x00" * (total - len(pkt))


def _objects_packet(rng, frame, n, q=9):
    o = np.zeros((n, 6), dtype="<i2")
    o[:, 0] = rng.integers(0, 256, n)
    o[:, 1] = rng.integers(-40, 41, n)
    o[:, 2] = rng.integers(0, 4000, n)
    o[:, 3] = rng.integers(-1500, 1500, n)
    o[:, 4] = rng.integers(20, 3600, n)
    o[:, 5] = rng.integers(-900, 300, n)
    return _wrap(frame, struct.pack("<HH", n, q) + o.tobytes(), n)


def _download(sb, r):
    S, N = sb.S, sb.max_pts
    return (r.status.download((S,), np.int32), r.frame_number.download((S,), np.uint32), r.n.download((S,), np.int32),
            r.dt.download((S,), np.float64), r.pts.download((S, N, 8), np.float64))


def _raw_rows(det_rows, N):
    """[N, 5] raw rows (x, y, z, doppler, peakVal) and their count from a [k, >= 5] array of decoded objects."""
    raw = np.zeros((N, 5))
    raw[: len(det_rows)] = det_rows[:, :5]
    return raw, len(det_rows)


@pytest.mark.parametrize("max_pts", [64, 600])
def test_recording_read_by_read(max_pts):
    """The 17 recorded streams as 17 scenes of ONE context, each with its own configParameters, one mmw_uart_read per recorded
    read() (a stream that has ended is unflagged).  After every call, per scene: RAISED exactly where the reference raised,
    dataOK, frameNumber, byteBufferLength and the buffer's bytes as recorded; when dataOK, n and the rows bit-equal to
    mmw_normalize of the recorded detObj.  The one read that announces 1100 objects (over_max_obj) is the only one that may
    answer OVERFLOW (n = MMW_BAD_FRAME) -- and its buffer is the reference's all the same.  max_pts 64 / 600: one and four rows
    per thread."""
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    streams = load_recording()
    S = len(streams)
    assert S == 17
    sb = SceneBatch(_lib.default_config(), S, max_pts)
    sb.open_radars([s.cfg for s in streams], t0=0.0)
    calls = max(len(s.reads) for s in streams)
    assert calls <= 258
    seen = {"raised": 0, "ok": 0, "overflow": [], "dropped": 0, "max_buf": 0}
    prev_len = [0] * S
    for k in range(calls):
        live = [s for s in range(S) if k < len(streams[s].reads)]
        chunks = [streams[s].reads[k].chunk if s in live else b"" for s in range(S)]
        r = sb.read_radars(chunks, now=1.0 + k, scenes=live)
        status, frame, n, dt, pts = _download(sb, r)
        raw = np.zeros((S, max_pts, 5))
        n_raw = np.zeros(S, np.int32)
        for s in live:
            rd = streams[s].reads[k]
            if rd.ok and rd.num_obj <= max_pts:
                raw[s], n_raw[s] = _raw_rows(rd.det, max_pts)
        want_pts, want_n = sb.normalize_host(raw, n_raw)
        for s in range(S):
            where = (streams[s].name, k)
            low = int(status[s]) & 255
            if s not in live:
                assert low == _lib.UART_SKIPPED and n[s] == 0 and dt[s] == 0.0, where
                continue
            rd = streams[s].reads[k]
            assert (low == _lib.UART_RAISED) == rd.raised, (where, low)
            fits = prev_len[s] + len(rd.chunk) < _lib.UART_BUFFER
            assert bool(status[s] & _lib.UART_CHUNK_DROPPED) == (not fits), where
            seen["dropped"] += int(not fits)
            if rd.ok and rd.num_obj > max_pts:
                assert low == _lib.UART_OVERFLOW and n[s] == _lib.BAD_FRAME and dt[s] == 0.0, (where, low, n[s])
                seen["overflow"].append((streams[s].name, rd.num_obj))
            else:
                assert (low == _lib.UART_POINTS) == bool(rd.ok), (where, low, rd.ok)
                assert n[s] == want_n[s], (where, n[s], want_n[s])
                assert same_bits(pts[s, : n[s]], want_pts[s, : want_n[s]]), where
            assert int(frame[s]) == rd.frame, (where, int(frame[s]), rd.frame)
            buf, blen, _ = sb.radar_state(s)
            assert blen == rd.buflen, (where, blen, rd.buflen)
            assert buf[:blen].tobytes() == rd.buf, where
            prev_len[s] = rd.buflen
            seen["raised"] += int(rd.raised)
            seen["ok"] += int(rd.ok)
            seen["max_buf"] = max(seen["max_buf"], blen)
    assert seen["raised"] >= 2 and seen["ok"] > 200 and seen["dropped"] >= 1 and seen["max_buf"] >= 22072, seen
    # only over_max_obj's 1100 objects exceed either max_pts (the largest packet beside it has 60)
    assert seen["overflow"] == [("over_max_obj", 1100)], seen
    sb.close()


def test_every_shift():
    """g = 0 .. 31 garbage bytes in front of a 3-object packet, then the next packet split at byte 7: the cut moves the buffer by
    every byte shift, the appends land on every alignment.  Buffer (all 2^15 bytes), length, status and points equal
    radar.UartFrameParser.feed on the same chunks."""
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    from mmwave_msc_amd.radar import UartFrameParser
    rng = np.random.default_rng(5)
    S, N = 32, 64
    p1, p2 = _objects_packet(rng, 11, 3), _objects_packet(rng, 12, 5)
    sb = SceneBatch(_lib.default_config(), S, N)
    sb.open_radars(CFGP, t0=10.0)
    parsers = [UartFrameParser(CFGP) for _ in range(S)]
    garbage = [bytes(rng.integers(9, 256, g, dtype=np.uint8)) for g in range(S)]
    oks = 0
    for k in range(3):
        chunks = [(garbage[g] + p1, p2[:7], p2[7:])[k] for g in range(S)]
        r = sb.read_radars(chunks, now=11.0 + k)
        status, frame, n, dt, pts = _download(sb, r)
        raw = np.zeros((S, N, 5))
        n_raw = np.zeros(S, np.int32)
        want = []
        for g in range(S):
            ok, fn, det = parsers[g].feed(chunks[g])
            want.append((ok, fn))
            if ok:
                raw[g], n_raw[g] = _raw_rows(np.stack([det[c] for c in ("x", "y", "z", "doppler", "peakVal")], axis=1).astype(np.float64), N)
        want_pts, want_n = sb.normalize_host(raw, n_raw)
        for g in range(S):
            ok, fn = want[g]
            assert int(status[g]) == (_lib.UART_POINTS if ok else _lib.UART_NONE), (g, k, status[g])
            assert int(frame[g]) == fn and n[g] == want_n[g] and same_bits(pts[g, : n[g]], want_pts[g, : want_n[g]]), (g, k)
            buf, blen, _ = sb.radar_state(g)
            assert blen == parsers[g].byteBufferLength and np.array_equal(buf, parsers[g].byteBuffer), (g, k, blen, parsers[g].byteBufferLength)
            oks += ok
    assert oks == 2 * S
    sb.close()


def test_reads_through_the_tracker():
    """Five scenes, ten reads: packets from radar.encode_tlv_bodies, chunked at random byte positions (empty chunks and two
    packets in one chunk among them).  Host path: UartFrameParser.feed -> normalize -> step with dt as main.py:44-47 forms it;
    device path: read_radars -> step_dev, nothing read back in between.  Status, frame number, dt, n and the rows equal at every
    read, tracks() bit-equal at the end."""
    from mmwave_msc_amd import _lib, radar
    from mmwave_msc_amd.radar import UartFrameParser
    from mmwave_msc_amd.synth import make_batch
    S, N, F = 5, 64, 10
    sb_dev = make_checked(S, N, "per_scene", db_min_samples=10)
    sb_host = make_checked(S, N, "per_scene", db_min_samples=10)
    assert sb_dev.step_kind() in (2, 4) and sb_dev.kalman_layout() == 0
    rng = np.random.default_rng(21)
    pts, cnt, _ = make_batch(range(60, 60 + S), F, N, 2)
    raw = np.zeros((F, S, N, 5))
    raw[..., 0:2] = pts[..., 0:2]
    raw[..., 2] = pts[..., 2] - sb_dev.cfg.s_height
    raw[..., 3:5] = pts[..., 6:8]
    bodies = radar.encode_tlv_bodies(raw, cnt, 9, CFGP["dopplerResolutionMps"])
    streams = []
    for s in range(S):
        pk = [_wrap(100 + f, bodies[f, s, : 4 + 12 * int(cnt[f, s])].tobytes(), int(cnt[f, s])) for f in range(F)]
        ends = np.cumsum([len(p) for p in pk])
        # read() decodes a packet only while at most 8 bytes of the next one have arrived (a whole magic word further on, the
        # cut to the LAST magic word throws the packet away): most chunks end there, two per scene anywhere around the boundary
        jitter = rng.integers(0, 9, F - 1)
        wild = rng.choice(F - 1, 2, replace=False)
        jitter[wild] = rng.integers(-40, 40, 2)
        cuts = np.clip(ends[:-1] + jitter, 0, ends[-1])
        if s == 0:
            cuts[2] = cuts[3] = ends[2] + 5      # read 3 delivers nothing ...
            cuts[4] = ends[5] + 9                # ... and read 4 two whole packets (the first of them is cut away, as there)
        cuts = np.concatenate([[0], np.sort(cuts), [ends[-1]]])
        blob = b"".join(pk)
        streams.append([blob[cuts[k]: cuts[k + 1]] for k in range(F)])
    assert streams[0][3] == b"" and streams[0][4].count(MAGIC) >= 2
    t0 = 1000.0
    sb_dev.open_radars(CFGP, t0=t0)
    parsers = [UartFrameParser(CFGP) for _ in range(S)]
    t_last = np.full(S, t0)
    frames = 0
    for k in range(F):
        now = t0 + 0.1 * (k + 1) + 0.003 * float(rng.random())
        chunks = [streams[s][k] for s in range(S)]
        r = sb_dev.read_radars(chunks, now)
        sb_dev.step_dev(r.pts, r.n, r.dt)
        status, frame, n, dt, got = _download(sb_dev, r)
        rows = np.zeros((S, N, 5))
        n_raw = np.zeros(S, np.int32)
        want_dt = np.zeros(S)
        for s in range(S):
            ok, fn, det = parsers[s].feed(chunks[s])
            if ok:
                want_dt[s] = now - t_last[s]
                t_last[s] = now
                rows[s], n_raw[s] = _raw_rows(np.stack([det[c] for c in ("x", "y", "z", "doppler", "peakVal")], axis=1).astype(np.float64), N)
            assert int(status[s]) == (_lib.UART_POINTS if ok else _lib.UART_NONE) and int(frame[s]) == fn, (k, s, status[s], frame[s], ok, fn)
            frames += ok
        want_pts, want_n = sb_host.normalize_host(rows, n_raw)
        sb_host.step_host(want_pts, want_n, want_dt)
        assert np.array_equal(dt.view(np.int64), want_dt.view(np.int64)), (k, dt, want_dt)
        assert np.array_equal(n, want_n), (k, n, want_n)
        for s in range(S):
            assert same_bits(got[s, : n[s]], want_pts[s, : want_n[s]]), (k, s)
    assert frames >= 4 * S, frames
    sb_dev.check(); sb_host.check()
    nt_d, nt_h = sb_dev.num_tracks(), sb_host.num_tracks()
    assert np.array_equal(nt_d, nt_h) and nt_d.sum() > 0, (nt_d, nt_h)
    td, th = sb_dev.tracks(cap=max(int(nt_d.max()), 1)), sb_host.tracks(cap=max(int(nt_h.max()), 1))
    for name in ("x", "P", "centroid", "spread_est", "group_disp_est", "lifetime", "point_num", "ring_n"):
        assert same_bits(td[name], th[name]), name
    sb_dev.close(); sb_host.close()


def test_sites_mount_each_scene():
    """Two scenes with different mounting (mmw_set_sites): read_radars is bit-equal to normalize_tlv_dev on the same bodies
    under the same sites, and the two scenes' rows differ from each other."""
    from mmwave_msc_amd import _lib, radar
    from mmwave_msc_amd.batch import SceneBatch
    rng = np.random.default_rng(8)
    S, N = 2, 64
    sb = SceneBatch(_lib.default_config(), S, N)
    sb.set_sites(_lib.make_sites(sb.cfg, S, s_height=[1.1, 2.0], s_tilt=[-12.0, 4.0]))
    sb.open_radars(CFGP, t0=0.0)
    pkt = _objects_packet(rng, 4, 40)
    r = sb.read_radars([pkt, pkt], now=0.5)
    status, frame, n, dt, pts = _download(sb, r)
    assert list(status) == [_lib.UART_POINTS] * 2 and list(frame) == [4, 4] and list(dt) == [0.5, 0.5]
    blob = np.frombuffer(pkt + pkt, dtype=np.uint8)
    b_pk = sb.buf("tlv_bytes", len(blob) + 16).upload(blob)
    b_of = sb.buf("tlv_off", S * 8).upload(np.array([44, len(pkt) + 44], np.int64))
    b_out, b_no = sb.buf("tlv_pts", S * N * 64), sb.buf("tlv_n", S * 4)
    sb.normalize_tlv_dev(b_pk.ptr, len(blob), b_of.ptr, radar.uart_cfg(CFGP), b_out.ptr, b_no.ptr)
    want_n, want = b_no.download((S,), np.int32), b_out.download((S, N, 8), np.float64)
    assert np.array_equal(n, want_n) and n.min() > 0, (n, want_n)
    for s in range(S):
        assert same_bits(pts[s, : n[s]], want[s, : n[s]]), s
    assert not np.array_equal(pts[0, : min(n)], pts[1, : min(n)])
    sb.close()


def test_refusals_and_state():
    """Chunk offsets of -1, decreasing, chunks_bytes + 1 and INT64_MAX give BADCHUNK for the scene they belong to, whose state
    stays as it was, while the other scenes read; set_state -> get_state carries all 2^15 bytes; mmw_reset_scenes leaves buffer
    and t_last alone; dt_out and t_last move on POINTS only; a read before mmw_uart_open, or with a NULL argument, is MMW_E_ARG."""
    import ctypes as C
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    rng = np.random.default_rng(13)
    S, N = 4, 64
    sb = SceneBatch(_lib.default_config(), S, N)
    out = [sb.buf(k, b) for k, b in (("p", S * N * 64), ("n", S * 4), ("dt", S * 8), ("st", S * 4), ("fr", S * 4))]
    pkt = _objects_packet(rng, 9, 6)
    blob = np.frombuffer(pkt * S, dtype=np.uint8)
    b_ch = sb.buf("ch", len(blob) + 16).upload(blob)
    L = len(pkt)
    good = np.arange(S + 1, dtype=np.int64) * L
    b_of = sb.buf("of", (S + 1) * 8).upload(good)
    with pytest.raises(_lib.MmwError) as ei:   # before open
        sb.read_radars_dev(b_ch.ptr, b_of.ptr, len(blob), 1.0, *[b.ptr for b in out])
    assert ei.value.code == _lib.E_ARG
    sb.open_radars(CFGP, t0=100.0)
    args = [sb.h, b_ch.ptr, b_of.ptr, len(blob), None, 1.0] + [b.ptr for b in out]
    for k in (1, 2, 6, 7, 8, 9, 10):            # a NULL argument (any but the flags)
        assert sb.L.mmw_uart_read(*[None if i == k else a for i, a in enumerate(args)]) == _lib.E_ARG, k

    def read(offs, now, nbytes=len(blob)):
        b_of.upload(np.asarray(offs, np.int64))
        sb.read_radars_dev(b_ch.ptr, b_of.ptr, nbytes, now, *[b.ptr for b in out])
        return (out[3].download((S,), np.int32), out[1].download((S,), np.int32), out[2].download((S,), np.float64))

    # a state with a recognisable tail: all 2^15 bytes travel both ways
    pattern = rng.integers(0, 256, _lib.UART_BUFFER, dtype=np.uint8)
    pattern[:64] = 0                            # (no magic word in front)
    for s in range(S):
        sb.set_radar_state(s, pattern, 5, 100.0 + s)
        buf, blen, t = sb.radar_state(s)
        assert np.array_equal(buf, pattern) and (blen, t) == (5, 100.0 + s), s
    i64 = np.iinfo(np.int64).max
    cases = [([-1, L, 2 * L, 3 * L, 4 * L], [0]),                      # negative start
             ([0, L, L - 1, 3 * L, 4 * L], [1]),                       # decreasing (scene 2's range, a byte and two packets, is valid)
             ([0, L, 2 * L, 3 * L, len(blob) + 1], [3]),               # past chunks_bytes
             ([0, L, 2 * L, 3 * L, i64], [3]),
             ([0, i64, 2 * L, 3 * L, 4 * L], [0, 1])]                  # scene 0 ends there, scene 1 starts there and decreases
    for offs, bad in cases:
        for s in range(S):
            sb.set_radar_state(s, pattern, 5, 100.0 + s)
        st, n, dt = read(offs, 200.0)
        for s in range(S):
            buf, blen, t = sb.radar_state(s)
            if s in bad:
                assert st[s] == _lib.UART_BADCHUNK and n[s] == 0 and dt[s] == 0.0, (offs, s, st)
                assert np.array_equal(buf, pattern) and (blen, t) == (5, 100.0 + s), (offs, s)
            else:
                # five stale bytes, then the packet: cut, decoded, dropped
                assert st[s] == _lib.UART_POINTS and n[s] > 0 and dt[s] == 200.0 - (100.0 + s) and t == 200.0, (offs, s, st, n, dt, t)
                assert blen == 0, (offs, s, blen)
    # dt and t_last move on POINTS only: an empty read, then half a packet, then the rest
    for s in range(S):
        sb.set_radar_state(s, np.zeros(_lib.UART_BUFFER, np.uint8), 0, 50.0)
    st, n, dt = read([0, 0, 0, 0, 0], 60.0)
    assert list(st) == [_lib.UART_NONE] * S and not dt.any() and [sb.radar_state(s)[2] for s in range(S)] == [50.0] * S
    half = L // 2
    st, n, dt = read([0, half, half, half, half], 61.0)
    assert list(st) == [_lib.UART_NONE] * S and not dt.any() and sb.radar_state(0)[1:] == (half, 50.0)
    # mmw_reset_scenes is the tracker's business: the reader keeps its bytes and its time
    before = sb.radar_state(0)
    sb.reset_scenes([1, 1, 0, 0])
    sb.reset()
    after = sb.radar_state(0)
    assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]
    flags = sb.buf("fl", S * 4).upload(np.array([1, 0, 0, 0], np.int32))
    b_of.upload(np.array([half, L, L, L, L], np.int64))
    sb.read_radars_dev(b_ch.ptr, b_of.ptr, len(blob), 62.5, *[b.ptr for b in out], flags.ptr)
    st, dt = out[3].download((S,), np.int32), out[2].download((S,), np.float64)
    assert list(st) == [_lib.UART_POINTS] + [_lib.UART_SKIPPED] * 3 and list(dt) == [12.5, 0.0, 0.0, 0.0], (st, dt)
    assert sb.radar_state(0)[2] == 62.5 and sb.radar_state(1)[1:] == (0, 50.0)
    sb.set_radar_time(70.0, scenes=[1])
    assert [sb.radar_state(s)[2] for s in range(S)] == [62.5, 70.0, 50.0, 50.0]
    # a chunk that does not fit is discarded, and says so
    sb.set_radar_state(2, pattern, _lib.UART_BUFFER - L, 50.0)
    st, n, dt = read(good, 80.0)
    assert st[2] == (_lib.UART_NONE | _lib.UART_CHUNK_DROPPED) and sb.radar_state(2)[1] == _lib.UART_BUFFER - L, st
    sb.close_radars()
    with pytest.raises(_lib.MmwError):
        sb.radar_state(0)
    sb.close()
