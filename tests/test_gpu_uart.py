"""mmw_parse_uart / radar.UartFrameParser (reference src/ReadDataIWR1443.py:27-262).  The parser is host code
inside the HIP library, so loading it needs the GPU box (marked gpu); no kernel runs."""
import os
import struct

import numpy as np
import pytest

from tests._uart_recording import DET_KEYS, load as load_recording, same_bits

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "uart.npz")


def _packet(frame, objs, qfmt=9, tlv_type=1, num_det=None):
    body = struct.pack("<HH", len(objs), qfmt) + b"".join(struct.pack("<6H", *[int(v) & 0xFFFF for v in o]) for o in objs)
    tlv = struct.pack("<II", tlv_type, len(body)) + body
    total = 36 + len(tlv)
    return bytes([2, 1, 4, 3, 6, 5, 8, 7]) + struct.pack("<IIIIIII", 0x01020304, total, 0xA1443, frame, 1, len(objs) if num_det is None else num_det, 1) + tlv


def test_buffer_discipline_matches_reference_recording():
    """Frame numbers, dataOK and the length of the byte buffer after every read, as recorded from the reference's
    read() (oracle/gen_golden.py gen_uart: the paths that run under numpy 2)."""
    from mmwave_msc_amd.radar import UartFrameParser
    g = np.load(GOLD, allow_pickle=True)
    cfg = g["cfg"]
    p = UartFrameParser({"rangeIdxToMeters": cfg[0], "dopplerResolutionMps": cfg[1], "numDopplerBins": cfg[2]})
    for i in range(int(g["n_chunks"])):
        ok, fn, det = p.feed(g[f"chunk{i}"].tobytes())
        assert ok == int(g[f"ok{i}"]) and fn == int(g[f"frame{i}"]), (i, ok, fn)
        assert p.byteBufferLength == int(g[f"buflen{i}"]), (i, p.byteBufferLength, int(g[f"buflen{i}"]))


def _replay(stream, max_obj=4096):
    """Feed a recorded stream (tests/golden/uart_decode.npz) to UartFrameParser read by read: None, or the first read that
    differs from the reference's -- raised or not, dataOK, frameNumber, byteBufferLength, the buffer's bytes, every detObj array."""
    from mmwave_msc_amd.radar import UartFrameParser
    p = UartFrameParser(stream.cfg, max_obj=max_obj)
    for r in stream.reads:
        try:
            ok, fn, det = p.feed(r.chunk)
            raised = False
        except ValueError:
            ok, fn, det, raised = 0, 0, {}, True
        if raised != r.raised or (ok, fn) != (r.ok, r.frame):
            return r.index, "raised/dataOK/frameNumber", (raised, ok, fn), (r.raised, r.ok, r.frame)
        if p.byteBufferLength != r.buflen or bytes(p.byteBuffer[: p.byteBufferLength]) != r.buf:
            return r.index, "byteBuffer", p.byteBufferLength, r.buflen
        if ok:
            if det["numObj"] != r.num_obj:
                return r.index, "numObj", det["numObj"], r.num_obj
            for c, key in enumerate(DET_KEYS):
                if not same_bits(det[key], r.det[:, c]):
                    return r.index, key, det[key][:4], r.det[:4, c]
    return None


def test_detected_points_decode():
    """UartFrameParser (mmw_parse_uart) replays every stream of the reference's read() recorded under its own numpy 1.26
    (tests/golden/uart_decode.npz, oracle/gen_uart_golden.py): dataOK, frameNumber, byteBufferLength, the buffer's bytes and
    x, y, z, doppler, peakVal, range bit-equal (NaN-aware) after every read, ValueError where the reference raised.  The
    streams reach the int16 wrap of every field, the doppler wrap threshold for fractional / tiny numDopplerBins, Q 0..70
    and up to 65535 (the int64 `2 ** Q` wraps: -2^63 at 63, 0 from 64 on), totalPacketLen 0 .. 48 with the bytes present,
    objects past the packet and past the received bytes (the stale bytes of the 2^15-byte buffer), packets split at every
    byte, several per chunk, garbage, and a chunk dropped by the maxBufferSize rule."""
    failed = {}
    for s in load_recording():
        d = _replay(s)
        if d is not None:
            failed[s.name] = d
    assert not failed, f"streams that differ from the reference's read() (first difference: read, what, got, want): {failed}"


def test_more_than_max_obj_objects_is_the_declared_difference():
    """The one declared difference of the host decode: a packet announcing more than max_obj objects raises MmwError
    (MMW_E_ARG) where the reference decodes it (1100 objects at the default max_obj = 1024); every read before is the reference's."""
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.radar import UartFrameParser
    s = next(s for s in load_recording() if s.name == "over_max_obj")
    p = UartFrameParser(s.cfg)
    for r in s.reads:
        if r.ok and r.num_obj > p.max_obj:
            with pytest.raises(_lib.MmwError) as ei:
                p.feed(r.chunk)
            assert ei.value.code == _lib.E_ARG
            return
        ok, fn, _ = p.feed(r.chunk)
        assert (ok, fn, p.byteBufferLength) == (r.ok, r.frame, r.buflen), r.index
    pytest.fail("the recording holds no packet over max_obj")


def test_find_tlv_on_the_recording_finds_what_read_decoded_and_refuses_stale_bytes():
    """mmw_find_tlv has no buffer history.  On the bytes each recorded read() saw (the buffer before it plus the chunk) it finds
    the body the reference decoded whenever that body lies in those bytes -- same bytes, count and frame number --, refuses
    every packet the reference completed from stale bytes of its 2^15-byte buffer or raised on, and never reports a body where
    the reference decoded none."""
    from mmwave_msc_amd import radar
    refused = hits = 0
    for s in load_recording():
        prev = b""
        for r in s.reads:
            before = prev + r.chunk if len(prev) + len(r.chunk) < radar.MAX_BUFFER else prev
            found, off, n, frame, start, plen = radar.find_tlv(before)
            where = (s.name, r.index, found)
            if r.ok and not r.raised and start + 48 + 12 * r.num_obj <= len(before):
                assert found and n == r.num_obj and frame == r.frame, where
                assert before[off: off + 4 + 12 * n] == r.body, where
                hits += 1
            else:
                assert not found and off == -1 and n == 0, where
                refused += int(r.ok or r.raised)
            prev = r.buf
    assert hits > 200 and refused >= 5, (hits, refused)


def test_parse_config_file(tmp_path):
    from mmwave_msc_amd.radar import parse_config_file
    cfg = tmp_path / "radar.cfg"
    cfg.write_text("sensorStop\nprofileCfg 0 77 7 7 58 0 0 68 1 256 5500 0 0 30\nframeCfg 0 2 16 0 100 1 0\nsensorStart\n")
    p = parse_config_file(str(cfg))
    assert p["numDopplerBins"] == 16.0 and p["numRangeBins"] == 256 and p["framePeriodicity"] == 100.0
    assert abs(p["rangeIdxToMeters"] - (3e8 * 5500 * 1e3) / (2 * 68 * 1e12 * 256)) < 1e-15
    assert abs(p["dopplerResolutionMps"] - 3e8 / (2 * 77 * 1e9 * (7 + 58) * 1e-6 * 16 * 3)) < 1e-15


def _tlv_case(rng, S, N, cfgp):
    """S chunks as a serial port might deliver them: most hold one complete detected-points packet (random object count, Q format,
    int16 fields incl. negative coordinates and doppler indices on both sides of the reference's wrap threshold), some none."""
    chunks, kinds = [], []
    for s in range(S):
        kind = int(rng.integers(0, 10))
        n = int(rng.integers(0, N + 1)) if kind != 3 else N
        o = np.zeros((n, 6), dtype=np.int64)
        o[:, 0] = rng.integers(0, 256, n)
        o[:, 1] = rng.integers(-40, 41, n)
        o[:, 2] = rng.integers(0, 4000, n)
        o[:, 3] = rng.integers(-1500, 1500, n)
        o[:, 4] = rng.integers(20, 3600, n)
        o[:, 5] = rng.integers(-900, 300, n)
        q = int(rng.choice([7, 8, 9, 9, 9]))
        lead = b"\x00" * int(2 * rng.integers(0, 4))            # (bodies 2-byte aligned, not always 4)
        if kind == 0:
            pkt = _packet(7 + s, o, qfmt=q, num_det=0)            # header announces no objects
        elif kind == 1:
            pkt = _packet(7 + s, o, qfmt=q, tlv_type=2)           # another TLV first
        elif kind == 2:
            pkt = _packet(7 + s, o, qfmt=q)[:-6] if n else _packet(7 + s, o, qfmt=q)   # the last object is not all there yet
        else:
            pkt = _packet(7 + s, o, qfmt=q)
        chunks.append(lead + pkt + (b"\x00\x00" if kind == 4 else b""))
        kinds.append(kind)
    return chunks, kinds


@pytest.mark.parametrize("N", [64, 200, 600])
def test_device_tlv_decode_and_normalize_equals_host_parse_then_normalize(N):
    """mmw_find_tlv + mmw_normalize_tlv (the GPU decodes the detected-points TLV of every scene's packet and normalises it in one
    kernel; ReadDataIWR1443.py:107-171, Utils.py:342-434) against mmw_parse_uart + mmw_normalize on the same bytes: the rows that
    reach track() and their counts bit-equal, scene by scene; scenes without a complete detected-points packet get n = 0.  Then both
    paths through mmw_step for three frames: identical association and track state."""
    import ctypes as C
    from mmwave_msc_amd import _lib, radar
    from mmwave_msc_amd.batch import SceneBatch
    rng = np.random.default_rng(40 + N)
    S = 48
    cfgp = {"rangeIdxToMeters": 0.0436, "dopplerResolutionMps": 0.1252, "numDopplerBins": 32.0}
    ucfg = radar.uart_cfg(cfgp)
    sb_dev = SceneBatch(_lib.default_config(db_min_samples=10), S, N)
    sb_host = SceneBatch(_lib.default_config(db_min_samples=10), S, N)
    L = _lib.load()
    n_rows = 0
    for frame in range(3):
        chunks, kinds = _tlv_case(rng, S, N, cfgp)
        # ---- host path: one mmw_parse_uart per packet, then mmw_normalize ----
        raw = np.zeros((S, N, 5))
        n_raw = np.zeros(S, np.int32)
        rcs = np.zeros(S, np.int32)
        for s, ch in enumerate(chunks):
            a = np.frombuffer(ch, dtype=np.uint8)
            rows = np.zeros((N, 5))
            n = C.c_int32(0)
            rc = L.mmw_parse_uart(a.ctypes.data, len(a), C.byref(ucfg), rows.ctypes.data, None, N, C.byref(n), None, None, None)
            assert rc in (0, 1), (s, rc)
            raw[s], n_raw[s], rcs[s] = rows, n.value, rc
        want_pts, want_n = sb_host.normalize_host(raw, n_raw)
        # ---- device path: the host only finds the bodies ----
        blob = b"".join(chunks)
        offs = np.full(S, -1, np.int64)
        base = 0
        for s, ch in enumerate(chunks):
            found, off, n_obj, _, _, _ = radar.find_tlv(ch)
            assert found == (rcs[s] == 1) and (not found or n_obj == n_raw[s]), (s, kinds[s], found, rcs[s])
            if found:
                assert n_obj <= N
                offs[s] = base + off
            base += len(ch)
        b_pk = sb_dev.buf("tlv_bytes", len(blob) + 16).upload(np.frombuffer(blob, dtype=np.uint8))
        b_of = sb_dev.buf("tlv_off", S * 8).upload(offs)
        b_out = sb_dev.buf("tlv_pts", S * N * 64)
        b_no = sb_dev.buf("tlv_n", S * 4)
        sb_dev.normalize_tlv_dev(b_pk.ptr, len(blob), b_of.ptr, ucfg, b_out.ptr, b_no.ptr)
        got_n = b_no.download((S,), np.int32)
        got_pts = b_out.download((S, N, 8), np.float64)
        assert np.array_equal(got_n, want_n), (frame, got_n, want_n)
        for s in range(S):
            assert np.array_equal(got_pts[s, : got_n[s]], want_pts[s, : want_n[s]]), (frame, s, kinds[s])
        n_rows += int(got_n.sum())
        # ---- both through TrackBuffer.track ----
        dt = np.full(S, 0.1)
        b_dt = sb_dev.buf("tlv_dt", S * 8).upload(dt)
        b_as = sb_dev.buf("tlv_assoc", S * N * 4)
        sb_dev.step_dev(b_out.ptr, b_no.ptr, b_dt.ptr, b_as.ptr)
        a_host, _, _ = sb_host.step_host(want_pts, want_n, dt)
        a_dev = b_as.download((S, N), np.int32)
        for s in range(S):
            assert np.array_equal(a_dev[s, : got_n[s]], a_host[s, : want_n[s]]), (frame, s)
    assert n_rows > S * N // 8
    nt_d, nt_h = sb_dev.num_tracks(), sb_host.num_tracks()
    assert np.array_equal(nt_d, nt_h)
    td, th = sb_dev.tracks(cap=max(int(nt_d.max()), 1)), sb_host.tracks(cap=max(int(nt_h.max()), 1))
    for name in ("x", "P", "centroid", "spread_est", "group_disp_est", "lifetime", "point_num", "ring_n"):
        assert np.array_equal(td[name], th[name]), name
    sb_dev.check(); sb_host.check()
    sb_dev.close(); sb_host.close()


def _edge_packets(source, N):
    """Packets (from the magic word on) that mmw_find_tlv accepts with at most N objects: every one of the recording
    (tests/golden/uart_decode.npz, the streams with CFG A's configParameters), or synthetic ones with Q in {0, 62, 63, 64, 65535}
    and, in half of them, all six fields over their full u16 range."""
    from mmwave_msc_amd import radar
    if source == "recording":
        streams = load_recording()
        cfgp = streams[0].cfg
        out = []
        for s in streams:
            if s.cfg != cfgp:
                continue
            prev = b""
            for r in s.reads:
                before = prev + r.chunk if len(prev) + len(r.chunk) < radar.MAX_BUFFER else prev
                found, off, n, _, start, _ = radar.find_tlv(before)
                if found and n <= N:
                    out.append(before[start:])
                prev = r.buf
        return cfgp, out
    rng = np.random.default_rng(77)
    cfgp = {"rangeIdxToMeters": 0.0436, "dopplerResolutionMps": 0.1252, "numDopplerBins": 32.0}
    out = []
    for i in range(96):
        n = int(rng.integers(1, N + 1))          # (_packet announces len(objs) objects in the header: 0 would be no body)
        if i % 2:
            o = rng.integers(0, 65536, size=(n, 6))
        else:
            o = np.zeros((n, 6), dtype=np.int64)
            o[:, 0] = rng.integers(0, 256, n)
            o[:, 1] = rng.integers(-40, 41, n)
            o[:, 2] = rng.integers(0, 4000, n)
            o[:, 3:6] = rng.integers(-3000, 3000, size=(n, 3))
            o[: n // 2, 4] = -o[: n // 2, 4]     # (y < 0 and Q = 63: y / -2^63 > 0, a row the scene filter keeps)
        out.append(_packet(300 + i, o, qfmt=int((0, 62, 63, 64, 65535)[i % 5])))
    return cfgp, out


@pytest.mark.parametrize("source", ["recording", "q_edges"])
def test_device_tlv_decode_equals_host_parse_on_edge_packets(source):
    """mmw_find_tlv + mmw_normalize_tlv against mmw_parse_uart + mmw_normalize on the same bytes for the packets of the
    reference recording and for Q formats 0, 62, 63, 64, 65535 with full-range fields: rows and counts bit-equal (NaN-aware)
    scene by scene, then three mmw_steps on both paths -- association, sticky error bits (the reference's ValueError frames,
    should a non-finite row reach apply_DBscan) and track state identical."""
    import ctypes as C
    from mmwave_msc_amd import _lib, radar
    from mmwave_msc_amd.batch import SceneBatch
    S, N = 48, 64
    cfgp, packets = _edge_packets(source, N)
    assert len(packets) >= S, len(packets)
    ucfg = radar.uart_cfg(cfgp)
    sb_dev = SceneBatch(_lib.default_config(db_min_samples=3), S, N)
    sb_host = SceneBatch(_lib.default_config(db_min_samples=3), S, N)
    L = _lib.load()
    n_rows = nonfinite = 0
    for frame in range(3):
        chunks = [packets[(frame * S + s) % len(packets)] for s in range(S)]
        raw = np.zeros((S, N, 5))
        n_raw = np.zeros(S, np.int32)
        for s, ch in enumerate(chunks):
            a = np.frombuffer(ch, dtype=np.uint8)
            rows = np.zeros((N, 5))
            n = C.c_int32(0)
            rc = L.mmw_parse_uart_cap(a.ctypes.data, len(a), len(a), C.byref(ucfg), rows.ctypes.data, None, N, C.byref(n), None, None, None)
            assert rc == _lib.UART_POINTS, (frame, s, rc)
            raw[s], n_raw[s] = rows, n.value
            nonfinite += int((~np.isfinite(rows[: n.value, :3])).any())
        want_pts, want_n = sb_host.normalize_host(raw, n_raw)
        blob = b"".join(ch + b"\x00" * (len(ch) & 1) for ch in chunks)   # (bodies 2-byte aligned: every chunk starts at its magic word)
        offs = np.full(S, -1, np.int64)
        base = 0
        for s, ch in enumerate(chunks):
            found, off, n_obj, _, _, _ = radar.find_tlv(ch)
            assert found and n_obj == n_raw[s], (frame, s)
            offs[s] = base + off
            base += len(ch) + (len(ch) & 1)
        b_pk = sb_dev.buf("tlv_bytes", len(blob) + 16).upload(np.frombuffer(blob, dtype=np.uint8))
        b_of = sb_dev.buf("tlv_off", S * 8).upload(offs)
        b_out = sb_dev.buf("tlv_pts", S * N * 64)
        b_no = sb_dev.buf("tlv_n", S * 4)
        sb_dev.normalize_tlv_dev(b_pk.ptr, len(blob), b_of.ptr, ucfg, b_out.ptr, b_no.ptr)
        got_n = b_no.download((S,), np.int32)
        got_pts = b_out.download((S, N, 8), np.float64)
        assert np.array_equal(got_n, want_n), (frame, got_n, want_n)
        for s in range(S):
            assert same_bits(got_pts[s, : got_n[s]], want_pts[s, : want_n[s]]), (frame, s)
        n_rows += int(got_n.sum())
        dt = np.full(S, 0.1)
        b_dt = sb_dev.buf("tlv_dt", S * 8).upload(dt)
        b_as = sb_dev.buf("tlv_assoc", S * N * 4)
        sb_dev.step_dev(b_out.ptr, b_no.ptr, b_dt.ptr, b_as.ptr)
        a_host, _, _ = sb_host.step_host(want_pts, want_n, dt, raise_nonfinite=False, check=False)
        a_dev = b_as.download((S, N), np.int32)
        for s in range(S):
            assert np.array_equal(a_dev[s, : got_n[s]], a_host[s, : want_n[s]]), (frame, s)
        assert np.array_equal(sb_dev.errors(), sb_host.errors()), frame
    assert n_rows > 0 and (source == "recording" or nonfinite > 0), (n_rows, nonfinite)
    nt_d, nt_h = sb_dev.num_tracks(), sb_host.num_tracks()
    assert np.array_equal(nt_d, nt_h)
    td, th = sb_dev.tracks(cap=max(int(nt_d.max()), 1)), sb_host.tracks(cap=max(int(nt_h.max()), 1))
    for name in ("x", "P", "centroid", "spread_est", "group_disp_est", "lifetime", "point_num", "ring_n"):
        assert same_bits(td[name], th[name]), name
    sb_dev.close(); sb_host.close()


def test_find_tlv_agrees_with_the_recorded_uart_session():
    """The byte chunks of the reference's recorded read() session (tests/golden/uart.npz).  The recording holds no DECODED packet
    -- under numpy 2 the reference's decode branch raises, so the generator could only record the other paths (no magic word,
    incomplete packet, no objects announced, another TLV first) --: on every buffer state of the session mmw_find_tlv reports the
    frame number the reference read from the header and no detected-points body, as mmw_parse_uart does."""
    from mmwave_msc_amd import radar
    g = np.load(GOLD, allow_pickle=True)
    cfg = g["cfg"]
    cfgp = {"rangeIdxToMeters": float(cfg[0]), "dopplerResolutionMps": float(cfg[1]), "numDopplerBins": float(cfg[2])}
    p = radar.UartFrameParser(cfgp)
    complete = 0
    for i in range(int(g["n_chunks"])):
        chunk = g[f"chunk{i}"].tobytes()
        before = (bytes(p.byteBuffer[: p.byteBufferLength]) + chunk) if p.byteBufferLength + len(chunk) < radar.MAX_BUFFER else bytes(p.byteBuffer[: p.byteBufferLength])
        ok, fn, det = p.feed(chunk)
        found, off, n_obj, frame, start, plen = radar.find_tlv(before)
        assert ok == int(g[f"ok{i}"]) == 0 and not found and off == -1 and n_obj == 0, i
        assert frame == fn == int(g[f"frame{i}"]), (i, frame, fn)
        complete += int(plen > 0)
    assert complete >= 3


def test_device_tlv_decode_refuses_bodies_outside_the_buffer_or_the_context():
    """mmw_normalize_tlv reads nothing outside packets[0 .. packets_bytes): an offset that is odd or beyond the buffer, a body
    whose announced objects run past its end, and a body that announces more than max_pts objects (mmw_parse_uart: MMW_E_ARG for
    those bytes) all give n_out = MMW_BAD_FRAME for THAT scene -- the mmw_step that follows raises its bad-count bit -- while the
    scenes beside it decode as usual."""
    import struct
    from mmwave_msc_amd import _lib, radar
    from mmwave_msc_amd.batch import SceneBatch
    N, S = 64, 6
    cfgp = {"rangeIdxToMeters": 0.0436, "dopplerResolutionMps": 0.1252, "numDopplerBins": 32.0}
    ucfg = radar.uart_cfg(cfgp)
    rng = np.random.default_rng(3)

    def body(n_announced, n_present, q=9):
        o = rng.integers(-200, 200, size=(n_present, 6)).astype("<i2")
        o[:, 4] = np.abs(o[:, 4]) + 300      # y > 0: the scene filter keeps rows
        return struct.pack("<HH", n_announced, q) + o.tobytes()

    good = body(20, 20)
    blob = good + body(N + 1, N + 1) + good + body(30, 30)      # scene 1 announces max_pts + 1 objects; the last body gets truncated below
    o1, o2, o3 = len(good), len(good) + 4 + 12 * (N + 1), 2 * len(good) + 4 + 12 * (N + 1)
    nbytes = len(blob) - 12 * 5                                   # scene 3: five of its thirty objects lie outside the buffer
    offs = np.array([0, o1, o2, o3, o2 + 1, nbytes - 2], np.int64)   # scene 4: odd offset; scene 5: the 4-byte head does not fit
    sb = SceneBatch(_lib.default_config(), S, N)
    b_pk = sb.buf("tlv_bytes", len(blob) + 16).upload(np.frombuffer(blob, dtype=np.uint8))
    b_of = sb.buf("tlv_off", S * 8).upload(offs)
    b_out = sb.buf("tlv_pts", S * N * 64)
    b_no = sb.buf("tlv_n", S * 4)
    sb.normalize_tlv_dev(b_pk.ptr, nbytes, b_of.ptr, ucfg, b_out.ptr, b_no.ptr)
    got = b_no.download((S,), np.int32)
    assert got[0] > 0 and got[2] == got[0], got
    assert list(got[[1, 3, 4, 5]]) == [_lib.BAD_FRAME] * 4, got
    b_dt = sb.buf("tlv_dt", S * 8).upload(np.full(S, 0.1))
    sb.step_dev(b_out.ptr, b_no.ptr, b_dt.ptr)
    with pytest.raises(_lib.MmwError) as ei:
        sb.check()
    assert ei.value.code == _lib.E_ARG
    err = sb.errors()
    assert [bool(e & 8) for e in err] == [False, True, False, True, True, True], err
    sb.close()

    # Offsets at the ends of the int64 range and of the buffer (bounds are compared by subtraction: `off + 4` would overflow),
    # and a body whose 4 + 12 num bytes end exactly at packets_bytes, which is accepted: it decodes as the same body does
    # in the middle of the buffer.  Its last object's y word is 1, so the 4-byte head at packets_bytes - 4 announces one
    # object that cannot fit.
    tail = bytearray(body(20, 20))
    tail[-4:-2] = struct.pack("<H", 1)
    blob = bytes(tail) * 2
    nbytes = len(blob)
    i64 = np.iinfo(np.int64).max
    offs = np.array([0, len(tail), i64, i64 - 3, nbytes - 3, nbytes - 4], np.int64)
    sb = SceneBatch(_lib.default_config(), S, N)
    b_pk = sb.buf("tlv_bytes", nbytes + 16).upload(np.frombuffer(blob, dtype=np.uint8))
    b_of = sb.buf("tlv_off", S * 8).upload(offs)
    b_out = sb.buf("tlv_pts", S * N * 64)
    b_no = sb.buf("tlv_n", S * 4)
    sb.normalize_tlv_dev(b_pk.ptr, nbytes, b_of.ptr, ucfg, b_out.ptr, b_no.ptr)
    got = b_no.download((S,), np.int32)
    pts = b_out.download((S, N, 8), np.float64)
    assert got[0] > 0 and got[1] == got[0] and np.array_equal(pts[1, : got[1]], pts[0, : got[0]]), got
    assert list(got[2:]) == [_lib.BAD_FRAME] * 4, got
    b_dt = sb.buf("tlv_dt", S * 8).upload(np.full(S, 0.1))
    sb.step_dev(b_out.ptr, b_no.ptr, b_dt.ptr)
    err = sb.errors()
    assert [bool(e & 8) for e in err] == [False, False, True, True, True, True], err
    sb.close()
