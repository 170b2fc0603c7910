"""The byte mechanics of the device-resident radar readers (csrc/k_uart.hip: move_bytes, find_last_magic, the cut, the drop, the
len + cnt < 2^15 rule) at the full size of the 2^15-byte buffer and on bytes that tell positions apart.  Each case is one scene
of one context: a state planted with set_radar_state (a pattern in all 2^15 bytes and a length), ONE mmw_uart_read, and then
all 2^15 bytes, the length, t_last, status, frame number, n, dt and the rows equal to tests/_uart_ref.py's numpy restatement of
the reference's read(), which tests/test_uart_buffer.py pins to the reference's own recordings."""
import hashlib
import struct

import numpy as np
import pytest

from tests import _uart_ref as ref
from tests._uart_recording import load_buffer, same_bits

pytestmark = pytest.mark.gpu
MAGIC = bytes([2, 1, 4, 3, 6, 5, 8, 7])
CFGP = {"rangeIdxToMeters": 0.0436, "dopplerResolutionMps": 0.1252, "numDopplerBins": 32.0}
CAP = ref.CAP
LOG_COLS = ("x", "y", "z", "doppler", "peak_val")


def _fill(n, phase):
    """n bytes in 9 .. 255 that tell positions apart: never the 2 a magic word starts with, period 247 = 13 * 19 (coprime to the
    16-byte pieces and the 4096-byte passes), another phase another sequence."""
    return (9 + (131 * (np.arange(n, dtype=np.int64) + phase)) % 247).astype(np.uint8)


def _packet(frame, n_sent, phase, num_obj=None, total=None, q=9):
    """magic word, header, TLV head and n_sent objects of filler bytes; totalPacketLen and the body's numObj as asked."""
    size = 48 + 12 * n_sent
    head = MAGIC + struct.pack("<IIIIIII", 0x01020304, size if total is None else total, 0xA1443, frame, 77, max(n_sent, 1), 1)
    return head + struct.pack("<IIHH", 1, 4 + 12 * n_sent, n_sent if num_obj is None else num_obj, q) + _fill(12 * n_sent, phase).tobytes()


def _plant(buf, pos, what):
    """`what` written at buf[pos ...], cut off at the buffer's end"""
    w = np.frombuffer(what, np.uint8)[: CAP - pos]
    buf[pos: pos + len(w)] = w


class _Scenes:
    """A context of S scenes and, per scene, the restatement that follows it."""

    def __init__(self, S, max_pts, sites=False, log=False, cfgs=None):
        from mmwave_msc_amd import _lib
        from mmwave_msc_amd.batch import SceneBatch
        self.S, self.N, self.log = S, max_pts, log
        self.cfgs = [CFGP] * S if cfgs is None else cfgs
        self.sb = SceneBatch(_lib.default_config(), S, max_pts)
        if sites:
            self.sb.set_sites(_lib.make_sites(self.sb.cfg, S, s_height=list(np.linspace(1.1, 2.0, S)), s_tilt=list(np.linspace(-12.0, 4.0, S))))
        self.sb.open_radars(self.cfgs, t0=0.0)
        if log:
            self.sb.enable_radar_log()
        self.refs = [ref.UartReadRef(c, max_pts, t0=0.0) for c in self.cfgs]
        self.out = [self.sb.buf(k, b) for k, b in (("ub_p", S * max_pts * 64), ("ub_n", S * 4), ("ub_dt", S * 8), ("ub_st", S * 4), ("ub_fr", S * 4))]

    def plant(self, states):
        """states[s] = (buffer[2^15], length); the scenes beyond len(states) get an empty, zeroed reader"""
        zero = np.zeros(CAP, np.uint8)
        for s in range(self.S):
            buf, length = states[s] if s < len(states) else (zero, 0)
            self.sb.set_radar_state(s, buf, length, 100.0 + s)
            self.refs[s].set_state(buf, length, 100.0 + s)

    def read(self, chunks, now, lead=0, tail=b"", live=None):
        """One mmw_uart_read through the pointer form: `lead` filler bytes in front of the first chunk in the shared chunk buffer,
        the last chunk ends exactly at chunks_bytes, `tail` (up to 16 bytes) lies behind it in the padded allocation.  Checks every
        scene against its restatement and returns what the device gave."""
        sb, S, N = self.sb, self.S, self.N
        chunks = list(chunks) + [b""] * (S - len(chunks))
        blob = _fill(lead, 3).tobytes() + b"".join(bytes(c) for c in chunks)
        off = np.zeros(S + 1, np.int64)
        off[0] = lead
        off[1:] = lead + np.cumsum([len(c) for c in chunks])
        assert off[S] == len(blob) and len(tail) <= 16
        padded = np.zeros((len(blob) + 15) // 16 * 16 + 32, np.uint8)
        padded[: len(blob)] = np.frombuffer(blob, np.uint8)
        padded[len(blob): len(blob) + len(tail)] = np.frombuffer(tail, np.uint8)
        b_ch = sb.buf("ub_chunks", len(padded)).upload(padded)
        b_of = sb.buf("ub_off", (S + 1) * 8).upload(off)
        flags = None
        if live is not None:
            fl = np.zeros(S, np.int32)
            fl[list(live)] = 1
            flags = sb.buf("ub_flags", S * 4).upload(fl).ptr
        sb.read_radars_dev(b_ch.ptr, b_of.ptr, len(blob), now, *[b.ptr for b in self.out], flags)
        o = self.out
        got = dict(status=o[3].download((S,), np.int32), frame=o[4].download((S,), np.uint32), n=o[1].download((S,), np.int32),
                   dt=o[2].download((S,), np.float64), pts=o[0].download((S, N, 8), np.float64), off=off)
        scenes = range(S) if live is None else list(live)
        want = {s: self.refs[s].read(chunks[s], now) for s in scenes}
        raw = np.zeros((S, N, 5))
        n_raw = np.zeros(S, np.int32)
        for s, (st, fr, n, rows, dt) in want.items():
            if n > 0:
                raw[s, :n], n_raw[s] = rows, n
        want_pts, want_n = sb.normalize_host(raw, n_raw)
        for s, (st, fr, n, rows, dt) in want.items():
            assert int(got["status"][s]) == st, (s, int(got["status"][s]), st)
            assert int(got["frame"][s]) == fr, (s, int(got["frame"][s]), fr)
            k = int(got["n"][s])
            assert k == (n if n < 0 else want_n[s]), (s, k, n, want_n[s])
            assert got["dt"][s].tobytes() == np.float64(dt).tobytes(), (s, got["dt"][s], dt)
            if k > 0:
                assert same_bits(got["pts"][s, :k], want_pts[s, :k]), s
            buf, blen, t = sb.radar_state(s)
            r = self.refs[s]
            assert (blen, t) == (r.byteBufferLength, r.t_last), (s, blen, r.byteBufferLength, t, r.t_last)
            diff = np.nonzero(buf != r.byteBuffer)[0]
            assert len(diff) == 0, (s, "buffer bytes differ", len(diff), diff[:4], buf[diff[:4]], r.byteBuffer[diff[:4]])
        if self.log:
            self._check_log(want, now)
        got["want"] = want
        return got

    def _check_log(self, want, now):
        """the logged frames are the restatement's POINTS reads: frame number, count, time, and the six columns bit for bit"""
        d, rows = self.sb.radar_log_host()
        points = [s for s, w in sorted(want.items()) if (w[0] & 255) == ref.POINTS]
        assert list(d["scene"]) == points, (list(d["scene"]), points)
        for e in d:
            s = int(e["scene"])
            st, fr, n, raw, dt = want[s]
            assert (int(e["frame_number"]), int(e["count"]), float(e["t"])) == (fr, n, now), (s, e)
            mine = rows[e["first"]: e["first"] + e["count"]]
            for c, name in enumerate(LOG_COLS):
                assert same_bits(mine[name], raw[:, c]), (s, name)
            assert same_bits(mine["range"], self.refs[s].range), s

    def close(self):
        self.sb.close()


def _batches(cases, S):
    for i in range(0, len(cases), S):
        yield cases[i: i + S]


APPEND_LEN = (0, 1, 2, 3, 15, 16, 17, 4095, 4096, 4097)
APPEND_CHUNK = (1, 2, 3, 4, 15, 16, 17, 19, 20, 21, 4080, 4096, 4097, 8197, 12000)


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_append(lead):
    """Every planted length x every chunk length, three launches of 50 scenes; `lead` bytes in front of the first chunk move every
    chunk's start in the shared chunk buffer, so over the four runs each pair meets each source alignment.  No magic word anywhere:
    the append is all that acts, and whatever lies outside the appended range stays as planted."""
    pairs = [(l, c) for c in APPEND_CHUNK for l in APPEND_LEN]
    sc = _Scenes(50, 64)
    starts = set()
    for b, batch in enumerate(_batches(pairs, 50)):
        sc.plant([(_fill(CAP, 1000 * b + 7 * s), l) for s, (l, c) in enumerate(batch)])
        got = sc.read([_fill(c, 5000 + 100 * b + s).tobytes() for s, (l, c) in enumerate(batch)], now=200.0 + b, lead=lead)
        assert not got["status"].any() and [sc.refs[s].byteBufferLength for s in range(len(batch))] == [l + c for l, c in batch]
        starts |= {(int(got["off"][s]) % 4, c >= 4080) for s, (l, c) in enumerate(batch)}
    assert {a for a, long in starts if long} == {0, 1, 2, 3} and {a for a, long in starts if not long} == {0, 1, 2, 3}, sorted(starts)
    sc.close()


@pytest.mark.parametrize("odd", [1, 2, 3])
def test_append_ends_with_the_chunk_buffer(odd):
    """The last scene's chunk ends exactly at chunks_bytes, and chunks_bytes % 4 = 1, 2, 3: of the last dword only the bytes that
    belong to the chunk arrive.  Each of four chunks is once the one at the end, and every run happens twice with different bytes
    behind chunks_bytes in the padded allocation -- the second time magic words -- with the same result, the restatement's."""
    lens = [(0, 4097), (3, 8197), (4095, 19), (1, 12000), (17, 4080), (4097, 3), (16, 4096)]
    S = len(lens)
    lead = (odd - sum(c for l, c in lens)) % 4
    sc = _Scenes(S, 64)
    for last in range(4):
        order = [(k + last + 1) % S for k in range(S)]
        after = []
        for tail in (bytes(range(200, 216)), MAGIC + MAGIC):
            sc.plant([(_fill(CAP, 31 * o), lens[o][0]) for o in order])
            got = sc.read([_fill(lens[o][1], 900 + o).tobytes() for o in order], now=300.0, lead=lead, tail=tail)
            assert int(got["off"][S]) % 4 == odd and not got["status"].any()
            after.append([sc.sb.radar_state(s)[0].tobytes() for s in range(S)])
        assert after[0] == after[1], last
    sc.close()


def test_capacity_rule():
    """len + cnt = 32 767 is kept and 32 768 dropped: with a chunk of 1 byte and of 12 000 bytes, from an empty buffer, and with a
    pending packet in front that announces 32 767 bytes, which the kept chunk completes (decoded, and the whole buffer dropped by
    that odd length) and the dropped one does not."""
    pend = _packet(9, 3, 40, total=32767)
    cases = [(32766, 1), (32767, 1), (20767, 12000), (20768, 12000), (0, 32767), (0, 32768), (32767, 0), (20767, 12001)]
    states, chunks = [], []
    for s, (l, c) in enumerate(cases):
        states.append((_fill(CAP, 50 + s), l))
        chunks.append(_fill(c, 60 + s).tobytes())
    for l, c in ((20767, 12000), (20767, 12001), (32766, 1), (32766, 2)):
        buf = _fill(CAP, 70 + len(states))
        _plant(buf, 0, pend)
        states.append((buf, l))
        chunks.append(_fill(c, 80 + len(states)).tobytes())
    sc = _Scenes(len(states), 64)
    sc.plant(states)
    got = sc.read(chunks, now=400.0)
    st = [int(v) for v in got["status"]]
    D = ref.CHUNK_DROPPED
    assert st == [0, D, 0, D, 0, D, 0, D, ref.POINTS, D, ref.POINTS, D], st
    assert [sc.refs[s].byteBufferLength for s in range(len(states))] == [32767, 32767, 32767, 20768, 32767, 0, 32767, 20767, 0, 20767, 0, 32766]
    sc.close()


def _find_cases():
    """(length, [(position, whole header?)], classes) for test_find.  Positions come from the scan's own rule: limit = length - 8,
    the first pass starts at piece vt = (limit - 1) >> 4, pass p's thread tid takes piece vt - 256 p - tid, 16 positions each."""
    cases = []

    def pos(length, p, tid, j):
        v = ((length - 8 - 1) >> 4) - 256 * p - tid
        assert v >= 0 and 0 <= j < 16
        return 16 * v + j

    def add(length, positions, *classes):
        cases.append((length, [(q, True) if isinstance(q, int) else q for q in positions], set(classes)))

    L = 32767                                                   # limit 32759: eight passes, the top piece has 7 positions
    for j in range(16):
        add(L, [pos(L, 3, 100, j)], "residue", "middle pass")
    for tid in (0, 63, 64, 255):
        add(L, [pos(L, 0, tid, 5)], f"lane {tid}", "first pass")
    add(L, [pos(L, 7, 17, 9)], "last pass")
    add(L, [0], "position 0", "last pass")
    add(17, [0], "position 0")
    add(20001, [pos(20001, 4, 200, 0)], "last pass")
    # the word reaches into the next piece, which belongs to the lane before, the wave before, the pass before
    add(L, [pos(L, 2, 10, 12)], "straddles a piece")
    add(L, [pos(L, 2, 64, 13)], "straddles a wave")
    add(L, [pos(L, 1, 128, 15)], "straddles a wave")
    add(L, [pos(L, 1, 0, 9)], "straddles a pass")
    add(L, [pos(L, 5, 0, 15)], "straddles a pass")
    # limit - 1 counts and limit does not, alone and with a true word further down, for limit % 16 = 7, 0, 1, 15
    for length in (L, 4104, 4105, 4119, 25, 8207):
        lim = length - 8
        add(length, [lim - 1], "limit - 1")
        add(length, [(lim, False)], "limit alone")
        add(length, [pos(length, 0, 4, 3) if length > 100 else 0, (lim, False)], "limit behind a true one")
        add(length, [(lim + 1, False)], "limit alone")
    # two words: the last wins
    add(L, [(pos(L, 2, 40, 2), False), pos(L, 2, 40, 10)], "pair in a piece")
    add(L, [(pos(L, 6, 3, 0), False), pos(L, 6, 3, 8)], "pair in a piece")
    add(L, [pos(L, 2, 10, 3), pos(L, 2, 9, 3)], "pair in neighbouring lanes")
    add(L, [pos(L, 0, 1, 0), pos(L, 0, 0, 0)], "pair in neighbouring lanes")
    add(L, [pos(L, 3, 64, 7), pos(L, 3, 63, 7)], "pair in two waves")
    add(L, [pos(L, 4, 200, 1), pos(L, 4, 70, 14)], "pair in two waves")
    add(L, [pos(L, 0, 255, 4), pos(L, 0, 130, 4)], "pair in two waves")
    add(L, [pos(L, 5, 30, 6), pos(L, 1, 30, 6)], "pair in two passes")
    add(L, [pos(L, 7, 250, 0), pos(L, 6, 250, 0)], "pair in two passes")
    add(12345, [pos(12345, 3, 1, 11), pos(12345, 0, 254, 2)], "pair in two passes")
    # seven bytes of a magic word behind a true one
    add(L, [pos(L, 4, 77, 5), (pos(L, 1, 20, 9), MAGIC[:7] + b"\x09")], "prefix")
    add(9000, [pos(9000, 1, 5, 0), (pos(9000, 1, 5, 0) + 8, MAGIC[:7] + b"\x08")], "prefix")
    return cases


def test_find():
    """An empty chunk onto a planted buffer whose magic words head packets that announce 40 000 bytes: nothing is ever complete, so
    only the backward scan and the cut to what it found act."""
    cases = _find_cases()
    head = _packet(5, 1, 0, total=40000)[:36]
    reached = set()
    for length, positions, classes in cases:
        reached |= classes
    assert reached >= {"residue", "first pass", "middle pass", "last pass", "lane 0", "lane 63", "lane 64", "lane 255", "position 0",
                       "straddles a piece", "straddles a wave", "straddles a pass", "limit - 1", "limit alone", "limit behind a true one",
                       "pair in a piece", "pair in neighbouring lanes", "pair in two waves", "pair in two passes", "prefix"}
    assert len({p[0][0] % 16 for l, p, c in cases if "residue" in c}) == 16 and max(l for l, p, c in cases) == 32767
    sc = _Scenes(64, 64)
    for b, batch in enumerate(_batches(cases, 64)):
        states = []
        for s, (length, positions, classes) in enumerate(batch):
            buf = _fill(CAP, 11 * s + b)
            for q, what in positions:
                _plant(buf, q, head if what is True else MAGIC if what is False else what)
            states.append((buf, length))
        sc.plant(states)
        got = sc.read([b""] * len(batch), now=500.0 + b)
        assert not got["status"].any()
        for s, (length, positions, classes) in enumerate(batch):
            true = [q for q, what in positions if what is True or (what is False and q < length - 8)]
            want_len = length - max(true) if true and length > 16 else length
            assert sc.refs[s].byteBufferLength == want_len, (s, length, positions, sc.refs[s].byteBufferLength, want_len)
    sc.close()


def test_cut():
    """A magic word at position 1, 2, 3, 5, 16, 4095, 4096 or 4097 of about 30 000 bytes that tell positions apart: the cut is a move
    of the buffer onto itself over seven or eight passes, by every byte shift and by less than, exactly and more than a pass."""
    head = _packet(6, 1, 0, total=40000)[:36]
    cases = [(L, q) for L in (30001, 32767, 28672 + 16) for q in (1, 2, 3, 5, 16, 4095, 4096, 4097)]
    states = []
    for s, (L, q) in enumerate(cases):
        buf = _fill(CAP, 13 * s + 1)
        _plant(buf, q, head)
        states.append((buf, L))
    sc = _Scenes(len(cases), 64)
    sc.plant(states)
    got = sc.read([], now=600.0)
    assert not got["status"].any() and [r.byteBufferLength for r in sc.refs] == [L - q for L, q in cases]
    assert all(r.moves == [("cut", q, L - q)] for r, (L, q) in zip(sc.refs, cases))
    sc.close()


def test_drop():
    """A complete 3-object packet in front of up to 32 767 bytes, with totalPacketLen 0 .. len: decoded, and then that many bytes
    dropped -- a move onto itself by a length the wire chose (0 moves nothing, len leaves nothing)."""
    cases = []
    for L in (32767, 20003, 8200):
        cases += [(L, t) for t in (0, 1, 3, 4, 16, 17, 4095, 4096, 4097, L - 1, L)]
    cases += [(32766, 12001), (32767, 32765), (4200, 4199)]
    states = []
    for s, (L, t) in enumerate(cases):
        buf = _fill(CAP, 17 * s + 2)
        _plant(buf, 0, _packet(700 + s, 3, s, total=t))
        states.append((buf, L))
    sc = _Scenes(len(cases), 64)
    sc.plant(states)
    got = sc.read([], now=700.0)
    assert list(got["status"]) == [ref.POINTS] * len(cases) and list(got["n"] >= 0) == [True] * len(cases)
    assert [r.byteBufferLength for r in sc.refs] == [L - t for L, t in cases]
    assert all(r.moves[-1] == ("drop", t, L - t) for r, (L, t) in zip(sc.refs, cases))
    assert list(got["dt"]) == [700.0 - (100.0 + s) for s in range(len(cases))]
    sc.close()


VARIANTS = [pytest.param(False, False, id="plain"), pytest.param(True, False, id="log"), pytest.param(False, True, id="sites")]


@pytest.mark.parametrize("log,sites", VARIANTS)
def test_buffer_recording_read_by_read(log, sites):
    """tests/golden/uart_buffer.npz, every stream a scene of one context with max_pts 1024 (four rows per thread), one
    mmw_uart_read per recorded read(): the device equals the restatement (all 2^15 bytes and every word), and both equal what the
    reference recorded -- dataOK, frameNumber, raised, byteBufferLength, the SHA-256 of the buffer.  The 2726 objects announced are
    OVERFLOW here, the 2727 RAISED."""
    from mmwave_msc_amd import _lib
    streams = load_buffer()
    S = len(streams)
    sc = _Scenes(S, 1024, sites=sites, log=log, cfgs=[s.cfg for s in streams])
    sc.plant([])
    calls = max(len(s.reads) for s in streams)
    seen = {"points": 0, "rows": 0, "overflow": [], "raised": [], "dropped": 0, "deep": 0}
    for k in range(calls):
        live = [s for s in range(S) if k < len(streams[s].reads)]
        chunks = [streams[s].reads[k].chunk if s in live else b"" for s in range(S)]
        got = sc.read(chunks, now=1000.0 + k, live=live)
        for s in range(S):
            low = int(got["status"][s]) & 255
            if s not in live:
                assert low == _lib.UART_SKIPPED and got["n"][s] == 0, (s, k, low)
                continue
            rd, where = streams[s].reads[k], (streams[s].name, k)
            assert (low == ref.RAISED) == rd.raised and int(got["frame"][s]) == rd.frame, (where, low)
            assert (low in (ref.POINTS, ref.OVERFLOW)) == bool(rd.ok) and (low == ref.OVERFLOW) == (rd.ok and rd.num_obj > 1024), (where, low)
            buf, blen, _ = sc.sb.radar_state(s)
            assert blen == rd.buflen and hashlib.sha256(buf.tobytes()).digest() == rd.digest, where
            if low == ref.POINTS:
                assert got["want"][s][2] == rd.num_obj, where
                seen["points"] += 1
                seen["rows"] += int(got["n"][s])
                seen["deep"] += int(got["n"][s] > 256)
            seen["overflow"] += [rd.num_obj] if low == ref.OVERFLOW else []
            seen["raised"] += [where] if rd.raised else []
            seen["dropped"] += int(got["status"][s]) >> 8
    assert seen["overflow"] == [2726] and len(seen["raised"]) == 1 and seen["dropped"] >= 6 and seen["points"] >= 25, seen
    assert seen["deep"] >= 4 and seen["rows"] > 2000, seen   # (Q 15 keeps about half of a packet's rows in the room)
    sc.close()


@pytest.mark.parametrize("log,sites", VARIANTS)
def test_stale_objects_and_the_last_object_that_fits(log, sites):
    """max_pts 1024.  3 objects sent and 257, 300, 513, 900 and 1024 announced: the rest are decoded from the planted buffer's stale
    bytes, at rows 256 and above (the second to fourth row of a thread).  2726 announced is the last object that ends inside the
    buffer (OVERFLOW for any max_pts), 2727 reaches past it (RAISED: nothing dropped, nothing logged); 1025 is OVERFLOW."""
    nums = [257, 300, 513, 900, 1024, 1025, 2726, 2727, 65535, 255, 256]
    states, chunks = [], []
    for s, num in enumerate(nums):
        buf = _fill(CAP, 19 * s + 3)
        pk = _packet(800 + s, 3, s, num_obj=num, q=14 + s % 2)       # x, y, z within +-2 m: about half the rows pass normalize_data
        if s % 2:            # the packet is planted, the chunk brings only a few bytes behind it
            _plant(buf, 0, pk)
            states.append((buf, len(pk)))
            chunks.append(_fill(5, s).tobytes())
        else:                # the packet arrives behind 4099 stale bytes and is cut to the front first
            states.append((buf, 4099))
            chunks.append(pk + _fill(5, s).tobytes())
    sc = _Scenes(len(nums), 1024, sites=sites, log=log)
    sc.plant(states)
    got = sc.read(chunks, now=900.0)
    low = [int(v) & 255 for v in got["status"]]
    want = [ref.POINTS if n <= 1024 else ref.OVERFLOW if n <= 2726 else ref.RAISED for n in nums]
    assert low == want, (low, want)
    assert [w[2] for s, w in sorted(got["want"].items())] == [n if n <= 1024 else ref.BAD_FRAME if n <= 2726 else 0 for n in nums]
    sc.close()
