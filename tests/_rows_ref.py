"""The checker and the inputs of tests/test_gpu_row_producers.py, on the CPU alone (numpy and the C oracle; no GPU, no torch).

`expected_rows` -- oracle.c_oracle.normalize under a given mounting -- is the ONLY source of an expected value in those tests:
never SceneBatch.normalize_host, never another kernel.  The inputs are built so that a mistake in normalize_rows<R>'s ordered
compaction (csrc/mmw_normalize.hpp: R * 4 blocks of 64 rows, one ballot and one LDS count each) changes the output bytes:

  seam frames   every 64-row block keeps a count strictly between 0 and 64, no two blocks the same count, every row its own
                peakVal (the row index): a swapped, repeated or shifted block offset moves a row (tests/test_row_inputs.py
                shows it on the expected output, without a GPU)
  count lists   row counts on both sides of every block, wave-group (256 rows) and max_pts boundary, and the counts
                normalize_scene clamps
  edge rows     rows ON the scene filter's comparisons, the r == 0 branch by underflow, non-finite rows -- under the mounting
                tilt 0 / height 1.0, where every transformed value is exact -- at the rows lane 0, lane 63 and the first
                thread of each 256-row group own

tests/test_row_inputs.py asserts these properties on the oracle; the oracle itself is held against the reference's
normalize_data on the edge rows by tests/golden/normalize_edges.npz (tests/test_oracle_golden.py)."""
import struct
from typing import NamedTuple

import numpy as np

from oracle import c_oracle as co

MAX_PTS = (256, 257, 512, 513, 768, 1024)          # rows per thread: 1, 2, 2, 4, 4, 4
EXACT = {"s_height": 1.0, "s_tilt": 0.0}           # tilt_cos = 1, tilt_sin = 0: y' = y, z' = z + 1.0, no rounding
DEFAULT = {}                                       # the context's own S_HEIGHT / S_TILT
MOUNTINGS = (EXACT, DEFAULT, {"s_height": 1.1, "s_tilt": -12.0}, {"s_height": 2.2, "s_tilt": -20.0})
SENTINEL = -1.2345e300                             # what the tests prefill `pts` with: no row ever holds it
CFGP = {"rangeIdxToMeters": 0.0436, "dopplerResolutionMps": 0.1252, "numDopplerBins": 32.0}
QFMT = 9                                           # x, y, z = int16 / 512: exact in fp32 and fp64
MAGIC = bytes([2, 1, 4, 3, 6, 5, 8, 7])


class Scene(NamedTuple):
    tag: str
    raw: np.ndarray       # [max_pts, 5] (x, y, z, doppler, peakVal): every row filled, also those at and past n
    n: int                # the count the kernel is given (may lie outside 0 .. max_pts)
    mount: dict           # keyword arguments of default_config / make_sites: s_height, s_tilt


# ---------------------------------------------------------------------------------------------------------------- the checker
def mounting(cfg_or_site):
    """(s_height, tilt_cos, tilt_sin) of a config (mmw_config, OrcConfig), a site record (_lib.SITE_DTYPE) or a dict of
    s_height / s_tilt (degrees) -- the latter through default_config, i.e. np.cos(np.radians(.)) as Utils.py:315."""
    if isinstance(cfg_or_site, dict):
        cfg_or_site = co.default_config(**cfg_or_site)
    if isinstance(cfg_or_site, (np.void, np.ndarray)):
        return tuple(float(cfg_or_site[k]) for k in ("s_height", "tilt_cos", "tilt_sin"))
    return float(cfg_or_site.s_height), float(cfg_or_site.tilt_cos), float(cfg_or_site.tilt_sin)


def expected_rows(cfg_or_site, raw, n):
    """Utils.normalize_data by the C oracle on the first n raw rows (n clamped to 0 .. len(raw), as normalize_scene clamps it)
    under that mounting: [m, 8] float64."""
    cfg = co.default_config()
    cfg.s_height, cfg.tilt_cos, cfg.tilt_sin = mounting(cfg_or_site)
    raw = np.ascontiguousarray(raw, dtype=np.float64).reshape(-1, 5)
    n = min(max(int(n), 0), len(raw))
    return co.normalize(cfg, raw[:n])


# ------------------------------------------------------------------------------------------------------------------ raw rows
def _f32_exact(a):
    return a.astype(np.float32).astype(np.float64)


def ordinary_rows(rng, n):
    """Rows as a sensor sends them, fp32-exact: each of the filter's three comparisons keeps some and drops some."""
    raw = np.zeros((n, 5))
    raw[:, 0] = rng.uniform(-4, 4, n)
    raw[:, 1] = rng.uniform(-1, 9, n)
    raw[:, 2] = rng.uniform(-3, 2, n)
    raw[:, 3] = rng.normal(0, 0.6, n)
    raw = _f32_exact(raw)
    raw[:, 4] = np.arange(n)
    return raw


def kept_rows(rng, n):
    """fp32-exact rows every mounting of MOUNTINGS keeps (y 1 .. 2.5 m, z within 0.4 m of the sensor's height)."""
    raw = np.zeros((n, 5))
    raw[:, 0] = rng.uniform(-3, 3, n)
    raw[:, 1] = rng.uniform(1.0, 2.5, n)
    raw[:, 2] = rng.uniform(-0.4, 0.4, n)
    raw[:, 3] = rng.normal(0, 0.6, n)
    raw = _f32_exact(raw)
    raw[:, 4] = np.arange(n)
    return raw


def block_sizes(max_pts):
    return [min(64, max_pts - b) for b in range(0, max_pts, 64)]


def seam_counts(max_pts, rng):
    """One kept-row count per 64-row block: 0 < k < 64, k <= the block's rows (k < rows where the block has more than one),
    pairwise different."""
    sizes = block_sizes(max_pts)
    ks, used = [0] * len(sizes), set()
    for b in sorted(range(len(sizes)), key=lambda b: sizes[b]):     # (the short last block first: it has the fewest choices)
        hi = min(sizes[b] - 1, 63) if sizes[b] > 1 else 1
        k = next(int(k) for k in rng.permutation(np.arange(1, hi + 1)) if int(k) not in used)
        ks[b] = k
        used.add(k)
    return ks


def _seam_drops(max_pts, rng):
    """The rows to drop: per block a random set, so kept and dropped lanes interleave."""
    ks = seam_counts(max_pts, rng)
    drop = np.zeros(max_pts, bool)
    for b, (size, k) in enumerate(zip(block_sizes(max_pts), ks)):
        drop[64 * b + rng.choice(size, size - k, replace=False)] = True
    return drop, ks


def seam_frame(max_pts, seed):
    """(raw[max_pts, 5], counts per block): rows every mounting keeps, with z forced far below the floor (-50 m) on the rows to drop."""
    rng = np.random.default_rng(seed)
    raw = kept_rows(rng, max_pts)
    drop, ks = _seam_drops(max_pts, rng)
    raw[drop, 2] = -50.0
    return raw, ks


def count_list(max_pts, clamped=True):
    """The counts of the count scenes: both sides of every 64-row block edge that matters, of the 256-row groups and of max_pts;
    with clamped=True also -1, -7 and max_pts + 5, which normalize_scene clamps to 0 .. max_pts."""
    base = [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 767, 768, 769, max_pts - 1, max_pts]
    out = sorted({c for c in base if 0 <= c <= max_pts})
    return out + ([-1, -7, max_pts + 5] if clamped else [])


def edge_positions(max_pts):
    """Rows 0, 63, 64, 255, 256, 511, 512, 767, 768 and max_pts - 1, as far as max_pts allows: lane 0, lane 63, and the last and
    the first thread of every 256-row group."""
    return sorted({p for p in (0, 63, 64, 255, 256, 511, 512, 767, 768, max_pts - 1) if p < max_pts})


class Edge(NamedTuple):
    name: str
    row: tuple            # (x, y, z, doppler) -- peakVal is the row index in the frame
    kept: bool            # under EXACT
    vel: tuple = None     # columns 3..5 of the kept row where the edge is about them (nan = any NaN)


def edge_rows(f32=False):
    """The edge rows under EXACT.  f32=True: the rows an fp32 entry can be given -- every value exactly representable in float32;
    the one-ulp neighbours are float32's, and the rows that need 5e-324 or 1e+-200 (the smallest double, r == 0 by underflow,
    r == inf by overflow) have no float32 counterpart and are left out."""
    nan, inf = float("nan"), float("inf")
    if f32:
        above, below, tiny = 1.5 + 2.0 ** -23, float(np.nextafter(np.float32(-1.0), np.float32(0.0))), 2.0 ** -149
    else:
        # (nextafter(1.5, 2) is not enough: 1.5 + 2^-52 + 1.0 rounds back to 2.5)
        above, below, tiny = 1.5 + 2.0 ** -51, float(np.nextafter(-1.0, 0.0)), 5e-324
    rows = [
        Edge("z' == 2.5", (0.25, 2.0, 1.5, 0.125), True),
        Edge("z' == 2.5 + 1 ulp", (0.25, 2.0, above, 0.125), False),
        Edge("z' == 0", (0.25, 2.0, -1.0, 0.125), False),
        Edge("z' == 0 + 1 ulp", (0.25, 2.0, below, 0.125), True),
        Edge("y == 0", (1.0, 0.0, 0.0, 0.25), False),
        Edge("y == -0", (1.0, -0.0, 0.0, 0.25), False),
        Edge("y == smallest positive", (1.0, tiny, 0.0, 0.25), True),
        Edge("all zero", (0.0, 0.0, 0.0, 0.75), False),
        Edge("x NaN", (nan, 1.0, 0.0, 0.125), False),
        Edge("x +inf", (inf, 1.0, 0.0, 0.125), False),
        Edge("doppler NaN", (0.5, 2.0, -0.25, nan), True, (nan, nan, nan)),
        Edge("doppler +inf", (0.5, 2.0, -0.25, inf), True, (nan, nan, nan)),
    ]
    if not f32:
        rows += [
            Edge("r == 0 by underflow", (0.0, 1e-200, 0.0, 0.75), True, (0.0, 0.75, 0.0)),
            Edge("r == inf by overflow", (1e200, 1.0, 0.5, 0.75), True, (0.0, 0.0, 0.0)),
        ]
    return rows


def edge_frame(max_pts, edge, seed):
    """raw[max_pts, 5]: the edge row at every row of edge_positions, ordinary rows between them, peakVal = row index."""
    raw = ordinary_rows(np.random.default_rng(seed), max_pts)
    for p in edge_positions(max_pts):
        raw[p, :4] = edge.row
    return raw


def scene_group(max_pts, group, f32=False, sites=False):
    """The scenes of one context (at most 24).  "counts": three seam frames and one scene per count of count_list; "edges": one
    seam frame and one scene per edge row.  Without sites the whole context has one mounting -- DEFAULT for "counts", EXACT for
    "edges" --; with sites the scenes cycle through MOUNTINGS, the edge scenes staying under EXACT."""
    M = max_pts
    scenes = []

    def mount(i, exact=False):
        if not sites:
            return EXACT if group == "edges" else DEFAULT
        return EXACT if exact else MOUNTINGS[i % len(MOUNTINGS)]

    if group == "counts":
        for k in range(3):
            scenes.append(Scene(f"seam {k}", seam_frame(M, 1000 * M + k)[0], M, mount(len(scenes))))
        for c in count_list(M):
            scenes.append(Scene(f"count {c}", ordinary_rows(np.random.default_rng(77 * M + c + 7), M), c, mount(len(scenes))))
    elif group == "edges":
        scenes.append(Scene("seam", seam_frame(M, 1000 * M + 9)[0], M, mount(1)))
        for e, edge in enumerate(edge_rows(f32)):
            scenes.append(Scene(f"edge {edge.name}", edge_frame(M, edge, 31 * M + e), M, mount(e, exact=True)))
    else:
        raise ValueError(group)
    assert len(scenes) <= 24
    return scenes


# --------------------------------------------------------------------------------------------------- the radar's wire format
def tlv_objects(rng, n):
    """int16 objects (rangeIdx, dopplerIdx, peakVal, x, y, z) at Q = 9: doppler indices on both sides of the reference's wrap
    threshold, y from behind the sensor to 7 m with one object in sixteen at y == 0, z from 1.8 m below to 1.9 m above it."""
    o = np.zeros((n, 6), dtype=np.int16)
    o[:, 0] = rng.integers(0, 256, n)
    o[:, 1] = rng.integers(-40, 41, n)
    o[:, 2] = np.arange(n)
    o[:, 3] = rng.integers(-1500, 1500, n)
    o[:, 4] = rng.integers(-100, 3600, n)
    o[rng.random(n) < 1 / 16, 4] = 0
    o[:, 5] = rng.integers(-900, 1000, n)
    return o


def seam_objects(max_pts, seed):
    """(objects[max_pts, 6], counts per block): the seam frame in wire format.  The rows to drop are alternately 50 m below the
    sensor and at y == 0, z == 0 -- the latter has z' = s_height inside the scene and y' == 0 under every mounting, so only the
    `y > 0` comparison drops it."""
    rng = np.random.default_rng(seed)
    o = tlv_objects(rng, max_pts)
    o[:, 4] = rng.integers(512, 1281, max_pts)      # 1 .. 2.5 m
    o[:, 5] = rng.integers(-200, 201, max_pts)      # within 0.4 m of the sensor's height
    drop, ks = _seam_drops(max_pts, rng)
    idx = np.flatnonzero(drop)
    o[idx[0::2], 5] = -25600
    o[idx[1::2], 4] = 0
    o[idx[1::2], 5] = 0
    return o, ks


def tlv_bodies(objects, counts, max_pts):
    """Detected-points TLV bodies in radar.encode_tlv_bodies' layout, uint8 [S, stride]: u16 numObj, u16 Q, then ALL max_pts
    objects of the scene -- the ones past numObj are ordinary objects, not zeros, so a decode that ignored numObj would show."""
    stride = (4 + 12 * max_pts + 15) // 16 * 16
    out = np.zeros((len(objects), stride), dtype=np.uint8)
    for s, (o, c) in enumerate(zip(objects, counts)):
        assert o.shape == (max_pts, 6) and 0 <= c <= max_pts
        out[s, :4] = np.frombuffer(struct.pack("<HH", int(c), QFMT), dtype=np.uint8)
        out[s, 4: 4 + 12 * max_pts] = np.frombuffer(np.ascontiguousarray(o, dtype="<i2").tobytes(), dtype=np.uint8)
    return out


def tlv_group(max_pts):
    """(tags, objects[S], counts[S]) of one TLV context: three seam frames and one scene per count of count_list (no clamped
    counts: numObj is a u16, and more than max_pts objects is a refused body, not a clamped one)."""
    tags, objs, counts = [], [], []
    for k in range(3):
        tags.append(f"seam {k}"); objs.append(seam_objects(max_pts, 500 * max_pts + k)[0]); counts.append(max_pts)
    for c in count_list(max_pts, clamped=False):
        tags.append(f"count {c}"); objs.append(tlv_objects(np.random.default_rng(13 * max_pts + c), max_pts)); counts.append(c)
    assert len(tags) <= 24
    return tags, objs, counts


def decoded_rows(bodies, max_pts):
    """radar.decode_tlv_bodies_numpy (host numpy, pinned to the reference's recorded read() by tests/test_uart_decode.py):
    (raw[S, max_pts, 5] float64, counts[S]).  (The stride's padding decodes as one more row: cut.)"""
    from mmwave_msc_amd import radar
    raw, cnt = radar.decode_tlv_bodies_numpy(bodies, CFGP)
    return np.ascontiguousarray(raw[..., :max_pts, :]), cnt


def tlv_blob(bodies):
    """The bodies in one byte string with 0, 2, 4 or 6 bytes between them -- 2-byte aligned, not always 4 -- and their offsets."""
    parts, offs, base = [], [], 0
    for s, b in enumerate(bodies):
        lead = b"\x00" * (2 * ((s + 1) % 4))
        parts += [lead, b.tobytes()]
        offs.append(base + len(lead))
        base += len(lead) + b.nbytes
    return b"".join(parts), np.array(offs, np.int64)


def uart_packet(frame, body, n_obj, pad_to=32):
    """A UART packet around one detected-points TLV body (its first 4 + 12 n_obj bytes): magic word, the eight header words,
    the TLV head, padded to a multiple of 32 bytes as the sensor sends it (ReadDataIWR1443.py:85-113).  The header announces at
    least one object, so that a body with numObj = 0 is still decoded: the reference's dataOK = 1 with an empty detObj."""
    body = bytes(body[: 4 + 12 * n_obj])
    tlv = struct.pack("<II", 1, len(body)) + body
    total = (36 + len(tlv) + pad_to - 1) // pad_to * pad_to
    pkt = MAGIC + struct.pack("<IIIIIII", 0x01020304, total, 0xA1443, frame, 1, max(n_obj, 1), 1) + tlv
    return pkt + b"\x00" * (total - len(pkt))


# ------------------------------------------------------------------------------- the sensitivity argument, on expected outputs
def blocks_of(cfg_or_site, raw, n):
    """The expected output cut into what each 64-row block of the frame contributes."""
    raw = np.asarray(raw, np.float64).reshape(-1, 5)
    n = min(max(int(n), 0), len(raw))
    return [expected_rows(cfg_or_site, raw[b: min(b + 64, n)], min(b + 64, n) - b) for b in range(0, n, 64)]


def assemble(blocks, max_pts, order=None, shift=None, late=None):
    """What a compaction writes into a SENTINEL-filled pts[max_pts + 1, 8]: each block's rows at the running offset of the blocks
    before it in `order` (default: row order), block `shift[0]` moved by `shift[1]` rows; `late`: the block stored last (the
    stores of different blocks race).  -> (pts, n_out)."""
    order = list(range(len(blocks))) if order is None else list(order)
    out = np.full((max_pts + 1, 8), SENTINEL)
    offs, total = {}, 0
    for b in order:
        offs[b] = total
        total += len(blocks[b])
    if shift is not None:
        offs[shift[0]] += shift[1]
    for b in sorted(order, key=lambda b: b == late):
        lo = offs[b]
        rows = blocks[b]
        if lo < 0:
            rows, lo = rows[-lo:], 0
        out[lo: lo + len(rows)] = rows[: max(0, max_pts + 1 - lo)]
    return out, total
