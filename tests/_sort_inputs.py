"""Key frames for the 64-row sort of the feature maps (mmwave_msc_amd/csrc/mmw_sort.hpp), their reference, and a numpy model of
the network -- built on the CPU alone.  The one builder of tests/test_sort_inputs.py (which shows, without a GPU, that the frames
tell a wrong network from the right one) and tests/test_gpu_format_frames.py (which holds mmw_format_frames to the reference on
them, bit for bit).

The rule (include/mmw.h, mmw_format_frames): the 64 rows of a frame, zero pad rows included, ordered by the fp64 relative x as
np.argsort(kind="stable") orders them -- ties (-0.0 == 0.0) by row position, NaN behind everything else in row order.  Random
continuous x never ties, so the frames here do: a radar x is int16 / 2^Q and a person's fifty points share a handful of values.

Every real row carries a payload that names it (y = row + 1, z, doppler and intensity dyadic and distinct), so two rows of one
tie group exchanged change bytes; the rows of the buffer at and past a frame's count are junk no output may show.  Everything is
seeded, built once, cached and read-only."""
import functools
from typing import NamedTuple

import numpy as np

ROWS = 64
REF = (0.75, -1.25)                  # the (x, y) subtracted from an item's rows: key + 0.75 and back is exact for every key here
MU, STD = 12.5, 0.75                 # the intensity scale of the contexts (not the default one)

# (SZ, STRIDE) of the 21 compare-exchange steps, read off mmw_sort.hpp: bitonic_merge<2,1>, <4,2>, <8,4>, <16,8>, <32,16>, <64,32>,
# each going on with STRIDE / 2 down to 1
STEPS = tuple((sz, st) for sz in (2, 4, 8, 16, 32, 64) for st in (sz >> k for k in range(1, sz.bit_length())))
LAST_MERGE = tuple(i for i, (sz, _) in enumerate(STEPS) if sz == 64)


class KeyFrame(NamedTuple):
    tag: str
    keys: np.ndarray      # [min(count, 64)] fp64: the relative x of the real rows, in row order
    count: int            # what the caller passes: > 64 = the rows from 64 on are ignored, < 0 = the frame is absent

    @property
    def m(self):
        return max(0, min(int(self.count), ROWS))

    @property
    def zero_ref(self):
        """A key of -0.0 is x - ref_x only for ref_x == 0 (x - x is +0.0)."""
        return bool(np.any((self.keys == 0) & np.signbit(self.keys)))


def _kf(tag, keys, count=None):
    keys = np.asarray(keys, np.float64).copy()
    keys.setflags(write=False)
    kf = KeyFrame(tag, keys, len(keys) if count is None else int(count))
    assert kf.m == len(keys)
    return kf


ALPHABETS = {"pm1": (-1.0, 1.0), "halves": (-0.5, 0.0, 0.5), "zeros": (-0.0, 0.0, 0.25, -0.25),
             "eighths": tuple(k / 8.0 for k in range(-4, 5))}
SIZES = (0, 1, 2, 31, 32, 33, 63, 64)


@functools.lru_cache(maxsize=None)
def finite_frames():
    """The frames whose keys are not NaN: the reference order is the stable sort, and the network must give it."""
    rng = np.random.default_rng(20260)
    out = []
    for name, alpha in ALPHABETS.items():                  # real rows that tie with each other and (0.0, -0.0) with the pad rows
        for m in SIZES:
            out.append(_kf(f"{name} m={m}", rng.choice(np.array(alpha), size=m)))
    out.append(_kf("all equal 0.5", np.full(64, 0.5)))       # the identity permutation is required
    out.append(_kf("all equal -0.25 m=40", np.full(40, -0.25)))
    out.append(_kf("all zero m=40", np.zeros(40)))           # ... and among real rows and pad rows alike
    out.append(_kf("all -0.0 m=33", np.full(33, -0.0)))
    out.append(_kf("descending m=64", (32 - np.arange(64)) / 16.0))
    out.append(_kf("descending m=33", (16 - np.arange(33)) / 16.0))
    out.append(_kf("descending pairs m=64", (32 - np.arange(64) // 2) / 16.0))
    out.append(_kf("alternating m=64", np.where(np.arange(64) % 2 == 0, 0.5, -0.5)))
    out.append(_kf("alternating m=63", np.where(np.arange(63) % 2 == 0, -0.5, 0.5)))
    out.append(_kf("alternating with zero m=48", np.tile([0.25, 0.0, -0.25, 0.0], 12)))
    for m in (64, 32):                                       # b + 1 ulp before b, b descending: equal as fp32, not as fp64
        b = 1.25 - (np.arange(m // 2) + 1) / 256.0              # (below 1.25: b + REF[0] stays in [1, 2), where the ulp is b's)
        keys = np.stack([np.nextafter(b, np.inf), b], axis=1).reshape(-1)
        assert np.all(np.diff(keys) < 0) and np.array_equal(keys.astype(np.float32)[0::2], keys.astype(np.float32)[1::2])
        out.append(_kf(f"adjacent doubles m={m}", keys))
    out.append(_kf("inf among finite m=33", rng.choice(np.array([-np.inf, -1.0, 0.0, 1.0, np.inf]), size=33)))
    out.append(_kf("inf among finite m=64", rng.choice(np.array([-np.inf, -0.5, 0.5, np.inf]), size=64)))
    out.append(_kf("count 65", rng.choice(np.array(ALPHABETS["eighths"]), size=64), count=65))
    out.append(_kf("count 1000", rng.choice(np.array(ALPHABETS["halves"]), size=64), count=1000))
    out.append(_kf("count -1", np.zeros(0), count=-1))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def nan_frames():
    """Frames with NaN keys: the expectation is the reference's -- NaN rows last, behind +inf, in row order."""
    rng = np.random.default_rng(20261)
    nan = np.nan
    one = rng.choice(np.array(ALPHABETS["eighths"]), size=33)
    one[5] = nan
    several = rng.choice(np.array(ALPHABETS["halves"]), size=64)
    several[[0, 17, 18, 40, 63]] = nan
    beside = rng.choice(np.array([-1.0, 0.0, 1.0]), size=33)
    beside[[2, 30]] = nan
    beside[[1, 9, 31]] = np.inf                              # a +inf row before, between and behind the NaN rows
    both = rng.choice(np.array([-np.inf, 0.0, np.inf, nan]), size=64)
    both[[0, 63]] = nan, np.inf
    return (_kf("one NaN m=33", one), _kf("several NaN m=64", several), _kf("all NaN m=20", np.full(20, nan)),
            _kf("all NaN m=64", np.full(64, nan)), _kf("NaN beside +inf m=33", beside), _kf("NaN and both inf m=64", both),
            _kf("NaN in row 0 m=1", np.array([nan])))


# --------------------------------------------------------------------------------------------------------------- the buffers
def rows_of(kf, ref):
    """[64][8] fp64 as the caller uploads it: row r < m holds x = key + ref_x, y = ref_y + r + 1, z = (r + 1) / 8, doppler
    -(r + 1) / 4, intensity (r + 1) / 2; the rows from m on are junk (100 + r in every column)."""
    r = np.arange(ROWS, dtype=np.float64)
    out = np.repeat((100.0 + r)[:, None], 8, axis=1)
    m = kf.m
    out[:m, 0] = kf.keys + ref[0] if ref[0] != 0 else kf.keys        # (-0.0 + 0.0 is +0.0; -0.0 - 0.0 is -0.0)
    out[:m, 1] = ref[1] + r[:m] + 1
    out[:m, 2] = (r[:m] + 1) / 8
    out[:m, 3:6] = 0.5
    out[:m, 6] = -(r[:m] + 1) / 4
    out[:m, 7] = (r[:m] + 1) / 2
    return out


class Packed(NamedTuple):
    frames: np.ndarray    # [B][ring][64][8] fp64
    counts: np.ndarray    # [B][ring] int32
    ref: np.ndarray       # [B][2]
    src: tuple            # [B][ring] -> the KeyFrame (None: a frame added to fill the item, absent)
    ring: int


@functools.lru_cache(maxsize=None)
def pack(which, ring):
    """The frames of `which` ("finite" | "nan" | "all") as items of `ring` frames.  An item's frames share its ref: REF, or
    (0, REF[1]) for the items of the frames that hold a -0.0 key.  An item that is not full ends in absent frames (count -1), and
    one more item is added where B * ring would be a multiple of 4 (the kernel's workgroup is four frames)."""
    kfs = {"finite": finite_frames(), "nan": nan_frames(), "all": finite_frames() + nan_frames()}[which]
    items = []
    for zero in (False, True):
        group = [kf for kf in kfs if kf.zero_ref == zero]
        for i in range(0, len(group), ring):
            chunk = group[i: i + ring]
            items.append(((0.0 if zero else REF[0], REF[1]), chunk + [None] * (ring - len(chunk))))
    if (len(items) * ring) % 4 == 0:
        items.append((REF, [kfs[1]] + [None] * (ring - 1)))
    B = len(items)
    assert (B * ring) % 4 != 0
    frames, counts, ref = np.empty((B, ring, ROWS, 8)), np.empty((B, ring), np.int32), np.array([it[0] for it in items])
    for b, (rf, chunk) in enumerate(items):
        for k, kf in enumerate(chunk):
            kf = kf if kf is not None else _kf("absent", np.zeros(0), count=-1)
            frames[b, k], counts[b, k] = rows_of(kf, rf), kf.count
    for a in (frames, counts, ref):
        a.setflags(write=False)
    return Packed(frames, counts, ref, tuple(tuple(it[1]) for it in items), ring)


# -------------------------------------------------------------------------------------------------------------- the reference
def format_frames_ref(frames, counts, ref, mu, std, ring):
    """mmw_format_frames in plain numpy fp64 -> [B][ring][64][5] float32.  m = min(count, 64) rows of a frame are real (a negative
    count: the frame is absent, all zeros): (x - ref_x, y - ref_y, z, doppler, ((I - 0) - mu) / std); the others are zero pad
    rows; the 64 rows ordered by np.argsort(kind="stable") on the fp64 relative x; ONE rounding to float32 at the end."""
    frames = np.asarray(frames, np.float64).reshape(-1, ring, ROWS, 8)
    counts = np.asarray(counts).reshape(-1, ring)
    ref = np.asarray(ref, np.float64).reshape(-1, 2)
    out = np.zeros((len(frames), ring, ROWS, 5), np.float32)
    for b in range(len(frames)):
        for k in range(ring):
            m = max(0, min(int(counts[b, k]), ROWS))
            rows = np.zeros((ROWS, 5))
            p = frames[b, k, :m]
            with np.errstate(invalid="ignore"):
                rows[:m, 0] = p[:, 0] - ref[b, 0]
                rows[:m, 1] = p[:, 1] - ref[b, 1]
                rows[:m, 2] = p[:, 2] - 0
                rows[:m, 3] = p[:, 6] - 0
                rows[:m, 4] = ((p[:, 7] - 0) - mu) / std
            with np.errstate(over="ignore"):
                out[b, k] = rows[np.argsort(rows[:, 0], kind="stable")].astype(np.float32)
    return out


def keys64(kf):
    """The 64 keys the sort sees: the real rows' and the pad rows' zeros."""
    k = np.zeros(ROWS)
    k[: kf.m] = kf.keys
    return k


def reference_order(kf):
    return np.argsort(keys64(kf), kind="stable")


def rows5(kf):
    """The frame's 64 x 5 values in ROW order (no sort), float32: the real rows relative to the frame's ref, the pad rows zero."""
    rf = (0.0 if kf.zero_ref else REF[0], REF[1])
    p, m = rows_of(kf, rf), kf.m
    rows = np.zeros((ROWS, 5))
    with np.errstate(invalid="ignore"):
        rows[:m, 0], rows[:m, 1], rows[:m, 2], rows[:m, 3] = p[:m, 0] - rf[0], p[:m, 1] - rf[1], p[:m, 2], p[:m, 6]
        rows[:m, 4] = (p[:m, 7] - MU) / STD
    return rows.astype(np.float32)


def gathered(kf, order):
    """The frame's output, as uint32, when output row r is input row order[r]."""
    return rows5(kf)[np.asarray(order)].view(np.uint32)


# ------------------------------------------------------------------------------------------------------- the network's model
def network(keys, tags=None, drop=None, reverse=(), tie_larger=False, key32=False):
    """bitonic_step over STEPS on 64 (key, tag) pairs, lane by lane as the wave runs it -> the tags after the last step.
    The wrong rules: `drop` = a step left out, `reverse` = steps whose direction is turned round, tie_larger = ties to the LARGER
    tag, key32 = the comparison on the key rounded to float32."""
    key = np.asarray(keys, np.float64).copy()
    if key32:
        key = key.astype(np.float32).astype(np.float64)
    src = np.arange(ROWS) if tags is None else np.asarray(tags).copy()
    lane = np.arange(ROWS)
    for i, (sz, st) in enumerate(STEPS):
        if i == drop:
            continue
        ok, os_ = key[lane ^ st], src[lane ^ st]
        up, lower = (lane & sz) == 0, (lane & st) == 0
        if i in reverse:
            up = ~up
        with np.errstate(invalid="ignore"):
            other_less = (ok < key) | ((ok == key) & ((os_ > src) if tie_larger else (os_ < src)))
        take = np.where(up == lower, other_less, ~other_less)
        key, src = np.where(take, ok, key), np.where(take, os_, src)
    return src


def network_nan_last(keys, **kw):
    """sort_rows_store_nan_last: a NaN key sorts as +inf with bit 6 of its row set; the bit is masked off afterwards."""
    keys = np.asarray(keys, np.float64)
    nan = np.isnan(keys)
    return network(np.where(nan, np.inf, keys), tags=np.arange(ROWS) | np.where(nan, 64, 0), **kw) & 63
