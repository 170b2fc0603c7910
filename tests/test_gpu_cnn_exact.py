"""The CNN's matrix kernels bit for bit, through the C entries, on exactly summable operands (tests/_exact_operands.py; their
properties are asserted without a GPU in tests/test_exact_operands.py): every partial product is exact in fp32 and every sum is
exact in every order, so a GPU result that is not bit-equal to the fp64 reference is a bug, and where it differs names the tile,
the K-step or the tap.

Dense-1 (mmw_mars_dense1_split, csrc/k_dense.hip): each of the three instantiations of k_mars_dense1_t at KT = K / 32 of 1 to 5
and 8 (every prologue arm, every tail stretch), at the models' own K, with grids whose size is and is not a multiple of 8 (the
XCD-aware tile permutation), a plan of two launches, and leading dimensions with a sentinel behind the operands.  The rows come
from mmw_mars_dense1_plan -- the plan the launcher runs -- searched on the host; no row count assumes a CU count.
Convolutions (mmw_mars_conv3d, mmw_mars_conv2d, mmw_mars_conv_split): both forms of the fp32 3-D kernel and batches that make
every persistent sample loop go round.  Dense-2 and the small head: the wave-tile and workgroup seams, short K, padded rows."""
import ctypes as C

import numpy as np
import pytest

from tests import _exact_operands as xo

pytestmark = pytest.mark.gpu

FILL = -7.0     # what output buffers hold before a launch: no ReLU output, and no exact result of these cases


def _lib():
    from mmwave_msc_amd import _lib
    return _lib.load()


def _stream():
    import torch
    return torch.cuda.current_stream("cuda:0").cuda_stream


def _dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype))).to("cuda:0")


def _f32(a):
    """fp64 -> fp32, which the any-order condition makes exact."""
    b = a.astype(np.float32)
    assert np.array_equal(b.astype(np.float64), a)
    return b


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got.view(np.int32), want.view(np.int32)):
        bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
        first = [(tuple(int(i) for i in p), float(got[tuple(p)]), float(want[tuple(p)])) for p in bad[:6]]
        raise AssertionError(f"{what}: {len(bad)} of {got.size} values differ; first (index, got, want): {first}; "
                             f"index ranges {bad.min(axis=0).tolist()} .. {bad.max(axis=0).tolist()}")


def _ok(rc, L):
    assert rc == 0, (rc, (L.mmw_last_error(None) or b"").decode())


# ---------------------------------------------------------------- Dense-1 ----------------------------------------------------
INST = {"256x192": 0, "256x128": 1, "128x128": 2}


def _plan(L, rows, n):
    out = (C.c_int32 * 4)()
    _ok(L.mmw_mars_dense1_plan(rows, n, out), L)
    p = tuple(int(v) for v in out)
    assert p[0] + p[1] + p[2] == rows // 256 and (p[0] == 0 or p[1] == 0) and p[3] > 0 and (p[0] == 0 or n % 192 == 0)
    return p


def _grids(p, n):
    """workgroups of the (up to three) launches of plan p."""
    return {"256x192": p[0] * (n // 192), "256x128": p[1] * (n // 128), "128x128": 2 * p[2] * (n // 128)}


def _find(L, n, pred):
    """The smallest number of bands in 1 .. 400 whose plan satisfies pred(plan, grids)."""
    for bands in range(1, 401):
        p = _plan(L, bands * 256, n)
        if pred(p, _grids(p, n)):
            return bands, p
    return None, None


def _ref32(c):
    if not hasattr(c, "ref32"):
        c.ref32 = _f32(xo.dense1_ref(c))
    return c.ref32


def _run_dense1(L, c, bands, lda=None, ldw=None, cut=57):
    """c's base rows laid out over `bands` bands (tests/_exact_operands.band_rows), the last `cut` rows past the batch: SENTINEL
    in them and behind every row's 2 K values; the batch's output against the gathered fp64 product, bit for bit."""
    import torch
    K, N = c.K, c.N
    lda, ldw = lda or 2 * K, ldw or 2 * K
    rows = bands * 256
    batch = rows - cut
    idx = xo.band_rows(bands)
    a2 = _dev(xo.interleave(c.ah, c.al, lda))[_dev(idx)]
    a2[batch:] = xo.SENTINEL
    w2 = _dev(xo.interleave(c.wh, c.wl, ldw))
    bias = _dev(c.bias, np.float32)
    out = torch.full((rows, N), FILL, dtype=torch.float32, device="cuda:0")
    assert a2.shape == (rows, lda) and a2.is_contiguous() and w2.shape == (N, ldw) and a2.dtype == torch.float16
    _ok(L.mmw_mars_dense1_split(_stream(), a2.data_ptr(), lda, w2.data_ptr(), ldw, bias.data_ptr(), out.data_ptr(), rows, K, N), L)
    torch.cuda.synchronize()
    got = out[:batch].cpu().numpy()
    _same_bits(got, _ref32(c)[idx[:batch]], f"{c.name} bands={bands} lda={lda} ldw={ldw} plan={_plan(L, rows, N)}")


@pytest.mark.parametrize("K", xo.SHORT_K)
@pytest.mark.parametrize("inst", list(INST))
def test_dense1_short_k_on_every_instantiation(inst, K):
    """KT = 1, 2, 3, 4, 5 and 8 on each of <256, 2, 3, 2> (256 x 192), <256, 2, 2, 3> (256 x 128) and <128, 4, 1, 3> (half tiles):
    the prologue's KT > 1 and KT > 2 arms with their counted waits and the (T,T,F), (T,F,F), (F,F,F) tail stretches; families A
    (lo'.W_hi), B (hi.W_lo') and, at KT = 5, the mixed one."""
    L = _lib()
    N = xo.INST_N[inst]
    bands, p = _find(L, N, lambda p, g: p[INST[inst]] >= 1)
    assert bands is not None and p[INST[inst]] >= 1 and _grids(p, N)[inst] >= 1, (inst, N, p)     # the plan relied on is the plan reported
    for family in "AB" + ("M" if K == 160 else ""):
        _run_dense1(L, xo.dense1_case(family, K, N), bands)


@pytest.mark.parametrize("rem", [0, 1, 3, 7])
def test_dense1_tile_permutation_with_any_grid_remainder(rem):
    """t = f(blockIdx, gridDim) with r8 = nwg & 7: grids of the 256 x 128 instantiation with nwg % 8 of 0, 1, 3 and 7 (the half
    tiles' smallest grid adds 2): every tile computed exactly once, from its own band and feature block."""
    L = _lib()
    found = None
    for N in (128, 256):
        bands, p = _find(L, N, lambda p, g: p[1] >= 1 and g["256x128"] % 8 == rem)
        if bands is not None and (found is None or bands * N < found[0] * found[1]):
            found = (bands, N, p)
    assert found is not None, rem
    bands, N, p = found
    assert _grids(p, N)["256x128"] % 8 == rem and _grids(p, N)["256x128"] > 8
    _run_dense1(L, xo.dense1_case("A", 96, N), bands)


def test_dense1_half_tile_grid_remainder_is_not_zero_at_one_band():
    L = _lib()
    p = _plan(L, 256, 128)
    assert p[:3] == (0, 0, 1) and _grids(p, 128)["128x128"] % 8 == 2


def test_dense1_two_launches_in_one_call():
    """A main part of 256-row tiles and a tail of half tiles with row0 > 0, in one call."""
    L = _lib()
    found = None
    for N in (128, 256, 384):
        bands, p = _find(L, N, lambda p, g: p[0] + p[1] >= 1 and p[2] >= 1)
        if bands is not None and (found is None or bands * N < found[0] * found[1]):
            found = (bands, N, p)
    assert found is not None
    bands, N, p = found
    assert p[0] + p[1] >= 1 and p[2] >= 1 and sum(g > 0 for g in _grids(p, N).values()) == 2
    for family in "AB":
        _run_dense1(L, xo.dense1_case(family, 64, N), bands)


@pytest.mark.parametrize("inst,K", [("128x128", 64), ("256x192", 160), ("256x128", 32)])
def test_dense1_leading_dimensions_beyond_2k(inst, K):
    """lda > 2 K and ldw > 2 K, SENTINEL between the rows: a K-step or a row addressed with 2 K for the stride reads it."""
    L = _lib()
    N = xo.INST_N[inst]
    bands, p = _find(L, N, lambda p, g: p[INST[inst]] >= 1)
    assert bands is not None and p[INST[inst]] >= 1
    _run_dense1(L, xo.dense1_case("M" if K == 160 else "A", K, N), bands, lda=2 * K + 24, ldw=2 * K + 40)


@pytest.mark.parametrize("K,N,inst", [(6144, 1536, "256x192"), (6144, 1536, "128x128"), (2048, 512, "256x128"), (2048, 512, "128x128")])
def test_dense1_at_the_models_own_k(K, N, inst):
    """define_CNN_3D's 6144 -> 1536 and define_CNN's 2048 -> 512 (KT = 192 and 64) with the activation stride the models use
    (2 K + 256), on every instantiation their feature counts can reach; ranges shrunk until the any-order condition holds."""
    L = _lib()
    bands, p = _find(L, N, lambda p, g: p[INST[inst]] >= 1)
    assert bands is not None and p[INST[inst]] >= 1 and bands * 256 * (2 * K + 256) * 2 <= 110 << 20, (bands, p)
    for family in "AB":
        _run_dense1(L, xo.dense1_case(family, K, N), bands, lda=2 * K + 256)


def test_dense1_plan_entry_refuses_bad_shapes_and_sums_to_the_bands():
    L = _lib()
    out = (C.c_int32 * 4)()
    from mmwave_msc_amd import _lib as lib
    assert L.mmw_mars_dense1_plan(255, 128, out) == lib.E_ARG and L.mmw_mars_dense1_plan(256, 100, out) == lib.E_ARG
    assert L.mmw_mars_dense1_plan(256, 128, None) == lib.E_ARG
    for n in (128, 256, 384, 512, 1536):
        for bands in (1, 11, 33, 65, 124, 400):
            p = _plan(L, bands * 256, n)          # (asserts that the three counts are the bands and that N picks the main instantiation)
            assert all(v >= 0 for v in p) and (p[2] == 0 or 2 * p[2] * (n // 128) <= p[3] or p[0] + p[1] == 0), (n, bands, p)


# ---------------------------------------------------------------- convolutions -----------------------------------------------
def _n_cu(L):
    return _plan(L, 256, 128)[3]


def _conv_operands(c, n):
    return (_dev(_f32(c.x[:n])), _dev(_f32(c.w1).reshape(-1)), _dev(_f32(c.b1)), _dev(_f32(c.w2).reshape(-1)), _dev(_f32(c.b2)))


def _run_conv_f32(L, entry, c, n):
    import torch
    flat = c.out[0].size
    x, w1, b1, w2, b2 = _conv_operands(c, n)
    out = torch.full((n + 2, flat), FILL, dtype=torch.float32, device="cuda:0")
    _ok(getattr(L, entry)(_stream(), x.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), out.data_ptr(), n), L)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    _same_bits(got[:n], _f32(c.out[:n].reshape(n, flat)), f"{entry} {c.name} n={n}")
    assert np.all(got[n:] == FILL)                                   # rows past n are not written


def _run_conv_split(L, c, n):
    import torch
    from mmwave_msc_amd.mars import SPLIT_SCALE, deinterleave_split
    flat = c.out[0].size
    ld = 2 * flat + 256
    rows = (n + 255) // 256 * 256
    x, w1, b1, w2, b2 = _conv_operands(c, n)
    out16 = torch.full((rows, ld), xo.SENTINEL, dtype=torch.float16, device="cuda:0")
    flags = torch.zeros(1 + 2 + 64, dtype=torch.int32, device="cuda:0")     # [0] the range word, [1 ..] the fix-up list
    _ok(L.mmw_mars_conv_split(_stream(), c.frames, x.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), out16.data_ptr(),
                              ld, n, flags.data_ptr(), flags.data_ptr() + 4), L)
    torch.cuda.synchronize()
    hi, lo = deinterleave_split(out16[:n, :2 * flat].contiguous())
    rec = hi.double().cpu().numpy() + lo.double().cpu().numpy() / SPLIT_SCALE
    _same_bits(_f32(rec), _f32(xo.conv_out16_expected(c, n)), f"mmw_mars_conv_split {c.name} n={n}")
    assert np.array_equal(rec, xo.conv_out16_expected(c, n))
    assert int(flags[0]) == 0 and int(flags[1]) == 0                  # range_flag == 0, no sample listed
    rest = out16.cpu().numpy()
    assert np.all(rest[:n, 2 * flat:] == np.float16(xo.SENTINEL)) and np.all(rest[n:] == np.float16(xo.SENTINEL))


@pytest.mark.parametrize("n", [61, 513 + 7])
@pytest.mark.parametrize("family", "ABC")
def test_conv3d_fp32_both_forms(family, n):
    """k_mars_conv<3> (three workgroups per sample, at most 64 samples) and k_mars_conv<1> (grid 512: 520 samples make
    `b += gridDim.x` run under a comparison)."""
    L = _lib()
    assert n <= 64 or n > 512
    _run_conv_f32(L, "mmw_mars_conv3d", xo.conv_case(family, 3, xo.conv_batch(_n_cu(L))), n)


@pytest.mark.parametrize("n", [3, 1024 + 9])
@pytest.mark.parametrize("family", "ABC")
def test_conv2d_fp32_small_and_looping(family, n):
    """k_mars_conv2d: grid of at most 1024 workgroups, 1033 samples make its persistent loop go round."""
    L = _lib()
    _run_conv_f32(L, "mmw_mars_conv2d", xo.conv_case(family, 1, xo.conv_batch(_n_cu(L))), n)


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("frames", [3, 1])
@pytest.mark.parametrize("family", "ABC")
def test_conv_split_recompletes_to_the_fp64_convolution(family, frames, big):
    """k_mars_conv16<3> and <1>: hi + lo' / 2^11 of the split output, de-interleaved as mars.deinterleave_split does, IS the fp64
    convolution; batch 5 and batch 4 n_cu + 5 (a grid of n_cu workgroups x 4 sample-waves: every wave's loop goes round, the
    last five samples on a second pass of workgroups 0 and 1)."""
    L = _lib()
    n_cu = _n_cu(L)
    n = 4 * n_cu + 5 if big else 5
    c = xo.conv_case(family, frames, xo.conv_batch(n_cu))
    assert c.x.shape[0] >= n
    _run_conv_split(L, c, n)


@pytest.mark.parametrize("frames", [3, 1])
def test_conv_impulses_on_every_face_edge_and_corner(frames):
    """One-hot inputs against dyadic weights through every convolution kernel that serves the model: a mismatch is a single tap."""
    L = _lib()
    c = xo.conv_case("I", frames)
    n = c.x.shape[0]
    if frames == 3:
        _run_conv_f32(L, "mmw_mars_conv3d", c, n)        # k_mars_conv<1>
        _run_conv_f32(L, "mmw_mars_conv3d", c, 64)       # k_mars_conv<3>
    else:
        _run_conv_f32(L, "mmw_mars_conv2d", c, n)
    _run_conv_split(L, c, n)


# ---------------------------------------------------------------- Dense-2 and the small head ---------------------------------
@pytest.mark.parametrize("pad", [0, 12])
@pytest.mark.parametrize("K", xo.DENSE2_K)
def test_dense2_seams_short_k_and_padded_rows(K, pad):
    """mmw_mars_dense2: K of both models, one chunk of 32, a chunk plus a 4-wide remainder, two chunks; n_rows around the 32-row
    wave tile and the 128-row workgroup; ldh > k with SENTINEL in the padding; the 7 pad columns of the 64-wide tile and the rows
    past n_rows do not leak into the buffer behind kp."""
    import torch
    L = _lib()
    c = xo.dense2_case(K)
    ldh = K + pad
    hid = np.full((xo.DENSE2_ROWS, ldh), xo.SENTINEL, dtype=np.float32)
    hid[:, :K] = _f32(c.hidden)
    hidden, w, bias = _dev(hid), _dev(_f32(c.w)), _dev(_f32(c.bias))
    want = _f32(c.out)
    for n_rows in (1, 31, 32, 33, 127, 128, 129, 257):
        kp = torch.full((n_rows * 57 + 256,), FILL, dtype=torch.float32, device="cuda:0")
        _ok(L.mmw_mars_dense2(_stream(), hidden.data_ptr(), ldh, w.data_ptr(), bias.data_ptr(), kp.data_ptr(), n_rows, K), L)
        torch.cuda.synchronize()
        got = kp.cpu().numpy()
        _same_bits(got[:n_rows * 57].reshape(n_rows, 57), want[:n_rows], f"mmw_mars_dense2 K={K} ldh={ldh} n_rows={n_rows}")
        assert np.all(got[n_rows * 57:] == FILL), (K, n_rows)


@pytest.mark.parametrize("n_rows", [1, 3, 5, 64])
def test_head_small_row_templates(n_rows):
    """mmw_mars_head_small: the 2-, 4- and 8-row forms of its Dense-1 and its wave-per-output Dense-2, padded leading dimensions."""
    import torch
    L = _lib()
    c = xo.head_case()
    lda, ldw = c.K + 8, c.K + 4
    act = np.full((n_rows, lda), xo.SENTINEL, dtype=np.float32)
    act[:, :c.K] = _f32(c.act[:n_rows])
    w1 = np.full((c.N1, ldw), xo.SENTINEL, dtype=np.float32)
    w1[:, :c.K] = _f32(c.w1)
    d = [_dev(v) for v in (act, w1, _f32(c.b1), _f32(c.w2), _f32(c.b2))]
    hidden = torch.full((n_rows * c.N1 + 64,), FILL, dtype=torch.float32, device="cuda:0")
    kp = torch.full((n_rows * 57 + 64,), FILL, dtype=torch.float32, device="cuda:0")
    _ok(L.mmw_mars_head_small(_stream(), d[0].data_ptr(), lda, d[1].data_ptr(), ldw, d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
                              hidden.data_ptr(), kp.data_ptr(), n_rows, c.K, c.N1), L)
    torch.cuda.synchronize()
    h, k = hidden.cpu().numpy(), kp.cpu().numpy()
    _same_bits(h[:n_rows * c.N1].reshape(n_rows, c.N1), _f32(c.hidden[:n_rows]), f"head Dense-1 n_rows={n_rows}")
    _same_bits(k[:n_rows * 57].reshape(n_rows, 57), _f32(c.out[:n_rows]), f"head Dense-2 n_rows={n_rows}")
    assert np.all(h[n_rows * c.N1:] == FILL) and np.all(k[n_rows * 57:] == FILL)
