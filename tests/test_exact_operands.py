"""The operands of tests/test_gpu_cnn_exact.py (tests/_exact_operands.py) have the properties that let that file ask for bit
equality -- asserted here from the fp64 operands alone, without a GPU:

  * the any-order condition per output element and per case (per layer for the convolutions, the intermediate activation
    included): every term a multiple of a quantum q, sum |terms| < 2^24 q -- so every partial sum in every order is an fp32 number;
  * the operand rules: fp16 halves zero or normal, at most 22 significant bits where a kernel splits a value itself, lo'.lo' zero
    term by term, about a third zeros, both signs in every K-step, every row / sample distinct, ReLU clips some and keeps some;
  * sensitivity: the fp64 reference under each of a list of wrong rules (a dropped correction term in one K-step, a skipped or
    repeated K-step, exchanged feature blocks or rows; a shifted tap, wrap-around padding, exchanged channels or frames, a sample
    taken from another) differs from the right one in EVERY tile (Dense-1) or EVERY sample (convolutions).  A case that a wrong
    rule leaves unchanged anywhere is not a probe and fails here."""
import numpy as np
import pytest

from oracle.mars_np import _conv_same
from tests import _exact_operands as xo


def _distinct_rows(a):
    a = np.ascontiguousarray(a.reshape(a.shape[0], -1))
    return len(np.unique(a, axis=0)) == a.shape[0]


def _fp32_exact(v):
    return bool(np.all(v.astype(np.float32).astype(np.float64) == v))


@pytest.mark.parametrize("family,K,N", xo.dense1_case_keys())
def test_dense1_case_is_any_order_exact_and_a_probe(family, K, N):
    c = xo.dense1_case(family, K, N)
    KT = K // 32
    sa, sw = c.quanta
    # ---- operand rules ----
    for v, q in ((c.ah, sa), (c.al, sa), (c.wh, sw), (c.wl, sw)):
        assert xo.f16_exact_and_normal(v) and xo.multiple_of(v, q), c.name
    assert xo.multiple_of(c.bias, sa * sw) and c.q == sa * sw / xo.SPLIT
    for v in (c.ah, c.wh) + ((c.al,) if family == "A" else ()) + ((c.wl,) if family == "B" else ()):
        assert 0.28 < float((v == 0).mean()) < 0.39, c.name
        steps = v.reshape(v.shape[0], KT, 32)
        assert (steps > 0).any(axis=(0, 2)).all() and (steps < 0).any(axis=(0, 2)).all(), c.name      # both signs in every K-step
    lo_a, lo_w = (c.al != 0).any(axis=0), (c.wl != 0).any(axis=0)
    assert not (lo_a & lo_w).any(), c.name                                                          # lo'.lo' is zero term by term
    assert lo_a.any() == (family in "AM") and lo_w.any() == (family in "BM")
    if family == "M":
        assert (c.ah @ c.wl.T != 0).any() and (c.al @ c.wh.T != 0).any()
    assert _distinct_rows(np.concatenate([c.ah, c.al], axis=1)) and _distinct_rows(np.concatenate([c.wh, c.wl], axis=1))
    # ---- the any-order condition, per output element ----
    s = xo.dense1_abs_sum(c)
    assert s.shape == (xo.BASE_ROWS, N) and float(s.max()) < xo.TWO24 * c.q, (c.name, float(s.max()) / (xo.TWO24 * c.q))
    ref = xo.dense1_ref(c)
    assert _fp32_exact(ref) and _distinct_rows(ref)
    clipped = float((ref == 0).mean())
    assert 0.2 < clipped < 0.8, (c.name, clipped)
    # ---- sensitivity ----
    rules = xo.dense1_wrong_rules(c)
    want = {"skip K-step KT - 1", "exchange 32-column feature blocks c and c ^ 1", "exchange rows r and r ^ 32"}
    want |= {"drop lo'.W_hi in the last K-step"} if family in "AM" else set()
    want |= {"drop hi.W_lo' in the first K-step"} if family in "BM" else set()
    want |= {"swap the lo' halves of K-steps 0 and KT - 1", "use K-step KT - 2 twice"} if KT >= 2 else set()
    assert set(rules) == want, c.name
    for name, wrong in rules.items():
        assert xo.every_block_differs(ref, wrong), (c.name, name)


def test_band_rows_put_whole_blocks_of_distinct_base_rows_into_every_tile():
    idx = xo.band_rows(400)
    assert idx.shape == (400 * 256,) and idx.min() == 0 and idx.max() == xo.BASE_ROWS - 1
    for b in (0, 1, 7, 399):
        for half in (0, 1):                      # a 128-row half tile: 128 consecutive base rows (mod 512) = at least three aligned 32-row groups
            rows = idx[b * 256 + half * 128: b * 256 + half * 128 + 128]
            assert len(set(rows.tolist())) == 128
            whole = [g for g in range(xo.BASE_ROWS // 32) if set(range(32 * g, 32 * g + 32)) <= set(rows.tolist())]
            assert len(whole) >= 3
    assert len({tuple(idx[b * 256: b * 256 + 4]) for b in range(400)}) > 256     # bands differ: a tile computed from another band shows


def test_interleave_is_the_kernels_layout_with_the_sentinel_behind_it():
    hi = np.arange(2 * 64, dtype=np.float64).reshape(2, 64)
    lo = -hi
    a = xo.interleave(hi, lo, 2 * 64 + 24).astype(np.float64)
    assert np.array_equal(a[:, :32], hi[:, :32]) and np.array_equal(a[:, 32:64], lo[:, :32]) and np.array_equal(a[:, 64:96], hi[:, 32:])
    assert np.all(a[:, 128:] == xo.SENTINEL) and xo.f16_exact_and_normal([xo.SENTINEL])
    assert not xo.multiple_of([xo.SENTINEL], 2.0 ** -3) and xo.SENTINEL > 7 * 0.25     # no operand: finer than their quanta, larger than any hi


def _check_layer(c, x, w, b, q, where):
    """One convolution layer of a case: operand rules of the split form and the any-order condition on every output element."""
    xh, xl = xo.natural_split(x)
    wh, wl = xo.natural_split(w)
    assert np.array_equal(xh + xl / xo.SPLIT, x) and np.array_equal(wh + wl / xo.SPLIT, w), (c.name, where)   # <= 22 bits: the split is exact
    for v in (xh, xl, wh, wl, xo.natural_split(b)[0]):
        assert xo.f16_exact_and_normal(v), (c.name, where)
    assert not xl.any() or not wl.any(), (c.name, where)               # one factor of every product has lo' = 0
    assert xo.multiple_of(b, q), (c.name, where)
    bound = xo.conv_abs_bound(x, w, b)
    assert float(bound.max()) < xo.TWO24 * q, (c.name, where, float(bound.max()) / (xo.TWO24 * q))
    return bool(xl.any()), bool(wl.any())


@pytest.mark.parametrize("family,frames", xo.CONV_KEYS)
def test_conv_case_is_any_order_exact_and_a_probe(family, frames):
    c = xo.conv_case(family, frames)
    n = c.x.shape[0]
    assert n == xo.conv_batch() >= 4 * xo.NOMINAL_CU + 5
    # every product of quanta is a multiple of the layer's q (operands are integers times the quanta below)
    qx1, qw1 = {"A": (2.0 ** -10, 1.0), "B": (1.0, 2.0 ** -12), "C": (1.0, 1.0)}[family]
    assert xo.multiple_of(c.x, qx1) and xo.multiple_of(c.w1, qw1) and qx1 * qw1 == c.q1
    qw2 = c.q2 / c.q1
    assert xo.multiple_of(c.h1, c.q1) and xo.multiple_of(c.w2, qw2)
    lo1 = _check_layer(c, c.x, c.w1, c.b1, c.q1, "conv1")
    lo2 = _check_layer(c, c.h1, c.w2, c.b2, c.q2, "conv2")
    assert (lo1, lo2) == {"A": ((True, False), (True, False)), "B": ((False, True), (True, False)), "C": ((False, False), (False, True))}[family]
    oh, ol = xo.natural_split(c.out)
    assert np.array_equal(oh + ol / xo.SPLIT, c.out) and xo.f16_exact_and_normal(oh) and xo.f16_exact_and_normal(ol)   # the split output is exact
    assert float(np.abs(c.out).max()) < 65504.0 and float(np.abs(c.h1).max()) < 65504.0 and _fp32_exact(c.out) and _fp32_exact(c.h1)
    if family == "C":
        assert float(np.abs(c.h1).max()) < 2048 and xo.multiple_of(c.h1, 1.0)
    # zeros, signs, ReLU on both layers
    zero_x = float((c.x == 0).mean())
    assert (0.75 < zero_x < 0.85) if family == "C" else (0.28 < zero_x < 0.39)
    for w in (c.w1, c.w2):     # both signs in every tap (a K-step of the kernels is one tap or four) and for every output channel
        flat_w = w.reshape(-1, w.shape[-2], w.shape[-1])
        assert 0.2 < float((w == 0).mean()) < 0.45
        assert (flat_w > 0).any(axis=(1, 2)).all() and (flat_w < 0).any(axis=(1, 2)).all()
        assert (flat_w > 0).any(axis=(0, 1)).all() and (flat_w < 0).any(axis=(0, 1)).all()
    for act in (c.h1, c.out):
        z = (act.reshape(n, -1) == 0).mean(axis=1)
        assert 0.1 < float(z.min()) and float(z.max()) < 0.9, (c.name, float(z.min()), float(z.max()))          # in every sample
    # every sample distinct, in and out: a sample computed from sample b - grid, for any grid, shows
    assert _distinct_rows(c.x) and _distinct_rows(c.h1) and _distinct_rows(c.out)
    # ---- sensitivity: second layer on the final output, first layer on the intermediate activation of every sample and, for
    #      the first eight, carried through the second layer ----
    names = []
    for name, wrong in xo.conv_layer_rules(c.h1, c.w2, c.b2):
        assert xo.per_sample_changed(c.out, xo.relu(wrong)).all(), (c.name, "conv2", name)
        names.append(name)
    for name, wrong in xo.conv_layer_rules(c.x, c.w1, c.b1):
        h_wrong = xo.relu(wrong)
        assert xo.per_sample_changed(c.h1, h_wrong).all(), (c.name, "conv1", name)
        assert xo.per_sample_changed(c.out[:8], xo.relu(_conv_same(h_wrong[:8], c.w2, c.b2))).all(), (c.name, "conv1 -> out", name)
    taps = 27 if frames == 3 else 9
    assert len(names) == taps + 2 * (3 if frames == 3 else 2) + 1 + (2 if frames == 3 else 0)


@pytest.mark.parametrize("frames", [3, 1])
def test_impulse_case_touches_every_face_edge_and_corner(frames):
    c = xo.conv_case("I", frames)
    n = c.x.shape[0]
    flat = c.x.reshape(n, -1)
    assert ((flat != 0).sum(axis=1) == 1).all() and _distinct_rows(c.x) and _distinct_rows(c.out)
    pos = np.argwhere(c.x != 0)[:, 1:-1]
    dims = c.x.shape[1:-1]
    on_low, on_high = pos == 0, pos == np.array(dims) - 1
    for ax in range(len(dims)):
        assert on_low[:, ax].any() and on_high[:, ax].any()
    assert ((on_low | on_high).sum(axis=1) == len(dims)).any() and ((on_low | on_high).sum(axis=1) == 0).any()   # corners and the inside
    for w in (c.w1, c.w2):                      # dyadic weights, none zero: every tap shows
        m, _ = np.frexp(np.abs(w))
        assert np.all(m == 0.5)
    _check_layer(c, c.x, c.w1, c.b1, c.q1, "conv1")
    _check_layer(c, c.h1, c.w2, c.b2, c.q2, "conv2")
    assert _fp32_exact(c.out) and (c.out != 0).reshape(n, -1).any(axis=1).all()
    assert n > 64 and (frames == 1 or n <= 512)


@pytest.mark.parametrize("K", xo.DENSE2_K)
def test_dense2_case_is_any_order_exact(K):
    c = xo.dense2_case(K)
    assert xo.multiple_of(c.hidden[:, None, :1] * c.w[None, :, :1], c.q) and xo.multiple_of(c.bias, c.q)
    assert xo.multiple_of(c.hidden, 2.0 ** -4) and xo.multiple_of(c.w, 2.0 ** -2) and 2.0 ** -6 == c.q
    assert float(c.abs_sum.max()) < xo.TWO24 * c.q and _fp32_exact(c.out) and _fp32_exact(c.hidden) and _fp32_exact(c.w)
    assert _distinct_rows(c.hidden) and _distinct_rows(c.out) and _distinct_rows(c.out.T)
    # a column taken from its neighbour or a row from the row 32 or 128 further shows in every row; the last float4 of K dropped shows
    # in every row that has a value there
    assert (c.out[:, 1:] != c.out[:, :-1]).any(axis=1).all()
    assert (c.out[32:] != c.out[:-32]).any(axis=1).all() and (c.out[128:] != c.out[:-128]).any(axis=1).all()
    tail = c.hidden[:, -4:].any(axis=1)
    assert tail.mean() > 0.9 and ((c.out - c.hidden[:, -4:] @ c.w[:, -4:].T) != c.out).any(axis=1)[tail].all()


def test_head_case_is_any_order_exact():
    c = xo.head_case()
    assert xo.multiple_of(c.act, 2.0 ** -4) and xo.multiple_of(c.w1, 2.0 ** -2) and xo.multiple_of(c.b1, c.q1) and c.q1 == 2.0 ** -6
    assert xo.multiple_of(c.hidden, c.q1) and xo.multiple_of(c.w2, 2.0 ** -1) and xo.multiple_of(c.b2, c.q2) and c.q2 == c.q1 * 2.0 ** -1
    assert float(c.abs1.max()) < xo.TWO24 * c.q1 and float(c.abs2.max()) < xo.TWO24 * c.q2
    assert _fp32_exact(c.hidden) and _fp32_exact(c.out) and _distinct_rows(c.hidden) and _distinct_rows(c.out)
    z = float((c.hidden == 0).mean())
    assert 0.2 < z < 0.8
