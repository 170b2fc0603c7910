"""Exactly summable operands for the CNN's matrix kernels (tests/test_gpu_cnn_exact.py; their properties are asserted without a
GPU in tests/test_exact_operands.py).

Every operand is a small integer times a power of two, chosen so that a set of terms is ANY-ORDER EXACT: every term of an output
element (partial products, the 2^-11-scaled correction terms of the split arithmetic, the bias) is an integer multiple of a
quantum q = 2^e and sum |terms| < 2^24 q.  Every partial sum in every association is then an fp32 number, so a kernel's result
differs from the fp64 one in NO bit, whatever its summation order -- and a result that does differ names a wrong operand.

Families (in every product at least one factor has lo' = 0, so the split arithmetic's dropped lo'.lo' term is zero):
  A   weights of at most 11 bits, activations up to 22: exercises lo'.W_hi
  B   activations of at most 11 bits, weights up to 22: exercises hi.W_lo'
  M   Dense-1 only: lo' of the activations at even k, of the weights at odd k -- both corrections non-zero, lo'.lo' zero term by term
  C   convolutions only: second-layer weights up to 22 bits over first-layer outputs kept to at most 11 (sparse small inputs)
  I   convolutions only: one-hot inputs on every face, edge and corner against dyadic weights (a mismatch is one tap)
"""
import functools
from types import SimpleNamespace

import numpy as np

from oracle.mars_np import _conv_same

SPLIT = 2048.0
TWO24 = float(2 ** 24)
SENTINEL = 1365 * 2.0 ** -6   # 21.328125: an 11-bit fp16 value, NaN-free, an odd multiple of 2^-6 where the operands' quanta are 2^-2 and
                              # 2^-3: read as an operand it adds terms the reference does not have.  Padding and rows past the batch hold it
BASE_ROWS = 512            # distinct rows of a Dense-1 case; band b of the operand holds base[(r + 37 b) % 512]
NOMINAL_CU = 256           # the CU count the CPU-side cases are sized for (the GPU tests ask the library for the real one)


def relu(v):
    return np.where(v > 0, v, 0.0)


def _ints(rng, shape, m, p_zero=1.0 / 3.0):
    """About a third zeros, the rest +-[1, m] uniformly."""
    v = rng.integers(1, m + 1, size=shape) * rng.choice([-1, 1], size=shape)
    v[rng.random(size=shape) < p_zero] = 0
    return v.astype(np.float64)


def _wide(rng, shape, lo_bits, hi_bits, p_zero=1.0 / 3.0):
    """About a third zeros, the rest +-[2^lo_bits, 2^hi_bits): integers that need more than 11 significant bits."""
    v = rng.integers(2 ** lo_bits, 2 ** hi_bits, size=shape) * rng.choice([-1, 1], size=shape)
    v[rng.random(size=shape) < p_zero] = 0
    return v.astype(np.float64)


def f16_exact_and_normal(v):
    """v is held exactly by fp16 as zero or a NORMAL number."""
    v = np.asarray(v, dtype=np.float64)
    a = np.abs(v)
    with np.errstate(over="ignore"):
        back = v.astype(np.float16).astype(np.float64)
    return bool(np.all(back == v) and np.all((a == 0) | ((a >= 2.0 ** -14) & (a < 65504.0))))


def natural_split(a):
    """hi = fp16(a), lo' = fp16((a - hi) 2^11) as the kernels split an fp32 value (csrc/k_mars.hip split16), in fp64."""
    a = np.asarray(a, dtype=np.float64)
    hi = a.astype(np.float16).astype(np.float64)
    lo = ((a - hi) * SPLIT).astype(np.float16).astype(np.float64)
    return hi, lo


def multiple_of(v, q):
    v = np.asarray(v, dtype=np.float64) / q
    return bool(np.all(v == np.round(v)))


# ---------------------------------------------------------------- Dense-1 ----------------------------------------------------
def _mm(a, b):
    """a @ b.T, skipped when an operand is all zero (families A and B each have one)."""
    if not a.any() or not b.any():
        return np.zeros((a.shape[0], b.shape[0]))
    return a @ b.T


@functools.lru_cache(maxsize=None)
def dense1_case(family, K, N, seed=0):
    """hi / lo' of BASE_ROWS distinct activation rows and of N weight rows (independent fp16 arrays: Dense-1 takes them as given),
    a bias, and the quantum q of the terms.  The ranges shrink with K until the any-order condition holds."""
    rng = np.random.default_rng([K, N, seed, "ABM".index(family)])
    hm = 7 if K <= 256 else (2 if K <= 2048 else 1)
    wm = 7 if K <= 256 else 2
    lm = 1023 if K <= 2048 else 511
    sa, sw = 2.0 ** -2, 2.0 ** -3
    ah = _ints(rng, (BASE_ROWS, K), hm) * sa
    wh = _ints(rng, (N, K), wm) * sw
    al = np.zeros_like(ah)
    wl = np.zeros_like(wh)
    if family == "A":
        al = _ints(rng, (BASE_ROWS, K), lm) * sa
    elif family == "B":
        wl = _ints(rng, (N, K), lm) * sw
    else:
        al[:, 0::2] = _ints(rng, (BASE_ROWS, K), lm)[:, 0::2] * sa
        wl[:, 1::2] = _ints(rng, (N, K), lm)[:, 1::2] * sw
    bm = max(4, int(np.sqrt(K) * hm * wm / 4))
    bias = _ints(rng, (N,), bm) * (sa * sw)
    return SimpleNamespace(name=f"dense1-{family}-K{K}-N{N}", family=family, K=K, N=N, ah=ah, al=al, wh=wh, wl=wl, bias=bias,
                           q=sa * sw / SPLIT, quanta=(sa, sw))


def dense1_pre(c):
    return c.bias + _mm(c.ah, c.wh) + (_mm(c.ah, c.wl) + _mm(c.al, c.wh)) / SPLIT


def dense1_ref(c):
    """relu(bias + hi.W_hi + 2^-11 (hi.W_lo' + lo'.W_hi)) of the base rows, fp64."""
    return relu(dense1_pre(c))


def dense1_abs_sum(c):
    """sum |terms| per output element, the 2^-11-scaled correction terms and the bias included."""
    a = np.abs
    return a(c.bias) + _mm(a(c.ah), a(c.wh)) + (_mm(a(c.ah), a(c.wl)) + _mm(a(c.al), a(c.wh))) / SPLIT


def dense1_wrong_rules(c):
    """name -> the fp64 output of the base rows under a wrong rule.  A rule on a term the family keeps zero by construction
    (lo'.W_hi in B, hi.W_lo' in A) and the rules that need two K-steps at KT = 1 are not listed."""
    P = dense1_pre(c)
    KT = c.K // 32

    def m(a, w, s, t=None):
        t = s if t is None else t
        return _mm(a[:, 32 * s:32 * s + 32], w[:, 32 * t:32 * t + 32])

    def step(s, t=None):   # K-step s of the activations against K-step t of the weights
        return m(c.ah, c.wh, s, t) + (m(c.ah, c.wl, s, t) + m(c.al, c.wh, s, t)) / SPLIT

    out = {}
    if c.al.any():
        out["drop lo'.W_hi in the last K-step"] = relu(P - m(c.al, c.wh, KT - 1) / SPLIT)
    if c.wl.any():
        out["drop hi.W_lo' in the first K-step"] = relu(P - m(c.ah, c.wl, 0) / SPLIT)
    out["skip K-step KT - 1"] = relu(P - step(KT - 1))
    if KT >= 2:
        s, t = 0, KT - 1
        right = m(c.ah, c.wl, s) + m(c.ah, c.wl, t) + m(c.al, c.wh, s) + m(c.al, c.wh, t)
        swapped = m(c.ah, c.wl, s, t) + m(c.ah, c.wl, t, s) + m(c.al, c.wh, t, s) + m(c.al, c.wh, s, t)
        out["swap the lo' halves of K-steps 0 and KT - 1"] = relu(P + (swapped - right) / SPLIT)
        out["use K-step KT - 2 twice"] = relu(P - step(KT - 1) + step(KT - 2))
    R = relu(P)
    nb = c.N // 32
    out["exchange 32-column feature blocks c and c ^ 1"] = R.reshape(-1, nb, 32)[:, np.arange(nb) ^ 1].reshape(R.shape)
    out["exchange rows r and r ^ 32"] = R[np.arange(R.shape[0]) ^ 32]
    return out


def every_block_differs(ref, wrong):
    """Every aligned 32-row x 32-column block of the base output differs.  A tile of any of the three shapes, at any band's row
    offset (r + 37 b) % 512, contains whole such blocks."""
    d = (ref != wrong).reshape(ref.shape[0] // 32, 32, ref.shape[1] // 32, 32)
    return bool(d.any(axis=(1, 3)).all())


def band_rows(bands):
    """Base-row index of every row of `bands` 256-row bands: band b holds base[(r + 37 b) % BASE_ROWS]."""
    b, r = np.divmod(np.arange(bands * 256), 256)
    return (r + 37 * b) % BASE_ROWS


def interleave(hi, lo, ld):
    """(R, K) hi and lo' -> (R, ld) fp16 in runs of [hi 32 | lo' 32] (mars.interleave_split's layout), SENTINEL in the padding."""
    r, k = hi.shape
    out = np.full((r, ld), SENTINEL, dtype=np.float16)
    out[:, :2 * k] = np.stack([hi.reshape(r, k // 32, 32), lo.reshape(r, k // 32, 32)], 2).reshape(r, 2 * k)
    return out


# ---------------------------------------------------------------- convolutions -----------------------------------------------
def conv_batch(n_cu=NOMINAL_CU):
    """Samples of a convolution case: enough for every kernel's persistent loop (grids of 512, 1024 and 4 n_cu samples)."""
    return max(1024 + 9, 4 * n_cu + 5, 513 + 7)


def _impulse_case(frames):
    rng = np.random.default_rng([frames, 77])
    sp = ([0, 1, 2],) * (frames == 3) + ([0, 3, 7], [0, 4, 7])
    pos = np.array(np.meshgrid(*sp, indexing="ij")).reshape(len(sp), -1).T        # faces, edges, corners and the inside
    shape = ((3,) if frames == 3 else ()) + (8, 8, 5)
    x = np.zeros((2 * len(pos) * 5,) + shape)
    i = 0
    for sign in (1.0, -1.0):
        for p in pos:
            for ch in range(5):
                x[(i,) + tuple(p) + (ch,)] = sign * 2.0 ** (i % 4)
                i += 1
    k = (3,) * len(sp)
    w1 = rng.choice([-1.0, 1.0], size=k + (5, 16)) * 2.0 ** rng.integers(-2, 3, size=k + (5, 16))
    w2 = rng.choice([-1.0, 1.0], size=k + (16, 32)) * 2.0 ** rng.integers(-3, 2, size=k + (16, 32))
    return x, w1, np.zeros(16), w2, np.zeros(32), 2.0 ** -2, 2.0 ** -5


@functools.lru_cache(maxsize=None)
def conv_case(family, frames, n=None):
    """Inputs x (n, [3,] 8, 8, 5), Keras-layout kernels and biases of the conv pair, and the quanta q1, q2 of the two layers' terms."""
    n = conv_batch() if n is None else n
    rng = np.random.default_rng([frames, n, "ABCI".index(family)])
    sp = ((3,) if frames == 3 else ()) + (8, 8)
    k = (3,) * len(sp)
    if family == "A":      # inputs and first-layer outputs need lo', both kernels have at most 2 bits
        x = _wide(rng, (n,) + sp + (5,), 11, 13) * 2.0 ** -10
        w1, b1 = _ints(rng, k + (5, 16), 1), _ints(rng, (16,), 8)
        w2, b2 = _ints(rng, k + (16, 32), 2), _ints(rng, (32,), 64)
        q1 = q2 = 2.0 ** -10
    elif family == "B":    # 2-bit inputs against first-layer weights that need lo'; the wide first-layer outputs meet 1-bit weights
        x = _ints(rng, (n,) + sp + (5,), 3)
        w1, b1 = _wide(rng, k + (5, 16), 11, 12) * 2.0 ** -12, _ints(rng, (16,), 4)
        w2, b2 = _ints(rng, k + (16, 32), 1), _ints(rng, (32,), 8)
        q1 = q2 = 2.0 ** -12
    elif family == "C":    # sparse small inputs and weights keep the first layer's outputs to 11 bits; second-layer weights need lo'
        x = _ints(rng, (n,) + sp + (5,), 2, p_zero=0.8)
        w1, b1 = _ints(rng, k + (5, 16), 2), _ints(rng, (16,), 2)
        w2, b2 = _wide(rng, k + (16, 32), 11, 13) * 2.0 ** -12, _ints(rng, (32,), 16)
        q1, q2 = 1.0, 2.0 ** -12
    else:
        x, w1, b1, w2, b2, q1, q2 = _impulse_case(frames)
    c = SimpleNamespace(name=f"conv-{family}-frames{frames}", family=family, frames=frames, x=x, w1=w1, b1=b1, w2=w2, b2=b2, q1=q1, q2=q2)
    c.h1 = relu(_conv_same(x, w1, b1))            # the reference: oracle.mars_np._conv_same in fp64, ReLU = where(v > 0, v, +0.0)
    c.out = relu(_conv_same(c.h1, w2, b2))
    return c


def conv_abs_bound(x, w, b):
    """An upper bound of sum |terms| of one layer in the split form: |hi| + 2^-11 |lo'| <= (1 + 2^-10) |a| for both factors."""
    return _conv_same(np.abs(x), np.abs(w), np.abs(b)) * (1.0 + 2.0 ** -10) ** 2


def _tap_term(xp2, w, off, shift, sp):
    """The contribution of tap `off`, read `shift` positions away, from the input padded by TWO cells."""
    sl = (slice(None),) + tuple(slice(1 + o + s, 1 + o + s + m) for o, s, m in zip(off, shift, sp)) + (slice(None),)
    return np.tensordot(xp2[sl], w[off], axes=([-1], [0]))


def conv_layer_rules(x, w, b):
    """(name, wrong pre-activation) of one 'same' convolution layer under each wrong rule, one at a time (a generator: each is
    tens of MB at the full batch)."""
    nd = w.ndim - 2
    sp = x.shape[1:-1]
    pre = _conv_same(x, w, b)
    xp2 = np.pad(x, [(0, 0)] + [(2, 2)] * nd + [(0, 0)])
    last = (0,) * (nd - 1) + (1,)
    for off in np.ndindex(*([3] * nd)):
        yield f"tap {off} shifted by one position", pre + _tap_term(xp2, w, off, last, sp) - _tap_term(xp2, w, off, (0,) * nd, sp)
    for ax in range(nd):
        for side in (0, 1):
            # the face's outputs read the opposite face where 'same' padding has zeros: a convolution one dimension lower
            slab = np.take(x, sp[ax] - 1 if side == 0 else 0, axis=1 + ax)
            delta = _conv_same(slab, np.take(w, 0 if side == 0 else 2, axis=ax), 0.0)
            wrong = pre.copy()
            idx = [slice(None)] * pre.ndim
            idx[1 + ax] = 0 if side == 0 else sp[ax] - 1
            wrong[tuple(idx)] += delta
            yield f"wrap-around at face {side} of axis {ax}", wrong
    yield "input channels 0 and 1 exchanged", pre + _conv_same(x[..., [1, 0]] - x[..., [0, 1]], w[..., :2, :], 0.0)
    if nd == 3:
        for d in (0, 1):
            perm = [0, 1, 2]
            perm[d], perm[d + 1] = perm[d + 1], perm[d]
            yield f"frames {d} and {d + 1} exchanged", pre + _conv_same(x[:, perm] - x, w, 0.0)


def per_sample_changed(ref, wrong):
    return (ref != wrong).reshape(ref.shape[0], -1).any(axis=1)


def conv_out16_expected(c, n):
    """The flattened fp64 output of the first n samples: what hi + lo' / 2^11 of mmw_mars_conv_split must equal bit for bit."""
    return c.out[:n].reshape(n, -1)


# ---------------------------------------------------------------- Dense-2 and the small head ---------------------------------
DENSE2_ROWS = 257          # rows of a Dense-2 case: every n_rows of the GPU test is a prefix


@functools.lru_cache(maxsize=None)
def dense2_case(K):
    """fp32 operands (no split): 10-bit activations against 3-bit weights, 57 outputs."""
    rng = np.random.default_rng([K, 57])
    hidden = _ints(rng, (DENSE2_ROWS, K), 1023) * 2.0 ** -4
    w = _ints(rng, (57, K), 7) * 2.0 ** -2
    bias = _ints(rng, (57,), 4095) * 2.0 ** -6
    c = SimpleNamespace(name=f"dense2-K{K}", K=K, hidden=hidden, w=w, bias=bias, q=2.0 ** -6)
    c.abs_sum = np.abs(hidden) @ np.abs(w).T + np.abs(bias)
    c.out = hidden @ w.T + bias
    return c


@functools.lru_cache(maxsize=None)
def head_case(K=192, N1=40):
    """mmw_mars_head_small: Dense-1 + ReLU + Dense-2 in plain fp32; N1 = 40 is five whole column groups of 8, K = 192 leaves
    the last of a workgroup's 256 lanes without a float4."""
    rng = np.random.default_rng([K, N1, 5])
    act = _ints(rng, (64, K), 1023) * 2.0 ** -4
    w1 = _ints(rng, (N1, K), 7) * 2.0 ** -2
    b1 = _ints(rng, (N1,), 255) * 2.0 ** -6
    w2 = _ints(rng, (57, N1), 7) * 2.0 ** -1
    b2 = _ints(rng, (57,), 255) * 2.0 ** -7
    c = SimpleNamespace(name="head-small", K=K, N1=N1, act=act, w1=w1, b1=b1, w2=w2, b2=b2, q1=2.0 ** -6, q2=2.0 ** -7)
    c.abs1 = np.abs(act) @ np.abs(w1).T + np.abs(b1)
    c.hidden = relu(act @ w1.T + b1)
    c.abs2 = c.hidden @ np.abs(w2).T + np.abs(b2)
    c.out = c.hidden @ w2.T + b2
    return c


# ---------------------------------------------------------------- the cases both test files walk ------------------------------
SHORT_K = (32, 64, 96, 128, 160, 256)                  # KT = 1 .. 5 and 8: every prologue arm and every tail stretch of k_mars_dense1_t
INST_N = {"256x192": 384, "256x128": 256, "128x128": 128}   # a feature count at which the plan can give the instantiation a band
MODEL_KN = ((6144, 1536), (2048, 512))                 # define_CNN_3D's and define_CNN's Dense-1


def dense1_case_keys():
    """(family, K, N) of every Dense-1 case of tests/test_gpu_cnn_exact.py."""
    keys = []
    for n in sorted(set(INST_N.values())):
        keys += [(f, k, n) for k in SHORT_K for f in "AB"] + [("M", 160, n)]
    keys += [(f, k, n) for k, n in MODEL_KN for f in "AB"]
    return keys


CONV_KEYS = tuple((f, fr) for fr in (3, 1) for f in "ABC")
DENSE2_K = (1536, 512, 32, 36, 64)
