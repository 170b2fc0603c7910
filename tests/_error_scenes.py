"""Error scenes: finite inputs on which the reference's track() leaves a frame through an exception, built on the CPU alone
(numpy and the C oracle; no GPU, no torch).  The one builder of tests/test_error_scenes.py (which holds the oracle's return code
to the exception oracle/py_tracker.py raises under the installed numpy), of the `track_exceptions` golden (oracle/gen_golden.py:
the live reference on the same rows) and of tests/test_gpu_error_scenes.py (which holds the kernels to the oracle).

The two exceptions, and what they become here (include/mmw.h):

  numpy.linalg.LinAlgError  np.linalg.inv / det of a singular 6 x 6   rc -2  MMW_ERRBIT_SINGULAR  MMW_E_SINGULAR  MmwSingular
  ZeroDivisionError         _get_Rc, a = n / N_est                    rc -3  MMW_ERRBIT_DIVZERO   MMW_E_DIVZERO   MmwDivZero

Where track() can raise them, in program order (Tracking.py:683-703), and the scene that gets there:

  the gate matrix C = P[:6,:6] + diag((spread/2)^2) + group_disp_est (_calc_dist_fun)   SINGULAR   gate_zero, gate_rank5, gate_collinear
  associate_pointcloud, a = n / N_est                                                    DIVZERO    nest_zero
  update_state, den = (N_est - 1) N in _get_Rc                                           DIVZERO    update_divzero_est, update_divzero_pointnum
  update_state, S^-1                                                                     SINGULAR   update_singular
  two tracks of one _update_all, the singular one first | the zero denominator first               both_singular_first | both_divzero_first

Every scene runs under db_min_samples = 5 and fb_frames_batch = 0: one tight cluster of 12 rows is a track after frame 0.  A new
track has spread_est = 0, N_est = 0 and group_disp_est = kf_group_disp_est_init I, so under kf_p_init = kf_q_std =
kf_group_disp_est_init = 0 the gate matrix of frame 1 is the ZERO matrix whatever kf_spread_lim and the rows are: the three gate
scenes reach the same site with the three inputs the issue names (identical rows; all z equal; y = x + 2.5).  Under
kf_spread_lim[2] = 0 the clamps give spread_est[2] = 0 for any cluster, and with kf_enable_est a track's first association sets
N_est = n, coef = 0, S = P + Rm / n: a zero on the diagonal at z -- the update's SINGULAR, behind a gate that is regular
(0.1 I) because of the initial group_disp_est.

band_*: update_singular with kf_spread_lim[2] on the edges of the band in which this build's LU (lu6: one reciprocal per
pivot, then products) reports SINGULAR while LAPACK (which divides below sfmin) inverts: see band_edges().  near_*: the
neighbours that must NOT raise.  Bystanders: under the same configurations, inputs that do not fail.

Everything is fp64 holding float32-representable values, built once, cached and read-only."""
import functools
from typing import NamedTuple

import numpy as np

from oracle import c_oracle as co
from tests._edge_inputs import Frame, Scene, _ro, cfg_key

MAX_PTS, DT, N_CLUSTER = 64, 0.1, 12
DIM_X = (9, 6)
RC_SINGULAR, RC_DIVZERO = -2, -3
BASE = {"db_min_samples": 5, "fb_frames_batch": 0}
GATE_KW = dict(BASE, kf_p_init=0.0, kf_q_std=0.0, kf_group_disp_est_init=0.0)
FLAT_LIM = [0.5, 0.5, 0.0, 1.0, 1.0, 1.0]
UPD_KW = dict(BASE, kf_p_init=0.0, kf_q_std=0.0, kf_group_disp_est_init=0.1, kf_spread_lim=FLAT_LIM, kf_enable_est=1)
NEAR_LIM2 = 1e-100
NEAR_FRAMES = 5


class Replay(NamedTuple):
    frames: list          # a Frame per frame the oracle finished (None where cnt == 0)
    rc: int               # 0, or the first non-zero return code of orc_track_frame
    at: object            # the frame it arrived in, or None
    n_tracks_before: int  # tracks the scene held when the failing frame began (-1: no frame failed)
    assoc_at: object      # the failing frame's association (complete where the frame failed BEHIND _calc_dist_fun), or None


def replay(scene, **cfg_over):
    """The oracle on the scene's frames, up to and including the first one that fails."""
    orc = co.OracleScene(co.default_config(**{**scene.cfg, **cfg_over}), scene.max_pts)
    out = []
    for f in range(len(scene.cnt)):
        c = int(scene.cnt[f])
        if c == 0:
            out.append(None)
            continue
        before = orc.n_tracks
        try:
            a, lab = orc.track(scene.pts[f, :c], float(scene.dt[f]))
        except co.OracleNonFinite:
            raise
        except RuntimeError as e:
            return Replay(out, int(str(e).rsplit("rc=", 1)[1]), f, before, orc.last_assoc.copy())
        trk = orc.tracks()
        feat, owner = orc.features()
        rings = [[orc.track_ring_frame(t, k) for k in range(trk[t]["ring_len"])] for t in range(len(trk))]
        out.append(Frame(a, lab, orc.n_tracks, trk, orc.batch_ring(), feat, owner, rings))
    return Replay(out, 0, None, -1, None)


# ------------------------------------------------------------------------------------------------------------------ rows
def _cluster(seed, cx, cy, flat_z=False, identical=False, collinear=False):
    """12 rows within 6 / 64 of (cx, cy, 1): every column on a dyadic grid (float32-exact), the columns permuted independently so
    that the 6 x 6 dispersion of a plain cluster is regular.  flat_z: all z equal.  identical: 12 copies of one row.
    collinear: y = x + 2.5 exactly."""
    rng = np.random.default_rng(9100 + seed)
    k = np.arange(N_CLUSTER) - 6
    p = np.zeros((N_CLUSTER, 8))
    p[:, 0] = cx + rng.permutation(k) / 64.0
    p[:, 1] = cy + rng.permutation(k) / 64.0
    p[:, 2] = 1.0 + (0.0 if flat_z else rng.permutation(k) / 64.0)
    for m in (3, 4, 5):
        p[:, m] = rng.permutation(k) / 256.0
    p[:, 6] = rng.permutation(k) / 8.0
    p[:, 7] = 20.0 + rng.permutation(k)
    if collinear:
        p[:, 1] = p[:, 0] + 2.5
    if identical:
        p[:] = p[0]
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
    return p


def _stray(f):
    """Four rows no track of these scenes gates and apply_DBscan (min_samples 5) labels noise; other ones every frame."""
    p = np.zeros((4, 8))
    p[:, 0] = [-6.0, -2.0, 3.0, 7.0]
    p[:, 1] = [6.0 + f / 4.0, 7.0, 6.5, 7.5 - f / 8.0]
    p[:, 2] = [0.5, 1.0, 1.5, 2.0]
    p[:, 6], p[:, 7] = 0.25, 12.0
    return p


def _scene(tag, cfg, frames):
    assert 1 <= len(frames) <= 6 and all(len(r) <= MAX_PTS for r in frames)
    pts = np.zeros((len(frames), MAX_PTS, 8))
    for f, r in enumerate(frames):
        pts[f, : len(r)] = r
        pts[f, len(r):] = frames[0][np.arange(MAX_PTS - len(r)) % len(frames[0])]     # past the count: rows a track would take
    cnt = np.array([len(r) for r in frames], np.int32)
    dts = np.full(len(frames), DT)
    assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)
    _ro(pts, cnt, dts)
    return Scene(tag, dict(cfg), MAX_PTS, pts, cnt, dts)


def _kw(dim_x, base, **over):
    return dict(base, dim_x=int(dim_x), **over)


# ---------------------------------------------------------------------------------------------------------------- the band
def _upd_rc(dim_x, lim2):
    kw = _kw(dim_x, UPD_KW, kf_spread_lim=FLAT_LIM[:2] + [float(lim2)] + FLAT_LIM[3:])
    a = _cluster(1, -1.0, 2.0, flat_z=True)
    return replay(_scene("probe", kw, [a, a])).rc


def _edge(lo, hi, pred):
    """Adjacent doubles (lo, hi) with pred(lo) and not pred(hi): bisection on the exponent first (geometric mean), then on the
    value."""
    assert pred(lo) and not pred(hi)
    while np.nextafter(lo, np.inf) != hi:
        mid = float(np.sqrt(lo) * np.sqrt(hi)) if hi / lo > 4.0 else lo + (hi - lo) / 2
        if not lo < mid < hi:
            mid = float(np.nextafter(lo, np.inf))
        lo, hi = (mid, hi) if pred(mid) else (lo, mid)
    return float(lo), float(hi)


@functools.lru_cache(maxsize=None)
def band_edges(dim_x):
    """(zero_hi, nonzero_lo, pivot_lo, raises_hi, clean_lo): kf_spread_lim[2] of update_singular --
    zero_hi     the largest double for which (lim / 2)^2 is 0: S has an exact zero on its diagonal, LAPACK and lu6 both refuse it
    nonzero_lo  the smallest for which it is not.  S holds Rm / N, and the smallest denormal divided by the cluster's 12 rows is
                0 again: both still refuse it
    pivot_lo    the smallest for which (lim / 2)^2 / 12 is not 0: a denormal pivot; lu6 forms 1 / pivot = inf, 0 * inf = NaN
                reaches the next pivots, `!(best > 0)` reports the NaN pivot as singular -- LAPACK divides below sfmin and inverts
    raises_hi   the largest for which the oracle still returns -2 (1 / pivot overflows up to here)
    clean_lo    the smallest for which it does not.
    Found by bisection, the last two on the C oracle; nothing is hard-coded."""
    zero_hi, nonzero_lo = _edge(1e-170, 1e-150, lambda v: (v / 2) * (v / 2) == 0.0)
    _, pivot_lo = _edge(nonzero_lo, 1e-150, lambda v: ((v / 2) * (v / 2)) / N_CLUSTER == 0.0)
    raises_hi, clean_lo = _edge(pivot_lo, 1e-140, lambda v: _upd_rc(dim_x, v) == RC_SINGULAR)
    assert _upd_rc(dim_x, zero_hi) == RC_SINGULAR and _upd_rc(dim_x, NEAR_LIM2) == 0
    assert zero_hi < nonzero_lo < pivot_lo < raises_hi < clean_lo
    return zero_hi, nonzero_lo, pivot_lo, raises_hi, clean_lo


BAND_NAMES = ("band_zero_hi", "band_nonzero_lo", "band_pivot_lo", "band_raises_hi", "band_clean_lo")
BAND_DEVIATES = ("band_pivot_lo", "band_raises_hi")     # the oracle returns -2, numpy does not raise: the band's two ends


# -------------------------------------------------------------------------------------------------------------- the scenes
@functools.lru_cache(maxsize=None)
def scenes(dim_x):
    """name -> Scene.  Failing scenes stop being fed after their failing frame; near_* scenes run NEAR_FRAMES frames."""
    A = _cluster(1, -1.0, 2.0)
    flat = _cluster(2, -1.0, 2.0, flat_z=True)
    other = _cluster(3, 1.5, 2.0)
    out = {}

    def add(name, base, frames, **over):
        out[name] = _scene(name, _kw(dim_x, base, **over), frames)

    same = _cluster(4, -1.0, 2.0, identical=True)
    add("gate_zero", GATE_KW, [same, same], kf_spread_lim=[0.0] * 6)
    add("gate_rank5", GATE_KW, [flat, flat], kf_spread_lim=FLAT_LIM)
    line = _cluster(5, -1.0, 1.5, collinear=True)
    add("gate_collinear", GATE_KW, [line, line], kf_spread_lim=[0.0] * 6, kf_enable_est=1)
    add("update_singular", UPD_KW, [flat, flat])
    add("update_divzero_est", BASE, [A, A[3:4]], kf_enable_est=1)
    add("update_divzero_pointnum", BASE, [A, A[3:4]], kf_enable_est=0, kf_est_pointnum=1.0)
    add("nest_zero", BASE, [A, A[:4], A[4:6]], kf_enable_est=1, kf_a_n=2.0)
    one = other[5:6]
    add("both_singular_first", UPD_KW, [np.concatenate([flat, other]), np.concatenate([flat, one])])
    add("both_divzero_first", UPD_KW, [np.concatenate([other, flat]), np.concatenate([one, flat])])
    for name, lim2 in zip(BAND_NAMES, band_edges(dim_x)):
        add(name, UPD_KW, [flat] * (2 if name != "band_clean_lo" else NEAR_FRAMES), kf_spread_lim=FLAT_LIM[:2] + [lim2] + FLAT_LIM[3:])
    add("near_singular", UPD_KW, [flat] * NEAR_FRAMES, kf_spread_lim=FLAT_LIM[:2] + [NEAR_LIM2] + FLAT_LIM[3:])
    # (frames of 8 rows behind the first: with kf_enable_est = 0, N_est = max(10, n), and 12 rows would make coef = (N_est - n) / den
    #  = 0 and S = Rm / n singular at z in the UPDATE -- under any group_disp_est; this scene is the neighbour of the GATE's zero matrix)
    add("near_rank5", GATE_KW, [flat] + [flat[:8]] * (NEAR_FRAMES - 1), kf_spread_lim=FLAT_LIM, kf_group_disp_est_init=1e-300)
    add("near_divzero", BASE, [A, A[3:5], A[3:5], A, A[3:5]], kf_enable_est=1)
    return out


# what the oracle must answer: name -> (rc, frame)
EXPECT = {
    "gate_zero": (RC_SINGULAR, 1), "gate_rank5": (RC_SINGULAR, 1), "gate_collinear": (RC_SINGULAR, 1),
    "update_singular": (RC_SINGULAR, 1), "update_divzero_est": (RC_DIVZERO, 1), "update_divzero_pointnum": (RC_DIVZERO, 1),
    "nest_zero": (RC_DIVZERO, 2), "both_singular_first": (RC_SINGULAR, 1), "both_divzero_first": (RC_DIVZERO, 1),
    "band_zero_hi": (RC_SINGULAR, 1), "band_nonzero_lo": (RC_SINGULAR, 1), "band_pivot_lo": (RC_SINGULAR, 1),
    "band_raises_hi": (RC_SINGULAR, 1), "band_clean_lo": (0, None), "near_singular": (0, None), "near_rank5": (0, None), "near_divzero": (0, None),
}
# the site of the device code each failing scene reaches (the issue's table; DESIGN.md "Errors")
SITE = {
    "gate_zero": "gate", "gate_rank5": "gate", "gate_collinear": "gate", "nest_zero": "associate: n / N_est",
    "update_divzero_est": "update: (N_est - 1) N", "update_divzero_pointnum": "update: (N_est - 1) N",
    "update_singular": "update: S^-1", "both_singular_first": "update: S^-1, then (N_est - 1) N",
    "both_divzero_first": "update: (N_est - 1) N, then S^-1", "band_zero_hi": "update: S^-1", "band_nonzero_lo": "update: S^-1",
    "band_pivot_lo": "update: S^-1", "band_raises_hi": "update: S^-1",
}


@functools.lru_cache(maxsize=None)
def replays(dim_x):
    return {name: replay(sc) for name, sc in scenes(dim_x).items()}


def _by_scene(kw, rows):
    pts = np.zeros((len(rows), MAX_PTS, 8))
    for f, r in enumerate(rows):
        pts[f, : len(r)] = r
        pts[f, len(r):] = rows[0][np.arange(MAX_PTS - len(r)) % len(rows[0])]
    cnt, dts = np.array([len(r) for r in rows], np.int32), np.full(len(rows), DT)
    _ro(pts, cnt, dts)
    return Scene("bystander", kw, MAX_PTS, pts, cnt, dts)


@functools.lru_cache(maxsize=None)
def bystander(dim_x, key, frames):
    """(Scene, oracle Frames): a scene under the configuration `key` (cfg_key of a group), `frames` frames long, whose inputs do
    not fail -- the first of these that the oracle runs with rc == 0:
      the 12-row cluster every frame: a track that is gated and updated;
      clusters that are seen once and never again, between stray rows: tracks that are predicted, gated, age, and whose updates
        run on the spawn record (N_est = 0: den = -N) -- for the update-singular configurations, where every track fails at its
        first update WITH rows;
      stray rows only, no track ever -- for the gate configurations, where every track fails at its first gate."""
    kw = {k: list(v) if isinstance(v, tuple) else v for k, v in key}
    assert kw["dim_x"] == dim_x and cfg_key(kw) == key
    spots = [(-1.0, 2.0), (1.5, 3.0), (-2.5, 4.0)]
    c = _cluster(6, 1.0, 3.0)
    candidates = [[c] + [c[::-1].copy() for _ in range(frames - 1)],
                  [np.concatenate([_cluster(10 + f, *spots[f // 2]), _stray(f)]) if f % 2 == 0 and f // 2 < 3 else _stray(f) for f in range(frames)],
                  [_stray(f) for f in range(frames)]]
    for k, rows in enumerate(candidates):
        sc = _by_scene(kw, rows)
        r = replay(sc)
        if r.rc == 0:
            assert k == 2 or r.frames[-1].n_tracks >= 1, key
            return sc, r.frames
    raise AssertionError(("no bystander", key))


def groups(dim_x):
    """The scenes grouped by configuration: [(cfg_key, [names])], one context each."""
    g = {}
    for name, sc in scenes(dim_x).items():
        g.setdefault(cfg_key(sc.cfg), []).append(name)
    return list(g.items())


GROUP_IDS = ["gate_zero", "gate_rank5", "gate_collinear", "update_singular+both", "update_divzero_est+near_divzero", "update_divzero_pointnum",
             "nest_zero"] + list(BAND_NAMES) + ["near_singular", "near_rank5"]
