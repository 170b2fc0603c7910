"""The error scenes (tests/_error_scenes.py) on the CPU: the C oracle's return code, and the frame it arrives in, against the
exception the numpy restatement of track() (oracle/py_tracker.py: np.linalg.inv / det, Python's own division) raises on the same
rows under the installed numpy -- LinAlgError for -2, ZeroDivisionError for -3, none for 0; up to the failing frame the
associations and labels are equal.  No GPU.

The listed exception is the denormal-pivot band (band_pivot_lo .. band_raises_hi): the oracle's lu6 -- and by construction the
kernels' lu6_inverse_cols -- multiplies by the reciprocal of the pivot, which is inf for a pivot below about 5.6e-309; 0 * inf = NaN
reaches the next pivots and a NaN pivot is reported as singular.  LAPACK divides when |pivot| < sfmin and inverts.  The test
asserts the deviation as it stands at both ends of the band; aligning lu6 with LAPACK's sfmin rule is the follow-up (it sits on
the hot path of k_track, k_scene and k_predict and needs its own benchmark evidence): DESIGN.md, "Errors"."""
import warnings

import numpy as np
import pytest

from oracle.py_tracker import Params, PyScene
from tests import _error_scenes as es
from tests._fuzz import reference_overrides

EXC = {es.RC_SINGULAR: np.linalg.LinAlgError, es.RC_DIVZERO: ZeroDivisionError}
CASES = [(d, name) for d in es.DIM_X for name in es.EXPECT]


def _params(cfg):
    kw = {}
    for k, v in reference_overrides(cfg).items():
        if k == "MOTION_MODEL":
            kw["DIM_X"] = 6 if v == "CONST_VEL_MODEL" else 9
        else:
            kw[k] = v
    return Params(**kw)


def _py_replay(sc):
    """(frames [(assoc, labels)], exception class or None, frame) of the numpy restatement."""
    py, out = PyScene(_params(sc.cfg)), []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")               # (log(0), overflow in the near_* scenes: values, not exceptions)
        for f in range(len(sc.cnt)):
            try:
                out.append(py.track(sc.pts[f, : sc.cnt[f]], float(sc.dt[f])))
            except (np.linalg.LinAlgError, ZeroDivisionError) as e:
                return out, type(e), f
    return out, None, None


@pytest.mark.parametrize("dim_x,name", CASES)
def test_oracle_rc_is_the_exception_numpy_raises(dim_x, name):
    sc, r = es.scenes(dim_x)[name], es.replays(dim_x)[name]
    assert (r.rc, r.at) == es.EXPECT[name], (name, r.rc, r.at)
    assert np.array_equal(sc.pts.astype(np.float32).astype(np.float64), sc.pts) and len(sc.cnt) <= 6 and sc.max_pts == 64
    assert np.all(sc.dt == 0.1)
    frames, exc, at = _py_replay(sc)
    if r.rc:
        assert r.n_tracks_before >= 1, name                       # never all-noise against all-noise
        assert all(fr.n_tracks >= 1 for fr in r.frames), name
    else:
        assert len(r.frames) == es.NEAR_FRAMES and r.frames[-1].n_tracks >= 1, name
    if name in es.BAND_DEVIATES:
        # the known deviation: the oracle reports the NaN pivot as singular, LAPACK inverts (follow-up: lu6 by LAPACK's sfmin rule)
        assert r.rc == es.RC_SINGULAR and exc is None, (name, r.rc, exc)
        frames = frames[: r.at]
    else:
        assert exc is EXC.get(r.rc) and at == r.at, (name, r.rc, r.at, exc, at)
    assert len(frames) == len(r.frames)
    for f, (fr, (a, lab)) in enumerate(zip(r.frames, frames)):
        assert np.array_equal(fr.assoc, a), (name, f)
        assert (fr.labels is None) == (lab is None) and (lab is None or np.array_equal(fr.labels, lab)), (name, f)


@pytest.mark.parametrize("dim_x", es.DIM_X)
def test_band_edges_are_adjacent_doubles_in_order(dim_x):
    zero_hi, nonzero_lo, pivot_lo, raises_hi, clean_lo = es.band_edges(dim_x)
    assert (zero_hi / 2) ** 2 == 0.0 < (nonzero_lo / 2) ** 2 and np.nextafter(zero_hi, 1.0) == nonzero_lo
    assert ((nonzero_lo / 2) * (nonzero_lo / 2)) / 12 == 0.0 < ((pivot_lo / 2) * (pivot_lo / 2)) / 12
    assert np.nextafter(raises_hi, 1.0) == clean_lo
    assert 1e-163 < zero_hi < 1e-161 and 1e-162 < pivot_lo < 1e-160 and 1e-155 < raises_hi < 1e-150        # where the issue measured them
    # the band's upper edge is where 1 / pivot stops overflowing: pivot = (lim / 2)^2 / 12
    piv = lambda v: ((v / 2) * (v / 2)) / 12
    with np.errstate(over="ignore"):
        assert np.isinf(np.float64(1.0) / np.float64(piv(raises_hi))) and np.isfinite(np.float64(1.0) / np.float64(piv(clean_lo)))


@pytest.mark.parametrize("dim_x", es.DIM_X)
def test_both_scenes_spawn_the_two_tracks_in_the_intended_order(dim_x):
    """Frame 0 makes the flat-z cluster (x about -1) and the plain one (x about 1.5) tracks 0 | 1 and 1 | 0; in frame 1 the flat one
    takes all its rows (S singular) and the plain one ONE row ((N_est - 1) N == 0)."""
    for name, flat in (("both_singular_first", 0), ("both_divzero_first", 1)):
        r = es.replays(dim_x)[name]
        t = r.frames[0].tracks
        assert r.frames[0].n_tracks == 2 and r.n_tracks_before == 2
        assert t["centroid"][flat][0] < 0 < t["centroid"][1 - flat][0], name
        assert t["min_vals"][flat][2] == t["max_vals"][flat][2] and t["min_vals"][1 - flat][2] < t["max_vals"][1 - flat][2], name
        a = r.assoc_at
        assert int(np.sum(a == flat)) == es.N_CLUSTER and int(np.sum(a == 1 - flat)) == 1 and len(a) == es.N_CLUSTER + 1, (name, a)


@pytest.mark.parametrize("dim_x", es.DIM_X)
def test_update_singular_fails_behind_a_regular_gate(dim_x):
    """The frame-1 gate of update_singular did not fail: the association of the failing frame is complete, every row taken by
    track 0 -- the same rows the same scene associates under kf_spread_lim[2] = 1e-100 (near_singular), where S is regular."""
    r, near = es.replays(dim_x)["update_singular"], es.replays(dim_x)["near_singular"]
    sc, nsc = es.scenes(dim_x)["update_singular"], es.scenes(dim_x)["near_singular"]
    assert np.array_equal(sc.pts[:2], nsc.pts[:2]) and {k: v for k, v in sc.cfg.items() if k != "kf_spread_lim"} == {k: v for k, v in nsc.cfg.items() if k != "kf_spread_lim"}
    assert r.rc == es.RC_SINGULAR and r.at == 1 and near.rc == 0
    assert np.array_equal(r.assoc_at, near.frames[1].assoc) and np.all(r.assoc_at == 0) and len(r.assoc_at) == es.N_CLUSTER


@pytest.mark.parametrize("dim_x", es.DIM_X)
def test_every_group_has_a_bystander_that_does_not_fail(dim_x):
    groups = es.groups(dim_x)
    assert [n for _, names in groups for n in names].count("update_singular") == 1 and len(groups) == len(es.GROUP_IDS)
    assert sorted(n for _, names in groups for n in names) == sorted(es.EXPECT)
    with_tracks = 0
    for key, names in groups:
        sc, frames = es.bystander(dim_x, key, 6)
        assert len(frames) == 6 and sc.cfg == es.scenes(dim_x)[names[0]].cfg
        with_tracks += frames[-1].n_tracks >= 1
    assert with_tracks >= len(groups) - 3            # (no bystander can hold a track under the three gate configurations)
