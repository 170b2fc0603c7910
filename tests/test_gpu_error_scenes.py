"""The tracker's two error codes on FINITE inputs, site by site, every layout against the C oracle (tests/_error_scenes.py).

The reference's track() can leave a frame through numpy's LinAlgError (a singular 6 x 6) and through a ZeroDivisionError; here
they are sticky per-scene bits (MMW_ERRBIT_SINGULAR | MMW_ERRBIT_DIVZERO), MMW_E_SINGULAR | MMW_E_DIVZERO and MmwSingular |
MmwDivZero.  The device code raises them at eight places; the scene that reaches each:

  site (reference step)                                       device code                                   scene
  gate matrix C = P[:6,:6] + diag((spread/2)^2) + gd SINGULAR mmw_kalman.hpp predict_math (k_track, k_scene) gate_zero, gate_rank5, gate_collinear
                                                              mmw_kalman.hpp predict_math_cols (k_predict)  the same, track-wise layouts
  associate_pointcloud, a = n / N_est                DIVZERO  k_track.hip  `ne == 0.0`                      nest_zero
                                                              k_scene.hip  `ne == 0.0`                      nest_zero, one_workgroup
  update_state, den = (N_est - 1) N                  DIVZERO  mmw_kalman.hpp update_math (k_scene)          update_divzero_est, update_divzero_pointnum, one_workgroup
                                                              mmw_kalman.hpp update_math_bcast (k_post)     the same, the other layouts
  update_state, S^-1                                 SINGULAR mmw_kalman.hpp update_math (k_scene)          update_singular, band_*, one_workgroup
                                                              mmw_kalman.hpp update_math_bcast (k_post)     the same, the other layouts
  api_query.hip first_scene_error: which of the two the caller sees                                         both_singular_first, both_divzero_first

One context per (layout, dim_x, configuration); in front of, between and behind the group's scenes sit three bystanders: the same
configuration, inputs that do not fail (tests/_error_scenes.py: bystander).  NO expected value comes from a GPU call: every `want`
is the oracle's.  Up to the failing frame everything is compared by bits; on it the exception's class and code are those of the
lowest-numbered failing scene's oracle rc, errors() holds the oracle's bit for the failing scenes and 0 for bystanders and near_*
scenes; under check=False (the read-out form) the bystanders equal their oracles on that frame and on three more; reset_scenes on
the failed scenes gives them a fresh TrackBuffer -- in the track-wise layout too, where the update lists of the failed frame still
name the stale records.  These are error CODES on finite inputs: nothing here faults, and no row is NaN or infinite."""
import functools

import numpy as np
import pytest

from tests import _error_scenes as es
from tests._edge_inputs import cfg_key
from tests._golden import assert_tracks_match
from tests._layouts import LAYOUTS, make_checked

pytestmark = pytest.mark.gpu

STEP_KIND = {"per_scene": 2, "track_wise": 4, "track_wise+side_stream": 4, "one_workgroup": 1}
N_GROUPS = len(es.GROUP_IDS)
BY_FRAMES = 6


class Ctx:
    """The scenes of one configuration group with their bystanders: slot -> (name or None for a bystander, Scene, oracle frames)."""

    def __init__(self, dim_x, group, only=None):
        key, names = es.groups(dim_x)[group]
        names = [n for n in names if only is None or n in only]
        self.by_scene, self.by_frames = es.bystander(dim_x, key, BY_FRAMES)
        order = [None, names[0], None] + names[1:] + [None]
        self.names = order
        self.scenes = [self.by_scene if n is None else es.scenes(dim_x)[n] for n in order]
        self.replay = [None if n is None else es.replays(dim_x)[n] for n in order]
        self.failing = {s: r.rc for s, r in enumerate(self.replay) if r is not None and r.rc}
        ats = {self.replay[s].at for s in self.failing}
        assert len(ats) <= 1 and len(order) <= 16
        self.at = ats.pop() if ats else None
        self.cfg = dict(self.scenes[1].cfg)
        assert all(cfg_key(sc.cfg) == key for sc in self.scenes)

    def want(self, s, f):
        """The oracle's Frame of slot s after frame f (None: the frame failed, or the scene was not fed)."""
        if self.names[s] is None:
            return self.by_frames[f] if f < len(self.by_frames) else None
        fr = self.replay[s].frames
        return fr[f] if f < len(fr) else None

    def inputs(self, f, fed=None):
        """Frame f of every slot (`fed`: slot -> (Scene, frame) overrides; a scene behind its last frame gets cnt = 0)."""
        S = len(self.scenes)
        pts, n, dt = np.zeros((S, es.MAX_PTS, 8)), np.zeros(S, np.int32), np.full(S, es.DT)
        for s, sc in enumerate(self.scenes):
            sc, g = (fed or {}).get(s, (sc, f))
            if sc is not None and g < len(sc.cnt):
                pts[s], n[s], dt[s] = sc.pts[g], sc.cnt[g], sc.dt[g]
        return pts, n, dt


@functools.lru_cache(maxsize=None)
def _ctx(dim_x, group, only=None):
    return Ctx(dim_x, group, only)


def _make(layout, cx):
    sb = make_checked(len(cx.scenes), es.MAX_PTS, layout, **cx.cfg)
    assert sb.step_kind() == STEP_KIND[layout], (layout, sb.step_kind())
    return sb


def _compare(sb, out, want, cnt, where, rings=False):
    """Association, labels, db_n, the track list, the global ring (and the tracks' ring frames) of every slot with an oracle Frame."""
    assoc, labels, dbn = out
    ntr, trk = sb.num_tracks(), sb.tracks()
    ln, rn = sb.batch_ring()
    for s, w in enumerate(want):
        ctx = f"{where} slot {s}"
        if w is None:
            continue
        c = int(cnt[s])
        assert np.array_equal(assoc[s, :c], w.assoc), (ctx, assoc[s, :c].tolist(), w.assoc.tolist())
        assert (w.labels is None) == (dbn[s] < 0), (ctx, int(dbn[s]))
        if w.labels is not None:
            assert dbn[s] == len(w.labels) and np.array_equal(labels[s, : dbn[s]], w.labels), ctx
        assert ntr[s] == w.n_tracks, (ctx, int(ntr[s]), w.n_tracks)
        assert_tracks_match(trk[s, : ntr[s]], w.tracks, ctx=ctx, exact=True)
        assert ln[s] == len(w.batch_ring) and np.array_equal(rn[s, : ln[s]], w.batch_ring), (ctx, "the global ring")
        if rings:
            for t in range(w.n_tracks):
                for k, rows in enumerate(w.rings[t]):
                    assert np.array_equal(sb.track_ring_frame(s, t, k), rows), (ctx, "ring frame", t, k)


def _error_class(lib, rc):
    return {es.RC_SINGULAR: (lib.MmwSingular, lib.E_SINGULAR, lib.ERRBIT_SINGULAR),
            es.RC_DIVZERO: (lib.MmwDivZero, lib.E_DIVZERO, lib.ERRBIT_DIVZERO)}[rc]


def _check_bits(lib, cx, err, where):
    """errors(): the oracle's bit for every failing scene, 0 for every bystander and near_* scene."""
    for s in range(len(cx.scenes)):
        if s in cx.failing:
            assert err[s] & 3 & _error_class(lib, cx.failing[s])[2], (where, s, cx.names[s], int(err[s]))
            assert err[s] & ~3 == 0, (where, s, int(err[s]))
        else:
            assert err[s] == 0, (where, s, cx.names[s], int(err[s]))


def _run_up_to_failure(sb, cx, where):
    """Frames [0, at) (all frames where nothing fails), everything by bits; returns the frame to come."""
    last = cx.at if cx.at is not None else max(len(sc.cnt) for sc in cx.scenes)
    for f in range(last):
        pts, n, dt = cx.inputs(f)
        out = sb.step_host(pts, n, dt)
        _compare(sb, out, [cx.want(s, f) if n[s] else None for s in range(len(n))], n, (where, f), rings=True)
        assert not sb.errors().any(), (where, f)
    for s in cx.failing:                                          # never all-noise against all-noise
        assert sb.num_tracks()[s] == cx.replay[s].n_tracks_before >= 1, (where, s)
    return last


@pytest.mark.parametrize("group", range(N_GROUPS), ids=es.GROUP_IDS)
@pytest.mark.parametrize("dim_x", es.DIM_X)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_failing_frame_raises_the_oracles_error_and_reset_recovers(layout, dim_x, group):
    """Up to the failing frame by bits; on it step_host raises the class and code of the lowest-numbered failing scene's rc and
    errors() names exactly the failing scenes.  Then mmw_reset_scenes on the failed scenes alone, RIGHT behind the failed frame
    (the track-wise update lists still name their stale records): their bits clear and their next three frames equal a fresh
    OracleScene, while the bystanders carry on.  A group in which nothing fails (near_*, band_clean_lo) runs all its frames."""
    from mmwave_msc_amd import _lib
    cx, where = _ctx(dim_x, group), (layout, dim_x, es.GROUP_IDS[group])
    sb = _make(layout, cx)
    f = _run_up_to_failure(sb, cx, where)
    if cx.at is None:
        assert not cx.failing
        sb.check()
        sb.close()
        return
    first = min(cx.failing)
    cls, code, _ = _error_class(_lib, cx.failing[first])
    with pytest.raises(_lib.MmwError) as ei:
        sb.step_host(*cx.inputs(f))
    assert type(ei.value) is cls and ei.value.code == code, (where, type(ei.value).__name__, ei.value.code, cx.names[first], cx.failing[first])
    _check_bits(_lib, cx, sb.errors(), where)
    mask = np.zeros(len(cx.scenes), bool)
    mask[list(cx.failing)] = True
    sb.reset_scenes(mask)
    assert not sb.errors().any(), where
    assert all(sb.num_tracks()[s] == 0 for s in cx.failing)
    fresh = {s: (cx.by_scene, 0) for s in cx.failing}             # the recovered scenes start the bystander's frames from 0
    for k in range(3):
        g = f + 1 + k
        fed = {s: (cx.by_scene, k) for s in fresh}
        fed.update({s: (None, 0) for s, nm in enumerate(cx.names) if nm is not None and s not in cx.failing and g >= len(cx.scenes[s].cnt)})
        pts, n, dt = cx.inputs(g, fed)
        out = sb.step_host(pts, n, dt)
        want = [cx.by_frames[k] if s in fresh else (cx.want(s, g) if n[s] else None) for s in range(len(n))]
        _compare(sb, out, want, n, (where, "after the reset", g), rings=True)
        assert not sb.errors().any(), (where, g, sb.errors())
    assert sb.step_kind() == STEP_KIND[layout]
    sb.check()
    sb.close()


FAILING_GROUPS = [g for g, name in enumerate(es.GROUP_IDS) if not name.startswith("near_") and name != "band_clean_lo"]


@pytest.mark.parametrize("group", FAILING_GROUPS, ids=[es.GROUP_IDS[g] for g in FAILING_GROUPS])
@pytest.mark.parametrize("dim_x", es.DIM_X)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_read_out_form_leaves_the_bystanders_alone(layout, dim_x, group):
    """check=False: the failing frame raises nothing, its results are there.  The bystanders' (and the near_* scenes') association,
    labels, db_n, track lists and rings equal their oracles on that frame and on three more, on which the failed scenes are fed
    cnt = 0; the bits stay as they were, and mmw_check goes on reporting the first failing scene's code."""
    from mmwave_msc_amd import _lib
    cx, where = _ctx(dim_x, group), (layout, dim_x, es.GROUP_IDS[group])
    sb = _make(layout, cx)
    f = _run_up_to_failure(sb, cx, where)
    cls, code, _ = _error_class(_lib, cx.failing[min(cx.failing)])
    for g in range(f, f + 4):
        fed = {s: (None, 0) for s in cx.failing} if g > f else None
        pts, n, dt = cx.inputs(g, fed)
        out = sb.step_host(pts, n, dt, check=False)
        want = [None if s in cx.failing or not n[s] else cx.want(s, g) for s in range(len(n))]
        assert g > f or sum(w is not None for w in want) >= 3, where
        _compare(sb, out, want, n, (where, "read-out", g), rings=True)
        if g > f:
            assert all(out[2][s] == -1 for s in cx.failing), (where, g)
        _check_bits(_lib, cx, sb.errors(), (where, g))
        with pytest.raises(cls) as ei:
            sb.check()
        assert ei.value.code == code, (where, g, ei.value.code)
    sb.close()


# The known deviation ("Errors"): every track's update ORs its bit into the scene's word and the kernels go on, and
# first_scene_error tests DIVZERO before SINGULAR -- right for the NEXT frames of a scene whose division failed, whose inf / NaN
# the later inversions report as singular.  In ONE _update_all whose first track has a singular S and whose second has
# (N_est - 1) N == 0 the reference raises LinAlgError and mmw_check reports MMW_E_DIVZERO.  Telling the two apart needs a record
# written where the bit is set; every form of it that was built moved the register allocation of k_scene, k_track, k_predict and
# k_post past the spill ceilings of tests/test_cabi_exports.py, i.e. changed what an error-free frame executes: left for a change
# with its own benchmark evidence.  Only the code assertion of this one scene is marked; everything else about it is asserted.
KNOWN_DEVIATION = "both_singular_first"


def _two_failing_tracks(layout, dim_x, name):
    """(the code mmw_check reports on the failing frame, the code the oracle's rc maps to); everything else is asserted here."""
    from mmwave_msc_amd import _lib
    group = es.GROUP_IDS.index("update_singular+both")
    cx, where = _ctx(dim_x, group, (name,)), (layout, dim_x, name)
    assert cx.names == [None, name, None, None] and cx.failing == {1: es.EXPECT[name][0]}
    sb = _make(layout, cx)
    f = _run_up_to_failure(sb, cx, where)
    assert sb.num_tracks()[1] == 2
    cls, code, bit = _error_class(_lib, cx.failing[1])
    pts, n, dt = cx.inputs(f)
    out = sb.step_host(pts, n, dt, check=False)
    _compare(sb, out, [None if s == 1 else cx.want(s, f) for s in range(4)], n, (where, f), rings=True)
    err = sb.errors()
    assert err[1] & bit and err[1] & ~3 == 0 and err[0] == err[2] == err[3] == 0, (where, err)
    codes = []
    for g in (f, f + 1):
        with pytest.raises(_lib.MmwError) as ei:
            sb.check()
        assert isinstance(ei.value, (_lib.MmwSingular, _lib.MmwDivZero)), (where, type(ei.value))
        codes.append(ei.value.code)
        if g == f:                                                 # one more frame on the broken scene: its failing frame's rows again
            sb.step_host(*cx.inputs(f + 1, {1: (cx.scenes[1], f)}), check=False)
    assert codes[0] == codes[1], (where, "the reported code changed with the next frame", codes)
    assert sb.errors()[0] == sb.errors()[2] == sb.errors()[3] == 0, where
    sb.close()
    return codes[0], code, where


@pytest.mark.parametrize("name", ["both_singular_first", "both_divzero_first"])
@pytest.mark.parametrize("dim_x", es.DIM_X)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_two_failing_tracks_report_the_error_the_reference_raises_first(layout, dim_x, name):
    """One _update_all with a singular S on one track and (N_est - 1) N == 0 on the other, in both list orders: the reference
    raises for the track it updates FIRST (rc -2 | -3 of the oracle; LinAlgError | ZeroDivisionError of py_tracker and the live
    reference: tests/golden/track_exceptions.npz).  The scene's word holds the oracle's bit, the bystanders stay bit-equal and
    clean, mmw_check's code is the oracle's rc, and after one more frame on the broken scene under check=False it is still that
    code (the case the comment in first_scene_error describes).  For both_singular_first the code assertion alone is the known
    deviation: test_both_singular_first_reports_linalgerror."""
    got, want, where = _two_failing_tracks(layout, dim_x, name)
    if name != KNOWN_DEVIATION:
        assert got == want, (where, "mmw_check reports", got, "the oracle's rc maps to", want)


@pytest.mark.xfail(strict=True, reason="known deviation: both bits are set in one _update_all and first_scene_error reports DIVZERO first; the reference "
                                       "raises LinAlgError for the track it updates first (DESIGN.md, Errors)")
@pytest.mark.parametrize("dim_x", es.DIM_X)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_both_singular_first_reports_linalgerror(layout, dim_x):
    """The one assertion the kernels miss: measured on an MI355X under all four layouts and both dim_x, mmw_check reports -3
    (MMW_E_DIVZERO) where the oracle's rc -2 maps to -2 (MMW_E_SINGULAR)."""
    got, want, where = _two_failing_tracks(layout, dim_x, KNOWN_DEVIATION)
    assert got == want, (where, "mmw_check reports", got, "the oracle's rc maps to", want)


@pytest.mark.parametrize("dim_x", es.DIM_X)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_fp32_entry_reports_the_same_errors(layout, dim_x):
    """mmw_step_f32 on the update_singular group (every row is float32-exact): up to the failing frame by bits, then mmw_check
    raises the first failing scene's class and the bits are the oracle's; the bystanders' results of the failing frame are theirs."""
    from mmwave_msc_amd import _lib
    cx, where = _ctx(dim_x, es.GROUP_IDS.index("update_singular+both")), (layout, dim_x, "fp32")
    sb = _make(layout, cx)
    S, M = len(cx.scenes), es.MAX_PTS
    b_a, b_l, b_n = sb.buf("assoc", S * M * 4), sb.buf("labels", S * sb.UM * 4), sb.buf("db_n", S * 4)
    for f in range(cx.at + 1):
        pts, n, dt = cx.inputs(f)
        p32 = pts.astype(np.float32)
        assert np.array_equal(p32.astype(np.float64), pts)
        b_p, b_c, b_d = sb.buf("pts32", S * M * 32).upload(p32), sb.buf("n", S * 4).upload(n), sb.buf("dt", S * 8).upload(dt)
        b_a.upload(np.full(S * M, -7, np.int32)); b_l.upload(np.full(S * sb.UM, -7, np.int32)); b_n.upload(np.full(S, -7, np.int32))
        sb.step_dev_f32(b_p.ptr, b_c.ptr, b_d.ptr, b_a.ptr, b_l.ptr, b_n.ptr)
        sb.synchronize()
        out = (b_a.download((S, M), np.int32), b_l.download((S, sb.UM), np.int32), b_n.download((S,), np.int32))
        want = [None if (f == cx.at and s in cx.failing) else cx.want(s, f) for s in range(S)]
        _compare(sb, out, want, n, (where, f))
    cls, code, _ = _error_class(_lib, cx.failing[min(cx.failing)])
    with pytest.raises(cls) as ei:
        sb.check()
    assert ei.value.code == code
    _check_bits(_lib, cx, sb.errors(), where)
    sb.close()


@pytest.mark.parametrize("name,exc", [("update_singular", np.linalg.LinAlgError), ("update_divzero_est", ZeroDivisionError), ("nest_zero", ZeroDivisionError),
                                      ("gate_zero", np.linalg.LinAlgError)])
def test_dropin_trackbuffer_raises_what_the_reference_raises(monkeypatch, name, exc):
    """tracking.TrackBuffer on a failing scene: `except np.linalg.LinAlgError` and `except ZeroDivisionError` catch what the
    reference would have raised, on the frame it would have raised it."""
    from mmwave_msc_amd import constants as const
    from mmwave_msc_amd.tracking import BatchedData, TrackBuffer
    from tests._fuzz import reference_overrides
    sc, r = es.scenes(9)[name], es.replays(9)[name]
    for k, v in reference_overrides(sc.cfg).items():
        monkeypatch.setattr(const, k, getattr(const, v) if k == "MOTION_MODEL" else v)
    tb, batch = TrackBuffer(max_pts=es.MAX_PTS), BatchedData()
    caught = None
    for f in range(len(sc.cnt)):
        tb.dt = float(sc.dt[f])
        try:
            tb.track(sc.pts[f, : sc.cnt[f]], batch)
        except (np.linalg.LinAlgError, ZeroDivisionError) as e:
            caught = (type(e), f)
            break
        assert np.array_equal(tb.last_assoc, r.frames[f].assoc), (name, f)
    assert caught is not None and issubclass(caught[0], exc) and caught[1] == r.at, (name, caught, r.at)
    assert issubclass(caught[0], np.linalg.LinAlgError) == (exc is np.linalg.LinAlgError)
