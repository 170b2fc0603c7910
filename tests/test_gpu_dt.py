"""The tracker on finite frame intervals outside 0.05 .. 0.2 s, every layout against the C oracle, bit for bit.

Every other differential test draws dt from that band or uses 0.1 / 2^-3.  dt enters the step as `lifetime + dt` in the predict --
F carries dtm and dtm^2 / 2, Q dtm^4 / 4 .. dtm, the 6 x 6 gate matrix is inverted from the result; the arithmetic exists three
times, in k_predict (track-wise), k_track (per scene) and k_scene (one workgroup) -- and as `lifetime += dt`, `lifetime > lim`;
and it is per scene and per frame: one k_predict launch walks tracks of scenes with different dt.  A kernel that drops a term
that is tiny at 0.1 s, or sums the lifetime in another order, passes everything else.

  schedules   tests/_fuzz.py DT_SCHEDULES (zero, tiny, short, inexact, long1, long5, long60, hour, negative, mixed, per_scene) on
              the seeds of tests/_dt_cases.py, which are chosen so that the odd intervals meet live tracks (asserted on the oracle
              here too, and without a GPU in tests/test_reference_dt.py, which also holds the oracle to the live reference on the
              same seeds): tests/test_gpu_fuzz.py::run_case with the intervals replaced, <= 4 scenes of <= 300 points, 12 frames
  edges       tests/_edge_inputs.py dt_edges: 0.1 + 0.2 > 0.3 == 0.15 + 0.15 against a limit of 0.3, lifetime + dt == 0, a lifetime
              that stands still over five dt = 0 frames, a 60 s predict with rows an ulp inside and outside its gate; each asserted
              on the oracle first (tests/test_edge_inputs.py), for dim_x 6 and 9

NO expected value comes from a GPU call.  Any finite double is an interval; NaN and +-inf are not pinned here."""
import functools

import numpy as np
import pytest

from tests import _dt_cases as dc
from tests import _edge_inputs as ei
from tests._fuzz import DT_SCHEDULES, draw_case, dt_schedule
from tests._golden import F64_FIELDS, assert_tracks_match
from tests._layouts import LAYOUTS, make_checked

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _reference(seed, name):
    """Once per (seed, schedule): the case, its intervals, and the oracle's tally under them with the conditions that make the
    pair worth a GPU run (tests/_dt_cases.py: check).  run_case steps its own oracle scenes beside the context, frame by frame."""
    case = draw_case(seed, **dc.GPU_SIZE)
    dts = dt_schedule(case, name)
    dts.setflags(write=False)
    return case, dts, dc.check(seed, name, dc.GPU_SIZE["max_scenes"])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", DT_SCHEDULES)
@pytest.mark.parametrize("seed", dc.SEEDS)
def test_interval_schedule_vs_oracle(seed, name, layout):
    from tests.test_gpu_fuzz import run_case
    case, dts, tally = _reference(seed, name)
    seen = run_case(dict(case), layout, dts=dts)
    assert "raised" not in seen and tally["raised"] == 0


# ------------------------------------------------------------------------------------------------------------ planted edges
@functools.lru_cache(maxsize=None)
def _want_edges(dim_x, group):
    eqs = [ei.dt_edges(dim_x)[name] for name in ei.dt_edge_groups(dim_x)[group]]
    want = [ei.replay(eq.scene) for eq in eqs]
    for eq, w in zip(eqs, want):
        eq.check(w)
    return eqs, want


def _bits_equal(got, want, ctx):
    """x, P, lifetime and the rest of the fp64 state by their bits: +0.0 is not -0.0 here."""
    for name in F64_FIELDS:
        g, w = np.ascontiguousarray(got[name]).view(np.uint64), np.ascontiguousarray(want[name]).view(np.uint64)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError(f"{ctx}: field {name} differs in its bits at {bad[:6].tolist()} ({len(bad)} entries): got "
                                 f"{np.asarray(got[name])[tuple(bad[0])]!r} want {np.asarray(want[name])[tuple(bad[0])]!r}")


@pytest.mark.parametrize("group", range(4), ids=["dynamic_sums", "static_sums", "dtm_zero+stands_still", "long_predict"])
@pytest.mark.parametrize("dim_x", ei.DIM_X)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_interval_edges_vs_oracle(layout, dim_x, group):
    """One context per configuration of the interval edges; after every frame association, labels, db_n, the track list -- every
    fp64 field by its bits -- and the global ring against the oracle's replay of the same rows and intervals."""
    from tests.test_gpu_decision_edges import STEP_KIND
    eqs, want = _want_edges(dim_x, group)
    scenes = [eq.scene for eq in eqs]
    S, M = len(scenes), scenes[0].max_pts
    assert all(sc.cfg == scenes[0].cfg and sc.max_pts == M for sc in scenes)
    sb = make_checked(S, M, layout, **scenes[0].cfg)
    assert sb.step_kind() == STEP_KIND[layout] and sb.cfg.dim_x == dim_x
    for f in range(max(len(sc.cnt) for sc in scenes)):
        pts, n, dt = np.zeros((S, M, 8)), np.zeros(S, np.int32), np.full(S, ei.DT)
        for s, sc in enumerate(scenes):
            if f < len(sc.cnt):
                pts[s], n[s], dt[s] = sc.pts[f], sc.cnt[f], sc.dt[f]
        assoc, labels, dbn = sb.step_host(pts, n, dt)
        ntr = sb.num_tracks()
        trk = sb.tracks()
        ln, rn = sb.batch_ring()
        for s, sc in enumerate(scenes):
            ctx = f"{layout} dim_x {dim_x} scene {s} ({sc.tag}) frame {f}"
            if f >= len(sc.cnt):
                assert dbn[s] == -1, ctx
                w = want[s][-1]                                   # the scene is as its last frame left it
            else:
                w = want[s][f]
                c = max(int(sc.cnt[f]), 0)
                assert np.array_equal(assoc[s, :c], w.assoc), (ctx, assoc[s, :c].tolist(), w.assoc.tolist())
                assert (w.labels is None) == (dbn[s] < 0), (ctx, int(dbn[s]))
                if w.labels is not None:
                    assert dbn[s] == len(w.labels) and np.array_equal(labels[s, : dbn[s]], w.labels), ctx
            assert ntr[s] == w.n_tracks, (ctx, int(ntr[s]), w.n_tracks)
            assert_tracks_match(trk[s, : ntr[s]], w.tracks, ctx=ctx, exact=True)
            _bits_equal(trk[s, : ntr[s]], w.tracks, ctx)
            assert ln[s] == len(w.batch_ring) and np.array_equal(rn[s, : ln[s]], w.batch_ring), (ctx, "the global ring")
    assert sb.step_kind() == STEP_KIND[layout]
    sb.check()
    sb.close()
