"""Association and track lifecycle ON their decision edges (tests/_edge_inputs.py), every layout against the C oracle.

The fuzz and parity tests compare what track() decided; a random point sits some 1e14 ulps from `d < tr_gate` and from the
nearest `d_j < d_k`, so a gate distance d = log|det C| + y'C^-1 y that is wrong in its last bits passes them all.  These scenes
put rows on the surface itself -- pairs of ADJACENT doubles the oracle decides differently, run under five adjacent gates --, on
exact ties between tracks, and on the equality side of `lifetime > lim`, `speed < tr_vel_thres`, the spread clamps, `nj > N_est`,
`T < tr_max_tracks`, `total > model_min_input`, 64 | 65 and ring_rows | ring_rows + 1 rows, and (`feature_ties`) on equal x among
a track's rows and x equal to the centroid's in the feature maps' sort.  That the inputs are that sharp is shown without a GPU
in tests/test_edge_inputs.py.

NO expected value in this file comes from a GPU call: every `want` is oracle.c_oracle.OracleScene's on the same rows under the
context's own tr_gate.  Everything is compared by bits after every frame: association, labels, db_n, the track list, the global
ring; the records after the probe frame carry the probes' rows, so a flipped decision also shows in point_num, the centroid
and P.  Rows of the input buffer at and beyond the frame's count lie well inside a gate: gating one changes the same fields."""
import functools

import numpy as np
import pytest

from tests import _edge_inputs as ei
from tests._golden import assert_tracks_match
from tests._layouts import LAYOUTS, make_checked

pytestmark = pytest.mark.gpu

# mmw_step_kind of a context of a few scenes under each layout: _predict_all inside k_track and the records through the scalar
# cache in the same launch (2), k_predict before k_track (4), k_scene (1)
STEP_KIND = {"per_scene": 2, "track_wise": 4, "track_wise+side_stream": 4, "one_workgroup": 1}


@functools.lru_cache(maxsize=None)
def _want_gate(max_pts, dim_x, gate_k):
    probes = ei.gate_context(max_pts, dim_x)
    gate = probes[0].gates[gate_k]
    assert all(p.gates == probes[0].gates for p in probes)
    want = [ei.replay(p.scene, tr_gate=gate) for p in probes]
    for p, w in zip(probes, want):
        assert np.array_equal(w[p.frame].assoc, p.assoc[gate_k])
    return probes, gate, want


@functools.lru_cache(maxsize=None)
def _want_ties(max_pts, dim_x):
    probes, ties = ei.tie_context(max_pts, dim_x)
    scenes = [p.scene for p in probes] + [t.scene for t in ties]
    return probes, ties, scenes, [ei.replay(sc) for sc in scenes]


@functools.lru_cache(maxsize=None)
def _want_equalities(group):
    eqs = [ei.equality_scenes()[name] for name in ei.equality_groups()[group]]
    return eqs, [ei.replay(eq.scene) for eq in eqs]


def _context(layout, scenes, **over):
    kw = dict(scenes[0].cfg, **over)
    assert all(sc.cfg == scenes[0].cfg and sc.max_pts == scenes[0].max_pts for sc in scenes)
    sb = make_checked(len(scenes), scenes[0].max_pts, layout, **kw)
    assert sb.step_kind() == STEP_KIND[layout], (layout, sb.step_kind())
    assert sb.cfg.tr_gate == kw.get("tr_gate", 4.5) and sb.track_cap == kw["track_cap"]
    return sb


def _compare_frame(sb, scenes, want, f, out, where, features=(), rings=()):
    """Everything the context holds after frame f against the oracle's Frame of every scene."""
    assoc, labels, dbn = out
    ntr = sb.num_tracks()
    trk = sb.tracks()
    ln, rn = sb.batch_ring()
    feat = owner = None
    if any(f in fs for fs in features):
        feat, owner = sb.features_host()
    row = 0
    for s, sc in enumerate(scenes):
        w = want[s][f] if f < len(want[s]) else None
        ctx = f"{where} scene {s} ({sc.tag}) frame {f}"
        if w is None:                                            # the frame never reached track(): the scene is as it was
            assert dbn[s] == -1, ctx
            row += 0 if feat is None else int(np.sum(owner[:, 0] == s))
            continue
        c = int(sc.cnt[f])
        if not np.array_equal(assoc[s, :c], w.assoc):
            bad = np.flatnonzero(assoc[s, :c] != w.assoc)
            raise AssertionError(f"{ctx}: association differs on {len(bad)} rows, first {bad[:8].tolist()}: got {assoc[s, bad[:8]].tolist()} "
                                 f"want {w.assoc[bad[:8]].tolist()}")
        assert (w.labels is None) == (dbn[s] < 0), (ctx, int(dbn[s]))
        if w.labels is not None:
            assert dbn[s] == len(w.labels) and np.array_equal(labels[s, : dbn[s]], w.labels), ctx
        assert ntr[s] == w.n_tracks, (ctx, int(ntr[s]), w.n_tracks)
        assert_tracks_match(trk[s, : ntr[s]], w.tracks, ctx=ctx, exact=True)
        assert ln[s] == len(w.batch_ring) and np.array_equal(rn[s, : ln[s]], w.batch_ring), (ctx, "the global ring")
        if features and f in features[s]:
            k = len(w.owner)
            assert np.all(owner[row: row + k, 0] == s) and np.array_equal(owner[row: row + k, 1], w.owner), (ctx, "feature owners")
            assert np.array_equal(feat[row: row + k], w.feat), (ctx, "feature tensors")
            row += k
        elif feat is not None:
            row += int(np.sum(owner[:, 0] == s))
        if rings and f in rings[s]:
            for t in range(w.n_tracks):
                for k, rows in enumerate(w.rings[t]):
                    assert np.array_equal(sb.track_ring_frame(s, t, k), rows), (ctx, "ring frame", t, k)
    if feat is not None:
        assert row == len(owner), where


def _inputs(scenes, f):
    S, M = len(scenes), scenes[0].max_pts
    pts, n, dt = np.zeros((S, M, 8)), np.zeros(S, np.int32), np.full(S, ei.DT)
    for s, sc in enumerate(scenes):
        if f < len(sc.cnt):
            pts[s], n[s], dt[s] = sc.pts[f], sc.cnt[f], sc.dt[f]
    return pts, n, dt


def _run(sb, layout, scenes, want, where, **kw):
    for f in range(max(len(sc.cnt) for sc in scenes)):
        out = sb.step_host(*_inputs(scenes, f))
        _compare_frame(sb, scenes, want, f, out, where, **kw)
    assert sb.step_kind() == STEP_KIND[layout]                   # ... to the end
    sb.check()
    sb.close()


@pytest.mark.parametrize("gate_k", range(5), ids=["G-2ulp", "G-1ulp", "G", "G+1ulp", "G+2ulp"])
@pytest.mark.parametrize("dim_x", ei.DIM_X)
@pytest.mark.parametrize("max_pts", ei.MAX_PTS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_gate_surface_vs_oracle(layout, max_pts, dim_x, gate_k):
    """Four scenes (three tracks, one with twelve: the T > 10 arm of k_track's column sums, a longer gate chain) whose fourth frame
    holds pairs of rows an ulp apart on a ray, one inside a track's gate and one outside (G = 4.5), at rows 0, n - 1, both sides
    of every q * 256 + tid seam and all over the frame; max_pts gives 1, 2 and 4 points per thread.  One context per gate G - 2 ulp
    .. G + 2 ulp: between the outermost two an eighth to a third of the probe rows changes its decision in the oracle
    (tests/test_edge_inputs.py), and the context must follow."""
    probes, gate, want = _want_gate(max_pts, dim_x, gate_k)
    scenes = [p.scene for p in probes]
    sb = _context(layout, scenes, tr_gate=gate)
    _run(sb, layout, scenes, want, (layout, max_pts, dim_x, gate_k))


@pytest.mark.parametrize("dim_x", ei.DIM_X)
@pytest.mark.parametrize("max_pts", ei.MAX_PTS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_ties_between_tracks_vs_oracle(layout, max_pts, dim_x):
    """`d_j < d_k` and first-best on a tie: rows that pass from track j to track k between two adjacent doubles (gates that
    overlap: tr_gate = 16, targets 1.3 m apart), and the exact tie -- clusters that are exact translations of each other, the row
    at the exact midpoint of the predicted positions, d_A == d_B -- with the clusters in either order: the midpoint goes to
    track 0, its neighbours 2^-10 to either side to A and to B."""
    probes, ties, scenes, want = _want_ties(max_pts, dim_x)
    for tie, w in zip(ties, want[len(probes):]):
        ei.check_exact_tie(tie, w)
    sb = _context(layout, scenes)
    _run(sb, layout, scenes, want, (layout, max_pts, dim_x))


@pytest.mark.parametrize("dim_x", ei.DIM_X)
@pytest.mark.parametrize("max_pts", [320, 1024])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_fp32_entry_on_the_gate(layout, max_pts, dim_x):
    """mmw_step_f32 / load_point_row<true> with 2 and 4 points per thread.  A float32 row cannot be moved onto the surface, so the
    gate is moved onto the row (_edge_inputs.f32_gate_probe): d == g exactly -- the row, at rows 0, n - 1 and both sides of every
    seam, is refused by the context created with tr_gate = g and taken by the one created with nextafter(g)."""
    fp = ei.f32_gate_probe(max_pts, dim_x)
    sc, M = fp.scene, max_pts
    for gate, taken in ((fp.gate, False), (fp.gate_up, True)):
        want = ei.replay(sc, tr_gate=gate)
        assert np.all((want[fp.frame].assoc[fp.rows] == fp.track) == taken)
        sb = _context(layout, [sc], tr_gate=gate)
        b_a, b_l, b_n = sb.buf("assoc", M * 4), sb.buf("labels", sb.UM * 4), sb.buf("db_n", 4)
        for f in range(len(sc.cnt)):
            p32 = sc.pts[f].astype(np.float32)
            assert np.array_equal(p32.astype(np.float64), sc.pts[f])                 # the fp32 entry sees the oracle's values
            b_p = sb.buf("pts32", M * 32).upload(p32)
            b_c, b_d = sb.buf("n", 4).upload(sc.cnt[f: f + 1]), sb.buf("dt", 8).upload(sc.dt[f: f + 1])
            b_a.upload(np.full(M, -7, np.int32)); b_l.upload(np.full(sb.UM, -7, np.int32)); b_n.upload(np.full(1, -7, np.int32))
            sb.step_dev_f32(b_p.ptr, b_c.ptr, b_d.ptr, b_a.ptr, b_l.ptr, b_n.ptr)
            sb.synchronize()
            out = (b_a.download((1, M), np.int32), b_l.download((1, sb.UM), np.int32), b_n.download((1,), np.int32))
            _compare_frame(sb, [sc], [want], f, out, (layout, max_pts, dim_x, "taken" if taken else "refused"))
            if f == fp.frame:
                assert np.all((out[0][0, fp.rows] == fp.track) == taken), (layout, max_pts, dim_x, gate, out[0][0, fp.rows])
        assert sb.step_kind() == STEP_KIND[layout]
        sb.check()
        sb.close()


@pytest.mark.parametrize("group", range(len(ei.equality_groups())), ids=["+".join(g) for g in ei.equality_groups()])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_equality_scenes_vs_oracle(layout, group):
    """The equality side of every comparison track() takes (tests/_edge_inputs.py equality_scenes: constants exact in binary, the
    equality asserted on the oracle, the oracle equal to the reference's recording -- tests/test_edge_inputs.py): a context per
    configuration; after every frame association, labels, db_n, the track list and the global ring; features_host() owners and
    tensors on the frames of the feature scenes; the stored ring frames where a track takes 64 | 65 and ring_rows | ring_rows + 1
    rows."""
    eqs, want = _want_equalities(group)
    scenes = [eq.scene for eq in eqs]
    sb = _context(layout, scenes)
    if "ring_rows" in scenes[0].cfg:
        assert sb.ring_rows == scenes[0].cfg["ring_rows"]
    _run(sb, layout, scenes, want, (layout, ei.equality_groups()[group]), features=[eq.feature_frames for eq in eqs],
         rings=[eq.ring_frames for eq in eqs])
