"""The decision-edge inputs of tests/_edge_inputs.py are sharp -- shown here on the C oracle alone, without a GPU -- and the
oracle's decisions on the equality scenes are the reference's (tests/golden/decision_edges.npz, recorded from the reference by
oracle/gen_golden.py --only decision_edges).

Sharpness of the gate probes: the probe rows (two per ray) whose association differs between the gates G - k ulp and G + k ulp,
G = 4.5, per scene (seed, tracks) = (1, 3), (2, 3), (3, 3), (4, 12) of a context:

  dim_x  max_pts  probe rows   +-1 ulp              +-2 ulp
      6      256         216    34 /  40 /  34 /  28    49 /  71 /  72 /  57
      6      320         272    45 /  47 /  41 /  32    67 /  86 /  87 /  66
      6     1024         888   124 / 134 / 128 / 100   241 / 280 / 282 / 197
      9      256         216    29 /  34 /  35 /  21    62 /  66 /  57 /  36
      9      320         272    36 /  40 /  40 /  23    78 /  79 /  70 /  41
      9     1024         888   122 / 127 / 125 /  88   254 / 267 / 238 / 170

At least one eighth of a scene's probe rows must flip within +-2 ulp (test_gate_sweep_moves_an_eighth_of_the_probes); at +-64
ulp all of them do.  The tie probes do not move with the gate at all: they sit on `d_j < d_k`, not on `d < tr_gate`."""
import json
import os

import numpy as np
import pytest

from tests import _edge_inputs as ei
from tests._golden import GOLDEN, F64_FIELDS, INT_FIELDS, assert_tracks_match

CONTEXTS = [(m, d) for m in ei.MAX_PTS for d in ei.DIM_X]


def _all_probes(max_pts, dim_x):
    return ei.gate_context(max_pts, dim_x) + ei.tie_context(max_pts, dim_x)[0]


@pytest.mark.parametrize("max_pts,dim_x", CONTEXTS)
def test_pairs_are_adjacent_doubles_that_decide_differently(max_pts, dim_x):
    for p in _all_probes(max_pts, dim_x):
        assert np.array_equal(p.t[:, 1], np.nextafter(p.t[:, 0], np.inf)), p.scene.tag
        a = replay_probe_frame(p, p.gates[2])
        assert np.array_equal(a, p.assoc[2])
        assert np.array_equal(a[p.pos[:, 0]], p.track) and np.all(a[p.pos[:, 1]] != p.track), p.scene.tag
    for p in ei.tie_context(max_pts, dim_x)[0]:                       # the row passes from one track to ANOTHER
        a = p.assoc[2]
        assert np.array_equal(a[p.pos[:, 1]], p.other) and np.all(p.other >= 0) and np.all(p.other != p.track), p.scene.tag
        assert len(p.pos) >= 16 and len(set(map(tuple, np.stack([p.track, p.other], 1).tolist()))) >= 2


def replay_probe_frame(p, gate, **kw):
    return ei.replay(p.scene, upto=p.frame + 1, tr_gate=gate, **kw)[p.frame].assoc


@pytest.mark.parametrize("max_pts,dim_x", CONTEXTS)
def test_gate_sweep_moves_an_eighth_of_the_probes(max_pts, dim_x):
    for p in ei.gate_context(max_pts, dim_x):
        a = np.stack([replay_probe_frame(p, g) for g in p.gates])
        assert np.array_equal(a, p.assoc)                              # what the GPU test expects IS the oracle under that gate
        rows = p.pos.reshape(-1)
        flips = {k: int(np.sum(a[2 - k, rows] != a[2 + k, rows])) for k in (1, 2)}
        print(f"dim_x {dim_x} max_pts {max_pts} {p.scene.tag}: {len(rows)} probe rows, {flips[1]} flip within +-1 ulp, {flips[2]} within +-2 ulp")
        assert flips == p.flips and 8 * flips[2] >= len(rows), (p.scene.tag, flips, len(rows))
        taken = (a[:, rows] >= 0).sum(axis=1)
        assert np.all(np.diff(taken) >= 0) and taken[-1] > taken[0], taken     # a wider gate takes more
        wide = replay_probe_frame(p, p.gates[2] + 64 * (p.gates[3] - p.gates[2]), track_cap=64)   # (the refused rows cluster: room for them)
        narrow = replay_probe_frame(p, p.gates[2] - 64 * (p.gates[3] - p.gates[2]), track_cap=64)
        assert np.all(wide[p.pos[:, 1]] == p.track) and np.all(narrow[p.pos[:, 0]] != p.track), p.scene.tag   # at +-64 ulp: all


@pytest.mark.parametrize("max_pts,dim_x", CONTEXTS)
def test_history_does_not_depend_on_the_gate(max_pts, dim_x):
    for p in ei.gate_context(max_pts, dim_x):
        runs = [ei.replay(p.scene, upto=p.frame, tr_gate=g) for g in p.gates]
        for f in range(p.frame):
            ref = runs[2][f]
            assert ref.n_tracks == {3: 3, 12: 12}[len(np.unique(p.track))]
            for r in runs:
                assert r[f].tracks.tobytes() == ref.tracks.tobytes() and np.array_equal(r[f].assoc, ref.assoc), (p.scene.tag, f)


@pytest.mark.parametrize("max_pts,dim_x", CONTEXTS)
def test_probes_are_spread_over_the_frame_and_the_buffer_past_n_is_inside_a_gate(max_pts, dim_x):
    for p in _all_probes(max_pts, dim_x):
        sc = p.scene
        n = int(sc.cnt[p.frame])
        rows = set(p.pos.reshape(-1).tolist())
        assert {0, n - 1} <= rows and {s for s in ei.SEAMS if s < n} <= rows and n < max_pts, sc.tag
        quarters = np.histogram(sorted(rows), bins=4, range=(0, n))[0]
        assert quarters.min() * 6 > quarters.max(), quarters
        for f in range(1, len(sc.cnt)):                                # rows at and beyond n: a kernel that gated them would take them
            whole = sc._replace(cnt=np.where(np.arange(len(sc.cnt)) == f, max_pts, sc.cnt).astype(np.int32))
            a = ei.replay(whole, upto=f + 1)[f].assoc
            assert np.all(a[int(sc.cnt[f]):] >= 0), (sc.tag, f)


@pytest.mark.parametrize("max_pts", ei.MAX_PTS + (128,))
@pytest.mark.parametrize("gate", [ei.GATE, ei.TIE_GATE])
def test_exact_tie_goes_to_the_first_track_in_both_orders(max_pts, gate):
    for dim_x in ei.DIM_X:
        for order in ("AB", "BA"):
            tie = ei.exact_tie(ei.gate_kw(dim_x, gate), max_pts, order)
            fr = ei.replay(tie.scene)
            ei.check_exact_tie(tie, fr)
            n = int(tie.scene.cnt[tie.frame])
            assert {s for s in (256, 512, 768) if s < n - 1} <= set(tie.mid.tolist()) and 1 in tie.mid and n - 2 in tie.mid
            assert fr[tie.frame].tracks["point_num"].sum() == n       # every row of the frame went to A or to B


@pytest.mark.parametrize("name", list(ei.equality_scenes()))
def test_equality_is_met_exactly_and_the_next_frame_behaves(name):
    eq = ei.equality_scenes()[name]
    eq.check(ei.replay(eq.scene))


@pytest.mark.parametrize("dim_x", ei.DIM_X)
@pytest.mark.parametrize("name", list(ei.dt_edges(6)))
def test_interval_edge_sits_where_it_is_claimed(name, dim_x):
    """The frame-interval edges (inexact lifetime sums on both sides of `lifetime > lim`, lifetime + dt == 0, a lifetime that stands
    still, a 60 s predict with rows on both sides of its gate): each scene's own check, on an oracle replay."""
    eq = ei.dt_edges(dim_x)[name]
    eq.check(ei.replay(eq.scene))


def test_interval_edges_decide_differently_on_one_rounding():
    """0.1 + 0.2 and 0.15 + 0.15 against the limit 0.3: the first pair drops the track on its second frame, the second keeps it, for
    the dynamic and for the static track; an interval of 2^-60 is absorbed, one of 2^-54 is not."""
    assert 0.1 + 0.2 == float.fromhex("0x1.3333333333334p-2") and 0.15 + 0.15 == 0.3 == float.fromhex("0x1.3333333333333p-2")
    for dim_x in ei.DIM_X:
        e = ei.dt_edges(dim_x)
        for which, kept in (("dynamic", 1), ("static", 0)):
            over, equal = ei.replay(e[f"{which}_sum_over"].scene), ei.replay(e[f"{which}_sum_equal"].scene)
            assert [fr.n_tracks for fr in over] == [2, 2, 1, 1] and [fr.n_tracks for fr in equal] == [2, 2, 2, 2, 1, 1]
            assert over[2].tracks["is_static"][0] == equal[4].tracks["is_static"][0] == kept     # the OTHER track is the one left
        assert len(ei.dt_edge_groups(dim_x)) == 4


def test_equality_constants_are_exact_in_binary():
    a, n = ei._n_est_constants()
    assert (1 - a) * float(n) + a * float(n) != float(n)
    for f in range(1, 8):
        assert sum([ei.EQ_DT] * f) == f / 8
    assert np.sqrt((0.1875 * 0.1875 + 0.25 * 0.25) + 0.0) == 0.3125
    assert 0.125 * 4 / 2 == ei.SPREAD_LIM[0] and 0.25 * 4 / 2 == 2 * ei.SPREAD_LIM[1]


@pytest.mark.parametrize("name", list(ei.equality_scenes()))
def test_oracle_equals_the_reference_recording(name):
    """Integers (association, labels, n_tracks, is_static, point_num, ring_len, ring_n, the global ring, feature owners) and
    `lifetime` exact; the other floats within tests/_golden.py's tolerance, as tests/test_oracle_golden.py compares a recording."""
    z = np.load(os.path.join(GOLDEN, "decision_edges.npz"), allow_pickle=False)
    sc = ei.equality_scenes()[name].scene
    g = {k[len(name) + 2:]: z[k] for k in z.files if k.startswith(name + "__")}
    assert np.array_equal(g["pts"], sc.pts) and np.array_equal(g["cnt"], sc.cnt) and np.array_equal(g["dt"], sc.dt), "the recording is of other inputs"
    assert json.loads(str(g["cfg"])) == json.loads(json.dumps(sc.cfg))
    frames = ei.replay(sc)
    for f, fr in enumerate(frames):
        c, ctx = int(sc.cnt[f]), f"{name} f{f}"
        assert np.array_equal(fr.assoc, g["assoc"][f, :c]), ctx
        dbn = int(g["db_n"][f])
        assert (fr.labels is None) == (dbn < 0), ctx
        if dbn >= 0:
            assert np.array_equal(fr.labels, g["labels"][f, :dbn]), ctx
        nt = int(g["n_tracks"][f])
        assert fr.n_tracks == nt, ctx
        want = g["tracks"][f, :nt]
        assert np.array_equal(fr.tracks["lifetime"], want["lifetime"]), ctx
        assert_tracks_match(fr.tracks, want, ctx=ctx)
        assert len(fr.batch_ring) == g["ring_len"][f] and np.array_equal(fr.batch_ring, g["ring_n"][f, : len(fr.batch_ring)]), ctx
        assert np.array_equal(fr.owner, g["owner"][f, : int(g["n_feat"][f])]), ctx
    assert set(INT_FIELDS + F64_FIELDS) <= set(g["tracks"].dtype.names)
