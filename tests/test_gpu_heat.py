"""The dwell heat maps (mmw_heat_*, include/mmw.h) on the GPU: per scene zero or one grid, per cell the time live tracks spent in it,
the samples taken in it and the visits that began in it, exported as a stream compaction of the cells with samples > 0.

Expected values come from tests/_heat_ref.py, a numpy restatement of the header section applied to the state read back with
`tracks()` / `num_tracks()` after each step; it carries its own grids, cells, uid memory and scene words.  Every field of every row
and cell is compared by its bytes, `dwell` included -- there is no tolerance anywhere: both sides take one fp64 subtraction and one
fp64 division per coordinate, one subtraction per interval and one addition per credited interval, tracks in list order (the library
is built with -ffp-contract=off).

What a sample reads is what the track records hold when its kernel runs, so the edge cases plant positions through an edited
snapshot blob (tests/_snap_plant.py) and sample several times without a step in between: the uids stay, the
positions and times are chosen."""
import numpy as np
import pytest

from tests._feature_run import BASE, REPORT, S2, TRACKS, HeatRun, cut, nothing_else_moves, same_pair, settled, step_empty
from tests._heat_ref import HeatRef, cell_of
from tests._layouts import make_checked
from tests._report_scenes import CFG_KW, F, N, S, scenario
from tests._snap_plant import FAR, directory, dts as _dts, plant_state, plant_tracks, plant_xy as _plant_xy, record_at

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
NO_GRID = (5, 17)
NOUNS = HeatRun.nouns


def _settled(n_scenes=S2, frames=4, cells=128, **cfg):
    """A context whose scenes hold tracks that stay (lifetimes of 100 s), heat enabled behind them."""
    return settled(lambda sb, data: HeatRun(sb, cells, data), n_scenes, frames, long_lived=True, **cfg)


def _room(s, cap_shape, x0=-4.0, y0=0.0):
    """The grid of scene s in the scenario tests: nx * ny of 63, 64, 65 and the enabled capacity in turn, wide and tall by turns; the
    capacity grid covers the whole room, the small ones a strip of it.  cell = 0.25 and corners on multiples of it: every boundary is exact."""
    small = [(21, 3), (4, 16), (13, 5), (3, 21), (16, 4), (5, 13)]
    if s % 4 == 3:
        return dict(x0=x0, y0=y0, cell=0.25, max_gap=(INF if s % 8 == 3 else 0.25), nx=cap_shape[0], ny=cap_shape[1], id=100 + s)
    nx, ny = small[s % 6]
    return dict(x0=-0.25 * (nx // 2), y0=1.0 + 0.25 * (s % 5), cell=0.25, max_gap=(INF if s % 2 else 0.25), nx=nx, ny=ny, id=100 + s)


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("timed", [True, False], ids=["t", "ordinal"])
@pytest.mark.parametrize("layout,cells,cap_shape", [("per_scene", 4096, (64, 64)), ("one_workgroup", 1023, (33, 31))])
def test_scenario_sampled_and_exported_after_every_step(layout, cells, cap_shape, timed):
    """24 scenes x 96 points x 12 frames; scenes 5 and 17 have no grid.  A capacity that is a multiple of 4 and one that is not: both
    load widths of the count pass."""
    sb = make_checked(S, N, layout, **CFG_KW)
    run = HeatRun(sb, cells)
    run.set_grids([[_room(s, cap_shape)] if s not in NO_GRID else [] for s in range(S)])
    assert {int(g["nx"]) * int(g["ny"]) for g in run.ref.grid if g is not None} == {63, 64, 65, cells}
    rows = cells_ = None
    for f in range(F):
        run.step(f)
        run.sample(t=0.125 * f if timed else None)
        rows, cells_ = run.compare((layout, f))
        assert len(rows) == S - len(NO_GRID) and not np.isin(rows["scene"] - BASE, NO_GRID).any()
        assert (rows["calls"] == f + 1).all() and (rows["t_last"] == (0.125 * f if timed else float(f))).all()
    sb.check()
    sb.close()
    tally = run.ref.tally
    print("heat tallies", layout, timed, sorted(tally.items()), "cells", len(cells_), "outside", int(rows["outside"].sum()))
    # the scenario shows something: somebody stayed in a cell, somebody walked into another, somebody left the room
    assert ((cells_["samples"] >= 2) & (cells_["dwell"] > 0.0)).any()
    for key in ("credited", "revisit", "expired", "outside", "fresh"):
        assert tally[key] >= 1, (key, sorted(tally.items()))
    if timed:
        assert tally["gap_refused"] == 0                     # (0.125 <= 0.25)
    else:
        assert tally["gap_refused"] >= 1                     # (an interval of 1.0 against max_gap = 0.25)


# 2 ------------------------------------------------------------------------------------------------------------------------
def test_tracks_that_share_a_cell_add_in_list_order():
    """2, 3, 5 and all 64 tracks of a scene in ONE cell, sampled five times without a step: every call adds its interval once per track,
    one after another -- 0.1 three times is not 0.3, and behind 2^53 an interval of 2 added 64 times is lost 64 times."""
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    n = 3
    sb = SceneBatch(_lib.default_config(tr_max_tracks=64, db_min_samples=12, track_cap=64, tr_lifetime_dynamic=100.0, tr_lifetime_static=100.0), n, N)
    assert sb.track_cap == 64
    pts, cnt, dts = cut(n)
    for f in range(4):
        sb.step_host(pts[f].astype(np.float64), cnt[f], dts[f])
    assert (sb.num_tracks() >= 1).all()
    plant_tracks(sb, 0, list(range(7, -1, -1)), x0_step=0.05)      # x = 0, 0.05 .. 0.35
    plant_tracks(sb, 1, list(range(10, 18)), x0_step=0.05)
    plant_tracks(sb, 2, list(range(63, -1, -1)), x0_step=0.0)      # 64 tracks at x = 0
    ntr, trk = sb.num_tracks(), sb.tracks()
    assert ntr.tolist() == [8, 8, 64]
    sb.enable_heat(65)
    ref = HeatRef(n, 64, 65)
    # a row of cells through the tracks' y; scene 0: [-0.15, 0.1) holds x = 0, 0.05; scene 1: [-0.125, 0.125) holds three, the next cell five
    ys = [np.floor(float(trk[s, 0]["x"][1]) * 4.0) / 4.0 - 0.25 for s in range(n)]
    ng, gt = _lib.make_heat_grids([[dict(x0=x0, y0=ys[s], cell=0.25, max_gap=INF, nx=5, ny=13, id=s)] for s, x0 in enumerate((-0.15, -0.125, -0.125))])
    sb.set_heat_grids((ng, gt))
    ref.set_grids(range(n), ng, gt)
    big = 2.0 ** 53
    for k, t in enumerate((0.0, 0.1, big, big + 2.0, big + 6.0)):
        sb.sample_heat(t=t)
        ref.sample(sb.tracks(), sb.num_tracks(), t=np.full(n, t))
        rows, cells = sb.heat_host(scene_base=BASE)
        same_pair((rows, cells), ref.export(BASE), ("shared", k), NOUNS)
        if k == 0:
            assert {2, 3, 5, 64} <= set(cells["samples"].tolist()), cells["samples"].tolist()
        if k == 1:                                           # 0.1 added twice, three times, 64 times in a row
            assert 0.1 + 0.1 + 0.1 in cells["dwell"].tolist() and 0.1 + 0.1 in cells["dwell"].tolist()
    assert ref.tally["shared_max"] == 64
    c64 = cells[cells["samples"] == 5 * 64]
    want = 0.0
    for dt in (0.1, big - 0.1, 2.0, 4.0):
        for _ in range(64):
            want = want + dt
    assert len(c64) == 1 and float(c64["dwell"][0]) == want and want != 64 * 0.1 + 64 * (big - 0.1) + 64 * 2.0 + 64 * 4.0
    sb.check()
    sb.close()


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_boundaries_signed_zero_and_non_finite_positions():
    from mmwave_msc_amd import _lib
    run = _settled(2, cells=16)
    sb, ref = run.sb, run.ref
    below = lambda v: float(np.nextafter(v, -INF))
    # scene 0: grid 4 x 3 at (-1, 0.5): x spans [-1, 0), y spans [0.5, 1.25)
    g0 = dict(x0=-1.0, y0=0.5, cell=0.25, max_gap=1.0, nx=4, ny=3, id=1)
    xy0 = [(-1.0, 0.5), (below(-1.0), 0.5), (-1.0, below(0.5)), (-2.0 ** -53, 0.5), (below(0.0), 0.5), (0.0, 0.5), (-1.0, below(1.25)), (-1.0, 1.25),
           (-0.75, 0.75), (NAN, 0.5), (-1.0, NAN), (INF, 0.5), (-INF, 0.5), (-1.0, INF), (-1.0, -INF), (NAN, NAN)]
    # scene 1: the corner at the origin: -0.0 lies in cell 0 on either axis, the largest value below 0 is outside
    g1 = dict(x0=0.0, y0=0.0, cell=0.25, max_gap=1.0, nx=2, ny=2, id=2)
    xy1 = [(-0.0, -0.0), (0.0, -0.0), (-0.0, 0.25), (below(0.0), 0.0), (0.0, below(0.0)), (0.5, 0.0), (0.0, 0.5), (below(0.5), below(0.5))]
    _plant_xy(sb, 0, list(range(len(xy0))), xy0)
    _plant_xy(sb, 1, list(range(len(xy1))), xy1)
    assert sb.num_tracks().tolist() == [len(xy0), len(xy1)]
    run.set_grids([[g0], [g1]])
    run.sample(t=0.0)
    run.sample(t=0.5)
    rows, cells = run.compare("boundaries")
    # by hand: scene 0 -- inside are entries 0, 3, 6, 8 (cells 0, 3, 8, 5); scene 1 -- inside are 0, 1 (cell 0), 2 (cell 2), 7 (cell 3)
    assert [cell_of(g0, *p) for p in xy0] == [0, -1, -1, 3, -1, -1, 8, -1, 5] + [-1] * 7
    assert [cell_of(g1, *p) for p in xy1] == [0, 0, 2, -1, -1, -1, -1, 3]
    assert rows["outside"].tolist() == [2 * 12, 2 * 4] and rows["count"].tolist() == [4, 3]
    assert [(int(c["scene"]) - BASE, int(c["cell"]), int(c["samples"]), int(c["visits"]), float(c["dwell"])) for c in cells] == [
        (0, 0, 2, 1, 0.5), (0, 3, 2, 1, 0.5), (0, 5, 2, 1, 0.5), (0, 8, 2, 1, 0.5), (1, 0, 4, 2, 1.0), (1, 2, 2, 1, 0.5), (1, 3, 2, 1, 0.5)]
    sb.close()


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_max_gap_at_its_bound_and_intervals_that_are_zero_negative_or_nan():
    run = _settled(S2, cells=64)
    sb, ref = run.sb, run.ref
    for s in range(S2):                                      # one track per scene, in cell 9 of an 8 x 8 grid at the origin
        _plant_xy(sb, s, [40 + s], [(0.3, 0.3)])
    gaps = [1.0, 1.0, 1.0, INF, 2.0 ** -1074]
    run.set_grids([[dict(x0=0.0, y0=0.0, cell=0.25, max_gap=gaps[s], nx=8, ny=8, id=s)] for s in range(S2)])
    up2 = float(np.nextafter(2.0, INF))                      # 2 + 2^-51: the interval behind t = 1 is 1 + 2^-51, the one in front of t = 3 is 1 - 2^-51, both exact
    tiny = 2.0 ** -1074
    # scene 0: dt == max_gap, then just above it, then just below; 1: dt == 0, then negative; 2: a NaN t poisons this interval and the
    # next; 3: max_gap = +inf takes 1e300 and an infinite interval, not inf - inf; 4: the smallest max_gap there is takes the smallest
    # interval there is, twice, and not the next longer one
    ts = [[0.0, 1.0, up2, 3.0], [0.0, 0.0, -1.0, -0.5], [0.0, NAN, 1.0, 1.5], [0.0, 1e300, INF, INF], [0.0, tiny, 2 * tiny, 4 * tiny]]
    want = [[0.0, 1.0, 1.0, 1.0 + (3.0 - up2)], [0.0, 0.0, 0.0, 0.5], [0.0, 0.0, 0.0, 0.5], [0.0, 1e300, INF, INF], [0.0, tiny, 2 * tiny, 2 * tiny]]
    assert up2 - 1.0 > 1.0 and 3.0 - up2 < 1.0
    for k in range(4):
        run.sample(t=[ts[s][k] for s in range(S2)])
        rows, cells = run.compare(("gap", k))
        assert cells["cell"].tolist() == [9] * S2 and cells["samples"].tolist() == [k + 1] * S2 and cells["visits"].tolist() == [1] * S2
        assert cells["dwell"].tolist() == [want[s][k] for s in range(S2)], (k, cells["dwell"].tolist())
    assert ref.tally["gap_refused"] >= 1 and ref.tally["dt_not_positive"] >= 3
    sb.close()


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_visits_across_a_return_a_reset_and_a_restore():
    """Track 0 of each scene is planted alone in a grid far from everybody else, with a velocity of 1 m/s along x and no process noise:
    an empty frame moves it by its predict multiplier (tests/_snap_plant.py: dts), so it steps into the next cell
    and back.  Then one scene is reset and all are restored between samples."""
    n = 3
    run = _settled(n, cells=64, kf_q_std=0.0)
    sb, ref = run.sb, run.ref
    blob = bytearray(sb.snapshot())
    ents = directory(blob)
    for sc in range(n):
        plant_state(blob, record_at(ents, sc), [FAR + 0.125, 2.125, 1.0, 1.0, 0.0, 0.0])
    blob = bytes(blob)
    sb.restore(blob)
    run.set_grids([[dict(x0=FAR, y0=2.0, cell=0.25, max_gap=INF, nx=8, ny=8, id=s)] for s in range(n)])
    dts = _dts([[0.25, -0.25]] * n)

    def mine(cells, s):
        return [(int(c["cell"]), int(c["samples"]), int(c["visits"]), float(c["dwell"])) for c in cells if c["scene"] == BASE + s]

    run.sample(t=0.0)                                        # fresh in cell 0
    step_empty(sb, dts[0])
    assert [float(sb.tracks()["x"][s, 0, 0]) for s in range(n)] == [FAR + 0.375] * n
    run.sample(t=0.5)                                        # cell 1: a visit, and the interval goes to the cell it is in now
    step_empty(sb, dts[1])
    assert [float(sb.tracks()["x"][s, 0, 0]) for s in range(n)] == [FAR + 0.125] * n
    run.sample(t=1.0)                                        # back in cell 0: a second visit
    rows, cells = run.compare("there and back")
    for s in range(n):
        assert mine(cells, s) == [(0, 2, 2, 0.5), (1, 1, 1, 0.5)]
    # reset_scenes: scene 1 is empty -- its cells are kept, nothing is added; the others go on
    sb.reset_scenes(np.isin(np.arange(n), (1,)))
    ref.rebase([1])
    run.sample(t=1.5)
    rows, cells = run.compare("reset_scenes")
    assert mine(cells, 1) == [(0, 2, 2, 0.5), (1, 1, 1, 0.5)] and mine(cells, 0) == [(0, 3, 2, 1.0), (1, 1, 1, 0.5)]
    assert rows["calls"].tolist() == [4] * n
    # restore: the same people under the same uids are NEW: a visit, no interval -- in every scene, the one that was never reset included
    sb.restore(blob)
    ref.rebase()
    run.sample(t=2.0)
    rows, cells = run.compare("restore")
    assert mine(cells, 0) == [(0, 4, 3, 1.0), (1, 1, 1, 0.5)] and mine(cells, 1) == [(0, 3, 3, 0.5), (1, 1, 1, 0.5)]
    run.sample(t=2.5)                                        # ... and from there on intervals count again
    rows, cells = run.compare("after restore")
    assert mine(cells, 2) == [(0, 5, 3, 1.5), (1, 1, 1, 0.5)]
    sb.reset()
    ref.rebase()
    run.sample(t=3.0)
    rows, cells = run.compare("reset")
    assert mine(cells, 2) == [(0, 5, 3, 1.5), (1, 1, 1, 0.5)] and rows["calls"].tolist() == [7] * n
    sb.close()


# 6 ------------------------------------------------------------------------------------------------------------------------
def _whole_room(n, cells=1024, max_gap=INF):
    return [[dict(x0=-4.0, y0=0.0, cell=0.25, max_gap=max_gap, nx=32, ny=32, id=s)] for s in range(n)]


def test_clear_cuts_windows_keeps_the_uid_memory_and_a_refused_export_clears_nothing():
    from mmwave_msc_amd import _lib
    run = _settled(S2, cells=1024)
    sb, ref = run.sb, run.ref
    run.set_grids(_whole_room(S2))
    for f in range(4, 7):
        run.step(f)
        run.sample(t=0.125 * f)
    want_r, want_c = ref.export(BASE)
    n_r, n_c = len(want_r), len(want_c)
    assert n_r == S2 and n_c > S2
    # one too small for the rows and, separately, for the cells, in CLEAR mode: MMW_E_CAPACITY with both counts, nothing written --
    # the payload and 64 guard bytes on either side are as they were -- and nothing cleared
    G = 64
    sent_r, sent_c = np.full(n_r * 48 + 2 * G, 0xA5, np.uint8), np.full(n_c * 24 + 2 * G, 0x5A, np.uint8)
    b_r, b_c = sb.alloc(sent_r.nbytes).upload(sent_r), sb.alloc(sent_c.nbytes).upload(sent_c)
    for ticket, (cap_r, cap_c) in enumerate(((n_r - 1, n_c), (n_r, n_c - 1), (0, 0))):
        sb.heat_dev(b_r.ptr + G, cap_r, b_c.ptr + G, cap_c, clear=True, scene_base=BASE, ticket=ticket)
        with pytest.raises(_lib.MmwError) as ei:
            sb.heat_wait(ticket)
        assert ei.value.code == _lib.E_CAPACITY and ei.value.needed == (n_r, n_c)
        assert b_r.download((sent_r.nbytes,), np.uint8).tobytes() == sent_r.tobytes() and b_c.download((sent_c.nbytes,), np.uint8).tobytes() == sent_c.tobytes()
    run.compare("KEEP after the refused CLEARs")
    # exactly enough: written between the guards, which stay
    sb.heat_dev(b_r.ptr + G, n_r, b_c.ptr + G, n_c, clear=True, scene_base=BASE, ticket=1)
    assert sb.heat_wait(1) == (n_r, n_c)
    raw_r, raw_c = b_r.download((sent_r.nbytes,), np.uint8), b_c.download((sent_c.nbytes,), np.uint8)
    same_pair((np.frombuffer(raw_r[G:-G].tobytes(), _lib.HEAT_ROW_DTYPE), np.frombuffer(raw_c[G:-G].tobytes(), _lib.HEAT_CELL_DTYPE)), ref.export(BASE, clear=True), "CLEAR", NOUNS)
    for raw, sent in ((raw_r, sent_r), (raw_c, sent_c)):
        assert raw[:G].tobytes() == sent[:G].tobytes() and raw[-G:].tobytes() == sent[-G:].tobytes()
    for b in (b_r, b_c):
        b.free()
    rows, cells = run.compare("KEEP behind the CLEAR")
    assert len(rows) == S2 and len(cells) == 0 and not rows["calls"].any() and not rows["t_last"].any()
    # the next window holds only new data, and the uid memory was kept: somebody still in their cell gets the interval and no visit
    run.step(7)
    run.sample(t=0.125 * 7)
    rows, cells = run.compare("new window")
    assert (rows["calls"] == 1).all() and (rows["t_first"] == 0.875).all() and int(cells["samples"].sum()) + int(rows["outside"].sum()) == int(sb.num_tracks().sum())
    assert ((cells["visits"] == 0) & (cells["dwell"] > 0.0)).any()
    sb.check()
    sb.close()


def test_accumulator_over_clear_windows_equals_one_run_that_never_cleared():
    from mmwave_msc_amd import heat
    n = 6
    a, b = (HeatRun(make_checked(n, N, "per_scene", **CFG_KW), 1024, cut(n)) for _ in range(2))
    for run in (a, b):
        run.set_grids(_whole_room(n))
    acc = heat.Accumulator()
    for f in range(F):
        for run in (a, b):
            run.step(f)
            run.sample(t=0.125 * f)
        if f % 4 == 3:
            acc.add(*a.compare(("window", f), clear=True))
    rows, cells = b.compare("never cleared")
    assert acc.windows == 3 and int(cells["visits"].sum()) > 0
    for s in range(n):
        for field in ("samples", "visits"):
            assert acc.dense(BASE + s, field).tolist() == heat.dense(rows, cells, BASE + s, field).tolist(), (s, field)
        np.testing.assert_allclose(acc.dense(BASE + s, "dwell"), heat.dense(rows, cells, BASE + s, "dwell"), rtol=1e-12, atol=0.0)   # (the windows' sums are added in another order)
        assert (acc.calls[BASE + s], acc.outside[BASE + s]) == (int(rows["calls"][s]), int(rows["outside"][s]))
        assert (acc.t_first[BASE + s], acc.t_last[BASE + s]) == (0.0, 0.125 * (F - 1))
    for run in (a, b):
        run.sb.check()
        run.sb.close()


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_flags_scene_base_four_tickets_and_a_set_call_zeroes_its_scenes_only():
    from mmwave_msc_amd import _lib
    run = _settled(S2, cells=67)                             # (67: no scene's words but the first start on 16 bytes)
    sb, ref = run.sb, run.ref
    grid = lambda s, i: dict(x0=-3.0, y0=0.25 * s, cell=1.0, max_gap=INF, nx=6, ny=11, id=i)
    run.set_grids([[grid(s, s)] if s != 2 else [] for s in range(S2)])
    for f in range(4, 8):
        run.step(f)
        run.sample(t=0.125 * f, scenes=None if f % 2 else [0, 2, 3])     # (scene 2 is asked and has no grid)
    assert ref.calls.tolist() == [4, 2, 0, 4, 2]
    rows, cells = run.compare("all")
    assert (rows["scene"] - BASE).tolist() == [0, 1, 3, 4] and len(cells) > 4
    # scene_flags subsets: rows and cells of the flagged scenes with a grid, `first` counted from the subset's start
    for sub in ([3], [1, 2, 4], [2], []):
        r, c = run.compare(("subset", sub), scenes=sub)
        assert (r["scene"] - BASE).tolist() == [s for s in sub if s != 2] and (len(r) == 0 or r["first"][0] == 0)
    # four tickets outstanding on one state, each with its own subset and base, waited for in another order
    subs = ([0], [1, 3], None, [4])
    bufs = []
    for k, sub in enumerate(subs):
        want = ref.export(100 * k, scenes=sub)
        b_r, b_c = sb.alloc(max(1, len(want[0])) * 48), sb.alloc(max(1, len(want[1])) * 24)
        sb.heat_dev(b_r.ptr, len(want[0]), b_c.ptr, len(want[1]), flags_ptr=sb._scene_flags(sub, "heat_flags_%d" % k), scene_base=100 * k, ticket=k)
        bufs.append((b_r, b_c, want))
    for k in (2, 0, 3, 1):
        b_r, b_c, want = bufs[k]
        assert sb.heat_wait(k) == (len(want[0]), len(want[1]))
        same_pair((b_r.download((len(want[0]),), _lib.HEAT_ROW_DTYPE), b_c.download((len(want[1]),), _lib.HEAT_CELL_DTYPE)), want, ("ticket", k), NOUNS)
        b_r.free(); b_c.free()
    with pytest.raises(_lib.MmwError) as ei:
        sb.heat_wait(0)                                      # nothing outstanding under it any more
    assert ei.value.code == _lib.E_ARG
    # a set call on scenes 3 and 2: scene 3 starts over under its new grid, scene 2 gets one; 0, 1 and 4 keep every cell and word
    before = run.compare("before the set call", scenes=[0, 1, 4])
    run.set_grids([[grid(3, 33)], [grid(2, 22)]], scenes=[3, 2])
    rows, cells = run.compare("set")
    assert (rows["scene"] - BASE).tolist() == [0, 1, 2, 3, 4] and rows["id"].tolist() == [0, 1, 22, 33, 4]
    assert rows["count"][2] == 0 and rows["count"][3] == 0 and rows["calls"][2] == 0 and rows["calls"][3] == 0
    same_pair(run.compare("the others", scenes=[0, 1, 4]), before, "untouched by the set call", NOUNS)
    run.step(8)
    run.sample(t=1.0)
    rows, cells = run.compare("sampled behind the set call")
    assert rows["calls"].tolist() == [5, 3, 1, 1, 3] and not cells["dwell"][np.isin(cells["scene"] - BASE, (2, 3))].any()   # (no interval across the set call)
    sb.check()
    sb.close()


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    from mmwave_msc_amd import _lib
    run = _settled(S2, cells=64)
    sb, ref = run.sb, run.ref
    good = dict(x0=-4.0, y0=0.0, cell=1.0, max_gap=1.0, nx=8, ny=8, id=3)
    run.set_grids([[dict(good, id=s)] for s in range(S2)])
    for f in range(4, 6):
        run.step(f)
        run.sample(t=0.125 * f)
    before_tab = sb.get_heat_grids()
    before = run.compare("before")
    bad = [dict(x0=NAN), dict(x0=INF), dict(y0=-INF), dict(y0=NAN), dict(cell=NAN), dict(cell=INF), dict(cell=0.0), dict(cell=-1.0), dict(max_gap=NAN),
           dict(max_gap=0.0), dict(max_gap=-1.0), dict(nx=0), dict(ny=0), dict(nx=-1), dict(nx=9, ny=8), dict(nx=65536, ny=65536), dict(nx=2 ** 31 - 1, ny=2)]
    for over in bad:
        with pytest.raises(_lib.MmwError) as ei:
            sb.set_heat_grids([[good], [good], [dict(good, **over)]], scenes=[3, 1, 0])
        assert ei.value.code == _lib.E_ARG and "entry 2" in str(ei.value), (over, str(ei.value))
    ng, gt = _lib.make_heat_grids([[good]])
    gt[0, 0]["reserved_"] = 1
    for table, scenes in (((ng, gt), None), ((np.array([2], np.int32), _lib.make_heat_grids([[good]])[1]), None), ([[good]], [S2]), ([[good], [good]], [1, 1]),
                          ([[good]] * (S2 + 1), None)):
        with pytest.raises(_lib.MmwError) as ei:
            sb.set_heat_grids(table, scenes=scenes)
        assert ei.value.code == _lib.E_ARG
    # the export's arguments
    buf = sb.alloc(256)
    calls = (lambda: sb.heat_dev(None, 1, buf.ptr, 1), lambda: sb.heat_dev(buf.ptr, 1, None, 1), lambda: sb.heat_dev(buf.ptr, -1, buf.ptr, 1),
             lambda: sb.heat_dev(buf.ptr + 4, 1, buf.ptr, 1), lambda: sb.heat_dev(buf.ptr, 1, buf.ptr + 4, 1), lambda: sb.heat_dev(buf.ptr, 1, buf.ptr, 1, ticket=4),
             lambda: sb.heat_dev(buf.ptr, 1, buf.ptr, 1, ticket=-1), lambda: sb.heat_dev(buf.ptr, 1, buf.ptr, 1, flags_ptr=buf.ptr + 2),
             lambda: sb._chk(sb.L.mmw_heat_async(sb.h, buf.ptr, 1, buf.ptr, 1, None, 2, 0, 0)), lambda: sb._chk(sb.L.mmw_heat_async(sb.h, buf.ptr, 1, buf.ptr, 1, None, -1, 0, 0)),
             lambda: sb.heat_wait(2), lambda: sb.heat_wait(7), lambda: sb.sample_heat_dev(buf.ptr + 2, None), lambda: sb.sample_heat_dev(None, buf.ptr + 4))
    for k, call in enumerate(calls):
        with pytest.raises(_lib.MmwError) as ei:
            call()
        assert ei.value.code == _lib.E_ARG, k
    for bad_cells in (-1, _lib.HEAT_CELLS_MAX + 1):
        with pytest.raises(_lib.MmwError) as ei:
            sb.enable_heat(bad_cells)
        assert ei.value.code == _lib.E_ARG
    # ... and all of that left the mirrors and the state as they were
    after_tab = sb.get_heat_grids()
    assert before_tab[0].tobytes() == after_tab[0].tobytes() and before_tab[1].tobytes() == after_tab[1].tobytes() and after_tab[0].tolist() == [1] * S2
    same_pair(run.compare("after"), before, "state", NOUNS)
    run.step(6)
    run.sample(t=0.75)
    rows, cells = run.compare("goes on")                     # (a refused set call bumped no generation: the intervals across it count)
    assert float(cells["dwell"].sum()) > float(before[1]["dwell"].sum()) > 0.0
    # disabled: every call but the getter is refused; enabled again: everything starts over
    sb.disable_heat()
    sb.disable_heat()
    for call in (lambda: sb.sample_heat(), lambda: sb.sample_heat_dev(None, None), lambda: sb.set_heat_grids([[good]]), lambda: sb.heat_dev(buf.ptr, 1, buf.ptr, 1),
                 lambda: sb.heat_wait(0), lambda: sb.heat_host()):
        with pytest.raises(_lib.MmwError) as ei:
            call()
        assert ei.value.code == _lib.E_ARG
    ng, gt = sb.get_heat_grids()
    assert ng.tolist() == [0] * S2 and gt.tobytes() == bytes(S2 * 48)
    buf.free()
    sb.enable_heat(_lib.HEAT_CELLS_MAX)
    assert sb.get_heat_grids()[0].tolist() == [0] * S2
    rows, cells = sb.heat_host()
    assert len(rows) == 0 and len(cells) == 0
    sb.set_heat_grids([[dict(good, nx=64, ny=64)]], scenes=[4])
    sb.sample_heat()
    rows, cells = sb.heat_host()
    assert rows.tolist() == [(4, 3, 64, 64, 0, len(cells), 1, int(rows["outside"][0]), 0.0, 0.0)] and (cells["visits"] == cells["samples"]).all()
    sb.check()
    sb.close()


def test_nothing_else_moves():
    """Two contexts on the same frames, one with heat maps sampled and exported (KEEP and CLEAR) behind every step: tracks and report are
    the same bytes; and before mmw_heat_enable every heat call is refused."""
    from mmwave_msc_amd import _lib
    a = make_checked(S, N, "per_scene", **CFG_KW)
    b = make_checked(S, N, "per_scene", **CFG_KW)
    for sb in (a, b):
        sb.enable_report()
    buf = a.alloc(64)
    for call in (lambda: a.set_heat_grids([[(0.0, 0.0, 1.0, 1.0, 1, 1)]]), lambda: a.sample_heat(), lambda: a.heat_dev(buf.ptr, 1, buf.ptr, 1),
                 lambda: a.heat_wait(0), lambda: a.heat_host()):
        with pytest.raises(_lib.MmwError) as ei:
            call()
        assert ei.value.code == _lib.E_ARG
    buf.free()
    assert a.get_heat_grids()[0].tolist() == [0] * S
    run = HeatRun(a, 1024)
    run.set_grids(_whole_room(S, max_gap=0.25))

    def drive(f):
        run.sample(t=0.125 * f)
        if f % 4 == 3:
            run.compare(("moves", f), clear=(f == 7))

    nothing_else_moves(a, b, scenario(), F, drive, at_end=TRACKS + REPORT)
    for sb in (a, b):
        sb.check()
        sb.close()
