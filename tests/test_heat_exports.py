"""The dwell heat maps (mmw_heat_*, include/mmw.h) as far as a machine without a GPU can check them: the entries exist and refuse a
missing context, the grid, rows and cells have the sizes the kernels pin (tests/test_abi.py holds every layout and prototype to the
header), the kernels of csrc/k_heat.hip compile without scratch, spilled registers, LDS or atomics and bring no scan or slot table
of their own, the host-side pieces -- `_lib.make_heat_grids`, `heat.dense`, `heat.centres`, `heat.Accumulator` -- do what they say
on hand-made arrays, and the numpy restatement of the sampling rules (tests/_heat_ref.py) gives what a dozen samples worked out by
hand give, boundary values included."""
import os
import re

import numpy as np
import pytest

from mmwave_msc_amd import _lib, heat
from tests import _abi
from tests._heat_ref import HeatRef, cell_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mmwave_msc_amd", "csrc")
ENTRIES = ("mmw_heat_enable", "mmw_set_heat_grids", "mmw_get_heat_grids", "mmw_heat_sample", "mmw_heat_async", "mmw_heat_wait", "mmw_heat")
INF, NAN = float("inf"), float("nan")


def test_every_heat_entry_exists_and_refuses_a_null_context():
    L = _lib.load()   # (declares every prototype: AttributeError if one is missing)
    assert L.mmw_heat_enable(None, 4) == _lib.E_ARG
    assert L.mmw_set_heat_grids(None, None, 0, None, None) == _lib.E_ARG
    assert L.mmw_get_heat_grids(None, None, None) == _lib.E_ARG
    assert L.mmw_heat_sample(None, None, None) == _lib.E_ARG
    assert L.mmw_heat_async(None, None, 0, None, 0, None, 0, 0, 0) == _lib.E_ARG
    assert L.mmw_heat_wait(None, 0, None, None) == _lib.E_ARG
    assert L.mmw_heat(None, None, 0, None, 0, None, 0, 0, None, None) == _lib.E_ARG


def test_heat_layouts_match_the_c_structs():
    lay = _abi.c_layout()
    pairs = (("mmw_heat_grid", _lib.HEAT_GRID_DTYPE, 48), ("mmw_heat_row", _lib.HEAT_ROW_DTYPE, 48), ("mmw_heat_cell", _lib.HEAT_CELL_DTYPE, 24))
    for cname, dt, size in pairs:
        assert lay[cname]["size"] == size == dt.itemsize, cname
        assert not _abi.struct_mismatches(cname, dt, lay[cname]), cname
        assert _lib.ABI_STRUCTS[cname] is dt
    assert _lib.HEAT_CELLS_MAX == 4096 and _lib.HEAT_GRIDS_MAX == 1 and (_lib.HEAT_KEEP, _lib.HEAT_CLEAR) == (0, 1)
    assert _lib.HEAT_ROW_DTYPE.fields["t_first"][1] == 32 and _lib.HEAT_CELL_DTYPE.fields["dwell"][1] == 16
    # the sizes are pinned where the kernels and the C-ABI are compiled
    for name in ("k_heat.hip", "api_heat.hip"):
        txt = open(os.path.join(CSRC, name)).read()
        for cname, _, size in pairs:
            assert re.search(r"static_assert\(sizeof\(%s\) == %d\b" % (cname, size), txt), (name, cname)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "k_heat.hip" in mk and "api_heat.hip" in mk
    protos = _abi.header_prototypes()
    for name in ENTRIES:
        assert name in _lib.sig and name in protos, name
        assert not _abi.prototype_mismatches(name, _lib.sig[name], protos[name]), name


def test_heat_kernels_use_no_scratch_no_lds_no_atomics_and_no_scan_of_their_own():
    """The compiler's resource report and the source text only."""
    from tests._isa import _device_isa, _kernel_report, assert_clean
    rep, _ = _device_isa(("k_heat",))["k_heat"]
    rows = _kernel_report(rep)
    names = [k[0] for k in rows]
    assert len(names) == 5, names                            # (k_heat_write twice: KEEP and CLEAR)
    for k, n in (("k_heat_zero", 1), ("k_heat_sample", 1), ("k_heat_count", 1), ("k_heat_write", 2)):
        assert sum(k in nm for nm in names) == n, (k, names)
    assert_clean(rows)
    for name, scratch, vspill, vgprs, occ, sspill in rows:
        assert occ >= 4, (name, occ)
        assert re.search(r"LDS Size \[bytes/block\]: (\d+)", rep.split("remark: Function Name: " + name)[1]).group(1) == "0", name
    src = open(os.path.join(CSRC, "k_heat.hip")).read()
    assert "launch_pair_scan(" in src and "__shared__" not in src and not re.search(r"atomic\w*\s*\(", src)
    # the shared parts are the shared ones, not copies
    assert '#include "mmw_uidlist.hpp"' in src and "uid_slots_pick(" in src and "uid_slots_done(" in src and "wave_scene()" in src
    for own in (r"\bint\s+uid_find\s*\(", r"\bstruct\s+UidGen\b", r"\bwave_scene\s*\(\s*\)\s*\{", r"int wave_excl_sum\(", r"void\s+k_uid_rebase\s*\(", r"void\s+k_pair_scan\s*\("):
        assert not re.search(own, src), own
    api = open(os.path.join(CSRC, "api_heat.hip")).read()
    assert "export_alloc(" in api and "scene_table_send(" in api and "sample_begin(" in api and "export_issue(" in api
    assert "c->hs.ug.gen" in open(os.path.join(CSRC, "api_export.hip")).read()   # resets reach the heat maps' generation


def test_make_heat_grids_round_trips_tuples_and_dicts():
    ng, gt = _lib.make_heat_grids([
        [(-1.0, 2.0, 0.25, 1.5, 8, 4, 77)],
        [],
        [dict(x0=0.5, y0=-0.5, cell=0.125, nx=3, ny=21)],
        [(0.0, 0.0, 1.0, INF, 1, 1)],
    ])
    assert ng.tolist() == [1, 0, 1, 1] and gt.shape == (4, 1) and gt.dtype == _lib.HEAT_GRID_DTYPE
    g = gt[0, 0]
    assert (g["x0"], g["y0"], g["cell"], g["max_gap"], g["nx"], g["ny"], g["id"], g["reserved_"]) == (-1.0, 2.0, 0.25, 1.5, 8, 4, 77, 0)
    assert gt[1].tobytes() == bytes(48)
    g = gt[2, 0]
    assert (g["x0"], g["y0"], g["cell"], g["max_gap"], g["nx"], g["ny"], g["id"]) == (0.5, -0.5, 0.125, INF, 3, 21, 0)
    assert gt[3, 0]["max_gap"] == INF and gt[3, 0]["id"] == 0
    # ... and back through the pair form, as `set_heat_grids` takes either
    again = _lib.make_heat_grids([[{f: gt[i, 0][f] for f in _lib.HEAT_FIELDS}] if ng[i] else [] for i in range(4)])
    assert again[0].tobytes() == ng.tobytes() and again[1].tobytes() == gt.tobytes()
    with pytest.raises(ValueError):
        _lib.make_heat_grids([[(0, 0, 1, 1, 1, 1), (0, 0, 1, 1, 1, 1)]])
    with pytest.raises(ValueError):
        _lib.make_heat_grids([[(0, 0, 1, 1, 1)]])
    with pytest.raises(AttributeError):
        _lib.make_heat_grids([[dict(x0=0, y0=0, cell=1, nx=1, ny=1, margin=0)]])


def _hand_export():
    rows = np.array([(7, 70, 3, 2, 0, 2, 5, 1, 0.5, 2.5), (9, 90, 2, 2, 2, 0, 0, 0, 0.0, 0.0), (10, 91, 1, 4, 2, 1, 3, 0, 1.0, 3.0)], _lib.HEAT_ROW_DTYPE)
    cells = np.array([(7, 1, 4, 2, 1.5), (7, 5, 1, 1, 0.25), (10, 3, 3, 1, 2.0)], _lib.HEAT_CELL_DTYPE)
    return rows, cells


def test_dense_and_centres_on_hand_made_arrays():
    rows, cells = _hand_export()
    d = heat.dense(rows, cells, 7, "dwell")
    assert d.shape == (2, 3) and d.dtype == np.float64 and d.tolist() == [[0.0, 1.5, 0.0], [0.0, 0.0, 0.25]]
    assert heat.dense(rows, cells, 7, "samples").tolist() == [[0, 4, 0], [0, 0, 1]]
    assert heat.dense(rows, cells, 7, "visits").tolist() == [[0, 2, 0], [0, 0, 1]]
    assert heat.dense(rows, cells, 9).tolist() == [[0.0, 0.0], [0.0, 0.0]]                 # a row without a cell
    assert heat.dense(rows, cells, 10, "samples").tolist() == [[0], [0], [0], [3]]
    with pytest.raises(KeyError):
        heat.dense(rows, cells, 8)
    with pytest.raises(ValueError):
        heat.dense(rows, cells, 7, "count")
    xs, ys = heat.centres(rows[0], dict(x0=-1.0, y0=2.0, cell=0.5))
    assert xs.tolist() == [-0.75, -0.25, 0.25] and ys.tolist() == [2.25, 2.75]


def test_accumulator_folds_windows_and_starts_over_on_a_new_shape():
    rows, cells = _hand_export()
    acc = heat.Accumulator()
    acc.add(rows, cells)
    rows2 = np.array([(7, 70, 3, 2, 0, 2, 2, 4, 3.0, 3.5)], _lib.HEAT_ROW_DTYPE)
    cells2 = np.array([(7, 0, 1, 1, 0.0), (7, 1, 2, 0, 1.0)], _lib.HEAT_CELL_DTYPE)
    acc.add(rows2, cells2)
    assert acc.windows == 2
    assert acc.dense(7, "dwell").tolist() == [[0.0, 2.5, 0.0], [0.0, 0.0, 0.25]]
    assert acc.dense(7, "samples").tolist() == [[1, 6, 0], [0, 0, 1]] and acc.dense(7, "visits").tolist() == [[1, 2, 0], [0, 0, 1]]
    assert (acc.calls[7], acc.outside[7], acc.t_first[7], acc.t_last[7]) == (7, 5, 0.5, 3.5)
    assert acc.calls[9] == 0 and 9 not in acc.t_first and acc.dense(10, "samples").tolist() == [[0], [0], [0], [3]]
    # an empty window changes nothing; another shape for scene 7 starts it over
    acc.add(np.zeros(0, _lib.HEAT_ROW_DTYPE), np.zeros(0, _lib.HEAT_CELL_DTYPE))
    assert acc.dense(7, "samples").sum() == 8
    acc.add(np.array([(7, 70, 2, 2, 0, 1, 1, 0, 9.0, 9.0)], _lib.HEAT_ROW_DTYPE), np.array([(7, 3, 1, 1, 0.0)], _lib.HEAT_CELL_DTYPE))
    assert acc.dense(7, "samples").tolist() == [[0, 0], [0, 1]] and (acc.calls[7], acc.t_first[7]) == (1, 9.0)


def _tracks(*scenes):
    """tracks[S, 8] / ntr[S] of hand-made scenes: a list of (uid, x, y) per scene."""
    trk = np.zeros((len(scenes), 8), _lib.TRACK_DTYPE)
    ntr = np.zeros(len(scenes), np.int32)
    for s, lst in enumerate(scenes):
        ntr[s] = len(lst)
        for j, (uid, x, y) in enumerate(lst):
            trk[s, j]["uid"], trk[s, j]["x"][0], trk[s, j]["x"][1] = uid, x, y
    return trk, ntr


GRID = dict(x0=-1.0, y0=0.5, cell=0.25, max_gap=1.0, nx=4, ny=3, id=5)


def test_cell_of_at_every_boundary_by_hand():
    below = lambda v: float(np.nextafter(v, -INF))
    # x spans [-1, 0), y spans [0.5, 1.25): the corner, the last ulp inside, the first value outside, and what is no position
    assert cell_of(GRID, -1.0, 0.5) == 0
    assert cell_of(GRID, below(-1.0), 0.5) == -1 and cell_of(GRID, -1.0, below(0.5)) == -1
    assert cell_of(GRID, -2.0 ** -53, 0.5) == 3 and cell_of(GRID, 0.0, 0.5) == -1           # x0 + nx * cell itself is outside ...
    assert cell_of(GRID, below(0.0), 0.5) == -1                                             # ... and so is what the ONE subtraction rounds onto it
    assert cell_of(GRID, -1.0, below(1.25)) == 8 and cell_of(GRID, -1.0, 1.25) == -1
    assert cell_of(GRID, -0.75, 0.75) == 5 and cell_of(GRID, below(-0.75), below(0.75)) == 0
    assert cell_of(GRID, -0.3, 1.1) == 2 * 4 + 2
    for bad in (NAN, INF, -INF):
        assert cell_of(GRID, bad, 0.5) == -1 and cell_of(GRID, -1.0, bad) == -1
    # -0.0 is a position like any other: with the corner at 0 it lies in cell 0, just as 0.0 does
    g0 = dict(GRID, x0=0.0, y0=0.0)
    assert cell_of(g0, -0.0, -0.0) == 0 and cell_of(g0, 0.0, 0.0) == 0 and cell_of(g0, below(0.0), 0.0) == -1
    assert cell_of(dict(g0, x0=-0.0), -0.0, 0.0) == 0


def test_the_restatement_gives_a_dozen_hand_computed_samples():
    """One scene, grid 4 x 3 at (-1, 0.5), cell 0.25, max_gap 1: twelve track samples over six calls, every count worked out by hand."""
    ng, gt = _lib.make_heat_grids([[GRID]])
    ref = HeatRef(1, 8, 16)
    ref.set_grids([0], ng, gt)
    A, B, C = 10, 11, 12
    # call 1, t = 0.5: A in cell 0, B in cell 5: fresh -- a sample and a visit each, no time
    ref.sample(*_tracks([(A, -1.0, 0.5), (B, -0.75, 0.75)]), t=[0.5])
    # call 2, t = 1.0: A stays (0.5 s to cell 0, no visit); B moves into cell 0 as well (visit, 0.5 s to cell 0: the cell it is in NOW)
    ref.sample(*_tracks([(A, -0.9, 0.6), (B, -0.8, 0.7)]), t=[1.0])
    # call 3, t = 2.0: dt = 1.0 == max_gap counts for A (cell 0); B steps outside: `outside`, nothing else
    ref.sample(*_tracks([(A, -0.9, 0.6), (B, 0.0, 0.7)]), t=[2.0])
    # call 4, t = 3.0 + one ulp: dt just above max_gap: a sample for A, no time; B comes back into cell 0: a visit, and its dt (too long) is refused too
    t4 = float(np.nextafter(3.0, INF))
    ref.sample(*_tracks([(A, -0.9, 0.6), (B, -0.8, 0.7)]), t=[t4])
    # call 5, the same t again: dt == 0 credits nothing; C is born in cell 11; B has expired
    ref.sample(*_tracks([(A, -0.9, 0.6), (C, -0.01, 1.24)]), t=[t4])
    # call 6, t going backwards: dt < 0 credits nothing; C at NaN is outside
    ref.sample(*_tracks([(A, -0.9, 0.6), (C, NAN, 1.0)]), t=[1.0])
    rows, cells = ref.export(scene_base=3)
    assert rows.tolist() == [(3, 5, 4, 3, 0, 3, 6, 2, 0.5, 1.0)]
    assert cells.tolist() == [(3, 0, 8, 3, 2.0), (3, 5, 1, 1, 0.0), (3, 11, 1, 1, 0.0)]
    assert ref.tally["credited"] == 3 and ref.tally["gap_refused"] == 2 and ref.tally["dt_not_positive"] == 2 and ref.tally["expired"] == 1
    # KEEP changes nothing; CLEAR restarts cells and words and keeps the uid memory: A's next interval counts, and no new visit
    again = ref.export(scene_base=3)
    assert again[0].tobytes() == rows.tobytes() and again[1].tobytes() == cells.tobytes()
    ref.export(clear=True)
    assert ref.export()[0].tolist() == [(0, 5, 4, 3, 0, 0, 0, 0, 0.0, 0.0)] and len(ref.export()[1]) == 0
    ref.sample(*_tracks([(A, -0.9, 0.6)]), t=[1.5])
    rows, cells = ref.export()
    assert rows.tolist() == [(0, 5, 4, 3, 0, 1, 1, 0, 1.5, 1.5)] and cells.tolist() == [(0, 0, 1, 0, 0.5)]
    # a rebase voids the memory and keeps the cells: the next sample is a visit without time
    ref.rebase([0])
    ref.sample(*_tracks([(A, -0.9, 0.6)]), t=[2.0])
    assert ref.export()[1].tolist() == [(0, 0, 2, 1, 0.5)]
    # t == None: the call ordinal (8 calls asked the scene so far)
    ref.sample(*_tracks([(A, -0.9, 0.6)]), t=None)
    assert ref.export()[0]["t_last"][0] == 8.0 and ref.export()[1]["dwell"][0] == 0.5     # (dt = 6 > max_gap)


def test_tracks_that_share_a_cell_add_one_after_another():
    """Three tracks in one cell: every call adds its interval three times in a row, which is not the interval times three once the
    sum is large -- 3 * 2^53 + 2 rounds back to 3 * 2^53 each time, 3 * 2^53 + 6 rounds to 3 * 2^53 + 8."""
    ng, gt = _lib.make_heat_grids([[dict(GRID, max_gap=INF)]])
    ref = HeatRef(1, 8, 16)
    ref.set_grids([0], ng, gt)
    three = [(1, -0.9, 0.6), (2, -0.9, 0.6), (3, -0.9, 0.6)]
    big = 2.0 ** 53
    ref.sample(*_tracks(three), t=[0.0])
    ref.sample(*_tracks(three), t=[big])
    assert float(ref.export()[1]["dwell"][0]) == 3.0 * big
    ref.sample(*_tracks(three), t=[big + 2.0])
    d = float(ref.export()[1]["dwell"][0])
    assert d == 3.0 * big and d != 3.0 * big + 3 * 2.0
    ref.sample(*_tracks(three[:1]), t=[big + 6.0])          # ... and ONE interval of 4 moves it
    assert float(ref.export()[1]["dwell"][0]) == 3.0 * big + 4.0
