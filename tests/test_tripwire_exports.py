"""Tripwires (mmw_tripwires_*, include/mmw.h) as far as a machine without a GPU can check them: the entries refuse a missing context,
the table entries, rows and events have the sizes the kernels pin (tests/test_abi.py holds every layout and prototype to the
header), the kernels of csrc/k_tripwire.hip compile without scratch, spilled registers or LDS and bring no scan or generation bump of
their own, and the host-side pieces -- `_lib.make_tripwires`, `tripwires.Tally` and `tripwires.sides` -- do what they say on hand-made
input."""
import os
import re

import numpy as np
import pytest

from mmwave_msc_amd import _lib
from tests import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mmwave_msc_amd", "csrc")


def test_every_tripwire_entry_refuses_a_null_context():
    L = _lib.load()   # (declares every prototype: AttributeError if one is missing)
    assert L.mmw_tripwires_enable(None, 4) == _lib.E_ARG
    assert L.mmw_set_tripwires(None, None, 0, None, None) == _lib.E_ARG
    assert L.mmw_get_tripwires(None, None, None) == _lib.E_ARG
    assert L.mmw_tripwires_sample(None, None, None) == _lib.E_ARG
    assert L.mmw_tripwires_async(None, None, 0, None, 0, 0, 0) == _lib.E_ARG
    assert L.mmw_tripwires_wait(None, 0, None, None) == _lib.E_ARG
    assert L.mmw_tripwires(None, None, 0, None, 0, 0, None, None) == _lib.E_ARG


def test_tripwire_layouts_match_the_c_structs():
    lay = _abi.c_layout()
    pairs = (("mmw_tripwire", _lib.TRIPWIRE_DTYPE, 48), ("mmw_tripwire_row", _lib.TRIPWIRE_ROW_DTYPE, 32),
             ("mmw_tripwire_event", _lib.TRIPWIRE_EVENT_DTYPE, 32))
    for cname, dt, size in pairs:
        assert lay[cname]["size"] == size == dt.itemsize, cname
        assert not _abi.struct_mismatches(cname, dt, lay[cname]), cname
        assert _lib.ABI_STRUCTS[cname] is dt
    assert _lib.TRIPWIRES_MAX == 16 and _lib.TRIPWIRE_LOG_MAX == 4096
    assert (_lib.TW_FORWARD, _lib.TW_BACKWARD, _lib.TW_REBASED) == (1, 2, 3)
    assert _lib.TRIPWIRE_EVENT_DTYPE.fields["t"][1] == 24
    # the sizes are pinned where the kernels and the C-ABI are compiled
    for name in ("k_tripwire.hip", "api_tripwire.hip"):
        txt = open(os.path.join(CSRC, name)).read()
        for cname, _, size in pairs:
            assert re.search(r"static_assert\(sizeof\(%s\) == %d\b" % (cname, size), txt), (name, cname)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "k_tripwire.hip" in mk and "api_tripwire.hip" in mk
    for name in ("mmw_tripwires_enable", "mmw_set_tripwires", "mmw_get_tripwires", "mmw_tripwires_sample", "mmw_tripwires_async",
                 "mmw_tripwires_wait", "mmw_tripwires"):
        assert name in _lib.sig, name


def test_tripwire_kernels_use_no_scratch_no_lds_and_no_scan_of_their_own():
    from tests._isa import _device_isa, _kernel_report, assert_clean, kernel_body
    rep, asm = _device_isa(("k_tripwire",))["k_tripwire"]
    rows = _kernel_report(rep)
    names = [k[0] for k in rows]
    for k in ("k_tripwire_sample", "k_tripwire_count", "k_tripwire_write"):
        assert sum(k in n for n in names) == 1, (k, names)
    assert len(names) <= 4, names                       # (... and at most the kernel that zeroes the listed scenes' counters)
    assert not any("scan" in n or "rebase" in n for n in names), names   # (the scan and the generation bump are k_scan.hip's)
    assert "k_pair_scan" not in asm and "k_uid_rebase" not in asm
    assert_clean(rows)
    for name, scratch, vspill, vgprs, occ, sspill in rows:
        body = kernel_body(asm, name, ".Lfunc_end")
        assert "scratch_" not in body, name
        assert not re.search(r"\bds_(read|write)", body), name          # no LDS (the cross-lane moves are in registers)
        assert "atomic" not in body, name
        assert occ >= 4, (name, occ)
        assert re.search(r"LDS Size \[bytes/block\]: (\d+)", rep.split("remark: Function Name: " + name)[1]).group(1) == "0", name
    # the wire table is read with scalar loads: a wire's six doubles come without a vector load of their own
    sample = kernel_body(asm, [n for n in names if "k_tripwire_sample" in n][0], ".Lfunc_end")
    assert re.search(r"s_load_dwordx(4|8|16)", sample), "k_tripwire_sample: no wide scalar load"
    src = open(os.path.join(CSRC, "k_tripwire.hip")).read()
    assert "launch_pair_scan(" in src and "__shared__" not in src
    # the shared parts are the shared ones, not copies
    assert '#include "mmw_uidlist.hpp"' in src and "uid_find(" in src and "wave_scene()" in src
    for own in (r"\bint\s+uid_find\s*\(", r"\bstruct\s+UidGen\b", r"\bwave_scene\s*\(\s*\)\s*\{", r"int wave_excl_sum\("):
        assert not re.search(own, src), own
    api = open(os.path.join(CSRC, "api_export.hip")).read()
    assert "c->tw.ug.gen" in api                        # the fourth consumer of the one generation bump


def test_make_tripwires_takes_dicts_and_tuples():
    nw, wt = _lib.make_tripwires([
        [dict(ax=-1.0, ay=8.0, bx=-1.0, by=0.0, margin=0.03, id=70), (0.0, 2.0, 4.0, 2.0)],
        [],
        [(0.0, 1.0, 0.0, 2.0, 0.25), (0.0, 1.0, 0.0, 2.0, 0.5, -9), dict(ax=1, ay=2, bx=3, by=4)],
    ])
    assert nw.dtype == np.int32 and nw.tolist() == [2, 0, 3]
    assert wt.dtype == _lib.TRIPWIRE_DTYPE and wt.shape == (3, 16)
    assert wt[0, 0].tolist() == (-1.0, 8.0, -1.0, 0.0, 0.03, 70, 0)
    assert wt[0, 1].tolist() == (0.0, 2.0, 4.0, 2.0, 0.0, 1, 0)           # margin 0, id = the wire's index
    assert wt[2, 0].tolist() == (0.0, 1.0, 0.0, 2.0, 0.25, 0, 0)
    assert wt[2, 1].tolist() == (0.0, 1.0, 0.0, 2.0, 0.5, -9, 0)
    assert wt[2, 2].tolist() == (1.0, 2.0, 3.0, 4.0, 0.0, 2, 0)
    assert wt[1].tobytes() == bytes(16 * 48) and wt[0, 2:].tobytes() == bytes(14 * 48)   # entries past a scene's wires stay zero
    full = _lib.make_tripwires([[(0, 0, 0, 1)] * 16])
    assert full[0].tolist() == [16]
    with pytest.raises(ValueError):
        _lib.make_tripwires([[(0, 0, 0, 1)] * 17])
    with pytest.raises(ValueError):
        _lib.make_tripwires([[(0, 1, 0)]])
    with pytest.raises(AttributeError):
        _lib.make_tripwires([[dict(ax=0, ay=0, bx=0, by=1, radius=2)]])


def _events(*rows):
    return np.array(list(rows), _lib.TRIPWIRE_EVENT_DTYPE).reshape(-1)


def test_tally_folds_forward_backward_and_rebased():
    from mmwave_msc_amd.tripwires import Tally
    F, B, R = _lib.TW_FORWARD, _lib.TW_BACKWARD, _lib.TW_REBASED
    t = Tally()
    # uid 5 goes forward and back through door 70 inside ONE array: both are counted, and it is not inside any more
    t.apply(_events((4, 5, F, 0, 70, 0, 1.0), (4, 6, F, 0, 70, 1, 1.0), (4, 5, B, 0, 70, 0, 1.5), (4, 6, F, 3, 71, 1, 1.5), (5, 5, F, 0, 70, 0, 1.5)))
    assert t.counts() == {(4, 70): (2, 1, 1), (4, 71): (1, 0, 1), (5, 70): (1, 0, 1)}
    assert t.went_forward(4, 70) == {6} and t.went_forward(4, 71) == {6} and t.went_forward(5, 70) == {5} and t.went_forward(9, 9) == frozenset()
    assert t.net(4, 70) == 1 and t.net(4, 99) == 0
    t.apply(_events())                                          # an export without events
    # two wires with one id fold into one counter (a doorway as a polyline)
    t.apply(_events((4, 7, F, 1, 70, 2, 2.0)))
    assert t.counts()[(4, 70)] == (3, 1, 2) and t.went_forward(4, 70) == {6, 7}
    # a uid that went forward before the log began only counts
    t.apply(_events((5, 8, B, 0, 70, 1, 2.0)))
    assert t.counts()[(5, 70)] == (1, 1, 0) and t.went_forward(5, 70) == {5}
    # REBASED empties the scene's sets and nobody else's; the counts go on
    t.apply(_events((4, -1, R, -1, -1, 2, 3.0), (4, 0, F, 0, 70, 0, 3.0)))
    assert t.went_forward(4, 70) == {0} and t.went_forward(4, 71) == frozenset() and t.went_forward(5, 70) == {5}
    assert t.counts() == {(4, 70): (4, 1, 3), (4, 71): (1, 0, 1), (5, 70): (1, 1, 0)}
    with pytest.raises(ValueError):
        Tally().apply(_events((1, 2, 9, 0, 0, 0, 0.0)))
    with pytest.raises(ValueError):
        Tally().apply(_events((1, 2, 0, 0, 0, 0, 0.0)))


def test_sides_in_the_headers_operation_order():
    """Values whose products are exact: a wire from (1, 8) to (1, 0) (dx = 0, dy = -8, len2 = 64) and one from (0, 0) to (4, 2)
    (len2 = 20)."""
    from mmwave_msc_amd.tripwires import sides
    _, wt = _lib.make_tripwires([[(1.0, 8.0, 1.0, 0.0, 0.25), (0.0, 0.0, 4.0, 2.0)]])
    w = wt[0, :2]
    x, y = np.array([[1.5], [0.5], [1.0], [3.0], [np.nan], [np.inf]]), np.array([[4.0], [8.0], [0.0], [9.0], [1.0], [1.0]])
    with np.errstate(invalid="ignore"):
        u, c, inside = sides(w, x, y)
    # wire 0: rx = x - 1, ry = y - 8; u = -8 ry; c = dx ry - dy rx = 8 rx
    assert u[:4, 0].tolist() == [32.0, 0.0, 64.0, -8.0] and c[:4, 0].tolist() == [4.0, -4.0, 0.0, 16.0]
    assert inside[:, 0].tolist() == [True, True, True, False, False, False]        # u == 0 and u == len2 are inside; NaN and inf are not
    # wire 1: u = 4 x + 2 y; c = 4 y - 2 x
    assert u[:4, 1].tolist() == [14.0, 18.0, 4.0, 30.0] and c[:4, 1].tolist() == [13.0, 31.0, -2.0, 30.0]
    assert inside[:, 1].tolist() == [True, True, True, False, False, False]
    # the band of wire 0 is 0.25 * sqrt(64) = 2: (1.5, 4) is beyond it on the positive side, (1.25, 4) exactly on it
    assert sides(w[0], 1.25, 4.0)[1] == 2.0 == w[0]["margin"] * np.sqrt(64.0)
    assert sides(w, x, y)[0].shape == (6, 2)
