"""Zone occupancy (mmw_set_zones / mmw_zones_*, include/mmw.h) as far as a machine without a GPU can check it: the entries refuse
a missing context, the table entries, rows and events have the sizes the kernels pin (tests/test_abi.py holds every layout and
prototype to the header), the kernels of csrc/k_zone.hip compile without scratch or spilled registers and bring no scan of their
own, and the two host-side pieces -- `_lib.make_zones` and `zones.Roster` -- do what they say on hand-made input."""
import os
import re

import numpy as np
import pytest

from mmwave_msc_amd import _lib
from tests import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mmwave_msc_amd", "csrc")


def test_every_zone_entry_refuses_a_null_context():
    L = _lib.load()   # (declares every prototype: AttributeError if one is missing)
    assert L.mmw_set_zones(None, None, 0, None, None) == _lib.E_ARG
    assert L.mmw_get_zones(None, None, None) == _lib.E_ARG
    assert L.mmw_clear_zones(None) == _lib.E_ARG
    assert L.mmw_has_zones(None) == _lib.E_ARG
    assert L.mmw_zones_async(None, None, 0, None, 0, 0, 0) == _lib.E_ARG
    assert L.mmw_zones_wait(None, 0, None, None) == _lib.E_ARG
    assert L.mmw_zones(None, None, 0, None, 0, 0, None, None) == _lib.E_ARG


def test_zone_layouts_match_the_c_structs():
    lay = _abi.c_layout()
    pairs = (("mmw_zone", _lib.ZONE_DTYPE, 48), ("mmw_zone_row", _lib.ZONE_ROW_DTYPE, 32), ("mmw_zone_event", _lib.ZONE_EVENT_DTYPE, 24))
    for cname, dt, size in pairs:
        assert lay[cname]["size"] == size == dt.itemsize, cname
        assert not _abi.struct_mismatches(cname, dt, lay[cname]), cname
        assert _lib.ABI_STRUCTS[cname] is dt
    assert _lib.ZONES_MAX == 16 and (_lib.ZEV_ENTER, _lib.ZEV_LEAVE, _lib.ZEV_REBASED) == (1, 2, 3)
    # the sizes are pinned where the kernels and the C-ABI are compiled
    for name in ("k_zone.hip", "api_zone.hip"):
        txt = open(os.path.join(CSRC, name)).read()
        for cname, _, size in pairs:
            assert re.search(r"static_assert\(sizeof\(%s\) == %d\b" % (cname, size), txt), (name, cname)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "k_zone.hip" in mk and "api_zone.hip" in mk


def test_zone_kernels_use_no_scratch_no_lds_and_no_scan_of_their_own():
    from tests._isa import _device_isa, _kernel_report, assert_clean, kernel_body
    rep, asm = _device_isa(("k_zone",))["k_zone"]
    rows = _kernel_report(rep)
    names = [k[0] for k in rows]
    for k in ("k_zone_count", "k_zone_write"):
        assert sum(k in n for n in names) == 1, (k, names)
    assert len(names) == 2, names                       # (the scan and the generation bump are k_scan.hip's)
    assert "k_pair_scan" not in asm and "scan" not in " ".join(names)
    assert_clean(rows)
    for name, scratch, vspill, vgprs, occ, sspill in rows:
        body = kernel_body(asm, name, ".Lfunc_end")
        assert "scratch_" not in body, name
        assert not re.search(r"\bds_(read|write)", body), name          # no LDS (the cross-lane moves are in registers)
        assert "atomic" not in body, name
        assert occ >= 4, (name, occ)
    # the zone table is read with scalar loads: the walk's five doubles of a zone come without a vector load of their own
    count = kernel_body(asm, [n for n in names if "k_zone_count" in n][0], ".Lfunc_end")
    assert re.search(r"s_load_dwordx(4|8|16)", count), "k_zone_count: no wide scalar load"
    src = open(os.path.join(CSRC, "k_zone.hip")).read()
    assert "launch_pair_scan(" in src and "__shared__" not in src


def test_make_zones_takes_dicts_and_tuples():
    nz, zt = _lib.make_zones([
        [dict(x0=-1.0, x1=1.0, y0=0.0, y1=np.inf, margin=0.1, id=70), (0.0, 2.0, -np.inf, 4.0)],
        [],
        [(0.0, 1.0, 0.0, 1.0, 0.25), (0.0, 1.0, 0.0, 1.0, 0.5, -9), dict(x0=1, x1=2, y0=3, y1=4)],
    ])
    assert nz.dtype == np.int32 and nz.tolist() == [2, 0, 3]
    assert zt.dtype == _lib.ZONE_DTYPE and zt.shape == (3, 16)
    assert zt[0, 0].tolist() == (-1.0, 1.0, 0.0, np.inf, 0.1, 70, 0)
    assert zt[0, 1].tolist() == (0.0, 2.0, -np.inf, 4.0, 0.0, 1, 0)       # margin 0, id = the zone's index
    assert zt[2, 0].tolist() == (0.0, 1.0, 0.0, 1.0, 0.25, 0, 0)
    assert zt[2, 1].tolist() == (0.0, 1.0, 0.0, 1.0, 0.5, -9, 0)
    assert zt[2, 2].tolist() == (1.0, 2.0, 3.0, 4.0, 0.0, 2, 0)
    assert zt[1].tobytes() == bytes(16 * 48) and zt[0, 2:].tobytes() == bytes(14 * 48)   # entries past a scene's zones stay zero
    full = _lib.make_zones([[(0, 1, 0, 1)] * 16])
    assert full[0].tolist() == [16]
    with pytest.raises(ValueError):
        _lib.make_zones([[(0, 1, 0, 1)] * 17])
    with pytest.raises(ValueError):
        _lib.make_zones([[(0, 1, 0)]])
    with pytest.raises(AttributeError):
        _lib.make_zones([[dict(x0=0, x1=1, y0=0, y1=1, radius=2)]])


def _events(*rows):
    return np.array(list(rows), _lib.ZONE_EVENT_DTYPE).reshape(-1)


def test_roster_folds_enter_leave_and_rebased():
    from mmwave_msc_amd.zones import Roster
    E, L, R = _lib.ZEV_ENTER, _lib.ZEV_LEAVE, _lib.ZEV_REBASED
    r = Roster()
    r.apply(_events((4, 0, E, 1, 71, 0), (4, 0, E, 2, 72, 0), (4, 3, E, 1, 71, 1), (5, 0, E, 0, 80, 0)))
    assert r.occupied() == {(4, 1): {0, 3}, (4, 2): {0}, (5, 0): {0}}
    assert r.count(4, 1) == 2 and r.count(4, 9) == 0 and r.zones_of(4, 0) == [1, 2] and r.ids[(4, 2)] == 72
    r.apply(_events((4, 0, L, 2, 72, 0), (4, 7, E, 2, 72, 2)))
    assert r.occupied() == {(4, 1): {0, 3}, (4, 2): {7}, (5, 0): {0}}
    r.apply(_events())                                          # an export without events
    # REBASED voids the scene's memberships and nobody else's; the ENTERs behind it are the scene's new roster
    r.apply(_events((4, -1, R, -1, -1, 1), (4, 0, E, 0, 70, 0)))
    assert r.occupied() == {(4, 0): {0}, (5, 0): {0}}
    r.apply(_events((5, 0, L, 0, 80, 0)))
    assert r.occupied() == {(4, 0): {0}}
    # a stream with a hole in it is noticed
    with pytest.raises(ValueError):
        Roster().apply(_events((1, 2, L, 0, 0, 0)))
    with pytest.raises(ValueError):
        Roster().apply(_events((1, 2, E, 0, 0, 0), (1, 2, E, 0, 0, 1)))
    with pytest.raises(ValueError):
        Roster().apply(_events((1, 2, 9, 0, 0, 0)))
