"""The stance watch (mmw_stance_*, include/mmw.h) as far as a machine without a GPU can check it: the entries refuse a missing
context, the rule, rows and events have the sizes the kernels pin (tests/test_abi.py holds every layout and prototype to the
header), the kernels of csrc/k_stance.hip compile without scratch, spilled registers or LDS and bring no scan or generation bump of
their own, and the host-side pieces -- `_lib.make_stance_rules`, `stance.Watch` and `stance.classify` -- do what they say on
hand-made input."""
import os
import re

import numpy as np
import pytest

from mmwave_msc_amd import _lib
from tests import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mmwave_msc_amd", "csrc")
ENTRIES = ("mmw_stance_enable", "mmw_set_stance_rules", "mmw_get_stance_rules", "mmw_stance_sample", "mmw_stance_async", "mmw_stance_wait", "mmw_stance")


def test_every_stance_entry_refuses_a_null_context():
    L = _lib.load()   # (declares every prototype: AttributeError if one is missing)
    assert L.mmw_stance_enable(None, 4) == _lib.E_ARG
    assert L.mmw_set_stance_rules(None, None, 0, None, None) == _lib.E_ARG
    assert L.mmw_get_stance_rules(None, None, None) == _lib.E_ARG
    assert L.mmw_stance_sample(None, None, None) == _lib.E_ARG
    assert L.mmw_stance_async(None, None, 0, None, 0, 0, 0) == _lib.E_ARG
    assert L.mmw_stance_wait(None, 0, None, None) == _lib.E_ARG
    assert L.mmw_stance(None, None, 0, None, 0, 0, None, None) == _lib.E_ARG


def test_stance_layouts_match_the_c_structs():
    lay = _abi.c_layout()
    pairs = (("mmw_stance_rule", _lib.STANCE_RULE_DTYPE, 64), ("mmw_stance_row", _lib.STANCE_ROW_DTYPE, 48), ("mmw_stance_event", _lib.STANCE_EVENT_DTYPE, 32))
    for cname, dt, size in pairs:
        assert lay[cname]["size"] == size == dt.itemsize, cname
        assert not _abi.struct_mismatches(cname, dt, lay[cname]), cname
        assert _lib.ABI_STRUCTS[cname] is dt
    assert _lib.STANCE_RULES_MAX == 1 and _lib.STANCE_LOG_MAX == 4096
    assert (_lib.STANCE_UNKNOWN, _lib.STANCE_UPRIGHT, _lib.STANCE_LOW, _lib.STANCE_LYING) == (0, 1, 2, 3)
    assert (_lib.SEV_CHANGE, _lib.SEV_FALL, _lib.SEV_LONG_LIE, _lib.SEV_REBASED) == (1, 2, 3, 4)
    assert _lib.STANCE_EVENT_DTYPE.fields["t"][1] == 24
    # the sizes are pinned where the kernels and the C-ABI are compiled
    for name in ("k_stance.hip", "api_stance.hip"):
        txt = open(os.path.join(CSRC, name)).read()
        for cname, _, size in pairs:
            assert re.search(r"static_assert\(sizeof\(%s\) == %d\b" % (cname, size), txt), (name, cname)
        assert re.search(r"static_assert\(sizeof\(StanceRule\) == 80 && sizeof\(StanceCount\) == 16\b", txt), name
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "k_stance.hip" in mk and "api_stance.hip" in mk
    for name in ENTRIES:
        assert name in _lib.sig, name


def test_stance_kernels_use_no_scratch_no_lds_and_no_scan_of_their_own():
    """The compiler's resource report and the source text only."""
    from tests._isa import _device_isa, _kernel_report, assert_clean
    rep, _ = _device_isa(("k_stance",))["k_stance"]
    rows = _kernel_report(rep)
    names = [k[0] for k in rows]
    assert len(names) == 4, names
    for k in ("k_stance_zero", "k_stance_sample", "k_stance_count", "k_stance_write"):
        assert sum(k in n for n in names) == 1, (k, names)
    assert_clean(rows)
    for name, scratch, vspill, vgprs, occ, sspill in rows:
        assert occ >= 4, (name, occ)
        assert re.search(r"LDS Size \[bytes/block\]: (\d+)", rep.split("remark: Function Name: " + name)[1]).group(1) == "0", name
    src = open(os.path.join(CSRC, "k_stance.hip")).read()
    assert "launch_pair_scan(" in src and "__shared__" not in src and not re.search(r"atomic\w*\s*\(", src)
    # the shared parts are the shared ones, not copies
    assert '#include "mmw_uidlist.hpp"' in src and "uid_slots_pick(" in src and "uid_slots_done(" in src and "wave_scene()" in src
    for own in (r"\bint\s+uid_find\s*\(", r"\bstruct\s+UidGen\b", r"\bwave_scene\s*\(\s*\)\s*\{", r"int wave_excl_sum\(", r"void\s+k_uid_rebase\s*\(", r"void\s+k_pair_scan\s*\("):
        assert not re.search(own, src), own
    api = open(os.path.join(CSRC, "api_export.hip")).read()
    assert "c->ss.ug.gen" in api and "c->tw.ug.gen" in api     # the fifth consumer of the one generation bump
    assert re.search(r"kMax = 5\b", open(os.path.join(CSRC, "mmw_kernels.hpp")).read())


def test_make_stance_rules_defaults_tuples_and_dicts():
    nr, rt = _lib.make_stance_rules([
        [{}],
        [],
        [dict(h_stand=1.25, h_lie=0.5, margin=0.125, fall_window=0.25, long_lie=0.5, max_gap=0.5, id=70)],
        [(1.0, 0.25)],
        [(1.5, 0.5, 0.0, 2.0, float("inf"), 0.25, -9)],
        [dict(long_lie=0.0)],
    ])
    assert nr.dtype == np.int32 and nr.tolist() == [1, 0, 1, 1, 1, 1]
    assert rt.dtype == _lib.STANCE_RULE_DTYPE and rt.shape == (6, 1) and rt.dtype.itemsize == 64
    f = lambda r: tuple(r[k].item() for k in _lib.STANCE_FIELDS) + (int(r["reserved_"]), r["pad_"].tolist())
    assert f(rt[0, 0]) == (1.2, 0.5, 0.1, 1.5, 30.0, 0.5, 0, 0, [0, 0])            # the defaults
    assert rt[1].tobytes() == bytes(64)                                            # no rule: the entry stays zero
    assert f(rt[2, 0]) == (1.25, 0.5, 0.125, 0.25, 0.5, 0.5, 70, 0, [0, 0])
    assert f(rt[3, 0]) == (1.0, 0.25, 0.1, 1.5, 30.0, 0.5, 0, 0, [0, 0])           # a tuple cut short: the rest are the defaults
    assert f(rt[4, 0]) == (1.5, 0.5, 0.0, 2.0, float("inf"), 0.25, -9, 0, [0, 0])
    assert f(rt[5, 0]) == (1.2, 0.5, 0.1, 1.5, 0.0, 0.5, 0, 0, [0, 0])
    with pytest.raises(ValueError):
        _lib.make_stance_rules([[{}, {}]])                                         # at most one rule per scene
    with pytest.raises(ValueError):
        _lib.make_stance_rules([[(1, 2, 3, 4, 5, 6, 7, 8)]])
    with pytest.raises(AttributeError):
        _lib.make_stance_rules([[dict(h_stand=1.0, torso_angle=2)]])


def _events(*rows):
    return np.array(list(rows), _lib.STANCE_EVENT_DTYPE).reshape(-1)


def test_watch_folds_changes_falls_long_lies_and_rebased():
    from mmwave_msc_amd.stance import LOW, LYING, UPRIGHT, Watch
    Cg, Fl, Ll, Rb = _lib.SEV_CHANGE, _lib.SEV_FALL, _lib.SEV_LONG_LIE, _lib.SEV_REBASED
    w = Watch()
    # (scene, uid, kind, from, to, slot, t)
    w.apply(_events((4, 5, Cg, 0, UPRIGHT, 0, 1.0), (4, 6, Cg, 0, LYING, 1, 1.0), (5, 5, Cg, 0, LOW, 0, 1.0)))
    assert w.state == {(4, 5): (UPRIGHT, 1.0), (4, 6): (LYING, 1.0), (5, 5): (LOW, 1.0)}
    assert w.down() == {(4, 6)} and w.alarmed() == frozenset()                     # lying from the first look on: down, not alarmed
    w.apply(_events())                                                             # an export without events
    w.apply(_events((4, 5, Cg, UPRIGHT, LOW, 0, 1.25), (4, 5, Fl, LOW, LYING, 0, 1.5), (4, 6, Ll, LYING, LYING, 1, 1.5)))
    assert w.state[(4, 5)] == (LYING, 1.5) and w.state[(4, 6)] == (LYING, 1.0)     # a LONG_LIE leaves `since` alone
    assert w.down() == {(4, 5), (4, 6)} and w.alarmed() == {(4, 5), (4, 6)}
    assert (w.falls, w.long_lies) == (1, 1)
    # getting up ends the alarm; the other scene's uid 5 is somebody else
    w.apply(_events((4, 5, Cg, LYING, LOW, 0, 3.0)))
    assert w.down() == {(4, 6)} and w.alarmed() == {(4, 6)} and w.state[(5, 5)] == (LOW, 1.0)
    # REBASED empties the scene and nobody else's
    w.apply(_events((4, -1, Rb, 0, 0, 2, 4.0), (4, 0, Cg, 0, UPRIGHT, 0, 4.0)))
    assert w.state == {(4, 0): (UPRIGHT, 4.0), (5, 5): (LOW, 1.0)} and w.down() == frozenset() and w.alarmed() == frozenset()
    # a LONG_LIE of a uid the log never classed (its CHANGE was lost) still shows it down
    w.apply(_events((5, 9, Ll, LYING, LYING, 1, 5.0)))
    assert w.down() == {(5, 9)} and w.alarmed() == {(5, 9)}
    w.forget(5, 9)
    assert w.down() == frozenset() and w.alarmed() == frozenset()
    with pytest.raises(ValueError):
        Watch().apply(_events((1, 2, 9, 0, 0, 0, 0.0)))
    with pytest.raises(ValueError):
        Watch().apply(_events((1, 2, 0, 0, 0, 0, 0.0)))


def test_classify_in_the_headers_operation_order():
    """h_stand 1.25, h_lie 0.5, margin 0.125: up_hi 1.375, up_lo 1.125, lie_hi 0.625, lie_lo 0.375, gap2 0.25 -- all exact."""
    from mmwave_msc_amd.stance import LOW, LYING, UNKNOWN, UPRIGHT, classify
    rule = _lib.make_stance_rules([[(1.25, 0.5, 0.125, 0.25, 0.5, 0.5)]])[1][0, 0]

    def kp(head, g=(0.0, 0.0, 0.0)):
        k = np.zeros(57, np.float32)
        k[22] = head
        k[1], k[20], k[39] = g
        return k

    up = lambda x: np.nextafter(np.float32(x), np.float32(np.inf))
    # (old, head) -> new: "above" is strict, and which boundary counts depends on the old class
    table = [
        (UNKNOWN, 1.25, LOW), (UNKNOWN, up(1.25), UPRIGHT), (UNKNOWN, 0.5, LYING), (UNKNOWN, up(0.5), LOW),
        (UPRIGHT, 1.125, LOW), (UPRIGHT, up(1.125), UPRIGHT), (UPRIGHT, 0.375, LYING), (UPRIGHT, up(0.375), LOW),
        (LOW, 1.375, LOW), (LOW, up(1.375), UPRIGHT), (LOW, 0.375, LYING), (LOW, up(0.375), LOW),
        (LYING, 0.625, LYING), (LYING, up(0.625), LOW), (LYING, 1.375, LOW), (LYING, up(1.375), UPRIGHT),
        (LOW, -0.0, LYING), (UPRIGHT, 1.25, UPRIGHT), (LYING, 0.5, LYING),
    ]
    for old, head, want in table:
        assert classify(rule, kp(head), old) == (want, True), (old, float(head))
    # not plausible: the class stays; NaN and inf heads, a gap beyond max_gap; s == gap2 exactly is plausible, a NaN s too
    assert classify(rule, kp(np.nan), LOW) == (LOW, False) and classify(rule, kp(np.inf), UPRIGHT) == (UPRIGHT, False)
    assert classify(rule, kp(-np.inf), UNKNOWN) == (UNKNOWN, False)
    assert classify(rule, kp(2.0, (0.5, 0.0, 0.0)), LYING) == (UPRIGHT, True)
    assert classify(rule, kp(2.0, (up(0.5), 0.0, 0.0)), LYING) == (LYING, False)
    assert classify(rule, kp(2.0, (0.0, np.nan, 0.0)), LYING) == (UPRIGHT, True)
    # arrays: kp[n, 57] against old[n]
    new, ok = classify(rule, np.stack([kp(2.0), kp(1.0), kp(0.25), kp(np.nan)]), np.array([LYING, LYING, UPRIGHT, LOW]))
    assert new.tolist() == [UPRIGHT, LOW, LYING, LOW] and ok.tolist() == [True, True, True, False]
    # a dict works as a rule, with the defaults for what it leaves out
    assert classify(dict(h_stand=1.0), kp(1.05), UNKNOWN) == (UPRIGHT, True) and classify({}, kp(1.15), UNKNOWN) == (LOW, True)
