"""The live-track report (mmw_report_*, include/mmw.h) as far as a machine without a GPU can check it: the entries refuse
a missing context, the rows and events have the sizes the kernels pin (tests/test_abi.py holds every layout and prototype to
the header), and the kernels of csrc/k_report.hip compile without scratch or spilled registers and store the rows in 16-byte pieces."""
import os
import re

import numpy as np

from mmwave_msc_amd import _lib
from tests import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_report_entries():
    L = _lib.load()   # (declares every prototype: AttributeError if one is missing)
    # without a context every entry refuses its arguments instead of touching a device
    assert L.mmw_report_enable(None, 1) == _lib.E_ARG
    assert L.mmw_report_async(None, None, 0, None, 0, 0, 0) == _lib.E_ARG
    assert L.mmw_report_wait(None, 0, None, None) == _lib.E_ARG
    assert L.mmw_report(None, None, 0, None, 0, 0, None, None) == _lib.E_ARG


def test_report_layouts_match_the_c_structs():
    lay = _abi.c_layout()
    rdt, edt = _lib.TRACK_REPORT_DTYPE, _lib.TRACK_EVENT_DTYPE
    assert (lay["mmw_track_report"]["size"], lay["mmw_track_event"]["size"]) == (324, 16) == (rdt.itemsize, edt.itemsize)
    # every field a row shares with the track table has the table's type and shape
    for f in ("scene", "slot", "point_num", "lifetime", "x", "centroid", "keypoints", "fade_x", "fade_z", "fade_size"):
        assert rdt.fields[f][0] == _lib.SUMMARY_DTYPE.fields[f][0], f
    # both sizes are pinned where the kernels and the C-ABI are compiled
    for name in ("k_report.hip", "api_report.hip"):
        txt = open(os.path.join(ROOT, "mmwave_msc_amd", "csrc", name)).read()
        assert re.search(r"static_assert\(sizeof\(mmw_track_report\) == 324", txt), name
        assert re.search(r"static_assert\(sizeof\(mmw_track_event\) == 16", txt), name


def test_report_kernels_use_no_scratch_and_store_rows_in_16_byte_pieces():
    from tests._isa import _device_isa, _kernel_report, assert_clean, kernel_body
    rep, asm = _device_isa(("k_report",))["k_report"]
    rows = _kernel_report(rep)
    names = [k[0] for k in rows]
    for k in ("k_report_baseline", "k_report_count"):
        assert sum(k in n for n in names) == 1, (k, names)
    assert sum("k_report_write" in n for n in names) == 2, names   # the context's window, and each scene's own site
    assert len(names) == 4, names                                   # (the scan and the generation bump are k_scan.hip's)
    assert_clean(rows)
    for name, scratch, vspill, vgprs, occ, sspill in rows:
        body = kernel_body(asm, name)
        assert "scratch_" not in body, name
        if "k_report_write" in name:
            # the image goes LDS -> global in 16-byte pieces (ds_read_b128 + global_store_dwordx4), not a lane per row
            assert "ds_read_b128" in body and "global_store_dwordx4" in body, name
            assert occ >= 4, (name, occ)


def test_the_exports_share_one_scan_kernel_without_scratch():
    """k_scan.hip holds the one two-array offset scan of the library, k_pair_scan: no scratch, no spilled register.  The three
    kernels it replaced are in no export's device code, and its launcher is declared once and defined once.  (Its second kernel
    is k_uid_rebase: test_one_generation_bump_and_one_uid_match_for_report_zones_and_trails.)"""
    from tests._isa import _device_isa, _kernel_report, assert_clean, kernel_body
    isa = _device_isa(("k_scan", "k_report", "k_cloud", "k_skeleton"))
    rep, asm = isa["k_scan"]
    rows = _kernel_report(rep)
    assert len(rows) == 2 and sum("k_uid_rebase" in r[0] for r in rows) == 1, rows
    rows = [r for r in rows if "k_pair_scan" in r[0]]
    assert len(rows) == 1, rows
    name, scratch, vspill, vgprs, occ, sspill = rows[0]
    assert_clean(rows)
    body = kernel_body(asm, name, ".Lfunc_end")
    assert "s_endpgm" in body and "scratch_" not in body, name
    for f, (_, a) in isa.items():
        for old in ("k_%s_scan" % e for e in ("report", "cloud", "skel")):   # (the three copies this kernel replaced)
            assert old not in a, (f, old)
        assert ("k_pair_scan" in a) == (f == "k_scan"), f
    csrc = os.path.join(ROOT, "mmwave_msc_amd", "csrc")
    pat = r"\bvoid\s+launch_pair_scan\s*\("
    assert len(re.findall(pat, open(os.path.join(csrc, "mmw_kernels.hpp")).read())) == 1
    assert len(re.findall(pat, open(os.path.join(csrc, "k_scan.hip")).read())) == 1
    for fn in sorted(os.listdir(csrc)):
        if fn.endswith((".hip", ".hpp")) and fn not in ("mmw_kernels.hpp", "k_scan.hip"):
            assert not re.search(pat, open(os.path.join(csrc, fn)).read()), fn
    # the 1024-thread scan loop is written once, in the primitive all five scans use
    loop = "for (int o = 1; o < 1024; o <<= 1)"
    holders = [fn for fn in sorted(os.listdir(csrc)) if fn.endswith((".hip", ".hpp")) and loop in open(os.path.join(csrc, fn)).read()]
    assert holders == ["mmw_scan.hpp"] and open(os.path.join(csrc, "mmw_scan.hpp")).read().count(loop) == 1, holders
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "k_scan.hip" in mk and "mmw_scan.hpp" in mk and "api_export.hip" in mk


def test_one_generation_bump_and_one_uid_match_for_report_zones_and_trails():
    """k_uid_rebase (k_scan.hip) is the one kernel that bumps a generation word -- no scratch, no LDS, no spilled register -- with
    one launcher and one host entry; the three kernels and the three host wrappers it replaced are gone.  The match of two uid
    lists, uid_find, is written once, in the header the three by-uid consumers include."""
    from tests._isa import _device_isa, _kernel_report, assert_clean, kernel_body
    isa = _device_isa(("k_scan", "k_report", "k_zone", "k_trail"))
    rep, asm = isa["k_scan"]
    rows = [r for r in _kernel_report(rep) if "k_uid_rebase" in r[0]]
    assert len(rows) == 1, rows
    assert_clean(rows)
    body = kernel_body(asm, rows[0][0], ".Lfunc_end")
    assert "scratch_" not in body and not re.search(r"\bds_(read|write)", body), rows[0][0]
    assert re.search(r"LDS Size \[bytes/block\]: (\d+)", rep.split("remark: Function Name: " + rows[0][0])[1]).group(1) == "0"
    olds = ("k_report_rebase", "k_zone_rebase", "k_trail_rebase")
    for f, (_, a) in isa.items():
        for old in olds:
            assert old not in a, (f, old)
        assert ("k_uid_rebase" in a) == (f == "k_scan"), f
    csrc = os.path.join(ROOT, "mmwave_msc_amd", "csrc")
    src = {fn: open(os.path.join(csrc, fn)).read() for fn in sorted(os.listdir(csrc)) if fn.endswith((".hip", ".hpp"))}
    for fn, txt in src.items():
        for old in olds:
            assert old not in txt, (fn, old)
        for old in ("report_rebase", "zone_rebase", "trail_rebase"):   # (the host wrappers, and the launchers' names with them)
            assert old not in txt, (fn, old)
    launcher = r"\bvoid\s+launch_uid_rebase\s*\("
    assert {fn: len(re.findall(launcher, txt)) for fn, txt in src.items() if re.search(launcher, txt)} == {"k_scan.hip": 1, "mmw_kernels.hpp": 1}
    entry = r"\bint\s+uid_rebase\s*\("
    assert {fn: len(re.findall(entry, txt)) for fn, txt in src.items() if re.search(entry, txt)} == {"api_export.hip": 1, "mmw_ctx.hpp": 1}
    find = r"\bint\s+uid_find\s*\("
    assert {fn: len(re.findall(find, txt)) for fn, txt in src.items() if re.search(find, txt)} == {"mmw_uidlist.hpp": 1}
    for fn in ("k_report.hip", "k_zone.hip", "k_trail.hip"):
        assert '#include "mmw_uidlist.hpp"' in src[fn] and "uid_find(" in src[fn], fn
    assert "mmw_uidlist.hpp" in open(os.path.join(csrc, "Makefile")).read()


def test_table_kernels_still_compile_without_scratch_after_sharing_their_body():
    """k_table<false> / k_table<true> call the function the report rows come from (mmw_summary.hpp)."""
    from tests._isa import _device_isa, _kernel_report, assert_clean
    rep, _ = _device_isa(("k_misc",))["k_misc"]
    rows = [k for k in _kernel_report(rep) if "k_table" in k[0]]
    assert len(rows) == 2, rows
    assert_clean(rows)
    src = open(os.path.join(ROOT, "mmwave_msc_amd", "csrc", "k_misc.hip")).read()
    assert "summary_fields(" in src and "summary_fields(" in open(os.path.join(ROOT, "mmwave_msc_amd", "csrc", "k_report.hip")).read()


def test_report_dtype_arrays_are_plain_bytes():
    rows = np.zeros(3, _lib.TRACK_REPORT_DTYPE)
    assert rows.nbytes == 3 * 324 and rows.view(np.uint8).shape == (3 * 324,)
