"""The live tracks' point clouds (mmw_clouds_*, include/mmw.h) as far as a machine without a GPU can check them: the entries refuse
a missing context, the directory entries and points have the sizes and field types the kernels pin (tests/test_abi.py holds every
layout and prototype to the header), and the kernels of csrc/k_cloud.hip compile without scratch or spilled registers and move rows and points as 16-byte pieces."""
import os
import re

import numpy as np

from mmwave_msc_amd import _lib
from tests import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS_T = ["scene", "slot", "uid", "first", "count", "frames", "newest", "dropped"]
FIELDS_P = ["x", "y", "z", "track"]


def test_header_declares_and_library_exports_the_cloud_entries():
    L = _lib.load()   # (declares every prototype: AttributeError if one is missing)
    # without a context every entry refuses its arguments instead of touching a device
    assert L.mmw_clouds_async(None, None, 0, None, 0, 0, 0, 0) == _lib.E_ARG
    assert L.mmw_clouds_wait(None, 0, None, None) == _lib.E_ARG
    assert L.mmw_clouds(None, None, 0, None, 0, 0, 0, None, None) == _lib.E_ARG


def test_cloud_layouts_match_the_c_structs():
    lay = _abi.c_layout()
    tdt, pdt = _lib.CLOUD_TRACK_DTYPE, _lib.CLOUD_POINT_DTYPE
    assert (lay["mmw_cloud_track"]["size"], lay["mmw_cloud_point"]["size"]) == (32, 16) == (tdt.itemsize, pdt.itemsize)
    assert list(tdt.names) == FIELDS_T and list(pdt.names) == FIELDS_P
    for f in FIELDS_T:
        assert tdt.fields[f][0] == np.dtype("i4"), f
    for f in FIELDS_P:
        assert pdt.fields[f][0] == np.dtype("i4" if f == "track" else "f4"), f
    # both sizes are pinned where the kernels and the C-ABI are compiled
    for name in ("k_cloud.hip", "api_cloud.hip"):
        txt = open(os.path.join(ROOT, "mmwave_msc_amd", "csrc", name)).read()
        assert re.search(r"static_assert\(sizeof\(mmw_cloud_track\) == 32", txt), name
        assert re.search(r"static_assert\(sizeof\(mmw_cloud_point\) == 16", txt), name


def test_cloud_launcher_is_declared_once_and_the_files_are_built():
    csrc = os.path.join(ROOT, "mmwave_msc_amd", "csrc")
    decl = open(os.path.join(csrc, "mmw_kernels.hpp")).read()
    assert len(re.findall(r"\bvoid\s+launch_clouds\s*\(", decl)) == 1
    assert len(re.findall(r"\bvoid\s+launch_pair_scan\s*\(", decl)) == 1
    assert len(re.findall(r"\bvoid\s+launch_pair_scan\s*\(", open(os.path.join(csrc, "k_scan.hip")).read())) == 1
    assert not re.search(r"\bvoid\s+launch_pair_scan\s*\(", open(os.path.join(csrc, "k_cloud.hip")).read())
    for name in ("api_cloud.hip", "api_context.hip"):
        assert not re.search(r"\bvoid\s+launch_clouds\s*\(", open(os.path.join(csrc, name)).read()), name
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "k_cloud.hip" in mk and "api_cloud.hip" in mk
    assert "export_free(c->cloud)" in open(os.path.join(csrc, "api_context.hip")).read()   # (mmw_destroy releases the scratch)
    # the product build knows nothing of the diagnostic switch that makes k_cloud_write ignore the slot permutation
    assert "MMW_MUTANT_CLOUD_IDENT_SLOTS" not in mk


def test_cloud_kernels_use_no_scratch_and_move_16_byte_pieces():
    from tests._isa import _device_isa, _kernel_report, assert_clean, kernel_body
    rep, asm = _device_isa(("k_cloud",))["k_cloud"]
    rows = _kernel_report(rep)
    names = [k[0] for k in rows]
    assert sum("k_cloud_count" in n for n in names) == 1, names
    assert sum("k_cloud_write" in n for n in names) == 2, names   # MMW_CLOUD_POINTS and MMW_CLOUD_ROWS
    assert len(names) == 3, names                                 # (the scan is k_pair_scan of k_scan.hip)
    assert_clean(rows)
    for name, scratch, vspill, vgprs, occ, sspill in rows:
        body = kernel_body(asm, name, ".Lfunc_end")   # (the whole kernel: one that returns early has more than one s_endpgm)
        assert "s_endpgm" in body, name
        assert "scratch_" not in body, name
        if "k_cloud_write" in name:
            # ROWS: a row moves as four 16-byte pieces; POINTS: x, y arrive as one 16-byte load and a point leaves as one 16-byte store
            assert "global_load_dwordx4" in body and "global_store_dwordx4" in body, name
            assert occ >= 4, (name, occ)


def test_cloud_dtype_arrays_are_plain_bytes():
    d = np.zeros(3, _lib.CLOUD_TRACK_DTYPE)
    p = np.zeros(5, _lib.CLOUD_POINT_DTYPE)
    assert d.nbytes == 3 * 32 and d.view(np.uint8).shape == (3 * 32,)
    assert p.nbytes == 5 * 16 and p.view(np.uint8).shape == (5 * 16,)
