"""The live tracks' skeletons (mmw_skeletons_*, include/mmw.h) as far as a machine without a GPU can check them: the entries refuse a
missing context, the numpy layout has the offsets pinned here (tests/test_abi.py holds every layout and prototype to the header),
mmw_skeleton_tables gives the reference's bones and
joint colours (tests/golden/skeleton_tables.json: Visualizer.py:100-142 as plain data), the kernels of csrc/k_skeleton.hip compile
without scratch or spilled registers and store 16-byte pieces, and the numpy restatement the GPU tests compare with
(tests/_skeleton_ref.py) reproduces three entries computed by hand.

No live run of the reference's Visualizer pins that restatement -- it imports Qt, pyqtgraph and matplotlib; the pin is the five
numpy lines of update_posture (Visualizer.py:274-283) as read."""
import ctypes as C
import json
import os
import re

import numpy as np

from mmwave_msc_amd import _lib
from tests import _abi
from tests import _skeleton_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["scene", "slot", "uid", "row", "flags", "gap", "joint", "reserved_"]


def test_header_declares_and_library_exports_the_skeleton_entries():
    code = _abi.header_code()
    assert code.index("mmw_clouds(") < code.index("typedef struct mmw_skeleton") < code.index("mmw_snapshot_header")   # after the clouds
    L = _lib.load()   # (declares every prototype: AttributeError if one is missing)
    # without a context every entry refuses its arguments instead of touching a device
    assert L.mmw_skeletons_async(None, None, 0, 0, 0, 0) == _lib.E_ARG
    assert L.mmw_skeletons_wait(None, 0, None, None) == _lib.E_ARG
    assert L.mmw_skeletons(None, None, 0, 0, 0, None, None) == _lib.E_ARG


def test_skeleton_layout_matches_the_c_struct():
    lay = _abi.c_layout()["mmw_skeleton"]
    size, off, joint_bytes = lay["size"], {f: lay["fields"][f][0] for f in FIELDS}, lay["fields"]["joint"][1]
    sdt = _lib.SKELETON_DTYPE
    assert size == 256 == sdt.itemsize
    assert list(sdt.names) == FIELDS
    assert [off[f] for f in FIELDS] == [0, 4, 8, 12, 16, 20, 24, 252]
    for f in FIELDS:
        assert sdt.fields[f][1] == off[f], f
    assert joint_bytes == 19 * 3 * 4 and sdt.fields["joint"][0] == np.dtype(("f4", (19, 3)))
    assert sdt.fields["gap"][0] == np.dtype("f4")
    for f in ("scene", "slot", "uid", "row", "flags", "reserved_"):
        assert sdt.fields[f][0] == np.dtype("i4"), f
    assert np.zeros(3, sdt).view(np.uint8).shape == (3 * 256,)
    # the size is pinned where the kernels and the C-ABI are compiled
    for name in ("k_skeleton.hip", "api_skeleton.hip"):
        txt = open(os.path.join(ROOT, "mmwave_msc_amd", "csrc", name)).read()
        assert re.search(r"static_assert\(sizeof\(mmw_skeleton\) == 256", txt), name


def test_skeleton_tables_are_the_references():
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "skeleton_tables.json")))
    conn, cls = _lib.skeleton_tables()
    assert conn.shape == (18, 2) and conn.dtype == np.int32 and cls.shape == (19,)
    assert conn.tolist() == gold["connections"] and len(gold["connections"]) == 18
    assert ((conn >= 0) & (conn < 19)).all()
    assert len(gold["keypoint_colors"]) == 19
    assert [_lib.SKEL_CLASS_NAMES[c] for c in cls] == gold["keypoint_colors"]
    assert np.flatnonzero(cls == 2).tolist() == [3]           # the head, and only the head
    assert set(np.unique(conn)) == set(range(19))             # every joint hangs on a bone
    # either pointer may be left out
    L = _lib.load()
    p = C.POINTER(C.c_int32)()
    assert L.mmw_skeleton_tables(None, None) == 0
    assert L.mmw_skeleton_tables(C.byref(p), None) == 0 and [p[0], p[1], p[34], p[35]] == [0, 1, 2, 18]


def test_skeleton_launcher_is_declared_once_and_the_files_are_built():
    csrc = os.path.join(ROOT, "mmwave_msc_amd", "csrc")
    decl = open(os.path.join(csrc, "mmw_kernels.hpp")).read()
    assert len(re.findall(r"\bvoid\s+launch_skeletons\s*\(", decl)) == 1
    for name in ("api_skeleton.hip", "api_context.hip", "mmw_ctx.hpp"):
        assert not re.search(r"\bvoid\s+launch_skeletons\s*\(", open(os.path.join(csrc, name)).read()), name
    assert len(re.findall(r"\bvoid\s+launch_skeletons\s*\(", open(os.path.join(csrc, "k_skeleton.hip")).read())) == 1
    assert len(re.findall(r"\bvoid\s+launch_pair_scan\s*\(", decl)) == 1
    assert len(re.findall(r"\bvoid\s+launch_pair_scan\s*\(", open(os.path.join(csrc, "k_scan.hip")).read())) == 1
    assert not re.search(r"\bvoid\s+launch_pair_scan\s*\(", open(os.path.join(csrc, "k_skeleton.hip")).read())
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "k_skeleton.hip" in mk and "api_skeleton.hip" in mk
    assert "export_free(c->skel)" in open(os.path.join(csrc, "api_context.hip")).read()


def test_skeleton_kernels_use_no_scratch_and_store_16_byte_pieces():
    from tests._isa import _device_isa, _kernel_report, assert_clean, kernel_body
    rep, asm = _device_isa(("k_skeleton",))["k_skeleton"]
    rows = _kernel_report(rep)
    names = [k[0] for k in rows]
    for k in ("k_skel_count", "k_skel_write"):
        assert sum(k in n for n in names) == 1, (k, names)
    assert len(names) == 2, names                                 # (the scan is k_pair_scan of k_scan.hip)
    assert_clean(rows)
    for name, scratch, vspill, vgprs, occ, sspill in rows:
        body = kernel_body(asm, name, ".Lfunc_end")   # (the whole kernel: one that returns early has more than one s_endpgm)
        assert "s_endpgm" in body, name
        assert "scratch_" not in body, name
        if "k_skel_write" in name:
            # the body of an entry leaves as 16-byte pieces and as nothing else: not one narrower store in the kernel
            stores = re.findall(r"\b(global_store_\w+|buffer_store_\w+|flat_store_\w+)", body)
            assert stores and set(stores) == {"global_store_dwordx4"}, (name, stores)
            assert occ >= 4, (name, occ)


def _kp(**at):
    kp = np.zeros(57, np.float32)
    for k, v in at.items():
        kp[int(k[1:])] = v
    return kp


def test_restatement_reproduces_three_entries_computed_by_hand():
    f32 = np.float32
    # A: joint 0 at (0.5, height 1.0, depth 0.25) relative, track at (2, 3): mirrored -0.5 + 2, depth 0.25 + 3; all other joints at the track
    skipped, gap, joint = ref.skeleton_of(_kp(k0=0.5, k19=1.0, k38=0.25), 2.0, 3.0)
    assert (skipped, float(gap)) == (False, 0.0)
    assert joint[0].tolist() == [1.5, 3.25, 1.0] and (joint[1:] == f32([2.0, 3.0, 0.0])).all()
    # B: SpineMid - Neck = (1.0 - 0.25, 1.5 - 0.5, 0) = (0.75, 1.0, 0): s = 1.5625 > 0.25, gap 1.25; joints 1, 2 by hand, track at (-1, 0.5)
    skipped, gap, joint = ref.skeleton_of(_kp(k1=1.0, k2=0.25, k20=1.5, k21=0.5), -1.0, 0.5)
    assert (skipped, float(gap)) == (True, 1.25)
    assert joint[1].tolist() == [-2.0, 0.5, 1.5] and joint[2].tolist() == [-1.25, 0.5, 0.5] and joint[0].tolist() == [-1.0, 0.5, 0.0]
    # C: kp[0] = 1 + 2^-23 and x[0] = 2^-24 - 2^-50.  In fp64 the sum is -(1 + 2^-24 + 2^-50): past the midpoint of -1 and
    # -(1 + 2^-23), ONE rounding gives -(1 + 2^-23) = 0xBF800001.  In float32, x[0] rounds to 2^-24 first, the sum is the exact tie
    # -(1 + 2^-24), and ties-to-even gives -1 = 0xBF800000.  The reference computes the former.
    k0, x0 = f32(1.0) + f32(2.0 ** -23), 2.0 ** -24 - 2.0 ** -50
    skipped, gap, joint = ref.skeleton_of(_kp(k0=k0, k2=0.5), x0, 0.0)
    once, twice = joint[0, 0], ref.fp32_arithmetic_joint_x(k0, x0)
    assert once.view(np.uint32) == 0xBF800001 and np.asarray(twice, f32).view(np.uint32) == 0xBF800000
    assert once != twice
    assert (skipped, float(gap)) == (False, 0.5)   # (0 - 0.5, 0, 0): s = 0.25 is not > 0.25
    # ... and the reference's own in-place arithmetic on a float32 view with a shape-(1,) fp64 array gives the same bits
    view = _kp(k0=k0).reshape(3, -1)
    view[0] *= -1
    view[0] += np.array([x0])
    assert view[0, 0].view(np.uint32) == 0xBF800001
    # NaN: the comparison is false (drawn), gap NaN
    skipped, gap, _ = ref.skeleton_of(_kp(k1=np.nan), 0.0, 0.0)
    assert not skipped and np.isnan(gap)
