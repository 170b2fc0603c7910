"""Track trails (mmw_trails_*, include/mmw.h) as far as a machine without a GPU can check them: the restatement the GPU tests
compare against (tests/_trail_ref.py) does what the header says on hand-made states, the entries refuse a missing context, both
new files are compiled into the library, the three kernels of csrc/k_trail.hip take no scratch and no LDS, and the host helpers of
mmwave_msc_amd/trails.py do what they say on a hand-made pair of arrays.  (tests/test_abi.py holds every layout and prototype to
the header.)"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from mmwave_msc_amd import _lib
from tests._trail_ref import TrailRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mmwave_msc_amd", "csrc")
CAP = 4


def _state(*scenes):
    """(tracks[S, CAP] TRACK_DTYPE, num_tracks[S]) from one list per scene of (uid, x, y[, z[, is_static[, lifetime]]])."""
    trk = np.zeros((len(scenes), CAP), _lib.TRACK_DTYPE)
    ntr = np.zeros(len(scenes), np.int32)
    for s, rows in enumerate(scenes):
        ntr[s] = len(rows)
        for j, r in enumerate(rows):
            r = tuple(r) + (0.0, 0, 0.0)[len(r) - 3:]
            trk[s, j]["uid"], trk[s, j]["x"][:3], trk[s, j]["is_static"], trk[s, j]["lifetime"] = r[0], r[1:4], r[4], r[5]
    return trk, ntr


def _pts(points):
    return [(float(p["t"]), float(p["x"]), float(p["y"]), float(p["z"]), int(p["flags"])) for p in points]


def test_restatement_ring_wrap_position_change_slot_reuse_rebase_and_last():
    U, ST = _lib.TRAIL_UPDATED, _lib.TRAIL_STATIC
    ref = TrailRef(2, CAP, 2)
    # frame 0: scene 0 holds uids 5 and 6, scene 1 nobody
    st = _state([(5, 0.0, 0.0, 1.0), (6, 10.0, 0.0, 0.5, 1, 0.125)], [])
    ref.sample(*st, t=[0.5, 0.5])
    d, p = ref.export(*st, scene_base=3)
    assert d.tolist() == [(3, 0, 5, 0, 1, 1, 0.5, 0.0), (3, 1, 6, 1, 1, 1, 0.5, 0.0)]
    assert _pts(p) == [(0.5, 0.0, 0.0, 1.0, U), (0.5, 10.0, 0.0, 0.5, ST)]
    # frame 1: both walk
    st = _state([(5, 3.0, 4.0, 1.0), (6, 10.0, 1.0, 0.5)], [])
    ref.sample(*st, t=[1.0, 1.0])
    # frame 2: uid 5 is gone -- uid 6 drops from list position 1 to 0 and keeps its trail; uid 7 is born and takes uid 5's slot
    st = _state([(6, 10.0, 3.0, 0.5), (7, -1.0, -1.0, 0.0)], [(0, 1.0, 1.0, 1.0)])
    ref.sample(*st, t=[1.5, 1.5])
    d, p = ref.export(*st)
    assert d.tolist() == [(0, 0, 6, 0, 2, 3, 0.5, 3.0), (0, 1, 7, 2, 1, 1, 1.5, 0.0), (1, 0, 0, 3, 1, 1, 1.5, 0.0)]
    assert _pts(p) == [(1.0, 10.0, 1.0, 0.5, U), (1.5, 10.0, 3.0, 0.5, U),      # depth 2: uid 6's first sample was overwritten
                       (1.5, -1.0, -1.0, 0.0, U), (1.5, 1.0, 1.0, 1.0, U)]
    assert (ref.wraps, ref.moved, ref.reused) == (1, 1, 1)
    assert ref.trails[0][7].slot == 0 and ref.trails[0][6].slot == 1
    # last = 1: the newest point of every entry; total, t_first and travelled are the whole trail's
    d1, p1 = ref.export(*st, last=1)
    assert d1.tolist() == [(0, 0, 6, 0, 1, 3, 0.5, 3.0), (0, 1, 7, 1, 1, 1, 1.5, 0.0), (1, 0, 0, 2, 1, 1, 1.5, 0.0)]
    assert _pts(p1) == [_pts(p)[1], _pts(p)[2], _pts(p)[3]]
    # an export changes nothing; a track born since the last sample has an empty entry
    st2 = _state([(6, 10.0, 3.0, 0.5), (7, -1.0, -1.0, 0.0), (8, 0.0, 0.0, 0.0)], [(0, 1.0, 1.0, 1.0)])
    d2, p2 = ref.export(*st2)
    assert d2.tolist()[:3] == [(0, 0, 6, 0, 2, 3, 0.5, 3.0), (0, 1, 7, 2, 1, 1, 1.5, 0.0), (0, 2, 8, 3, 0, 0, 0.0, 0.0)] and len(p2) == 4
    # a rebase of scene 0: its entries are empty until the next sample, then its trails are new; scene 1 goes on; flags leave
    # scene 1 out of the second call, and t = None is the scene's call ordinal (3 earlier calls asked scene 0)
    ref.rebase([0])
    d, p = ref.export(*st)
    assert d.tolist() == [(0, 0, 6, 0, 0, 0, 0.0, 0.0), (0, 1, 7, 0, 0, 0, 0.0, 0.0), (1, 0, 0, 0, 1, 1, 1.5, 0.0)] and len(p) == 1
    ref.sample(*st, flags=[1, 0])
    d, p = ref.export(*st)
    assert d.tolist() == [(0, 0, 6, 0, 1, 1, 3.0, 0.0), (0, 1, 7, 1, 1, 1, 3.0, 0.0), (1, 0, 0, 2, 1, 1, 1.5, 0.0)]
    assert ref.ordinal.tolist() == [4, 3]
    # sampling twice without a step gives two samples; NaN stays, fp32 overflow is +inf
    st = _state([(6, np.nan, 3.0, 0.5), (7, 1e39, -1.0, -0.0)], [(0, 1.0, 1.0, 1.0)])
    ref.sample(*st)
    st = _state([(6, 10.0, 3.0, 0.5), (7, 1e39, -1.0, -0.0)], [(0, 1.0, 1.0, 1.0)])
    ref.sample(*st)
    d, p = ref.export(*st)
    assert np.isnan(d["travelled"][0]) and d["travelled"][1] == np.float64(1e39) + 1.0 and d["total"].tolist() == [3, 3, 3]
    assert p["x"][3] == np.inf and np.signbit(p["z"][3]) and d["travelled"][2] == 0.0


def test_every_trail_entry_refuses_a_null_context():
    L = _lib.load()   # (declares every prototype: AttributeError if one is missing)
    assert L.mmw_trails_enable(None, 4) == _lib.E_ARG
    assert L.mmw_trails_sample(None, None, None) == _lib.E_ARG
    assert L.mmw_trails_async(None, None, 0, None, 0, 0, 0, 0) == _lib.E_ARG
    assert L.mmw_trails_wait(None, 0, None, None) == _lib.E_ARG
    assert L.mmw_trails(None, None, 0, None, 0, 0, 0, None, None) == _lib.E_ARG


def test_trail_layouts_and_sources():
    assert _lib.TRAIL_TRACK_DTYPE.itemsize == 40 and _lib.TRAIL_POINT_DTYPE.itemsize == 24
    assert (_lib.TRAIL_DEPTH_MAX, _lib.TRAIL_STATIC, _lib.TRAIL_UPDATED) == (256, 1, 2)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*?[^\\])$", mk, re.M | re.S).group(1).split()
    assert "k_trail.hip" in srcs and "api_trail.hip" in srcs, srcs
    # the wave's prefix sum has one definition, shared with the zones' kernels
    for name in ("k_zone.hip", "k_trail.hip"):
        txt = open(os.path.join(CSRC, name)).read()
        assert '#include "mmw_wave.hpp"' in txt and not re.search(r"int wave_excl_sum\(", txt), name
    assert "launch_pair_scan(" in open(os.path.join(CSRC, "k_trail.hip")).read()


def test_trail_kernels_take_no_scratch_and_no_lds():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "k_trail.hip"), "-o", os.devnull],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", out.stderr)[1:]
    seen = {}
    for blk in blocks:
        name = blk.split()[0]
        seen[name] = (int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1)), int(re.search(r"LDS Size \[bytes/block\]: (\d+)", blk).group(1)))
    for k in ("k_trail_sample", "k_trail_count", "k_trail_write"):   # (the generation bump is k_uid_rebase of k_scan.hip)
        hit = [n for n in seen if k in n]
        assert len(hit) == 1, (k, sorted(seen))
        assert seen[hit[0]] == (0, 0), (k, seen[hit[0]])
    assert len(seen) == 3, sorted(seen)


def test_split_window_length_and_age():
    from mmwave_msc_amd import trails
    d = np.array([(2, 0, 9, 0, 3, 7, 0.25, 100.0), (2, 1, 11, 3, 0, 0, 0.0, 0.0), (4, 0, 0, 3, 1, 1, 2.0, 0.0)], _lib.TRAIL_TRACK_DTYPE)
    p = np.array([(1.0, 0.0, 0.0, 1.0, 2), (1.5, 3.0, 4.0, 1.0, 2), (2.0, 3.0, 4.5, 1.0, 0), (2.0, 7.0, 7.0, 0.0, 3)], _lib.TRAIL_POINT_DTYPE)
    parts = trails.split(d, p)
    assert [len(v) for v in parts] == [3, 0, 1]
    assert parts[0]["t"].tolist() == [1.0, 1.5, 2.0] and parts[2]["x"].tolist() == [7.0]
    assert np.shares_memory(parts[0], p)                                     # views, not copies
    wl = trails.window_length(d, p)
    assert wl.dtype == np.float32 and wl.tolist() == [5.5, 0.0, 0.0]
    ag = trails.age(d, p)
    assert ag.dtype == np.float64 and ag.tolist() == [1.75, 0.0, 0.0]
    assert trails.split(d[:0], p[:0]) == [] and len(trails.window_length(d[:0], p[:0])) == 0
