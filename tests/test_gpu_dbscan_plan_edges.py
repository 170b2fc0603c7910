"""The DBSCAN workers' LDS plan at its switches (csrc/mmw_dbqueue.hpp: one plan per kind of worker, shared by kernel and launcher;
csrc/mmw_balltree.hpp: the BallTree carve-up in front of it): contexts of 2 scenes whose ring capacity ring x max_pts sits on each of them --
256 | 257 (small class / large clouds), 511 | 512 | 513 (one exchange slot per thread of a 512-thread block / thread-per-point
or strided build), 1536 | 1538 (512- / 256-point neighbourhood rows), 1920 | 1922 (LDS / slabs in global memory).  The rings
fill with clutter that cannot hold a core point, the last frame brings one tight blob: the scene clusters its whole, full
ring, dbn == capacity -- the smallest shapes at which a wrong carve-up or a mis-sized scratch shows (an out-of-range LDS access
does not fault, it corrupts results).  Bit for bit against oracle/c, as tests/test_gpu_fuzz.py::run_case."""
import functools

import numpy as np
import pytest

from tests._golden import assert_tracks_match
from tests._layouts import make_checked

S = 2
SHAPES = [(1, 256), (1, 257), (1, 511), (2, 256), (1, 513), (2, 768), (2, 769), (2, 960), (2, 961)]   # (ring, max_pts)
assert [r * n for r, n in SHAPES] == [256, 257, 511, 512, 513, 1536, 1538, 1920, 1922]


def _clutter(n, f, s):
    """n points of a 16 x 8 x 8 lattice, 1.0 / 0.75 / 1.2 m apart in x / y / z and shifted per frame and scene: within
    2 eps / w_min (the reach of any BallTree neighbourhood, csrc/mmw_balltree.hpp) a point sees its two y- and two
    z-neighbours of its own frame and as many of every other frame of the ring -- far fewer than min_samples."""
    i = np.arange(n)
    p = np.zeros((n, 8))
    p[:, 0] = -8.0 + 1.0 * (i % 16) + 0.37 * f + 0.05 * s
    p[:, 1] = 1.0 + 0.75 * ((i // 16) % 8) + 0.11 * f
    p[:, 2] = -2.0 + 1.2 * (i // 128) + 0.07 * s
    p[:, 6] = 10.0 + (i % 7)
    p[:, 7] = 1.0
    return p


def _inputs(ring, n, min_samples):
    """[ring][S][n][8]: ring - 1 frames of clutter, then one with a blob of min_samples + 5 points in front of its clutter"""
    pts = np.zeros((ring, S, n, 8))
    for f in range(ring):
        for s in range(S):
            pts[f, s] = _clutter(n, f, s)
    b = min_samples + 5
    rng = np.random.default_rng(1234 + ring * 4096 + n)
    for s in range(S):
        blob = pts[ring - 1, s, :b]
        blob[:, 0:3] = np.array([0.53 + 0.4 * s, 2.9, 0.31]) + rng.uniform(-0.04, 0.04, size=(b, 3))
        blob[:, 3:6] = rng.uniform(-0.02, 0.02, size=(b, 3))
    return pts


@functools.lru_cache(maxsize=None)
def _reference(ring, n):
    """The oracle's answers, once per shape: per frame and scene (assoc, labels or None, n_tracks, track records)."""
    from oracle import c_oracle as co
    cfg = co.default_config(fb_frames_batch=ring - 1)
    pts = _inputs(ring, n, int(cfg.db_min_samples))
    scenes = [co.OracleScene(cfg, n) for _ in range(S)]
    frames = []
    for f in range(ring):
        row = []
        for s in range(S):
            oa, ol = scenes[s].track(pts[f, s], 0.1)
            row.append((oa, ol, scenes[s].n_tracks, scenes[s].tracks().copy(), scenes[s].batch_ring().copy()))
        frames.append(row)
    return pts, frames


def _check_reference(ring, n):
    pts, frames = _reference(ring, n)
    for f in range(ring):
        for s in range(S):
            oa, ol, ntr, _, _ = frames[f][s]
            assert np.all(oa == -1), (ring, n, f, s)                              # no track to be assigned to
            assert ol is not None and len(ol) == (f + 1) * n, (ring, n, f, s)   # apply_DBscan ran on everything so far
            if f < ring - 1:
                assert np.all(ol == -1) and ntr == 0, (ring, n, f, s)            # clutter: no core point, no track, the ring fills
            else:
                assert len(ol) == ring * n and ol.max() >= 0 and ntr >= 1, (ring, n, s, int(ol.max()), ntr)   # the whole, full ring; a cluster


@pytest.mark.parametrize("ring,n", SHAPES)
def test_inputs_fill_the_ring_and_cluster_on_the_oracle(ring, n):
    """The inputs, on the oracle alone: clutter without a core point while the ring fills, then at least one cluster
    out of a cloud of exactly ring x max_pts points."""
    _check_reference(ring, n)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["per_scene", "one_workgroup"])
@pytest.mark.parametrize("ring,n", SHAPES)
def test_full_ring_at_the_switches_of_the_lds_plan_vs_oracle(ring, n, layout):
    _check_reference(ring, n)
    pts, frames = _reference(ring, n)
    sb = make_checked(S, n, layout, fb_frames_batch=ring - 1)
    cnt, dts = np.full(S, n, dtype=np.int32), np.full(S, 0.1)
    for f in range(ring):
        assoc, labels, dbn = sb.step_host(pts[f], cnt, dts)
        ntr = sb.num_tracks()
        trk = sb.tracks(cap=max(int(ntr.max()), 1))
        ln, rn = sb.batch_ring()
        for s in range(S):
            oa, ol, ontr, otrk, oring = frames[f][s]
            assert np.array_equal(assoc[s, :n], oa), (ring, n, f, s)
            assert dbn[s] == len(ol) == (f + 1) * n, (ring, n, f, s, int(dbn[s]))
            assert np.array_equal(labels[s, : dbn[s]], ol), (ring, n, f, s)
            assert ntr[s] == ontr, (ring, n, f, s, int(ntr[s]), ontr)
            assert_tracks_match(trk[s, : ntr[s]], otrk, ctx=f"ring {ring} n {n} f{f} s{s}", exact=True)
            assert np.array_equal(rn[s, : ln[s]], oring), (ring, n, f, s)
    assert np.all(dbn == ring * n)   # the last step clustered the full ring of every scene
    sb.check()                       # (no bounded wait of the queue protocol gave up, no sticky error)
    sb.close()
