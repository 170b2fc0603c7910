"""Helpers shared by the parity tests: golden-file access and comparisons.

Tolerances (stated once, used everywhere):
  * integer outputs (association, DBSCAN labels, track count/order, point
    counts, ring lengths, static flag): bit-exact.
  * fp64 state vs the numpy/BLAS reference: |a-b| <= 1e-9 * max(1, |a|, |b|)
    (BLAS summation order / LAPACK LU / libm pow differ by a few ULP and are
    amplified by the 6x6 inverse; observed worst 2e-9 relative on ~1e-3 entries).
  * fp32 feature tensors: bit-exact (NaN equal to NaN) up to the order of rows with EQUAL x inside
    one 64-row frame.  The reference sorts with np.argsort's default (unstable,
    CPU-dispatch dependent) algorithm (Utils.py:513), so the order of tied rows
    is not defined by the reference; this build orders ties by row position.
    `canon_feat` sorts every tie group by the remaining columns on both sides, after asserting that both sides ARE sorted by
    x (assert_feat_equal).  Where both sides are this build's own stable sort -- GPU, C oracle, the numpy restatements -- the
    comparison is by bits and ties are not open (assert_feat_identical): tests/_sort_inputs.py has the frames that tie.
"""
import glob
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F64_TOL = 1e-9
INT_FIELDS = ("point_num", "is_static", "ring_len", "ring_n")
F64_FIELDS = ("x", "P", "centroid", "min_vals", "max_vals", "spread_est", "group_disp_est", "n_est", "lifetime")


def scenario_names():
    # (track_exceptions.npz is not a scenario: the error scenes of tests/_error_scenes.py, all in one file)
    names = sorted(os.path.basename(p)[len("track_"):-4] for p in glob.glob(os.path.join(GOLDEN, "track_*.npz")))
    return [n for n in names if n != "exceptions"]


def load_scenario(name):
    z = np.load(os.path.join(GOLDEN, f"track_{name}.npz"), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d["overrides"] = json.loads(str(d["overrides"]))
    return d


def scenario_tol(g):
    """fp64 tolerance against the recording of a scenario.  Runs of measurement-free frames (track() on empty clouds:
    the reference keeps updating with the stale centroid) multiply ULP-level differences by 1.5-2x per frame -- 3e-9
    after 28 such frames in `empty_tracked` --, so those scenarios are compared at 1e-7; integers stay exact and the GPU
    still equals the C oracle bit for bit."""
    return 1e-7 if g["overrides"].get("TRACK_EMPTY") else F64_TOL


def close64(a, b, tol=F64_TOL):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    scale = np.maximum(1.0, np.maximum(np.abs(a), np.abs(b)))
    return bool(np.all(np.abs(a - b) <= tol * scale))


def assert_tracks_match(got, want, ctx="", tol=F64_TOL, exact=False):
    assert len(got) == len(want), f"{ctx}: track count {len(got)} != {len(want)}"
    for name in INT_FIELDS:
        if not np.array_equal(got[name], want[name]):
            # (which tracks, and what else differs on them: one field of one track, a track's whole state, or the order of the list)
            rows = sorted({int(i) for i in np.argwhere(np.asarray(got[name]) != np.asarray(want[name]))[:, 0]})
            others = [n for n in INT_FIELDS + F64_FIELDS if n != name and not np.array_equal(np.asarray(got[n])[rows], np.asarray(want[n])[rows], equal_nan=n in F64_FIELDS)]
            raise AssertionError(f"{ctx}: int field {name} differs on tracks {rows} of {len(want)}: got {np.asarray(got[name]).tolist()} want "
                                 f"{np.asarray(want[name]).tolist()}; on those tracks these fields differ too: {others}")
    for name in F64_FIELDS:
        if exact:
            if not np.array_equal(got[name], want[name]):
                g, w = np.asarray(got[name], dtype=np.float64), np.asarray(want[name], dtype=np.float64)
                bad = np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))
                raise AssertionError(f"{ctx}: field {name} not bit-equal at {bad[:6].tolist()} ({len(bad)} entries): got {g[tuple(bad[0])]!r} want {w[tuple(bad[0])]!r}")
        else:
            assert close64(got[name], want[name], tol), (
                f"{ctx}: field {name} differs by {np.abs(np.asarray(got[name]) - np.asarray(want[name])).max():.3e}")


def overrides_to_cfg_kwargs(over):
    """Map reference-constant overrides stored in a fixture to config kwargs."""
    kw = {}
    for k, v in over.items():
        if k == "TR_MAX_TRACKS":
            kw["tr_max_tracks"] = int(v)
        elif k == "MOTION_MODEL":
            kw["dim_x"] = 6 if v == "CONST_VEL_MODEL" else 9
        elif k == "FB_FRAMES_BATCH":
            kw["fb_frames_batch"] = int(v)
        elif k == "KF_ENABLE_EST":
            kw["kf_enable_est"] = int(bool(v))
        elif k in ("TRACK_EMPTY", "BATCH_INIT", "BATCH_RESIZE", "NONFINITE"):
            pass   # not a constant: the scenario calls track() on its empty frames (see tests)
        elif k == "SEEK_INNER":
            kw["seek_inner"] = int(bool(v))
        elif k == "FB_FRAMES_BATCH_STATIC":
            kw["fb_frames_batch_static"] = int(v)
        elif k == "DB_POINTS_THRES":
            kw["db_points_thres"] = int(v)
        else:
            raise KeyError(k)
    return kw


def canon_feat(feat):
    """Canonical order inside equal-x groups of every 64-row frame (see module docstring).  Column 0 of every frame must be
    sorted already -- non-decreasing, NaN at the end --: a frame that is not is refused here, whatever its rows are; rows are then
    re-ordered (by the remaining columns) only inside runs of equal x, the NaN rows being one such run."""
    f = np.asarray(feat, dtype=np.float32)
    if f.size == 0:
        return f
    flat = f.reshape(-1, 64, 5).copy()
    for b in range(flat.shape[0]):
        blk = flat[b]
        x = blk[:, 0]
        isn = np.isnan(x)
        n = 64 - int(isn.sum())
        assert not isn[:n].any() and np.all(x[: n - 1] <= x[1:n]), f"frame {b}: column 0 is not sorted (non-decreasing, NaN last): {x.tolist()}"
        order = np.lexsort((blk[:, 4], blk[:, 3], blk[:, 2], blk[:, 1], np.where(isn, 0, x), isn))   # (x is sorted: only tie groups move)
        flat[b] = blk[order]
    return flat.reshape(f.shape)


def assert_feat_equal(got, want, ctx=""):
    """Equal up to the order of rows inside groups of equal x: for comparisons with the REFERENCE, whose tie order is open.  Both
    sides must be sorted by x."""
    got = np.asarray(got, dtype=np.float32)
    want = np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, f"{ctx}: feature shape {got.shape} != {want.shape}"
    # (equal_nan: a NaN doppler / peakVal of an assigned point travels into its track's feature map on both sides)
    assert np.array_equal(canon_feat(got), canon_feat(want), equal_nan=True), f"{ctx}: feature tensor differs"


def assert_feat_identical(got, want, ctx=""):
    """Equal bit for bit, as uint32 -- a -0.0 in the wrong row, or two rows of a tie group exchanged, is a difference: for
    comparisons where both sides are this project's own stable sort (GPU, C oracle, the numpy restatements).  A NaN equals a
    NaN whatever its sign and payload, which no operation of either side promises."""
    got = np.asarray(got, dtype=np.float32)
    want = np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, f"{ctx}: feature shape {got.shape} != {want.shape}"
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    if not same.all():
        bad = np.argwhere(~same)
        raise AssertionError(f"{ctx}: feature tensor not bit-equal at {len(bad)} entries, first {bad[:6].tolist()}: got {got[tuple(bad[0])]!r} "
                             f"want {want[tuple(bad[0])]!r}")
