"""Scenes of many targets on a grid: more live tracks in a scene than 16, 32 or 40, for tests/test_gpu_parity.py and the report,
skeleton, zone, trail and tripwire suites."""
import numpy as np


def grid_scene(seed, n_frames, n_pts, n_targets):
    """Targets on a 1.3 m grid (4 rows in y), 24 points each per frame, the rest clutter; fp32-representable."""
    rng = np.random.default_rng(seed)
    cols = (n_targets + 3) // 4
    centres = np.array([[-0.65 * (cols - 1) + 1.3 * (k // 4), 1.5 + 1.3 * (k % 4)] for k in range(n_targets)])
    vel = rng.normal(0.0, 0.08, size=(n_targets, 2))
    out = np.zeros((n_frames, n_pts, 8))
    per = 24
    for f in range(n_frames):
        c = centres + vel * 0.1 * f
        rows = []
        for k in range(n_targets):
            r = np.zeros((per, 8))
            r[:, 0:2] = c[k] + rng.normal(0.0, 0.08, size=(per, 2))
            r[:, 2] = rng.uniform(0.3, 1.5, size=per)
            r[:, 3:5] = vel[k] + rng.normal(0.0, 0.03, size=(per, 2))
            r[:, 5] = rng.normal(0.0, 0.03, size=per)
            rows.append(r)
        ncl = n_pts - per * n_targets
        cl = np.zeros((ncl, 8))
        cl[:, 0] = rng.uniform(-6.0, 6.0, size=ncl); cl[:, 1] = rng.uniform(0.3, 7.5, size=ncl); cl[:, 2] = rng.uniform(0.05, 2.4, size=ncl)
        cl[:, 3:6] = rng.normal(0.0, 0.05, size=(ncl, 3))
        fr = np.concatenate(rows + [cl])
        fr[:, 6] = rng.normal(0.0, 0.3, size=n_pts); fr[:, 7] = rng.gamma(1.0, 30.0, size=n_pts)
        out[f] = fr[rng.permutation(n_pts)]
    return out.astype(np.float32)


def many_tracks(shape):
    """(sb, pts[F][S][N][8], n_scenes, n_pts, frames, floor): "track_cap_40", the grid scenes of the skeleton tests (lanes past 16 in both
    scenes), or "track_cap_64", the report's scene of 36 targets beside one of 5 (lanes and uid slots past 32: the upper half of the
    64-bit ballots); `floor` is the track count a run must pass."""
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    from tests._layouts import make_checked
    if shape == "track_cap_40":
        n_s, n_pts, frames, floor = 2, 640, 3, 16
        sb = make_checked(n_s, n_pts, "per_scene", tr_max_tracks=28, db_min_samples=12, track_cap=40)
        pts = np.stack([grid_scene(4300 + s, frames, n_pts, 18 + 2 * s) for s in range(n_s)], axis=1)
    else:
        n_s, n_pts, frames, floor = 2, 1024, 5, 32
        sb = SceneBatch(_lib.default_config(tr_max_tracks=40, db_min_samples=12, track_cap=64), n_s, n_pts)
        assert sb.track_cap == 64
        pts = np.stack([grid_scene(4700, frames, n_pts, 36), grid_scene(4701, frames, n_pts, 5)], axis=1)
    return sb, pts, n_s, n_pts, frames, floor
