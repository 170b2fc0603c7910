"""The scenario of the live-track report tests (tests/test_gpu_report.py): S scenes of three walking targets that arrive late
and leave again, with track lifetimes short enough (0.25 s = three frames without a point) that the tracks of targets that
left expire inside the run -- every scene's track count rises and falls, and in some frames a scene gains one track and loses
another.  Generated once per session and shared, never modified."""
import functools

import numpy as np

S, N, F, T = 24, 96, 12, 4
# tr_gate: the gate test is log|det C| + y' C^-1 y < TR_GATE (Tracking.py:530-574) and log|det C| of a settled track is about -25, so
# at the default 4.5 a track whose target has left keeps taking clutter -- ONE point a frame resets its lifetime -- and never
# expires inside a 12-frame run.  At -5 it only takes points of its own target: tracks of targets that left expire after three
# frames.  Through the C oracle (oracle/c) on these 24 scenes x 12 frames: a scene's track count rises 71 times and falls 37
# times, and in 10 scene-frames a track is spawned while another expires.
CFG_KW = dict(tr_max_tracks=T, db_min_samples=12, tr_lifetime_dynamic=0.25, tr_lifetime_static=0.25, tr_gate=-5.0)


def presence_of(scene: int, n_frames: int = F) -> np.ndarray:
    """presence[F, 3]: target j of `scene` is in view from frame a_j to frame l_j - 1.  The first target is there from the start
    and leaves early, the second arrives about when the first one's track expires, the third arrives late and stays."""
    rng = np.random.default_rng(9100 + scene)
    p = np.zeros((n_frames, 3), dtype=bool)
    l0 = int(rng.integers(2, 5))
    p[:l0, 0] = True
    a1 = int(rng.integers(l0, l0 + 3))
    p[a1: a1 + int(rng.integers(3, 5)), 1] = True
    a2 = int(rng.integers(5, n_frames - 3))
    p[a2:, 2] = True
    return p


@functools.lru_cache(maxsize=None)
def scenario(n_scenes: int = S, n_pts: int = N, n_frames: int = F, seed: int = 5200):
    """(pts[F, S, N, 8] float32, cnt[F, S] int32, dt[F, S] float64); read-only."""
    from mmwave_msc_amd.synth import make_scene
    pts = np.zeros((n_frames, n_scenes, n_pts, 8), np.float32)
    cnt = np.zeros((n_frames, n_scenes), np.int32)
    dts = np.zeros((n_frames, n_scenes))
    for s in range(n_scenes):
        pts[:, s], cnt[:, s], dts[:, s] = make_scene(seed + s, n_frames, n_pts, 3, ragged=(s % 4 == 0), presence=presence_of(s, n_frames))
    for a in (pts, cnt, dts):
        a.setflags(write=False)
    return pts, cnt, dts
