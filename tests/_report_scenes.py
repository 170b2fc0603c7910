"""The scenario of the live-track report tests (tests/test_gpu_report.py) and of every uid-keyed export's: S scenes of three walking targets that arrive late
and leave again, with track lifetimes short enough (0.25 s = three frames without a point) that the tracks of targets that
left expire inside the run -- every scene's track count rises and falls, and in some frames a scene gains one track and loses
another.  Generated once per session and shared, never modified.  Behind it: the zone and wire tables several suites lay over
these scenes, and the host-side restatement of the report's events."""
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


def coming_and_going(n_scenes, n_pts, n_frames, seed=7000):
    """(pts, cnt, dt) of scenes of one target that arrives at frame 0, 1 or 2 and, in one scene of five, leaves again."""
    from mmwave_msc_amd.synth import make_scene
    pts, cnt, dts = np.zeros((n_frames, n_scenes, n_pts, 8), np.float32), np.zeros((n_frames, n_scenes), np.int32), np.zeros((n_frames, n_scenes))
    for s in range(n_scenes):
        presence = np.ones((n_frames, 1), bool)
        presence[: s % 3] = False
        presence[2 + s % 3:] = s % 5 != 0
        pts[:, s], cnt[:, s], dts[:, s] = make_scene(seed + s, n_frames, n_pts, 1, presence=presence)
    return pts, cnt, dts


def strips(n_scenes, margin=0.05):
    """16 zones per scene, strips x in [-3 + 0.375 k, -3 + 0.375 (k + 1)), any y, with ids that differ per scene."""
    from mmwave_msc_amd import _lib
    return _lib.make_zones([[(-3.0 + 0.375 * k, -3.0 + 0.375 * (k + 1), -np.inf, np.inf, margin, 1000 * s + k) for k in range(16)]
                            for s in range(n_scenes)])


def wires16(n_scenes, margin=0.03, y0=8.0, y1=0.0, x0=-2.0, pitch=0.25):
    """16 tripwires per scene from (c, y0) to (c, y1), c = x0 + pitch k; id = 100 + k."""
    from mmwave_msc_amd import _lib
    return _lib.make_tripwires([[(x0 + pitch * k, y0, x0 + pitch * k, y1, margin, 100 + k) for k in range(16)] for _ in range(n_scenes)])


def uid_lists(sb):
    """effective_tracks' uids per scene, in list order."""
    ntr, trk = sb.num_tracks(), sb.tracks()
    return [[int(u) for u in trk["uid"][s, : ntr[s]]] for s in range(sb.S)]


def host_events(prev, cur, rebased=(), scene_base=0):
    """What a report must say: per scene GONE in baseline order, then BORN in current order; one REBASED for a rebased scene."""
    from mmwave_msc_amd import _lib
    ev = []
    for s, (p, c) in enumerate(zip(prev, cur)):
        if s in rebased:
            ev.append((scene_base + s, -1, _lib.EV_REBASED, len(c)))
            continue
        ev += [(scene_base + s, u, _lib.EV_GONE, j) for j, u in enumerate(p) if u not in c]
        ev += [(scene_base + s, u, _lib.EV_BORN, j) for j, u in enumerate(c) if u not in p]
    return ev


def as_tuples(events):
    """A report's events as host_events lists them."""
    return [(int(e["scene"]), int(e["uid"]), int(e["kind"]), int(e["slot"])) for e in events]
