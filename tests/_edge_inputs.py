"""Decision-edge scenes: inputs ON the comparisons TrackBuffer.track takes its decisions by, built on the CPU alone (numpy and
the C oracle; no GPU, no torch).  The one builder of tests/test_edge_inputs.py (which proves the inputs sharp, on the oracle)
and tests/test_gpu_decision_edges.py (which holds the kernels to the oracle on them).

The fuzz scenes see only what track() decided, and a random point sits about 1e14 ulps from `d < tr_gate` and from the nearest
`d_j < d_k`: a gate distance d = log|det C| + y'C^-1 y that is wrong in its last bits decides every such point as before.  Here:

  gate_probes     pairs of rows (t_lo, t_hi) on a ray centre_j + t * dir, t_lo and t_hi ADJACENT doubles, the first taken by
                  track j and the second not: found by bisection on the oracle.  Run under the five adjacent gates
                  G - 2 ulp .. G + 2 ulp, a good part of these rows changes its decision (the counts: test_edge_inputs.py), so
                  they pin d to a few ulps
  tie_probes      the same along rays from track j towards track k under a gate wide enough that the two overlap: the row
                  passes from j to k between two adjacent doubles, which pins d_j - d_k
  exact_tie       two clusters that are exact translations of each other (coordinates multiples of 2^-8) and, one frame
                  later, a row at the exact midpoint of the predicted positions: C is bit-equal, the form is even in y, so
                  d_A == d_B, and the FIRST track takes the row, in either order of the clusters
  equality_scenes `lifetime > lim`, `speed < tr_vel_thres`, the spread clamps and `spread > old`, `nj > N_est`,
                  `T < tr_max_tracks`, `total > model_min_input`, 64 | 65 and ring_rows | ring_rows + 1 rows in a frame, each
                  with constants that make the equality exact in binary -- and asserted to be, here, on the oracle; and
                  `feature_ties`: equal x among a track's rows, and x equal to the centroid's, in the feature maps' sort
  dt_edges        frame intervals that are NOT exact in binary or lie far outside 0.05 .. 0.2 s: 0.1 + 0.2 > 0.3 == 0.15 + 0.15
                  against a lifetime limit of 0.3, lifetime + dt == 0, five frames of dt = 0, a 60 s predict with rows an ulp
                  inside and outside its gate (tests/test_gpu_dt.py)

Everything is seeded, fp64, built once, cached and read-only.  Rows of the input buffer at and beyond a frame's count are
copies of rows that lie well inside a gate: a kernel that gates a row past n changes point_num and the centroid."""
import functools
from typing import NamedTuple

import numpy as np

from oracle import c_oracle as co

GATE = 4.5                                           # TR_GATE of the gate probes
TIE_GATE = 16.0                                      # ... of the tie probes: the gates of neighbouring targets overlap
TIE_PITCH = 1.3                                      # ... whose targets stand this far apart (the gate probes': 1.6 m)
CTX_KW = {"fb_frames_batch": 0, "db_min_samples": 4, "tr_max_tracks": 16, "track_cap": 32}
HIST, DT = 3, 0.1                                    # frames before the probe frame
SEAMS = (255, 256, 511, 512, 767, 768)              # both sides of every q * 256 + tid seam of k_track / k_scene


class Scene(NamedTuple):
    tag: str
    cfg: dict             # keyword arguments of default_config (oracle.c_oracle and mmwave_msc_amd._lib alike)
    max_pts: int
    pts: np.ndarray       # [F, max_pts, 8]: every row filled, also those at and past cnt[f]
    cnt: np.ndarray       # [F] int32 (0: the frame never reaches track())
    dt: np.ndarray        # [F]


class Frame(NamedTuple):
    """What the oracle holds after one track() call."""
    assoc: np.ndarray
    labels: np.ndarray    # or None: apply_DBscan was not called
    n_tracks: int
    tracks: np.ndarray    # c_oracle.TRACK_DTYPE
    batch_ring: np.ndarray
    feat: np.ndarray
    owner: np.ndarray
    rings: list           # [track][k] -> rows the track's ring frame k stores


class Probes(NamedTuple):
    scene: Scene
    frame: int            # the probe frame
    pos: np.ndarray       # [R, 2] row of each pair's t_lo and t_hi row in the probe frame
    track: np.ndarray     # [R] the track the ray starts from
    other: np.ndarray     # [R] what takes the t_hi row under the scene's own gate (-1: nothing)
    t: np.ndarray         # [R, 2] t_lo, t_hi
    gates: tuple          # five adjacent doubles around the scene's tr_gate
    assoc: np.ndarray     # [5, n] the oracle's association of the probe frame under each gate
    flips: dict           # {1: k1, 2: k2}: probe rows whose decision differs between G - k ulp and G + k ulp


class Tie(NamedTuple):
    scene: Scene
    frame: int
    mid: np.ndarray       # rows at the exact midpoint
    to_a: np.ndarray      # rows 2^-10 towards cluster A
    to_b: np.ndarray
    a: int                # track index of cluster A (0 in order AB, 1 in order BA)


class Equality(NamedTuple):
    scene: Scene
    check: object         # check(frames): asserts, on an oracle replay, that the equality is met and what follows it
    feature_frames: tuple = ()
    ring_frames: tuple = ()


def cfg_key(kw):
    return tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in kw.items()))


def adjacent_gates(g, k=2):
    out = [float(g)]
    for _ in range(k):
        out = [float(np.nextafter(out[0], -np.inf))] + out + [float(np.nextafter(out[-1], np.inf))]
    return tuple(out)


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)


# ------------------------------------------------------------------------------------------------------------- the oracle
def replay(scene, upto=None, **cfg_over):
    """The oracle on the scene's frames [0, upto): a Frame per frame (None where cnt == 0)."""
    orc = co.OracleScene(co.default_config(**{**scene.cfg, **cfg_over}), scene.max_pts)
    out = []
    for f in range(len(scene.cnt) if upto is None else upto):
        c = int(scene.cnt[f])
        if c == 0:
            out.append(None)
            continue
        a, lab = orc.track(scene.pts[f, : max(c, 0)], float(scene.dt[f]))      # (c == -1: track() on an empty cloud)
        trk = orc.tracks()
        feat, owner = orc.features()
        rings = [[orc.track_ring_frame(t, k) for k in range(trk[t]["ring_len"])] for t in range(len(trk))]
        out.append(Frame(a, lab, orc.n_tracks, trk, orc.batch_ring(), feat, owner, rings))
    return out


class _Prober:
    """Association of arbitrary rows in the frame after a history: one oracle replay per call (a row's association does not
    depend on the other rows of its frame)."""

    def __init__(self, cfg_kw, hist, cnt, cap):
        self.cfg = co.default_config(**cfg_kw)
        self.hist, self.cnt, self.cap = hist, cnt, int(max(cap, max(cnt)))

    def scene(self):
        orc = co.OracleScene(self.cfg, self.cap)
        for f in range(len(self.cnt)):
            orc.track(self.hist[f][: self.cnt[f]], DT)
        return orc

    def __call__(self, rows6):
        rows = np.zeros((len(rows6), 8))
        rows[:, :6] = rows6
        return self.scene().track(rows, DT)[0]


def _bisect(prober, centre, dirs, inside, t_out):
    """t_lo, t_hi per ray, adjacent doubles: inside(association of centre + t_lo * dir), not inside(... t_hi ...)."""
    lo, hi = np.zeros(len(dirs)), np.full(len(dirs), float(t_out))
    assert np.all(inside(prober(centre))) and not np.any(inside(prober(centre + hi[:, None] * dirs)))
    for _ in range(80):
        if np.array_equal(np.nextafter(lo, np.inf), hi):
            break
        mid = lo + (hi - lo) / 2
        mid = np.where((mid <= lo) | (mid >= hi), lo, mid)
        ins = inside(prober(centre + mid[:, None] * dirs))
        lo, hi = np.where(ins, mid, lo), np.where(ins | (mid == lo), hi, mid)
    assert np.array_equal(np.nextafter(lo, np.inf), hi)
    return lo, hi


# --------------------------------------------------------------------------------------------------------------- histories
def _f32_exact(a):
    return a.astype(np.float32).astype(np.float64)


def _targets(rng, K, pitch):
    """K targets on a grid of `pitch` metres, four to a column, slow."""
    cols = (K + 3) // 4
    c = np.array([[-0.5 * pitch * (cols - 1) + pitch * (k // 4), 1.5 + pitch * (k % 4)] for k in range(K)])
    return c, rng.normal(0.0, 0.15, size=(K, 2))


def _target_rows(rng, centre, vel, n):
    p = np.zeros((n, 8))
    p[:, 0:2] = centre + rng.normal(0.0, 0.06, size=(n, 2))
    p[:, 2] = rng.uniform(0.6, 1.2, size=n)
    p[:, 3:5] = vel + rng.normal(0.0, 0.03, size=(n, 2))
    p[:, 5] = rng.normal(0.0, 0.03, size=n)
    p[:, 6] = rng.normal(0.0, 0.3, size=n)
    p[:, 7] = rng.gamma(1.0, 30.0, size=n)
    return p


def _clutter(rng, n):
    p = np.zeros((n, 8))
    p[:, 0] = rng.uniform(6.0, 9.0, size=n) * rng.choice([-1.0, 1.0], size=n)
    p[:, 1] = rng.uniform(0.3, 7.5, size=n)
    p[:, 2] = rng.uniform(0.05, 2.4, size=n)
    p[:, 3:6] = rng.normal(0.0, 0.05, size=(n, 3))
    p[:, 6] = rng.normal(0.0, 0.3, size=n)
    p[:, 7] = rng.gamma(1.0, 30.0, size=n)
    return p


def _ordinary_frame(rng, c, vel, f, per, n_clutter):
    """A frame of the targets' own rows (well inside their gates) and some clutter, float32-exact, shuffled; and the targets'
    rows alone (the filler of the buffer past the count)."""
    own = np.concatenate([_target_rows(rng, c[k] + vel[k] * DT * f, vel[k], per) for k in range(len(c))])
    rows = np.concatenate([own, _clutter(rng, n_clutter)])
    return _f32_exact(rows[rng.permutation(len(rows))]), _f32_exact(own)


def _fill(max_pts, rows, filler):
    out = np.empty((max_pts, 8))
    out[: len(rows)] = rows
    m = max_pts - len(rows)
    out[len(rows):] = filler[np.arange(m) % len(filler)]
    return out


def _history(cfg_kw, K, seed, pitch=1.6):
    rng = np.random.default_rng(seed)
    c, vel = _targets(rng, K, pitch)
    per = 16 if K <= 4 else 8
    frames = [_ordinary_frame(rng, c, vel, f, per, 4) for f in range(HIST)]
    hist, fill = [fr[0] for fr in frames], [fr[1] for fr in frames]
    cnt = [len(h) for h in hist]
    prober = _Prober(cfg_kw, hist, cnt, 1)
    trk = prober.scene().tracks()
    assert len(trk) == K and np.all(trk["lifetime"] == 0.0), (seed, K, len(trk))      # every target a live track
    centre = trk["x"][:, :6].copy()
    centre[:, :3] += DT * trk["x"][:, 3:6]                                             # (about where _predict_all puts the track)
    return rng, c, vel, per, hist, fill, cnt, centre


def _probe_positions(rng, n, m):
    """m rows of a frame of n for the probes: rows 0 and n - 1, both sides of every seam, the rest spread over the frame."""
    must = sorted({p for p in (0, n - 1) + SEAMS if p < n})
    rest = np.setdiff1d(np.arange(n), must)
    pos = np.concatenate([must, rng.choice(rest, m - len(must), replace=False)]).astype(int)
    return pos[rng.permutation(m)]


def _probe_scene(tag, cfg_kw, max_pts, rng, c, vel, per, hist, fill, probe_rows6):
    """History, the probe frame (probes at _probe_positions, ordinary rows between them) and one more ordinary frame."""
    K, m = len(c), len(probe_rows6)
    n = max_pts - 8
    ordinary, own = _ordinary_frame(rng, c, vel, HIST, max(1, -(-(n - m - 4) // K)), 4)
    ordinary = ordinary[: n - m]
    assert len(ordinary) == n - m and m >= 16
    pos = _probe_positions(rng, n, m)
    frame = np.zeros((n, 8))
    frame[np.setdiff1d(np.arange(n), pos)] = ordinary
    frame[pos, :6] = probe_rows6
    frame[pos, 6] = rng.normal(0.0, 0.3, size=m)
    frame[pos, 7] = rng.gamma(1.0, 30.0, size=m)
    after, own2 = _ordinary_frame(rng, c, vel, HIST + 1, per, 4)
    rows = hist + [frame, after]
    fills = fill + [own, own2]
    pts = np.stack([_fill(max_pts, r, fl) for r, fl in zip(rows, fills)])
    cnt = np.array([len(r) for r in rows], np.int32)
    _ro(pts, cnt)
    return Scene(tag, dict(cfg_kw), max_pts, pts, cnt, np.full(len(rows), DT)), pos


def _n_rays(max_pts, K):
    n = max_pts - 8
    return (n - max(n // 8, 2 * K + 4)) // 2


def _finish(tag, cfg_kw, max_pts, gates, built, rays, lo, hi, centre, dirs, j):
    rng, c, vel, per, hist, fill, cnt, _ = built
    rows6 = np.empty((2 * rays, 6))
    rows6[0::2] = centre + lo[:, None] * dirs
    rows6[1::2] = centre + hi[:, None] * dirs
    scene, pos = _probe_scene(tag, cfg_kw, max_pts, rng, c, vel, per, hist, fill, rows6)
    assoc = np.stack([replay(scene, upto=HIST + 1, tr_gate=g)[HIST].assoc for g in gates])
    pos = pos.reshape(rays, 2)
    flips = {k: int(np.sum(assoc[2 - k, pos] != assoc[2 + k, pos])) for k in (1, 2)}
    t = np.stack([lo, hi], axis=1)
    _ro(pos, assoc, t)
    return Probes(scene, HIST, pos, j, assoc[2, pos[:, 1]].copy(), t, gates, assoc, flips)


@functools.lru_cache(maxsize=None)
def _gate_probes(key, max_pts, seed, gates, K):
    cfg_kw = dict(key)
    built = _history(cfg_kw, K, seed)
    rng, hist, cnt, centres = built[0], built[4], built[6], built[7]
    rays = _n_rays(max_pts, K)
    j = np.arange(rays) % K
    dirs = rng.normal(0.0, 1.0, size=(rays, 6))
    dirs[:, 3:] *= 0.3
    prober = _Prober(cfg_kw, hist, cnt, rays)
    lo, hi = _bisect(prober, centres[j], dirs, lambda a: a == j, 64.0)
    return _finish(f"gate probes K={K} seed {seed}", cfg_kw, max_pts, gates, built, rays, lo, hi, centres[j], dirs, j)


def gate_probes(cfg_kw, max_pts, seed, gates=None, K=3):
    """Probes of the gate surface `d < tr_gate` of the K tracks a three-frame history leaves behind (cfg_kw: fb_frames_batch = 0).
    `gates`: five adjacent doubles around cfg_kw's tr_gate (default: adjacent_gates of it)."""
    assert cfg_kw.get("fb_frames_batch") == 0
    g = float(cfg_kw.get("tr_gate", GATE))
    gates = adjacent_gates(g) if gates is None else tuple(gates)
    assert len(gates) == 5 and gates[2] == g and all(np.nextafter(a, np.inf) == b for a, b in zip(gates, gates[1:]))
    return _gate_probes(cfg_key({**cfg_kw, "tr_gate": g}), int(max_pts), int(seed), gates, int(K))


@functools.lru_cache(maxsize=None)
def _tie_probes(key, max_pts, seed, K):
    cfg_kw = dict(key)
    built = _history(cfg_kw, K, seed, pitch=TIE_PITCH)
    rng, hist, cnt, centres = built[0], built[4], built[6], built[7]
    want = _n_rays(max_pts, K)
    pairs = [(a, b) for a in range(K) for b in range(K) if a != b and np.linalg.norm(centres[a, :2] - centres[b, :2]) < 1.1 * TIE_PITCH]
    cand = 3 * want
    jk = np.array([pairs[i % len(pairs)] for i in range(cand)])
    j, k = jk[:, 0], jk[:, 1]
    jitter = rng.normal(0.0, 0.08, size=(cand, 6))
    jitter[:, 3:] *= 0.3
    dirs = centres[k] - centres[j] + jitter
    prober = _Prober(cfg_kw, hist, cnt, cand)
    ends = prober(centres[j] + dirs)
    ok = (prober(centres[j]) == j) & (ends == k)
    j, k, dirs = j[ok], k[ok], dirs[ok]
    lo, hi = _bisect(prober, centres[j], dirs, lambda a: a == j, 1.0)
    edge = np.flatnonzero(prober(centres[j] + hi[:, None] * dirs) == k)[:want]       # the row passes from one track to another
    assert len(edge) >= want // 4, (len(edge), want)
    j, k, dirs, lo, hi = j[edge], k[edge], dirs[edge], lo[edge], hi[edge]
    g = float(cfg_kw["tr_gate"])
    return _finish(f"tie probes K={K} seed {seed}", cfg_kw, max_pts, adjacent_gates(g), built, len(edge), lo, hi, centres[j], dirs, j)


def tie_probes(cfg_kw, max_pts, seed, K=3):
    """Probes of `d_j < d_k`: rays from track j towards a neighbouring track k under cfg_kw's (wide) tr_gate; only the edges where
    the row passes from j to k are kept (Probes.other == k)."""
    assert cfg_kw.get("fb_frames_batch") == 0 and cfg_kw.get("tr_gate", GATE) >= 9
    return _tie_probes(cfg_key(cfg_kw), int(max_pts), int(seed), int(K))


# --------------------------------------------------------------------------------------------------------------- exact rows
def _exact_cluster(rng, centre, n, vel, half=16):
    """n rows within half / 256 of `centre` (a multiple of 2^-8 per coordinate): x on distinct multiples of 2^-10 (no ties in
    format_single_frame's sort), y and z on multiples of 2^-8, every row with the velocity `vel`; doppler and intensity dyadic."""
    assert n <= 8 * half
    p = np.zeros((n, 8))
    p[:, 0] = centre[0] + rng.permutation(np.arange(-4 * half, 4 * half))[:n] / 1024.0
    p[:, 1] = centre[1] + rng.integers(-half, half + 1, size=n) / 256.0
    p[:, 2] = centre[2] + rng.integers(-half, half + 1, size=n) / 256.0
    p[:, 3:6] = vel
    p[:, 6] = rng.integers(-8, 9, size=n) / 8.0
    p[:, 7] = rng.integers(0, 200, size=n) / 2.0
    return p


def _scene(tag, cfg_kw, max_pts, frames, dt, filler):
    pts = np.stack([_fill(max_pts, r, filler) for r in frames])
    cnt = np.array([len(r) for r in frames], np.int32)
    dts = np.full(len(frames), float(dt))
    _ro(pts, cnt, dts)
    return Scene(tag, dict(cfg_kw), max_pts, pts, cnt, dts)


EQ_DT = 0.125
EQ_KW = {"db_min_samples": 4, "track_cap": 16}
_LONE = np.array([[5.0, 7.0, 1.0, 0.0, 0.0, 0.0, 0.25, 12.0]])      # a row no track of these scenes ever gates


@functools.lru_cache(maxsize=None)
def _exact_tie(key, max_pts, order):
    cfg_kw = dict(key)
    rng = np.random.default_rng(97)
    vel = np.array([0.25, 0.5, 0.0])
    a = _exact_cluster(rng, (-0.75, 2.0, 1.0), 16, vel)
    b = a.copy()
    b[:, 0] += 1.5                                                   # an exact translation
    assert np.array_equal(b[:, 0] - 1.5, a[:, 0])
    first, second = (a, b) if order == "AB" else (b, a)
    f0 = np.concatenate([first, second])
    move = np.zeros(8)
    move[:3] = EQ_DT * vel                                           # (exact: 2^-5, 2^-4, 0)
    ca = a[:, :6].mean(axis=0)
    assert np.array_equal(ca * 16, a[:, :6].sum(axis=0))             # the centroid is exact
    mid = np.zeros(8)
    mid[:6] = ca
    mid[:3] += move[:3]
    mid[0] += 0.75                                                   # the midpoint of the two predicted positions
    n = max_pts - 8
    own = np.concatenate([a + move, b + move])
    f1 = own[np.arange(n) % len(own)].copy()
    at = sorted({p for p in (1, 9, n // 2, n - 2) + tuple(s for s in SEAMS if s % 256 == 0) if 0 < p < n - 1})
    at = [p for i, p in enumerate(at) if i == 0 or p - at[i - 1] > 2]
    for p in at:
        f1[p - 1], f1[p], f1[p + 1] = mid, mid, mid
        f1[p - 1, 0] -= 2.0 ** -10
        f1[p + 1, 0] += 2.0 ** -10
    f2 = np.concatenate([first, second]) + 2 * move
    at = np.array(at)
    scene = _scene(f"exact tie {order}", cfg_kw, max_pts, [f0, f1, f2], EQ_DT, own)
    return Tie(scene, 1, at, at - 1, at + 1, 0 if order == "AB" else 1)


def exact_tie(cfg_kw, max_pts, order):
    """Two clusters of 16 rows, B = A + (1.5, 0, 0) exactly, the same velocity; one frame later the row at the exact midpoint of the
    predicted positions -- at several rows of the frame, row 1 and the first row of every 256-row group among them -- between a
    row 2^-10 nearer to A and one 2^-10 nearer to B; every other row of that frame is a cluster row moved on.  order "AB" | "BA":
    which cluster comes first in frame 0, i.e. which one is track 0."""
    assert order in ("AB", "BA") and cfg_kw.get("fb_frames_batch") == 0
    return _exact_tie(cfg_key(cfg_kw), int(max_pts), order)


def check_exact_tie(tie, frames):
    fr = frames[tie.frame]
    assert frames[0].n_tracks == 2
    t = frames[0].tracks
    assert np.array_equal(t["P"][0], t["P"][1]) and np.array_equal(t["centroid"][0][1:], t["centroid"][1][1:])
    assert np.all(fr.assoc[tie.mid] == 0), (tie.scene.tag, fr.assoc[tie.mid])          # first best on a tie
    assert np.all(fr.assoc[tie.to_a] == tie.a) and np.all(fr.assoc[tie.to_b] == 1 - tie.a), tie.scene.tag


# ---------------------------------------------------------------------------------------------------------- equality scenes
def _lifetimes():
    """`lifetime > lim` (Tracking.py:513-528): dt = 2^-3; a dynamic and a static track lose their points after frame 0; the dynamic
    one is kept at lifetime == 0.5 (frame 4) and dropped at 0.625, the static one kept at 0.75 (frame 6) and dropped at 0.875."""
    kw = dict(EQ_KW, tr_lifetime_dynamic=0.5, tr_lifetime_static=0.75, tr_vel_thres=0.3125)
    rng = np.random.default_rng(11)
    dyn = _exact_cluster(rng, (-2.0, 2.0, 1.0), 16, (0.5, 0.25, 0.0))
    sta = _exact_cluster(rng, (1.0, 3.0, 1.0), 16, (0.0, 0.0, 0.0))
    scene = _scene("lifetimes", kw, 128, [np.concatenate([dyn, sta])] + [_LONE] * 7, EQ_DT, sta)

    def check(fr):
        assert fr[0].n_tracks == 2 and list(fr[0].tracks["is_static"]) == [0, 1]
        assert all(np.all(fr[f].assoc == -1) for f in range(1, 8))
        assert fr[4].n_tracks == 2 and list(fr[4].tracks["lifetime"]) == [0.5, 0.5]       # == lim: kept
        assert fr[5].n_tracks == 1 and fr[5].tracks["is_static"][0] == 1 and fr[5].tracks["lifetime"][0] == 0.625
        assert fr[6].n_tracks == 1 and fr[6].tracks["lifetime"][0] == 0.75               # == lim: kept
        assert fr[7].n_tracks == 0
    return Equality(scene, check)


def _speed():
    """`speed < tr_vel_thres` (Tracking.py:134): every row of one cluster moves at (0.1875, 0.25, 0), speed exactly 0.3125 ==
    tr_vel_thres: dynamic; the other cluster's vx is lower by 2^-20: static.  Both lose their points: they expire on different
    frames."""
    kw = dict(EQ_KW, tr_lifetime_dynamic=0.5, tr_lifetime_static=0.75, tr_vel_thres=0.3125)
    rng = np.random.default_rng(12)
    at = _exact_cluster(rng, (-2.0, 2.0, 1.0), 16, (0.1875, 0.25, 0.0))
    below = _exact_cluster(rng, (1.0, 3.0, 1.0), 16, (0.1875 - 2.0 ** -20, 0.25, 0.0))
    scene = _scene("speed", kw, 128, [np.concatenate([at, below])] + [_LONE] * 7, EQ_DT, below)

    def check(fr):
        v = fr[0].tracks["centroid"][:, 3:6]
        speed = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        assert speed[0] == 0.3125 and speed[1] < 0.3125 and list(fr[0].tracks["is_static"]) == [0, 1]
        assert fr[4].n_tracks == 2 and fr[5].n_tracks == 1 and fr[5].tracks["is_static"][0] == 1
        assert fr[6].n_tracks == 1 and fr[7].n_tracks == 0
    return Equality(scene, check)


SPREAD_LIM = (0.25, 0.25, 2.0, 1.0, 1.0, 0.25)


def _spread():
    """_estimate_measurement_spread (Tracking.py:246-268) with kf_spread_lim = SPREAD_LIM, kf_a_spr = 0.5.  Four static tracks; in
    frame 1 track 0 takes 3 rows (scaling (n + 1) / (n - 1) = 2) of extent 0.125 in x -- spread == lim -- and 0.25 in y -- spread ==
    2 lim --, track 1 the same with x and y swapped, track 2 one row, track 3 two rows (scaling 3) of extent 0.125: 0.375, between
    the clamps.  Frame 2 repeats the extents: spread == old.  Frame 3: smaller extents, the smoothing arm."""
    kw = dict(EQ_KW, kf_spread_lim=list(SPREAD_LIM), kf_a_spr=0.5, tr_max_tracks=4)
    rng = np.random.default_rng(13)
    centres = [(-3.0, 2.0, 1.0), (-1.0, 2.0, 1.0), (1.0, 2.0, 1.0), (3.0, 2.0, 1.0)]
    f0 = np.concatenate([_exact_cluster(rng, c, 16, (0.0, 0.0, 0.0)) for c in centres])

    def rows(c, offs):
        r = np.zeros((len(offs), 8))
        r[:, :3] = np.asarray(c) + np.array([(dx, dy, 0.0) for dx, dy in offs])
        r[:, 6], r[:, 7] = 0.25, 20.0
        return r

    def frame(e0, e3):
        return np.concatenate([rows(centres[0], [(-e0 / 2, -e0, ), (0.0, 0.0), (e0 / 2, e0)]),
                               rows(centres[1], [(-e0, -e0 / 2), (0.0, 0.0), (e0, e0 / 2)]),
                               rows(centres[2], [(0.0, 0.0)]), rows(centres[3], [(-e3 / 2, 0.0), (e3 / 2, 0.0)])])
    scene = _scene("spread", kw, 128, [f0, frame(0.125, 0.125), frame(0.125, 0.125), frame(0.0625, 0.0625)], EQ_DT, f0)

    def check(fr):
        assert fr[0].n_tracks == 4
        for f in (1, 2):
            t = fr[f].tracks
            assert list(t["point_num"]) == [3, 3, 1, 2] and fr[f].labels is None, f
            ext = t["max_vals"] - t["min_vals"]
            assert ext[0, 0] == 0.125 and ext[0, 1] == 0.25 and ext[1, 0] == 0.25 and ext[1, 1] == 0.125 and ext[3, 0] == 0.125
            assert ext[0, 0] * 4 / 2 == SPREAD_LIM[0] and ext[0, 1] * 4 / 2 == 2 * SPREAD_LIM[1]     # spread == lim, == 2 lim
            assert list(t["spread_est"][0]) == [0.25, 0.5, 2.0, 1.0, 1.0, 0.25]
            assert list(t["spread_est"][1]) == [0.5, 0.25, 2.0, 1.0, 1.0, 0.25]
            assert list(t["spread_est"][2]) == list(SPREAD_LIM) and t["spread_est"][3, 0] == 0.375
        assert np.array_equal(fr[1].tracks["spread_est"], fr[2].tracks["spread_est"])             # spread == old
        assert fr[3].tracks["spread_est"][0, 1] == 0.375 and fr[3].tracks["spread_est"][3, 0] == 0.3125   # the smoothing arm
    return Equality(scene, check)


def _n_est_constants():
    """(kf_a_n, N): the first pair for which (1 - a) * N + a * N differs from N in its bits -- otherwise both arms of
    `nj > N_est` store the same value and the equality tests nothing."""
    for a in (0.9, 0.7, 0.6, 0.3, 0.8, 0.1):
        for n in range(2, 13):
            if (1 - a) * float(n) + a * float(n) != float(n):
                return a, n
    raise AssertionError("no (kf_a_n, N) found")


def _n_est():
    """_estimate_point_num (Tracking.py:232-244) with kf_enable_est = 1: the track takes N rows in frame 1 (N_est = N), N again in
    frame 2 -- nj == N_est, the smoothing arm: (1 - a) N + a N, which differs from N in its bits -- and N again in frame 3."""
    a, n = _n_est_constants()
    kw = dict(EQ_KW, kf_enable_est=1, kf_a_n=a)
    rng = np.random.default_rng(14)
    c = (0.0, 2.0, 1.0)
    f0 = _exact_cluster(rng, c, 16, (0.0, 0.0, 0.0))
    scene = _scene("n_est", kw, 128, [f0] + [_exact_cluster(rng, c, n, (0.0, 0.0, 0.0)) for _ in range(3)], EQ_DT, f0)
    smoothed = (1 - a) * float(n) + a * float(n)
    assert smoothed != float(n)

    def check(fr):
        assert [int(fr[f].tracks["point_num"][0]) for f in (1, 2, 3)] == [n, n, n]
        assert fr[1].tracks["n_est"][0] == float(n)
        assert fr[2].tracks["n_est"][0] == smoothed != float(n)          # nj == N_est took the smoothing arm
        assert fr[3].tracks["n_est"][0] == (float(n) if n > smoothed else (1 - a) * smoothed + a * float(n))
    return Equality(scene, check)


_TRIGGER_KW = dict(EQ_KW, tr_max_tracks=3, fb_frames_batch=1, tr_lifetime_dynamic=0.125)


def _trigger():
    """`T < tr_max_tracks` (Tracking.py:693) with tr_max_tracks = 3, a ring of two frames, tr_lifetime_dynamic = dt.  Frame 0: three
    clusters, three tracks.  Frame 1: the dynamic track gets nothing (lifetime == lim: kept), two new clusters are unassigned, T ==
    tr_max_tracks: no call, the ring grows.  Frame 2: the dynamic track expires, T == tr_max_tracks - 1: the ring is clustered, two
    clusters, T = 4 > tr_max_tracks.  Frame 3: every row is taken while the ring is empty."""
    rng = np.random.default_rng(15)
    z = (0.0, 0.0, 0.0)
    old = [_exact_cluster(rng, (-3.0, 2.0, 1.0), 16, z), _exact_cluster(rng, (-1.0, 2.0, 1.0), 16, z)]
    dyn = _exact_cluster(rng, (1.0, 2.0, 1.0), 16, (0.5, 0.0, 0.0))
    new = [_exact_cluster(rng, (-3.0, 5.0, 1.0), 16, z), _exact_cluster(rng, (0.0, 5.0, 1.0), 16, z)]
    f0 = np.concatenate(old + [dyn])
    f12 = np.concatenate(old + new)
    scene = _scene("dbscan trigger", _TRIGGER_KW, 128, [f0, f12, f12[::-1].copy(), f12], EQ_DT, old[0])

    def check(fr):
        assert fr[0].n_tracks == 3 and len(fr[0].labels) == 48
        assert fr[1].n_tracks == 3 and fr[1].tracks["lifetime"][2] == 0.125 and fr[1].labels is None      # T == max: no call
        assert list(fr[1].batch_ring) == [32] and int(np.sum(fr[1].assoc == -1)) == 32
        assert fr[2].labels is not None and len(fr[2].labels) == 64 and fr[2].labels.max() == 1           # T == max - 1: clusters
        assert fr[2].n_tracks == 4 and len(fr[2].batch_ring) == 0                                         # ... past tr_max_tracks
        assert np.all(fr[3].assoc >= 0) and fr[3].labels is None and list(fr[3].batch_ring) == [0] and fr[3].n_tracks == 4
    return Equality(scene, check)


def _all_taken():
    """`U > 0` with T < tr_max_tracks: frame 1's rows are all taken while the ring is empty -- no call; frame 2 adds one row that
    nothing takes -- a call on one row."""
    rng = np.random.default_rng(16)
    z = (0.0, 0.0, 0.0)
    cl = [_exact_cluster(rng, (-3.0, 2.0, 1.0), 16, z), _exact_cluster(rng, (-1.0, 2.0, 1.0), 16, z)]
    f0 = np.concatenate(cl)
    scene = _scene("all taken", _TRIGGER_KW, 128, [f0, f0[::-1].copy(), np.concatenate([f0, _LONE])], EQ_DT, cl[0])

    def check(fr):
        assert fr[0].n_tracks == 2 and len(fr[0].batch_ring) == 0
        assert np.all(fr[1].assoc >= 0) and fr[1].labels is None and list(fr[1].batch_ring) == [0] and fr[1].n_tracks == 2
        assert fr[2].labels is not None and list(fr[2].labels) == [-1] and list(fr[2].batch_ring) == [0, 1]
    return Equality(scene, check)


_FEATURE_KW = dict(EQ_KW, fb_frames_batch=1, model_min_input=40, ring_rows=96)


def _min_input():
    """`total > model_min_input` (Tracking.py:720) with model_min_input = 40 and a ring of two frames: 20 + 20 rows == 40, not
    eligible; 20 + 21: eligible."""
    rng = np.random.default_rng(17)
    c, z = (0.0, 2.0, 1.0), (0.0, 0.0, 0.0)
    frames = [_exact_cluster(rng, c, m, z) for m in (20, 20, 21)]
    scene = _scene("model_min_input", _FEATURE_KW, 128, frames, EQ_DT, frames[0])

    def check(fr):
        assert list(fr[1].tracks["ring_n"][0][:2]) == [20, 20] and len(fr[1].owner) == 0       # == model_min_input
        assert list(fr[2].tracks["ring_n"][0][:2]) == [20, 21] and list(fr[2].owner) == [0]
    return Equality(scene, check, feature_frames=(0, 1, 2))


def _ring_rows():
    """One track takes exactly 64 rows (what format_single_frame reads), 65, ring_rows = 96 (what a ring frame stores) and 97."""
    rng = np.random.default_rng(18)
    c, z = (0.0, 2.0, 1.0), (0.0, 0.0, 0.0)
    frames = [_exact_cluster(rng, c, m, z) for m in (20, 64, 65, 96, 97)]
    scene = _scene("ring_rows", _FEATURE_KW, 128, frames, EQ_DT, frames[0])

    def check(fr):
        for f, m in ((1, 64), (2, 65), (3, 96), (4, 97)):
            assert fr[f].n_tracks == 1 and fr[f].tracks["point_num"][0] == m and fr[f].tracks["ring_n"][0][1] == m
            assert np.array_equal(fr[f].rings[0][1], scene.pts[f, : min(m, 96)]) and list(fr[f].owner) == [0]
    return Equality(scene, check, feature_frames=(1, 2, 3, 4), ring_frames=(1, 2, 3, 4))


def _tied_cluster(rng, centre, n, vel):
    """_exact_cluster with TIES in x, as a radar's quantised x gives them: x drawn with repetition from the seven multiples of 2^-6
    within 3 / 64 of the centre, every draw with its mirror image (and the centre itself once more where n is odd), so the sum of
    x is n * centre exactly, the centroid's x is the centre, and the rows on the centre have relative x == 0 -- the pad rows' key.
    y, z, doppler and intensity dyadic and DISTINCT per row: two rows of a tie group exchanged change the feature map."""
    assert 8 <= n <= 80
    o = rng.integers(-3, 4, size=n // 2)
    o[:2] = 0, 3                                                      # rows on the centre, always
    o = np.concatenate([o, -o, np.zeros(n % 2, dtype=o.dtype)])
    p = np.zeros((n, 8))
    p[:, 0] = centre[0] + o[rng.permutation(n)] / 64.0
    p[:, 1] = centre[1] + rng.permutation(np.arange(-40, 40))[:n] / 512.0
    p[:, 2] = centre[2] + rng.permutation(np.arange(-40, 40))[:n] / 512.0
    p[:, 3:6] = vel
    p[:, 6] = rng.permutation(np.arange(-40, 40))[:n] / 8.0
    p[:, 7] = rng.permutation(np.arange(1, 200))[:n] / 2.0
    assert np.sum(p[:, 0]) == n * centre[0]
    return p


def ties_by_larger_row(feat):
    """A feature tensor of the stable sort re-ordered as a sort that breaks ties by the LARGER row would leave it: every run of
    equal x reversed (the pad rows are the rows behind a frame's real ones)."""
    out = np.array(feat, np.float32).reshape(-1, 64, 5)
    for fr in out:
        x = fr[:, 0]
        start = 0
        for i in range(1, 65):
            if i == 64 or x[i] != x[start]:
                fr[start:i] = fr[start:i][::-1].copy()
                start = i
    return out.reshape(np.shape(feat))


def _feature_ties():
    """The feature maps' sort on tied keys from live tracks: one static track takes 20, 40, 64 and 65 rows of _tied_cluster about
    one centre.  In every feature map, every ring frame has real rows of equal relative x and real rows of relative x == 0, which
    tie with the pad rows; ordered by row position (the oracle's insertion sort) and not by the larger row."""
    rng = np.random.default_rng(19)
    c, z = (0.0, 2.0, 1.0), (0.0, 0.0, 0.0)
    sizes = (20, 40, 64, 65)
    frames = [_tied_cluster(rng, c, m, z) for m in sizes]
    scene = _scene("feature_ties", _FEATURE_KW, 128, frames, EQ_DT, frames[0])

    def check(fr):
        assert len(fr[0].owner) == 0                                  # 20 rows: not eligible yet
        for f in (1, 2, 3):
            assert fr[f].n_tracks == 1 and fr[f].tracks["point_num"][0] == sizes[f] and list(fr[f].owner) == [0]
            assert list(fr[f].tracks["ring_n"][0][:2]) == [sizes[f - 1], sizes[f]] and fr[f].tracks["centroid"][0][0] == c[0]
            feat = fr[f].feat.reshape(2, 64, 5)
            for k in range(2):
                real = feat[k][feat[k][:, 2] != 0]                    # (z is about 1 on a real row, 0 on a pad row)
                assert len(real) == min(64, sizes[f - 1 + k]) and len({r.tobytes() for r in real}) == len(real)
                vals, cnt = np.unique(real[:, 0], return_counts=True)
                assert cnt.max() >= 2 and len(vals) >= 3, (f, k, vals, cnt)        # a tie group of real rows
                assert np.any(real[:, 0] == 0), (f, k)                             # a real row that ties with the pad rows
            assert not np.array_equal(ties_by_larger_row(fr[f].feat), fr[f].feat), f
    return Equality(scene, check, feature_frames=(0, 1, 2, 3), ring_frames=(2, 3))


def _tie_equality(order):
    tie = exact_tie(dict(EQ_KW, fb_frames_batch=0), 128, order)
    return Equality(tie.scene, functools.partial(check_exact_tie, tie))


@functools.lru_cache(maxsize=None)
def equality_scenes():
    """name -> Equality.  Each builder's constants make its equality exact in binary; that it is met is asserted here, on the
    oracle, before anything else uses the scene."""
    out = {"lifetimes": _lifetimes(), "speed": _speed(), "spread": _spread(), "n_est": _n_est(), "dbscan_trigger": _trigger(),
           "all_taken": _all_taken(), "model_min_input": _min_input(), "ring_rows": _ring_rows(), "feature_ties": _feature_ties(),
           "exact_tie_AB": _tie_equality("AB"), "exact_tie_BA": _tie_equality("BA")}
    for eq in out.values():
        eq.check(replay(eq.scene))
    return out


def equality_groups():
    """The equality scenes grouped by configuration: one context each."""
    groups = {}
    for name, eq in equality_scenes().items():
        groups.setdefault(cfg_key(eq.scene.cfg), []).append(name)
    return list(groups.values())


# ------------------------------------------------------------------------------------------------- frame-interval edges
def _dt_scene(tag, cfg_kw, frames, dts, filler, max_pts=128):
    """_scene with an interval per frame; a frame given as None is track() on an empty cloud (cnt == -1, MMW_EMPTY_FRAME)."""
    assert len(dts) == len(frames)
    pts = np.stack([_fill(max_pts, np.zeros((0, 8)) if r is None else r, filler) for r in frames])
    cnt = np.array([-1 if r is None else len(r) for r in frames], np.int32)
    dts = np.array(dts, dtype=np.float64)
    _ro(pts, cnt, dts)
    return Scene(tag, dict(cfg_kw), max_pts, pts, cnt, dts)


def _two_clusters(seed):
    """A dynamic and a static cluster (tr_vel_thres = 0.3125), as _lifetimes: tracks 0 and 1 of the scene."""
    rng = np.random.default_rng(seed)
    dyn = _exact_cluster(rng, (-2.0, 2.0, 1.0), 16, (0.5, 0.25, 0.0))
    sta = _exact_cluster(rng, (1.0, 3.0, 1.0), 16, (0.0, 0.0, 0.0))
    return np.concatenate([dyn, sta]), sta


LIFETIME_SUM = 0.3     # 0.1 + 0.2 > 0.3 == 0.15 + 0.15 in binary64


def _lifetime_sums(dim_x, which):
    """`lifetime > lim` where the sums are NOT exact (Tracking.py:513-528), lim = 0.3 for the `which` ("dynamic" | "static") track
    and 0.75 for the other; both lose their points after frame 0.  Intervals 0.1, 0.2: 0.30000000000000004 > 0.3, dropped on the
    second frame.  Intervals 0.15, 0.15: == 0.3, kept; a frame of 2^-60 is absorbed (0.3 + 2^-60 == 0.3: half an ulp of 0.3 is
    2^-55), kept again; a frame of one ulp, 2^-54, drops it.  The predicts run with lifetime + dt = 0.1, 0.1 + 0.2, 0.15, 0.15 + 0.15."""
    e = 0 if which == "dynamic" else 1
    lims = {"tr_lifetime_dynamic": (LIFETIME_SUM, 0.75)[e], "tr_lifetime_static": (0.75, LIFETIME_SUM)[e]}
    kw = dict(EQ_KW, dim_x=int(dim_x), tr_vel_thres=0.3125, **lims)
    f0, sta = _two_clusters(21)
    over = _dt_scene(f"{which} lifetime 0.1 + 0.2", kw, [f0] + [_LONE] * 3, [EQ_DT, 0.1, 0.2, 0.1], sta)
    equal = _dt_scene(f"{which} lifetime 0.15 + 0.15", kw, [f0] + [_LONE] * 5, [EQ_DT, 0.15, 0.15, 2.0 ** -60, 2.0 ** -54, 0.1], sta)
    assert 0.1 + 0.2 > LIFETIME_SUM and 0.15 + 0.15 == LIFETIME_SUM
    assert LIFETIME_SUM + 2.0 ** -60 == LIFETIME_SUM and LIFETIME_SUM + 2.0 ** -54 == np.nextafter(LIFETIME_SUM, 1.0)

    def check_over(fr):
        assert fr[0].n_tracks == 2 and list(fr[0].tracks["is_static"]) == [0, 1]
        assert all(np.all(fr[f].assoc == -1) for f in range(1, 4))
        assert fr[1].n_tracks == 2 and list(fr[1].tracks["lifetime"]) == [0.1, 0.1]
        assert fr[2].n_tracks == 1 and fr[2].tracks["is_static"][0] == 1 - e and fr[2].tracks["lifetime"][0] == 0.1 + 0.2   # > 0.3: dropped
        assert fr[3].n_tracks == 1

    def check_equal(fr):
        assert fr[0].n_tracks == 2 and list(fr[0].tracks["is_static"]) == [0, 1]
        assert all(np.all(fr[f].assoc == -1) for f in range(1, 6))
        assert fr[2].n_tracks == 2 and list(fr[2].tracks["lifetime"]) == [LIFETIME_SUM] * 2                     # == 0.3: kept
        assert fr[3].n_tracks == 2 and list(fr[3].tracks["lifetime"]) == [LIFETIME_SUM] * 2                     # 2^-60: absorbed
        assert fr[4].n_tracks == 1 and fr[4].tracks["is_static"][0] == 1 - e and fr[4].tracks["lifetime"][0] > LIFETIME_SUM
        assert fr[5].n_tracks == 1
    return {f"{which}_sum_over": Equality(over, check_over), f"{which}_sum_equal": Equality(equal, check_equal)}


_STILL_KW = dict(EQ_KW, tr_lifetime_dynamic=0.5, tr_lifetime_static=0.75, tr_vel_thres=0.3125)


def _dtm_zero(dim_x):
    """lifetime + dt == 0: both tracks go unassigned for one frame of 0.125, then track() on an empty cloud with dt = -0.125: the
    predict runs with F = I and Q = Q(0) (kf_q_std on the last diagonal entry of every 3 x 3 block, nothing else), the lifetime is
    +0.0 again; a frame with the clusters' rows follows.  The twin with dt = +0.125 on the empty frame ends in another state."""
    kw = dict(_STILL_KW, dim_x=int(dim_x))
    f0, sta = _two_clusters(22)
    scene = _dt_scene("lifetime + dt == 0", kw, [f0, _LONE, None, f0], [EQ_DT, 0.125, -0.125, 0.125], sta)
    twin = _dt_scene("lifetime + dt == 0.25", kw, [f0, _LONE, None, f0], [EQ_DT, 0.125, 0.125, 0.125], sta)

    def check(fr):
        assert fr[1].n_tracks == 2 and list(fr[1].tracks["lifetime"]) == [0.125, 0.125] and 0.125 + -0.125 == 0.0
        assert fr[2].n_tracks == 2 and len(fr[2].assoc) == 0
        assert fr[2].tracks["lifetime"].tobytes() == np.zeros(2).tobytes()                     # +0.0, by its bits
        assert set(fr[3].assoc.tolist()) == {0, 1}                                             # both take their rows again
        other = replay(twin)
        assert list(other[2].tracks["lifetime"]) == [0.25, 0.25]
        for f in (2, 3):
            assert not np.array_equal(other[f].tracks["P"], fr[f].tracks["P"]) and not np.array_equal(other[f].tracks["x"], fr[f].tracks["x"])
    return {"dtm_zero": Equality(scene, check)}


def _stands_still(dim_x):
    """Five empty frames of dt = 0 leave the lifetime (0.125) and both tracks where they were; then a frame of the dynamic limit plus
    2^-50 drops the dynamic track.  The sharp form: a frame of lim - 0.125 brings the lifetime to == lim, kept, and a frame of 2^-50
    drops it."""
    kw = dict(_STILL_KW, dim_x=int(dim_x))
    lim = kw["tr_lifetime_dynamic"]
    f0, sta = _two_clusters(23)
    head, hdt = [f0, _LONE] + [None] * 5, [EQ_DT, 0.125] + [0.0] * 5
    plain = _dt_scene("lifetime stands still", kw, head + [_LONE, _LONE], hdt + [lim + 2.0 ** -50, 0.0], sta)
    sharp = _dt_scene("lifetime stands still, then == lim", kw, head + [_LONE, None, _LONE], hdt + [lim - 0.125, 2.0 ** -50, 0.0], sta)
    assert 0.125 + (lim - 0.125) == lim and lim + 2.0 ** -50 > lim

    def still(fr):
        for f in range(1, 7):
            assert fr[f].n_tracks == 2 and list(fr[f].tracks["lifetime"]) == [0.125, 0.125] and np.all(fr[f].assoc == -1), f
        assert not np.array_equal(fr[5].tracks["P"], fr[6].tracks["P"])                        # (the filter goes on: predict and update)

    def check_plain(fr):
        still(fr)
        assert fr[7].n_tracks == 1 and fr[7].tracks["is_static"][0] == 1 and fr[7].tracks["lifetime"][0] == 0.125 + (lim + 2.0 ** -50)
        assert fr[8].n_tracks == 1

    def check_sharp(fr):
        still(fr)
        assert fr[7].n_tracks == 2 and list(fr[7].tracks["lifetime"]) == [lim, lim]               # == lim: kept
        assert fr[8].n_tracks == 1 and fr[8].tracks["is_static"][0] == 1 and fr[8].tracks["lifetime"][0] == lim + 2.0 ** -50
        assert fr[9].n_tracks == 1
    return {"stands_still": Equality(plain, check_plain), "stands_still_sharp": Equality(sharp, check_sharp)}


LONG_DT = 60.0
LONG_RAYS = 12


def _long_predict(dim_x):
    """A predict over 60 s that is then gated.  Frame 0 makes one dynamic track; frame 1 comes 60 s later.  Its rows, per ray from the
    oracle's predicted position of the track (x + 60 v; P has grown by dtm^2 and Q(60) by dtm^4 / 4): the position itself and the
    point half-way to the gate surface -- taken --, the last double inside and the first outside (bisection on the oracle, as
    gate_probes), and the point one gate radius further out -- refused.  tr_gate is the first multiple of 8 under which the
    predicted position is inside at all, plus 8 (log|det C| alone is beyond the gates track() is used with).  A frame 0.125 s
    later repeats the taken rows."""
    f0 = _two_clusters(24)[0][:16]
    base = dict(EQ_KW, dim_x=int(dim_x), fb_frames_batch=0, tr_vel_thres=0.3125)

    def prober(gate):
        cfg = co.default_config(**dict(base, tr_gate=float(gate)))

        def probe(rows6):
            orc = co.OracleScene(cfg, max(len(rows6), len(f0)))
            orc.track(f0, EQ_DT)
            rows = np.zeros((len(rows6), 8))
            rows[:, :6] = rows6
            return orc.track(rows, LONG_DT)[0]
        return probe

    orc = co.OracleScene(co.default_config(**base), len(f0))
    orc.track(f0, EQ_DT)
    trk = orc.tracks()
    assert len(trk) == 1 and trk["is_static"][0] == 0
    centre = trk["x"][:1, :6].copy()
    centre[:, :3] += LONG_DT * trk["x"][:1, 3:6] + 0.5 * LONG_DT * LONG_DT * trk["x"][:1, 6:9]
    gate = next(g for g in range(8, 257, 8) if prober(g)(centre)[0] == 0) + 8
    kw = dict(base, tr_gate=float(gate))
    rng = np.random.default_rng(25)
    dirs = rng.normal(0.0, 1.0, size=(LONG_RAYS, 6))
    dirs[:, 3:] *= 0.3
    lo, hi = _bisect(prober(gate), centre, dirs, lambda a: a == 0, 1.0e7)
    rows6 = np.concatenate([centre, centre + 0.5 * lo[:, None] * dirs, centre + lo[:, None] * dirs,
                            centre + hi[:, None] * dirs, centre + 2.0 * hi[:, None] * dirs])
    want = np.concatenate([np.zeros(1 + 2 * LONG_RAYS, np.int32), np.full(2 * LONG_RAYS, -1, np.int32)])
    order = rng.permutation(len(rows6))
    f1 = np.zeros((len(rows6), 8))
    f1[:, :6] = rows6[order]
    f1[:, 6], f1[:, 7] = 0.25, 20.0
    want = want[order]
    taken = f1[want >= 0]
    scene = _dt_scene(f"60 s predict, gate {gate}", kw, [f0, f1, taken], [EQ_DT, LONG_DT, 0.125], taken)
    _ro(want, lo, hi)

    def check(fr):
        assert np.array_equal(np.nextafter(lo, np.inf), hi) and np.all(lo > 1.0)
        assert fr[0].n_tracks == 1 and np.array_equal(fr[1].assoc, want), (fr[1].assoc, want)
        assert fr[1].tracks["lifetime"][0] == 0.0 and fr[1].tracks["point_num"][0] == 1 + 2 * LONG_RAYS
        assert fr[1].labels is not None and len(fr[1].labels) == 2 * LONG_RAYS                 # the refused rows go to apply_DBscan
        assert gate > 16 and np.all(replay(scene, upto=2, tr_gate=float(gate - 16))[1].assoc == -1)   # log|det C| alone is beyond that
        assert fr[2].n_tracks >= 1 and np.all(np.isfinite(fr[2].tracks["P"])) and np.any(fr[2].assoc == 0)
    return {"long_predict": Equality(scene, check)}


@functools.lru_cache(maxsize=None)
def dt_edges(dim_x):
    """name -> Equality: the frame-interval edges, each asserted on the oracle before anything else uses it."""
    out = {}
    for part in (_lifetime_sums(dim_x, "dynamic"), _lifetime_sums(dim_x, "static"), _dtm_zero(dim_x), _stands_still(dim_x), _long_predict(dim_x)):
        out.update(part)
    for eq in out.values():
        eq.check(replay(eq.scene))
    return out


def dt_edge_groups(dim_x):
    """The interval edges grouped by configuration: one context each."""
    groups = {}
    for name, eq in dt_edges(dim_x).items():
        groups.setdefault(cfg_key(eq.scene.cfg), []).append(name)
    return list(groups.values())


# ------------------------------------------------------------------------------------------------- the contexts of the tests
GATE_SCENES =((1, 3), (2, 3), (3, 3), (4, 12))      # (seed, tracks) of the four scenes of a gate context: one has 12 tracks
TIE_SCENES = ((1, 3), (2, 3), (4, 12))
MAX_PTS = (256, 320, 1024)                           # 1, 2 and 4 points per thread of k_track / k_scene
DIM_X = (6, 9)


def gate_kw(dim_x, tr_gate=GATE):
    return dict(CTX_KW, dim_x=int(dim_x), tr_gate=float(tr_gate))


def gate_context(max_pts, dim_x):
    """The four Probes of one gate context (they share the five gates around GATE)."""
    return [gate_probes(gate_kw(dim_x), max_pts, seed, K=K) for seed, K in GATE_SCENES]


def tie_context(max_pts, dim_x):
    """(Probes of TIE_SCENES, the exact tie in both orders): one context under TIE_GATE."""
    kw = gate_kw(dim_x, TIE_GATE)
    return [tie_probes(kw, max_pts, seed, K=K) for seed, K in TIE_SCENES], [exact_tie(kw, max_pts, o) for o in ("AB", "BA")]


class F32Probe(NamedTuple):
    scene: Scene          # every value exactly representable in float32
    frame: int
    rows: np.ndarray      # where the probe row sits in the probe frame
    track: int
    gate: float           # d == gate exactly: the row is refused under `gate` ...
    gate_up: float        # ... and taken under nextafter(gate)


@functools.lru_cache(maxsize=None)
def f32_gate_probe(max_pts, dim_x, seed=1, K=3):
    """A float32 row cannot be moved onto the gate surface, so the gate is moved onto the row: the first gate probe's t_lo row
    rounded to float32, put at rows 0, n - 1, both sides of every seam and a few more; tr_gate bisected on the oracle until g and
    nextafter(g) decide differently, i.e. d == g exactly.  The rest of the scene is gate_probes' with the probe frame rounded to
    float32 (its other probe rows are then ordinary rows some 1e-6 off the surface)."""
    p = gate_probes(gate_kw(dim_x), max_pts, seed, K=K)
    sc, f = p.scene, p.frame
    n = int(sc.cnt[f])
    pts = sc.pts.copy()
    pts[f] = _f32_exact(pts[f])
    assert np.array_equal(_f32_exact(pts), pts)
    rows = np.array(sorted({q for q in (0, n - 1) + SEAMS if q < n} | set(p.pos[1:6, 0].tolist())))
    j = int(p.track[0])
    pts[f, rows] = pts[f, p.pos[0, 0]]
    _ro(pts)
    scene = sc._replace(tag=sc.tag + ", float32", pts=pts)

    def taken(g):
        a = replay(scene, upto=f + 1, tr_gate=g)[f].assoc[rows]
        assert np.all(a == a[0])
        return a[0] == j

    lo, hi = GATE - 2.0 ** -10, GATE + 2.0 ** -10
    assert not taken(lo) and taken(hi)
    while np.nextafter(lo, np.inf) != hi:
        mid = lo + (hi - lo) / 2
        lo, hi = (lo, mid) if taken(mid) else (mid, hi)
    before = [replay(scene, upto=f, tr_gate=g) for g in (GATE - 2.0 ** -10, lo, hi, GATE + 2.0 ** -10)]
    assert all(b[f - 1].tracks.tobytes() == before[0][f - 1].tracks.tobytes() for b in before)   # the history saw no gate move
    return F32Probe(scene, f, rows, j, float(lo), float(hi))
